"""Fixture generator for `robot.motion.contact_detection` / `robot.motion.screening` (tests/test_motion_screen_cpu.py,
tests/test_gpu_motion_screen.py): runs the REFERENCE's `foot_detect` (motion_source/count_pkl_contact_mask.py) and `check_conditions`
(smpl_retarget/motion_filter/utils/motion_filter.py) and records their inputs and outputs as tests/golden/motion_screen.npz (data only).

Build machine only, never imported by a test: it needs the reference checkout.  The modules around the two functions import hydra, joblib,
smpl_sim, a mesh library and a GPU SMPL model at the top, so neither file is imported: each is parsed at run time, the ONE function's node
is compiled out of the parsed file and run in a namespace that holds numpy — the two functions need nothing else, so the harness's import
shims are not involved.  Nothing of their text is copied.

    PYTHONPATH=<repo> python tools/gen_motion_screen_golden.py --reference <reference checkout>

Recorded:
    contact::<clip>::foot_pos [F,2,3] float32   the two ankle-roll links (extended-body indices 6 and 12, the script's constants: column 0
                                                = index 6 = left) of the four shipped clips by the ORACLE's FK (oracle/fk.py motion_fk, the
                                                float32 restatement of the reference's Humanoid_Batch.fk_batch; the fixture says so in `fk`)
    contact::<clip>::mask [F,2] float32         what foot_detect made of them
    verdict::<case>::dist [F] float64, ::params [eps, N], ::stable      the edge cases of the verdict rule and what check_conditions said
"""
import argparse
import ast
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pbhc_amd.motion_lib import load_motion_file  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "motion_screen.npz")
CLIPS = {"walk": ("g1_walk_45cms_23dof.npz", "g1_23dof"), "ue_walk": ("g1_ue_walk_23dof.npz", "g1_23dof"),
         "horse": ("Horse-stance_pose.npz", "g1_23dof"),
         "rig29": ("g1_rig_Skeleton_Sequence_converted_processed_g1_29dof_rev_1_0.npz", "g1_29dof")}
FEET = (6, 12)                                   # the script's fid_l, fid_r


def reference_function(path, name, namespace):
    """the function `name` of the reference file `path`, compiled from its node of the parsed file alone"""
    tree = ast.parse(open(path).read(), filename=path)
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = dict(namespace)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def verdict_cases():
    """name -> (dist, eps, N): stable frames are 0.05, unstable ones 0.5 (eps 0.1)"""
    lo, hi, eps = 0.05, 0.5, 0.1

    def seq(F, stable):
        d = np.full(F, hi)
        d[list(stable)] = lo
        return d

    N = 10
    cases = {
        "one_frame_stable": (seq(1, [0]), eps, N),
        "one_frame_unstable": (seq(1, []), eps, N),
        "len_N_gap": (seq(N, [0, N - 1]), eps, N),                       # F = N: the gap rule is off (n > N is strict), gap N - 1
        "len_N1_same_gap": (seq(N + 1, [0, N - 1, N]), eps, N),           # F = N + 1, the same gap N - 1: passes
        "len_N1_gap_N": (seq(N + 1, [0, N]), eps, N),                     # gap exactly N: fails (gap >= N)
        "gap_N_minus_1": (seq(40, [0, 5, 5 + N - 1, 20, 29, 38, 39]), eps, N),
        "gap_N": (seq(40, [0, 5, 5 + N, 20, 29, 38, 39]), eps, N),
        "only_ends_long": (seq(300, [0, 299]), eps, 100),
        "only_ends_short": (seq(100, [0, 99]), eps, 100),
        "first_unstable": (seq(30, range(1, 30)), eps, N),
        "last_unstable": (seq(30, range(0, 29)), eps, N),
        "all_stable_long": (seq(700, range(700)), eps, 100),              # more frames than a workgroup has threads
        "gap_spans_runs": (seq(700, list(range(0, 300)) + list(range(398, 700))), eps, 100),      # gap 99 across several threads' runs
        "gap_spans_runs_N": (seq(700, list(range(0, 300)) + list(range(399, 700))), eps, 100),    # gap 100
    }
    nan = seq(30, range(30))
    nan[14] = np.nan
    cases["nan_middle"] = (nan, eps, N)                                   # one NaN: a gap of 2, passes
    nan2 = seq(30, range(30))
    nan2[10:20] = np.nan
    cases["nan_run"] = (nan2, eps, N)                                     # stable 9 and 20: gap 11, fails
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    reference = os.path.abspath(args.reference)
    import torch

    from oracle.fk import motion_fk
    from tests.helpers import skel_from_golden

    foot_detect = reference_function(os.path.join(reference, "motion_source", "count_pkl_contact_mask.py"), "foot_detect", {"np": np})
    check_conditions = reference_function(os.path.join(reference, "smpl_retarget", "motion_filter", "utils", "motion_filter.py"), "check_conditions", {})
    arrs = {"fk": np.array("oracle/fk.py motion_fk (float32 torch, the restatement of the reference's Humanoid_Batch.fk_batch); feet = extended "
                           "bodies 6 (column 0) and 12 (column 1)")}
    for name, (fname, robot) in CLIPS.items():
        clip = load_motion_file(os.path.join(GOLDEN, "clips", fname))[0][1]
        skel = skel_from_golden(robot)
        assert [skel["body_names_ext"][i] for i in FEET] == ["left_ankle_roll_link", "right_ankle_roll_link"]
        pos = motion_fk(skel, clip["pose_aa"], clip["root_trans_offset"], 1.0 / int(clip["fps"]))["gts_t"]
        assert pos.dtype == torch.float32
        left, right = foot_detect(pos)
        mask = np.concatenate([left, right], axis=-1).astype(np.float32)
        assert mask.shape == (pos.shape[0], 2)
        arrs[f"contact::{name}::foot_pos"] = pos[:, list(FEET)].numpy().astype(np.float32)
        arrs[f"contact::{name}::mask"] = mask
        print(f"{name}: {mask.shape[0]} frames, contact share {mask.mean(0)}")
    for name, (d, eps, N) in verdict_cases().items():
        arrs[f"verdict::{name}::dist"] = d.astype(np.float64)
        arrs[f"verdict::{name}::params"] = np.array([eps, N], dtype=np.float64)
        arrs[f"verdict::{name}::stable"] = np.array(bool(check_conditions(list(d), epsilon_stab=eps, epsilon_stab_N=N)))
        print(f"{name}: F = {len(d)}, N = {N} -> {bool(arrs[f'verdict::{name}::stable'])}")
    np.savez_compressed(args.out, **arrs)
    print(f"wrote {args.out}: {os.path.getsize(args.out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
