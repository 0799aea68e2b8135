"""Fit key-point clips to the robot under `robot.motion.retarget` and write them as ordinary motion clips (the job of the reference's
smpl_retarget/phc_retarget/fit_smpl_motion.py after its SMPL forward pass, for a whole file of clips at once, on the GPU: `pbhc_retarget_fit`).

    python tools/retarget_motion.py --config <config.yaml> --in <keypoints.npz> --out <clips.npz> [--mjcf robot.xml]
        [--iterations N --dof-lr R --root-lr R --ground none|first_frame_min_body]

The input is an .npz in the layout of `save_motion_npz`: per clip `<name>::keypoints` [F, K, 3] (world frame, already scaled to the robot),
`<name>::fps`, and optionally `<name>::root_trans_offset` [F, 3], `<name>::root_rot_init` [F, 3] and `<name>::keypoint_names` [K].  The
config supplies the skeleton and robot.motion.retarget (joint_matches, limits, heading_from, ...); options override the key.  `--mjcf` names
the model `limits: mjcf` reads the joint ranges from (default: the config's asset, when that is an MJCF).  Clips of the input that already
hold a pose_aa are written through unchanged.  Output: an .npz through `save_motion_npz`, and the first / last loss of every fitted clip.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbhc_amd import _lib, motion_ingest  # noqa: E402
from pbhc_amd.motion_lib import load_motion_file, save_motion_npz  # noqa: E402
from pbhc_amd.motion_retarget import RetargetSettings  # noqa: E402
from pbhc_amd.skeleton import Skeleton  # noqa: E402
from pbhc_amd.utils.config import load_config  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", required=True)
    ap.add_argument("--in", dest="src", required=True, help=".npz of key-point clips")
    ap.add_argument("--out", required=True, help=".npz to write")
    ap.add_argument("--mjcf", default=None, help="the robot's MJCF, for limits: mjcf (default: the config's asset if it is one)")
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--dof-lr", type=float, default=None)
    ap.add_argument("--root-lr", type=float, default=None)
    ap.add_argument("--ground", default=None)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)

    cfg = load_config(args.config, {}, now="tool")
    mcfg = cfg.robot.motion
    node = dict(mcfg.get("retarget", None) or {})
    node["enable"] = True
    for key in ("iterations", "dof_lr", "root_lr", "ground"):
        if getattr(args, key) is not None:
            node[key] = getattr(args, key)
    mjcf = args.mjcf
    if mjcf is None:
        path = os.path.join(str(mcfg.asset.assetRoot), str(mcfg.asset.assetFileName))
        if not os.path.isabs(path) and not os.path.exists(path):
            path = os.path.join(_lib.ROOT, path)
        mjcf = path if path.endswith(".xml") else None
    settings = RetargetSettings.from_config(node, mjcf=mjcf)
    skel = Skeleton.from_motion_config(mcfg)
    named = load_motion_file(args.src)
    clips, report = motion_ingest.retarget([c for _, c in named], skel, args.device, settings)
    save_motion_npz(args.out, [(name, c) for (name, _), c in zip(named, clips)])
    print(f"wrote {args.out}: {len(clips)} clip(s), frames {[int(c['pose_aa'].shape[0]) for c in clips]}")
    for i, first, last in zip(report["clips"], report["first_loss"], report["last_loss"]):
        print(f"  {named[i][0]}: mean key-point distance {first * 1e3:.1f} mm -> {last * 1e3:.1f} mm after {settings.iterations} iterations")
    return 0


if __name__ == "__main__":
    sys.exit(main())
