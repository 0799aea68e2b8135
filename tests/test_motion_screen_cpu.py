"""`robot.motion.contact_detection` / `robot.motion.screening` on the CPU: option parsing and every refusal, the link masses of
`Skeleton.from_mjcf`, and `restate_*` — a numpy float64 restatement of the contact rule, the stability distance and the verdict rule, which
tests/test_gpu_motion_screen.py holds the kernels to.

The restatement is itself held to the reference: tests/golden/motion_screen.npz (tools/gen_motion_screen_golden.py) records what the
reference's `foot_detect` made of the four shipped clips' foot positions and what its `check_conditions` said of a set of distance
sequences; masks must be equal element for element, verdicts equal.
"""
import json
import os

import numpy as np
import pytest

from pbhc_amd import _lib, motion_screen
from pbhc_amd.motion_screen import ContactDetection, Screening
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN

FIXTURE = os.path.join(GOLDEN, "motion_screen.npz")
MJCF = {"g1_23dof": "g1_23dof_lock_wrist_fitmotionONLY.xml", "g1_29dof": "g1_29dof_rev_1_0.xml"}
SKELETON_JSON = {"g1_23dof": "skeleton_g1_23dof_lock_wrist_fitmotionONLY.json", "g1_29dof": "skeleton_g1_29dof_rev_1_0.json"}
CLIP_FILES = {"walk": "g1_walk_45cms_23dof.npz", "ue_walk": "g1_ue_walk_23dof.npz", "horse": "Horse-stance_pose.npz",
              "rig29": "g1_rig_Skeleton_Sequence_converted_processed_g1_29dof_rev_1_0.npz"}
CONTACT_CLIPS = ("walk", "ue_walk", "horse", "rig29")
_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = dict(np.load(FIXTURE))
    return _cache["fx"]


def verdict_cases():
    fx = fixture()
    return sorted({k.split("::")[1] for k in fx if k.startswith("verdict::")})


def skeleton_mjcf(robot):
    """both G1 models from the MJCF with the extended bodies of the JSON fixture (the MJCF route is the one that has link masses)"""
    if robot not in _cache:
        js = json.load(open(os.path.join(GOLDEN, SKELETON_JSON[robot])))
        B = len(js["body_names"])
        ext = [dict(joint_name=n, parent_name=js["body_names"][js["parents"][i]], pos=js["offsets"][i], rot=js["local_rot_wxyz"][i])
               for i, n in enumerate(js["body_names_ext"]) if i >= B]
        _cache[robot] = Skeleton.from_mjcf(os.path.join(GOLDEN, "mjcf", MJCF[robot]), ext)
    return _cache[robot]


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------------
def restate_contact(foot_pos, vel_threshold=0.002, height_threshold=0.12):
    """foot_pos [F,2,3] -> (mask [F,2] float32, dp2 [F,2], z [F,2]): frame 0 is 1; frame f >= 1 is 1 iff |p_f - p_(f-1)|^2 < vel_threshold and
    p_f.z < height_threshold.  dp2 (frame 0: inf) and z are returned for the bands of the GPU test."""
    p = np.asarray(foot_pos, dtype=np.float64)
    F = p.shape[0]
    dp2 = np.full((F, 2), np.inf)
    dp2[1:] = ((p[1:] - p[:-1]) ** 2).sum(-1)
    z = p[:, :, 2]
    mask = ((dp2 < vel_threshold) & (z < height_threshold)).astype(np.float32)
    mask[0] = 1.0
    return mask, dp2, z


def restate_fk(sk, pose_aa, trans):
    """float64 FK of the raw arrays -> (pos [F,Bx,3], rot [F,Bx,3,3]): p_i = R_p o_i + p_p, R_i = R_p L_i J_i"""
    from scipy.spatial.transform import Rotation as sRot

    pose = np.asarray(pose_aa, dtype=np.float64)[:, :sk.num_bodies_ext]
    F, Bx = pose.shape[:2]
    J = sRot.from_rotvec(pose.reshape(-1, 3)).as_matrix().reshape(F, Bx, 3, 3)
    q = np.asarray(sk.local_rot_wxyz, dtype=np.float64)
    L = sRot.from_quat(q[:, [1, 2, 3, 0]]).as_matrix()
    off = np.asarray(sk.offsets, dtype=np.float64)
    pos, rot = np.zeros((F, Bx, 3)), np.zeros((F, Bx, 3, 3))
    for i in range(Bx):
        p = int(sk.parents[i])
        if p < 0:
            pos[:, i], rot[:, i] = np.asarray(trans, dtype=np.float64), J[:, i]
        else:
            pos[:, i] = rot[:, p] @ off[i] + pos[:, p]
            rot[:, i] = rot[:, p] @ (L[i] @ J[:, i])
    return pos, rot


def restate_distance(sk, pose_aa, trans, cop_w=10.0, cop_k=100.0):
    """-> (d [F], scale [F]): the distance between the mass-weighted centre of the real bodies and the pressure-weighted centre of their
    origins, horizontal, with the ground at the lowest real-body origin of frame 0; scale = the largest |coordinate| of the frame's bodies"""
    B = sk.num_bodies
    pos, rot = restate_fk(sk, pose_aa, trans)
    pos, rot = pos[:, :B], rot[:, :B]
    m = np.asarray(sk.body_mass, dtype=np.float64)
    c = np.asarray(sk.body_com, dtype=np.float64)
    com = (m[None, :, None] * (pos + np.einsum("fbij,bj->fbi", rot, c))).sum(1) / m.sum()
    z = pos[:, :, 2] - pos[0, :, 2].min()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        w = np.where(z >= 0.0, np.exp(-cop_w * z), 1.0 - cop_k * z)
        cop = (w[:, :, None] * pos).sum(1) / (w.sum(1)[:, None] + 1e-6)
        d = np.linalg.norm((com - cop)[:, :2], axis=1)
    return d, np.abs(pos).max(axis=(1, 2))


def restate_verdict(dist, epsilon_stab=0.1, epsilon_stab_frames=100):
    """-> dict(stable, first_dist, last_dist, max_dist, unstable_share, max_gap): a frame is stable iff its distance is finite and below
    epsilon_stab; the clip iff its first and last frame are and, if F > N, no two consecutive stable frames lie >= N apart"""
    d = np.asarray(dist, dtype=np.float64)
    F, N = len(d), int(epsilon_stab_frames)
    ok = np.isfinite(d) & (d < epsilon_stab)
    idx = np.flatnonzero(ok)
    max_gap = int(np.diff(idx).max()) if len(idx) >= 2 else 0
    stable = bool(ok[0] and ok[-1] and not (F > N and max_gap >= N))
    return dict(stable=stable, first_dist=d[0], last_dist=d[-1], max_dist=float(np.where(np.isfinite(d), d, np.inf).max()),
                unstable_share=float((~ok).sum()) / F, max_gap=max_gap)


# ---- the restatement against the reference's recorded outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("clip", CONTACT_CLIPS)
def test_contact_restatement_equals_the_reference(clip):
    fx = fixture()
    mask, _, _ = restate_contact(fx[f"contact::{clip}::foot_pos"])
    want = fx[f"contact::{clip}::mask"]
    assert mask.shape == want.shape and want.dtype == np.float32
    assert np.array_equal(mask, want), (clip, int((mask != want).sum()))
    assert 0.0 < want[1:].mean() < 1.0 or clip == "horse"          # the fixture exercises both outcomes


@pytest.mark.parametrize("case", verdict_cases())
def test_verdict_restatement_equals_the_reference(case):
    fx = fixture()
    eps, N = fx[f"verdict::{case}::params"]
    got = restate_verdict(fx[f"verdict::{case}::dist"], eps, int(N))
    assert got["stable"] == bool(fx[f"verdict::{case}::stable"]), (case, got)


def test_verdict_cases_cover_the_edges():
    fx = fixture()
    got = {c: (len(fx[f"verdict::{c}::dist"]), int(fx[f"verdict::{c}::params"][1]), bool(fx[f"verdict::{c}::stable"]),
               restate_verdict(fx[f"verdict::{c}::dist"], *fx[f"verdict::{c}::params"])["max_gap"]) for c in verdict_cases()}
    assert got["one_frame_stable"] == (1, 10, True, 0)
    assert got["len_N_gap"] == (10, 10, True, 9) and got["len_N1_same_gap"] == (11, 10, True, 9) and got["len_N1_gap_N"] == (11, 10, False, 10)
    assert got["gap_N_minus_1"][2:] == (True, 9) and got["gap_N"][2:] == (False, 10)
    assert got["only_ends_long"] == (300, 100, False, 299) and got["only_ends_short"] == (100, 100, True, 99)
    assert not got["first_unstable"][2] and not got["last_unstable"][2]
    assert got["nan_middle"][2:] == (True, 2) and got["nan_run"][2:] == (False, 11)
    assert got["gap_spans_runs"][2:] == (True, 99) and got["gap_spans_runs_N"][2:] == (False, 100)


# ---- settings --------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_reference_constants():
    cd = ContactDetection.from_config({"enable": True})
    assert (cd.foot_bodies, cd.vel_threshold, cd.height_threshold, cd.overwrite) == (["left_ankle_roll_link", "right_ankle_roll_link"], 0.002, 0.12, False)
    assert cd.active and not ContactDetection.from_config({}).active and ContactDetection.from_config(None) is None
    sc = Screening.from_config({"enable": True})
    assert (sc.epsilon_stab, sc.epsilon_stab_frames, sc.cop_w, sc.cop_k, sc.action) == (0.1, 100, 10.0, 100.0, "report")
    assert sc.active and not Screening.from_config({}).active and Screening.from_config(None) is None
    for robot in MJCF:                                               # the reference's hard-coded indices 6 and 12, by name
        sk = Skeleton.from_json(os.path.join(GOLDEN, SKELETON_JSON[robot]))
        assert cd.foot_indices(sk) == [6, 12]
        p = motion_screen.to_c(cd, sc, sk)
        assert (p.foot[0], p.foot[1], p.vel_threshold, p.height_threshold) == (6, 12, 0.002, 0.12)
        assert (p.epsilon_stab, p.epsilon_stab_frames, p.cop_w, p.cop_k) == (0.1, 100, 10.0, 100.0)


def test_refusals():
    sk = Skeleton.from_json(os.path.join(GOLDEN, SKELETON_JSON["g1_23dof"]))
    with pytest.raises(_lib.PbhcError, match="unknown key"):
        ContactDetection.from_config({"enable": True, "threshold": 1.0})
    with pytest.raises(_lib.PbhcError, match="unknown key"):
        Screening.from_config({"enable": True, "epsilon": 1.0})
    with pytest.raises(_lib.PbhcError, match="left_toe"):
        ContactDetection.from_config({"enable": True, "foot_bodies": ["left_toe", "right_ankle_roll_link"]}).foot_indices(sk)
    with pytest.raises(_lib.PbhcError, match="two different"):
        ContactDetection(enable=True, foot_bodies=["left_ankle_roll_link"])
    with pytest.raises(_lib.PbhcError, match="two different"):
        ContactDetection(enable=True, foot_bodies=["left_ankle_roll_link", "left_ankle_roll_link"])
    with pytest.raises(_lib.PbhcError, match="vel_threshold"):
        ContactDetection(enable=True, vel_threshold=0.0)
    with pytest.raises(_lib.PbhcError, match="action"):
        Screening(enable=True, action="downweight")
    with pytest.raises(_lib.PbhcError, match="epsilon_stab_frames"):
        Screening(enable=True, epsilon_stab_frames=0)
    with pytest.raises(_lib.PbhcError, match="epsilon_stab"):
        Screening(enable=True, epsilon_stab=float("nan"))
    # screening needs link masses: a skeleton from the JSON fixture has none, and the message names the MJCF route
    with pytest.raises(_lib.PbhcError, match="MJCF"):
        Screening(enable=True).check_skeleton(sk)
    Screening(enable=True).check_skeleton(skeleton_mjcf("g1_23dof"))


def test_exclude_with_nothing_left_is_refused():
    assert motion_screen.kept_clips([True, False, True], "exclude") == [0, 2]
    assert motion_screen.kept_clips([True, False, True], "report") == [0, 1, 2]
    assert motion_screen.kept_clips([False], "report") == [0]
    with pytest.raises(_lib.PbhcError, match="empty"):
        motion_screen.kept_clips([False, False], "exclude")
    with pytest.raises(_lib.PbhcError, match="empty"):
        motion_screen.kept_clips([False], "exclude")            # a one-clip (WJX) library whose clip fails


# ---- link masses -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,total", [("g1_23dof", 31.69), ("g1_29dof", 33.34)])
def test_from_mjcf_reads_the_link_masses(robot, total):
    sk = skeleton_mjcf(robot)
    assert sk.body_mass.shape == (sk.num_bodies,) and sk.body_com.shape == (sk.num_bodies, 3)
    assert sk.body_mass.dtype == np.float32 and (sk.body_mass >= 0).all()
    assert abs(float(sk.body_mass.astype(np.float64).sum()) - total) < 0.005
    # the tables the kernels walk are those of the JSON fixture: masses are the only addition
    js = Skeleton.from_json(os.path.join(GOLDEN, SKELETON_JSON[robot]))
    assert sk.body_names_ext == js.body_names_ext and np.array_equal(sk.parents, js.parents)
    assert np.allclose(sk.offsets, js.offsets, atol=1e-7) and np.allclose(sk.local_rot_wxyz, js.local_rot_wxyz, atol=1e-7)
    assert js.body_mass is None and js.body_com is None


def test_a_body_without_inertial_weighs_nothing():
    sk = Skeleton.from_mjcf(os.path.join(GOLDEN, "mini_biped.xml"))
    assert sk.body_mass.shape == (sk.num_bodies,)
    root = __import__("xml.etree.ElementTree").etree.ElementTree.parse(os.path.join(GOLDEN, "mini_biped.xml")).getroot()
    have = {b.attrib["name"]: float(b.find("inertial").attrib["mass"]) for b in root.iter("body") if b.find("inertial") is not None}
    assert [float(m) for m in sk.body_mass] == [np.float32(have.get(n, 0.0)) for n in sk.body_names]


@pytest.mark.parametrize("robot", list(SKELETON_JSON))
def test_json_round_trip_without_masses_is_byte_identical(robot, tmp_path):
    sk = Skeleton.from_json(os.path.join(GOLDEN, SKELETON_JSON[robot]))
    sk.to_json(str(tmp_path / "s.json"))
    # what to_json wrote before masses existed: these six keys, in this order, indent 1
    want = json.dumps(dict(body_names=sk.body_names, body_names_ext=sk.body_names_ext, parents=sk.parents.tolist(), offsets=sk.offsets.tolist(),
                           local_rot_wxyz=sk.local_rot_wxyz.tolist(), dof_axis=sk.dof_axis.tolist()), indent=1)
    assert (tmp_path / "s.json").read_text() == want
    assert Skeleton.from_json(str(tmp_path / "s.json")).body_mass is None


def test_json_round_trip_carries_masses_when_present(tmp_path):
    sk = skeleton_mjcf("g1_23dof")
    sk.to_json(str(tmp_path / "s.json"))
    sk2 = Skeleton.from_json(str(tmp_path / "s.json"))
    assert np.array_equal(sk2.body_mass, sk.body_mass) and np.array_equal(sk2.body_com, sk.body_com)
    for a in ("parents", "offsets", "local_rot_wxyz", "dof_axis"):
        assert np.array_equal(getattr(sk, a), getattr(sk2, a)), a


# ---- the issue's CPU figures for the shipped clips, from the restatement ------------------------------------------------------------------
def test_shipped_clips_through_the_restatement():
    """walk and ue_walk stable; horse stance stable at N = 100 (largest gap 77) and not at N = 50; the 29-dof clip unstable, its last frames
    far above the ground, its last-frame distance about 9 m"""
    from pbhc_amd.motion_lib import load_motion_file

    out = {}
    for name, f in CLIP_FILES.items():
        clip = load_motion_file(os.path.join(GOLDEN, "clips", f))[0][1]
        sk = skeleton_mjcf("g1_29dof" if name == "rig29" else "g1_23dof")
        d, _ = restate_distance(sk, np.asarray(clip["pose_aa"], np.float32), np.asarray(clip["root_trans_offset"], np.float32))
        out[name] = (d, restate_verdict(d, 0.1, 100), restate_verdict(d, 0.1, 50))
        print(name, out[name][1], "closest |d - eps|", float(np.nanmin(np.abs(d - 0.1))))
    assert out["walk"][1]["stable"] and out["ue_walk"][1]["stable"]
    assert out["horse"][1]["stable"] and out["horse"][1]["max_gap"] == 77 and not out["horse"][2]["stable"]
    assert not out["rig29"][1]["stable"] and abs(out["rig29"][1]["last_dist"] - 9.0) < 0.1
