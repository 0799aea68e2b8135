"""`robot.motion.augmentation` on the CPU: option parsing, every refusal, the mirror tables of both shipped skeletons, and `restate` — a numpy
float64 restatement of the mirror rule and the speed rule, which tests/test_gpu_motion_augment.py holds the kernel to.

The mirror is checked against the oracle's FK: FK of the restated mirror of a clip must be the mirrored, permuted FK of the clip.  Joint
angles and rotations (up to the quaternion's sign) exactly — float multiplication and addition are symmetric under a sign flip, and the
shipped skeletons' local rotations are exactly symmetric — positions within (max chain depth + 2) x a, a the offset asymmetry the skeleton
check measured (1.0e-5 m for both skeletons): every link of a chain adds its offset's asymmetry once, rotated, and two more cover the float32
rounding of the chain's sums, which is far below a.  A wrong permutation or sign is off by centimetres.  Measured: 1.0e-5 – 1.05e-5 m.
Angular velocity is not part of the check: the reference's matrix -> quaternion sign choice is not mirror-symmetric, so its finite-difference
angular velocity differs where the sign flips.
"""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest

from pbhc_amd import _lib
from pbhc_amd.motion_augment import Augmentation, mirror_tables, out_frames
from pbhc_amd.motion_lib import MotionLib, load_motion_file
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, fixture_config, skel_from_golden
from tests.test_motion_interp_cpu import _q_from_rotvec, _rotvec_from_q, _slerp

SKELETONS = {"g1_23dof": "skeleton_g1_23dof_lock_wrist_fitmotionONLY.json", "g1_29dof": "skeleton_g1_29dof_rev_1_0.json"}
CLIP29 = "g1_rig_Skeleton_Sequence_converted_processed_g1_29dof_rev_1_0.npz"


def skeleton(robot):
    return Skeleton.from_json(os.path.join(GOLDEN, SKELETONS[robot]))


def load_clip(name):
    return dict(load_motion_file(os.path.join(GOLDEN, "clips", name))[0][1])


def cut(clip, a, b):
    return {k: (np.asarray(v)[a:b] if k in ("pose_aa", "root_trans_offset", "contact_mask") else v) for k, v in clip.items()}


def walk_with_mask():
    """the walk clip ships without a contact mask: the synthetic alternating one of tools/gen_motion_interp_golden.py"""
    walk = load_clip("g1_walk_45cms_23dof.npz")
    left = (np.arange(walk["pose_aa"].shape[0]) // 8) % 2 == 0
    walk["contact_mask"] = np.stack([left, ~left], axis=1).astype(np.float32)
    return walk


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------------
def frames_at_speed(F, s):
    """the issue's host formula: floor((F - 1) / s) + 1 in double, one less if the last sample would pass the last source frame"""
    Fo = math.floor((F - 1) / s) + 1
    return Fo - 1 if (Fo - 1) * s > F - 1 else Fo


def restate(clip, mirrored, speed, perm=None):
    """One clip -> (pose_aa, trans, contact or None) of one variant, float32: every interpolated value formed in float64 and rounded once.
    perm [Bx]: the body permutation of the mirror (mirror_tables(...).body_perm)."""
    pose, trans = np.asarray(clip["pose_aa"], np.float32), np.asarray(clip["root_trans_offset"], np.float32)
    contact = np.asarray(clip["contact_mask"], np.float32) if "contact_mask" in clip else None
    F = pose.shape[0]
    if speed != 1.0:
        Fo = frames_at_speed(F, speed)
        o_pose, o_trans = np.zeros((Fo,) + pose.shape[1:], np.float32), np.zeros((Fo, 3), np.float32)
        o_contact = None if contact is None else np.zeros((Fo, 2), np.float32)
        for k in range(Fo):
            x = k * float(speed)
            i0 = min(int(math.floor(x)), F - 1)
            i1 = min(i0 + 1, F - 1)
            t = x - i0
            if t == 0.0:
                o_pose[k], o_trans[k] = pose[i0], trans[i0]
            else:
                a, b = pose[i0].astype(np.float64), pose[i1].astype(np.float64)
                o_pose[k] = (a + t * (b - a)).astype(np.float32)
                o_pose[k, 0] = _rotvec_from_q(_slerp(_q_from_rotvec(a[0]), _q_from_rotvec(b[0]), t)).astype(np.float32)
                ta, tb = trans[i0].astype(np.float64), trans[i1].astype(np.float64)
                o_trans[k] = (ta + t * (tb - ta)).astype(np.float32)
            if contact is not None:
                o_contact[k] = contact[i0 if t < 0.5 else i1]
        pose, trans, contact = o_pose, o_trans, o_contact
    if mirrored:
        pose = pose[:, np.asarray(perm)] * np.array([-1.0, 1.0, -1.0], np.float32)
        trans = trans * np.array([1.0, -1.0, 1.0], np.float32)
        contact = None if contact is None else contact[:, ::-1].copy()
    return pose, trans, contact


# ---- option parsing and refusals -------------------------------------------------------------------------------------------------------
def test_options_are_parsed_and_variants_are_ordered_speed_major():
    a = Augmentation.from_config({"mirror": True, "speeds": [0.8, 1.25], "symmetry_tol": 2e-4})
    assert (a.mirror, a.speeds, a.symmetry_tol, a.num_variants, a.active) == (True, [0.8, 1.25], 2e-4, 6, True)
    assert [a.variant(v) for v in range(6)] == [(False, 1.0), (True, 1.0), (False, 0.8), (True, 0.8), (False, 1.25), (True, 1.25)]
    b = Augmentation.from_config({"speeds": [1.0, 2.0]})                        # 1.0 is always there and need not be listed
    assert (b.mirror, b.speeds, b.symmetry_tol, b.num_variants) == (False, [2.0], 1e-4, 2)
    assert [b.variant(v) for v in range(2)] == [(False, 1.0), (False, 2.0)]
    assert Augmentation.from_config(None) is None
    for off in ({}, {"mirror": False}, {"mirror": False, "speeds": []}, {"speeds": [1.0]}):
        assert not Augmentation.from_config(off).active                          # the same as the key absent
    p = a.to_c()
    assert (p.num_variants, p.num_speeds, p.mirror, list(p.speeds)[:2]) == (6, 2, 1, [0.8, 1.25])


def test_frame_counts_follow_the_host_formula():
    for F in (8, 9, 40, 122, 520):
        for s in (0.25, 0.5, 0.8, 1.0, 1.25, 1.3, 2.0, 4.0):
            Fo = out_frames(F, s)
            assert Fo == frames_at_speed(F, s) and (Fo - 1) * s <= F - 1 < Fo * s + 1e-9, (F, s, Fo)
    assert (out_frames(122, 0.5), out_frames(122, 2.0), out_frames(122, 1.3), out_frames(40, 1.3)) == (243, 61, 94, 31)
    a = Augmentation(mirror=True, speeds=[0.5, 2.0, 1.3])
    assert a.variant_frames(122) == [122, 122, 243, 243, 61, 61, 94, 94]


def test_bad_options_are_refused_with_the_keys_name():
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: unknown key\(s\) \['speed'\]"):
        Augmentation.from_config({"speed": [0.8]})
    for s in (0.2, 4.5, float("nan")):
        with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: speed .* outside \[0\.25, 4\.0\]"):
            Augmentation.from_config({"speeds": [0.8, s]})
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: 9 speeds"):
        Augmentation.from_config({"speeds": [0.55 + 0.1 * i for i in range(9)]})
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: .*twice"):
        Augmentation.from_config({"speeds": [0.8, 0.8]})
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: clip 1 has 20 frames, at speed 3\.0 that leaves 7, fewer than 8"):
        [Augmentation(speeds=[3.0]).variant_frames(F, f"clip {i}") for i, F in enumerate((40, 20))]


def test_a_v1_library_is_refused():
    mcfg = fixture_config("v1_g1_23dof_walk.yaml", 4, {"robot.motion.augmentation": {"mirror": True}}).robot.motion
    assert mcfg.motion_lib_type == "WJX"
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation with motion_lib_type WJX"):
        MotionLib.from_config(mcfg, skeleton("g1_23dof"), 4, "cpu")             # refused before anything touches a device
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: unknown key"):
        MotionLib.from_config(fixture_config("v2_g1_23dof_student.yaml", 4, {"robot.motion.augmentation": {"mirrored": True}}).robot.motion,
                              skeleton("g1_23dof"), 4, "cpu")
    assert "augmentation" not in fixture_config("v2_g1_23dof_student.yaml", 4).robot.motion    # absent by default


def test_export_refuses_bad_arguments_without_a_gpu():
    lib, E = _lib.lib(), _lib.K["PBHC_EINVAL"]
    csk = skeleton("g1_23dof").to_c()
    one = C.c_void_p(64)                                        # never dereferenced: every call below is refused before a launch

    def params(V=4, n=1, mirror=1, speeds=(2.0,)):
        p = _lib.PbhcMotionAugment()
        p.num_variants, p.num_speeds, p.mirror = V, n, mirror
        for k, s in enumerate(speeds):
            p.speeds[k] = s
        return p

    def call(p, total_in=10, M=2, total_out=32, contact=None, out_contact=None, perm=one, pose=one, out_pose=one):
        return lib.pbhc_motion_augment_batch(C.byref(csk), pose, one, contact, total_in, M, one, one, total_out, p, perm, out_pose, one, out_contact, None)

    # 10 frames in 2 clips at speeds 1.0 and 2.0: 10 + (4, 6] per mirror side, so 30 or 32 frames with the mirror
    assert call(params(), pose=None) == E and b"pbhc_motion_augment_batch" in lib.pbhc_last_error() and b"NULL" in lib.pbhc_last_error()
    assert call(params(), out_pose=None) == E
    assert call(params(), perm=None) == E                                                          # mirror without its permutation
    assert call(params(), contact=one) == E and b"contact in without contact out" in lib.pbhc_last_error()
    assert call(params(V=0)) == E and call(params(V=3)) == E                                        # V < 1, V that is not speeds x mirror
    assert call(params(V=18, n=9, speeds=(2.0,) * 8)) == E and b"at most 8" in lib.pbhc_last_error()
    for s in (0.2, 4.5, float("nan")):
        assert call(params(speeds=(s,))) == E and b"outside [0.25, 4]" in lib.pbhc_last_error()
    for total_out in (33, 20, 26, 34, 64, 0, -32):                                                  # odd with a mirror, too few, too many
        assert call(params(), total_out=total_out) == E and b"frames out" in lib.pbhc_last_error(), total_out
    assert call(params(V=2, n=0, speeds=()), total_out=22) == E                                     # the mirror alone: exactly 2 x 10
    assert call(params(), total_in=1) == E                                                          # fewer frames than clips


# ---- mirror tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", sorted(SKELETONS))
def test_mirror_tables_of_the_shipped_skeletons(robot):
    sk = skeleton(robot)
    mt = mirror_tables(sk, 1e-4)
    names = list(sk.body_names_ext)
    perm = mt.body_perm
    assert perm.shape == (sk.num_bodies_ext,) and np.array_equal(perm[perm], np.arange(len(names)))           # an involution
    for i, n in enumerate(names):
        if "left" in n or "right" in n:
            assert names[perm[i]] == n.replace("left", "@").replace("right", "left").replace("@", "right") and perm[i] != i
        else:
            assert perm[i] == i
    for n in ("pelvis", "waist_yaw_link", "waist_roll_link", "torso_link", "head_link"):
        assert perm[names.index(n)] == names.index(n)
    assert np.array_equal(mt.dof_perm, perm[1:1 + sk.num_dof] - 1) and np.array_equal(mt.dof_perm[mt.dof_perm], np.arange(sk.num_dof))
    for d in range(sk.num_dof):                                                  # -1 exactly on the roll and yaw joints
        n = names[d + 1]
        assert mt.dof_sign[d] == (-1.0 if ("roll" in n or "yaw" in n) else 1.0), n
        assert ("roll" in n) + ("yaw" in n) + ("pitch" in n) + ("knee" in n) + ("elbow" in n) + (n == "torso_link") == 1, n
    print(f"{robot}: offset asymmetry {mt.asymmetry:.3e} m")
    assert 0.0 < mt.asymmetry <= 1.01e-5                                         # the skeletons are symmetric to 1.0e-5 m, not exactly
    with pytest.raises(_lib.PbhcError, match="offset of body"):
        mirror_tables(sk, 5e-6)


def test_asymmetric_skeletons_are_refused_by_name():
    sk = skeleton("g1_23dof")
    bad = copy.deepcopy(sk)
    i = list(sk.body_names_ext).index("right_knee_link")
    bad.offsets[i, 2] += 1e-3
    with pytest.raises(_lib.PbhcError, match=r"robot\.motion\.augmentation: mirror: the offset of body '(right|left)_knee_link' differs .*'(right|left)_knee_link'"):
        mirror_tables(bad, 1e-4)
    assert mirror_tables(bad, 2e-3).asymmetry == pytest.approx(1e-3, rel=0.02)   # symmetry_tol is the user's to widen
    bad = copy.deepcopy(sk)
    bad.dof_axis[list(sk.body_names_ext).index("left_hip_roll_link") - 1] = [0.0, 0.0, 1.0]
    with pytest.raises(_lib.PbhcError, match=r"axis .* of the joint of body '(left|right)_hip_roll_link'"):
        mirror_tables(bad, 1e-4)
    bad = copy.deepcopy(sk)
    bad.local_rot_wxyz[list(sk.body_names_ext).index("left_elbow_link")] = [np.cos(0.1), np.sin(0.1), 0.0, 0.0]
    with pytest.raises(_lib.PbhcError, match=r"local rotation of body '(left|right)_elbow_link'"):
        mirror_tables(bad, 1e-4)
    bad = copy.deepcopy(sk)
    bad.parents[list(sk.body_names_ext).index("left_hand_link")] = 0
    with pytest.raises(_lib.PbhcError, match=r"body '(left|right)_hand_link' hangs on"):
        mirror_tables(bad, 1e-4)
    bad = copy.deepcopy(sk)
    bad.body_names_ext = [n.replace("right_hand_link", "right_palm_link") for n in sk.body_names_ext]
    with pytest.raises(_lib.PbhcError, match=r"has no partner"):
        mirror_tables(bad, 1e-4)


# ---- the restated mirror against the oracle's FK ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", sorted(SKELETONS))
def test_fk_of_the_mirrored_clip_is_the_mirrored_fk(robot):
    from oracle.fk import motion_fk

    clip = load_clip("g1_walk_45cms_23dof.npz") if robot == "g1_23dof" else cut(load_clip(CLIP29), 0, 40)
    sk, osk = skeleton(robot), skel_from_golden(robot)
    assert list(osk["body_names_ext"]) == list(sk.body_names_ext)
    mt = mirror_tables(sk, 1e-4)
    perm = mt.body_perm
    pose, trans, _ = restate(clip, True, 1.0, perm)
    dt = 1.0 / int(clip["fps"])
    src = motion_fk(osk, clip["pose_aa"], clip["root_trans_offset"], dt)
    mir = motion_fk(osk, pose, trans, dt)
    dof = src["dof_pos"].numpy()
    assert np.array_equal(mir["dof_pos"].numpy(), dof[:, mt.dof_perm] * mt.dof_sign), "joint angles: permuted and signed exactly"
    want_rot = src["grs_t"].numpy()[:, perm] * np.array([-1.0, 1.0, -1.0, 1.0], np.float32)       # xyzw: (-x, y, -z, w)
    got_rot = mir["grs_t"].numpy()
    assert np.all(np.all(got_rot == want_rot, axis=-1) | np.all(got_rot == -want_rot, axis=-1)), "rotations: exact up to the quaternion's sign"
    want_pos = src["gts_t"].numpy()[:, perm] * np.array([1.0, -1.0, 1.0], np.float32)
    err = float(np.abs(mir["gts_t"].numpy().astype(np.float64) - want_pos).max())
    bound = (int(sk.depth.max()) + 2) * mt.asymmetry
    print(f"{robot}: max |FK(mirror) - mirror(FK)| position {err:.3e} m, bound {bound:.3e} m (depth {int(sk.depth.max())}, a {mt.asymmetry:.3e})")
    assert err <= bound
    # and the restatement is an involution: mirroring twice gives the clip back
    again = restate(dict(pose_aa=pose, root_trans_offset=trans, fps=clip["fps"]), True, 1.0, perm)
    assert np.all(again[0] == np.asarray(clip["pose_aa"], np.float32)) and np.all(again[1] == np.asarray(clip["root_trans_offset"], np.float32))


def test_restated_time_scaling_hits_the_source_frames_it_should():
    walk = walk_with_mask()
    pose, trans, contact = (np.asarray(walk[k], np.float32) for k in ("pose_aa", "root_trans_offset", "contact_mask"))
    fast = restate(walk, False, 2.0)
    assert fast[0].shape[0] == 61 and np.all(fast[0] == pose[::2]) and np.all(fast[1] == trans[::2]) and np.all(fast[2] == contact[::2])
    slow = restate(walk, False, 0.5)
    assert slow[0].shape[0] == 243 and np.all(slow[0][::2] == pose) and np.all(slow[2][::2] == contact)
    mid = 0.5 * (pose[:-1, 1:].astype(np.float64) + pose[1:, 1:])
    assert np.abs(slow[0][1::2, 1:] - mid).max() <= 2e-7                                            # odd frames: the midpoints
    assert np.all(slow[2][1::2] == contact[1:])                                                      # t = 0.5 takes the later frame
    odd = restate(walk, False, 1.3)
    assert odd[0].shape[0] == 94 and set(np.unique(odd[2])) <= {0.0, 1.0} and not odd[0][:, 24:].any()
