"""`robot.motion.interpolation` on the CPU: a numpy float64 restatement of the lead-in / lead-out frames against the reference's own output
(tests/golden/motion_interp.npz, recorded from robot_motion_process/motion_interpolation_pkl.py by tools/gen_motion_interp_golden.py), the
config parsing, the default pose and every refusal.  The restatement (`restate`) is also what tests/test_gpu_motion_interp.py holds the
kernel against where the reference's script cannot run (other joint counts, batches, zero frame counts).

Bound: 1e-6 absolute on every element, the clip's own frames included.  That is 4 ulp of float32 at pi, the largest magnitude present, and 4 x
the 2.4e-7 measured between the restatement and the script (whose float32 round trips through quaternions it does not share).
"""
import os

import numpy as np
import pytest

from pbhc_amd import _lib
from pbhc_amd.motion_interp import Interpolation, knee_frames_ok
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, build_env_config, fixture_config

TOL = 1e-6
FIXTURE = os.path.join(GOLDEN, "motion_interp.npz")
# the script's hard-coded default pose (motion_interpolation_pkl.py:269-275)
SCRIPT_DEFAULT_POSE = np.array([0.0, 0.0, 0.80, 0.0, 0.0, 0.0, 1.0, -0.1, 0.0, 0.0, 0.3, -0.2, 0.0, -0.1, 0.0, 0.0, 0.3, -0.2, 0.0, 0.0, 0.0, 0.0,
                                0.2, 0.2, 0.0, 0.9, 0.2, -0.2, 0.0, 0.9])


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _q_from_rotvec(v):
    a = np.linalg.norm(v)
    if a < 1e-12:
        return np.array([0.5 * v[0], 0.5 * v[1], 0.5 * v[2], 1.0])
    return np.concatenate([v / a * np.sin(a / 2), [np.cos(a / 2)]])


def _rotvec_from_q(q):
    q = q / np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    nv = np.linalg.norm(q[:3])
    if nv < 1e-12:
        return 2.0 * q[:3]
    return q[:3] / nv * 2.0 * np.arctan2(nv, q[3])


def _zyx_from_q(q):
    x, y, z, w = q
    return (np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z)), np.arcsin(np.clip(2 * (w * y - z * x), -1, 1)),
            np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)))


def _q_from_zyx(yaw, pitch, roll):
    qz = np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])
    qy = np.array([0, np.sin(pitch / 2), 0, np.cos(pitch / 2)])
    qx = np.array([np.sin(roll / 2), 0, 0, np.cos(roll / 2)])
    return _qmul(_qmul(qz, qy), qx)


def _slerp(A, B, t):
    rel = _qmul(A * np.array([-1, -1, -1, 1.0]), B)
    return _qmul(A, _q_from_rotvec(t * _rotvec_from_q(rel)))


def _legs(s, e, N):
    """dofs 0..11 of N synthetic frames from s to e, one leg after the other, the knees through 1.0 rad"""
    h, k = N // 2, (N // 2) // 2
    out = np.zeros((N, 12))
    for leg in (0, 1):
        sl = slice(6 * leg, 6 * leg + 6)
        mov = np.linspace(s[sl], e[sl], h + 1, endpoint=False)[1:]
        mov[:, 3] = np.concatenate([np.linspace(s[sl][3], 1.0, k), np.linspace(1.0, e[sl][3], k + 1)])
        out[:, sl] = np.concatenate([mov, np.tile(mov[-1], (N - h, 1))]) if leg == 0 else np.concatenate([np.tile(mov[0], (N - h, 1)), mov])
    return out


def _knee_contact(N):
    h = N // 2
    mid = [[1.0, 1.0]] if N % 2 else []
    return np.array([[1.0, 1.0]] + [[0.0, 1.0]] * (h - 1) + mid + [[1.0, 0.0]] * (h - 1) + [[1.0, 1.0]]).reshape(-1, 2)[:N]


def _end(dof_axis, pose_f, trans_f, N, knee, default_pose, lead_in, Bx):
    """N synthetic frames at one end, from / to clip frame (pose_f [Bx,3], trans_f [3]) -> pose_aa [N,Bx,3], trans [N,3] in float64"""
    D = dof_axis.shape[0]
    axis = dof_axis.astype(np.float64)
    d = (pose_f[1:1 + D].astype(np.float32) * dof_axis).sum(-1, dtype=np.float32).astype(np.float64)     # the clip's joint values, float32 dot
    z0, q0, d0 = default_pose[2], default_pose[3:7] / np.linalg.norm(default_pose[3:7]), default_pose[7:]
    if lead_in:
        z = np.linspace(z0, float(trans_f[2]), N)
        t = np.linspace(0.0, 1.0, N)
        dof = np.linspace(d0, d, N + 1, endpoint=False)[1:]
        if knee:
            dof[:, :12] = _legs(d0[:12], d[:12], N)
    else:
        z = np.linspace(float(trans_f[2]), z0, N)
        t = np.linspace(1.0, 0.0, N)
        dof = np.linspace(d, d0, N + 1)[1:]
        if knee:
            dof[:, :12] = _legs(d[:12], d0[:12], N)
    yaw, pitch, roll = _zyx_from_q(_q_from_rotvec(pose_f[0].astype(np.float64)))
    _, pitch0, roll0 = _zyx_from_q(q0)
    A, B = _q_from_zyx(yaw, pitch0, roll0), _q_from_zyx(yaw, pitch, roll)
    pose = np.zeros((N, Bx, 3))
    for i in range(N):
        pose[i, 0] = _rotvec_from_q(_slerp(A, B, t[i]))
    pose[:, 1:1 + D] = dof_axis[None] * dof.astype(np.float32)[:, :, None]                                # float32 axis x float32 value
    trans = np.stack([np.full(N, float(trans_f[0])), np.full(N, float(trans_f[1])), z], axis=1)
    return pose, trans


def restate(dof_axis, pose_aa, trans, contact, n, m, knee, default_pose, contact_fill=0.5):
    """One clip -> (pose_aa, trans, contact or None) of the extended clip, float32 (every synthetic value rounded once from float64)."""
    pose_aa, trans = np.asarray(pose_aa, np.float32), np.asarray(trans, np.float32)
    default_pose = np.asarray(default_pose, np.float64).copy()
    default_pose[2:] = default_pose[2:].astype(np.float32)                   # the export takes the default pose as float32
    Bx = pose_aa.shape[1]
    parts_p, parts_t, parts_c = [pose_aa], [trans], [None if contact is None else np.asarray(contact, np.float32)]
    if n > 0:
        p, t = _end(dof_axis, pose_aa[0], trans[0], n, knee, default_pose, True, Bx)
        parts_p.insert(0, p.astype(np.float32)); parts_t.insert(0, t.astype(np.float32))
        parts_c.insert(0, _knee_contact(n) if knee else np.full((n, 2), contact_fill))
    if m > 0:
        p, t = _end(dof_axis, pose_aa[-1], trans[-1], m, knee, default_pose, False, Bx)
        parts_p.append(p.astype(np.float32)); parts_t.append(t.astype(np.float32))
        parts_c.append(_knee_contact(m) if knee else np.full((m, 2), contact_fill))
    out_c = None if contact is None else np.concatenate([np.asarray(c, np.float32) for c in parts_c])
    return np.concatenate(parts_p), np.concatenate(parts_t), out_c


# ---- fixture ---------------------------------------------------------------------------------------------------------------------------
def skeleton23():
    return Skeleton.from_json(os.path.join(GOLDEN, "skeleton_g1_23dof_lock_wrist_fitmotionONLY.json"))


_CASES = None


def load_cases():
    """-> {case: dict(source clip arrays (untrimmed), n, m, knee, clip_start, clip_end, default_pose [30], expected pose_aa / trans / contact)}"""
    global _CASES
    if _CASES is None:
        z = np.load(FIXTURE, allow_pickle=False)
        out = {}
        for case in sorted({k.split("::")[1] for k in z.files if k.startswith("case::")}):
            g = lambda k: z[f"case::{case}::{k}"]
            n, m, knee, start, end = (int(v) for v in g("params"))
            src = str(g("source"))
            pose0 = z[f"case::{case}::default_pose"] if f"case::{case}::default_pose" in z.files else SCRIPT_DEFAULT_POSE
            out[case] = dict(src=src, n=n, m=m, knee=bool(knee), clip_start=start, clip_end=end, default_pose=np.asarray(pose0, np.float64),
                             in_pose_aa=z[f"in::{src}::pose_aa"], in_trans=z[f"in::{src}::root_trans_offset"], in_contact=z[f"in::{src}::contact_mask"],
                             pose_aa=g("pose_aa"), trans=g("root_trans_offset"), contact=g("contact_mask"))
        _CASES = out
    return _CASES


def trimmed(c):
    end = c["in_pose_aa"].shape[0] if c["clip_end"] == -1 else c["clip_end"]
    s = slice(c["clip_start"], end)
    return c["in_pose_aa"][s], c["in_trans"][s], c["in_contact"][s]


CASE_NAMES = ["walk_lin_30_30", "walk_knee_30_30", "walk_lin_2_1", "horse_lin_1_2", "horse_knee_6_7", "horse_lin_30_30", "tilted_lin_30_30"]


def test_fixture_holds_the_cases_the_issue_names():
    cases = load_cases()
    assert sorted(cases) == sorted(CASE_NAMES)
    got = {(c["n"], c["m"], c["knee"]) for c in cases.values()}
    assert {(30, 30, False), (1, 2, False), (2, 1, False), (30, 30, True), (6, 7, True)} <= got
    t = cases["tilted_lin_30_30"]
    assert np.abs(t["default_pose"][3:6]).min() > 0.05 and t["in_pose_aa"].shape[0] == 122
    assert cases["horse_lin_1_2"]["pose_aa"].shape[0] == 40 + 3 and os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("case", CASE_NAMES)
def test_restatement_matches_the_reference_script(case):
    c = load_cases()[case]
    pose, trans, contact = trimmed(c)
    got = restate(skeleton23().dof_axis, pose, trans, contact, c["n"], c["m"], c["knee"], c["default_pose"])
    for name, a, b in zip(("pose_aa", "trans", "contact"), got, (c["pose_aa"], c["trans"], c["contact"])):
        assert a.shape == b.shape, name
        err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
        print(f"{case} {name}: max |restatement - script| = {err:.3e}")
        assert err <= TOL, (case, name, err)
    # the first lead-in frame is NOT the default pose, the last lead-out frame IS (joints; with knee_modify the legs' ramps never reach their
    # end point, knees excepted), and the extended bodies' rows are zero
    D, n, m = 23, c["n"], c["m"]
    axis = skeleton23().dof_axis
    d_last = (got[0][-1, 1:1 + D] * axis).sum(-1)
    same = [3, 9] + list(range(12, D)) if c["knee"] else list(range(D))
    np.testing.assert_array_equal(d_last[same], c["default_pose"][7:].astype(np.float32)[same])
    d_first = (got[0][0, 1:1 + D] * axis).sum(-1)
    assert np.abs(d_first - c["default_pose"][7:]).max() > 1e-4
    assert not got[0][:n, 1 + D:].any() and not got[0][got[0].shape[0] - m:, 1 + D:].any()


# ---- config parsing, default pose, refusals --------------------------------------------------------------------------------------------
def _robot(name="v1_g1_23dof_walk.yaml", overrides=None):
    return fixture_config(name, 4, overrides).robot


def test_default_pose_from_default_joint_angles_is_the_scripts_pose():
    rc = _robot(overrides={"robot.motion.interpolation": {"start_frames": 30, "end_frames": 30}})
    ip = Interpolation.from_config(rc.motion.interpolation, 23, robot=rc)
    np.testing.assert_array_equal(ip.default_pose, SCRIPT_DEFAULT_POSE)
    assert (ip.start_frames, ip.end_frames, ip.clip_start, ip.clip_end, ip.knee_modify, ip.contact) == (30, 30, 0, -1, False, 0.5)
    assert ip.active and ip.added == 60
    rc29 = _robot("v2_g1_29dof_teacher.yaml")
    ip29 = Interpolation.from_config({"start_frames": 2, "end_frames": 0}, 29, robot=rc29)
    assert ip29.default_pose.shape == (36,) and ip29.default_pose[2] == 0.8 and tuple(ip29.default_pose[3:7]) == (0.0, 0.0, 0.0, 1.0)
    np.testing.assert_array_equal(ip29.default_pose[7:], [float(rc29.init_state.default_joint_angles[n]) for n in rc29.dof_names])


def test_config_keys_are_parsed():
    rc = _robot()
    pose = list(np.linspace(-0.5, 0.5, 30))
    pose[3:7] = [0.0, 0.0, 0.6, 0.8]
    ip = Interpolation.from_config(dict(start_frames=6, end_frames=7, clip_start=3, clip_end=50, knee_modify=True, default_pose=pose, contact=0.25), 23, robot=rc)
    assert (ip.start_frames, ip.end_frames, ip.clip_start, ip.clip_end, ip.knee_modify, ip.contact) == (6, 7, 3, 50, True, 0.25)
    np.testing.assert_array_equal(ip.default_pose, np.asarray(pose))
    assert Interpolation.from_config(None, 23, robot=rc) is None
    assert not Interpolation.from_config(dict(start_frames=0, end_frames=0), 23, robot=rc).active
    clip = dict(pose_aa=np.zeros((60, 27, 3), np.float32), root_trans_offset=np.zeros((60, 3), np.float32), contact_mask=np.zeros((60, 2)), fps=30)
    cut = ip.trim(clip)
    assert cut["pose_aa"].shape[0] == 47 and cut["root_trans_offset"].shape[0] == 47 and cut["contact_mask"].shape[0] == 47 and cut["fps"] == 30
    with pytest.raises(_lib.PbhcError, match="unknown key"):
        Interpolation.from_config(dict(start_frame=3), 23, robot=rc)
    with pytest.raises(_lib.PbhcError, match="past the end"):
        Interpolation.from_config(dict(clip_start=60), 23, robot=rc).trim(clip)


def test_knee_frame_counts_are_the_ones_the_reference_accepts():
    assert [n for n in (30, 6, 7, 60, 4, 1, 2, 3, 0) if knee_frames_ok(n)] == [30, 6, 7, 2, 3, 0]


@pytest.mark.parametrize("n,m", [(60, 30), (30, 4), (1, 30)])
def test_bad_knee_modify_frame_count_is_refused(n, m):
    with pytest.raises(_lib.PbhcError, match=r"knee_modify cannot fill"):
        Interpolation.from_config(dict(start_frames=n, end_frames=m, knee_modify=True), 23, robot=_robot())


def test_knee_modify_needs_knees_at_dofs_3_and_9():
    rc = _robot()
    names = list(rc.dof_names)
    names[3], names[4] = names[4], names[3]
    with pytest.raises(_lib.PbhcError, match=r"dofs 3 and 9"):
        Interpolation(num_dof=23, default_pose=SCRIPT_DEFAULT_POSE, start_frames=6, end_frames=7, knee_modify=True, dof_names=names)
    with pytest.raises(_lib.PbhcError, match=r"dofs 3 and 9"):
        Interpolation(num_dof=23, default_pose=SCRIPT_DEFAULT_POSE, start_frames=6, end_frames=7, knee_modify=True)          # no names: not checkable
    rc29 = _robot("v2_g1_29dof_teacher.yaml")
    assert Interpolation.from_config(dict(start_frames=6, end_frames=7, knee_modify=True), 29, robot=rc29).knee_modify       # the 29-dof G1's are


def test_default_pose_of_wrong_length_is_refused():
    with pytest.raises(_lib.PbhcError, match=r"default_pose has 29 values, expected 7 \+ 23"):
        Interpolation.from_config(dict(default_pose=[0.0] * 6 + [1.0] + [0.0] * 22), 23, robot=_robot())
    with pytest.raises(_lib.PbhcError, match="non-zero quaternion"):
        Interpolation.from_config(dict(default_pose=[0.0] * 30), 23, robot=_robot())


@pytest.mark.parametrize("start,end", [(10, 10), (10, 5), (0, 0)])
def test_clip_end_not_after_clip_start_is_refused(start, end):
    with pytest.raises(_lib.PbhcError, match=r"clip_end .* <= clip_start"):
        Interpolation.from_config(dict(clip_start=start, clip_end=end), 23, robot=_robot())


def test_negative_frame_counts_are_refused():
    with pytest.raises(_lib.PbhcError, match=">= 0"):
        Interpolation.from_config(dict(start_frames=-1), 23, robot=_robot())


def test_absent_key_leaves_the_env_config_at_its_snapshot(monkeypatch):
    import json

    from pbhc_amd.envs import env_config
    from tools.gen_env_config_snapshot import CASES, FIXTURE as SNAP, build_case, snapshot

    cfgname = "v1_g1_23dof_walk.yaml"
    assert "interpolation" not in fixture_config(cfgname, 4).robot.motion
    monkeypatch.delenv("PBHC_ROW_HELP_SHARE", raising=False)
    monkeypatch.delenv("PBHC_ROLE0_HANDICAP", raising=False)
    for name in ("plain/v1_g1_23dof_walk", "plain/v2_g1_29dof_teacher"):
        monkeypatch.setattr(env_config, "PACKED_MAPS", CASES[name]["packed"])
        assert snapshot(*build_case(CASES[name])) == json.load(open(SNAP))[name]
    # and with the key present: it belongs to the motion library, not to the step's config image
    kw = dict(num_envs=4, seed=3, general=False, has_contact_mask=False)
    _, _, c0, L0 = build_env_config(cfgname, **kw)
    _, _, c1, L1 = build_env_config(cfgname, {"robot.motion.interpolation": {"start_frames": 30, "end_frames": 30}}, **kw)
    assert snapshot(c0, L0) == snapshot(c1, L1)


def test_export_refuses_bad_arguments_without_a_gpu():
    import ctypes as C

    lib, E = _lib.lib(), _lib.K["PBHC_EINVAL"]
    csk = skeleton23().to_c()
    p = _lib.PbhcMotionExtend()
    p.start_frames, p.end_frames, p.default_quat_xyzw[3], p.default_dof = 2, 1, 1.0, C.c_void_p(64)
    one = C.c_void_p(64)                                        # never dereferenced: every call below is refused before a launch
    call = lambda total_in, M, total_out, contact=None, out_contact=None: lib.pbhc_motion_extend_batch(
        C.byref(csk), one, one, contact, total_in, M, one, one, total_out, p, one, one, out_contact, None)
    assert call(10, 2, 15) == E and b"pbhc_motion_extend_batch" in lib.pbhc_last_error()          # 10 + 2 * 3 = 16
    assert call(10, 2, 16, contact=one) == E                                                        # contact in without contact out
    assert call(1, 2, 7) == E                                                                       # fewer frames than clips
    p.knee_modify = 1
    assert call(10, 2, 16) == E and b"knee_modify" in lib.pbhc_last_error()                          # 1 frame cannot hold the knee ramps
    p.knee_modify, p.default_quat_xyzw[3] = 0, 0.0
    assert call(10, 2, 16) == E and b"quaternion" in lib.pbhc_last_error()
