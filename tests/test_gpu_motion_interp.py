"""`robot.motion.interpolation` on the GPU: the one-launch extension kernel (`pbhc_motion_extend_batch`, csrc/pbhc_motion_extend.hip) against
the reference script's recorded output (tests/golden/motion_interp.npz) and against the float64 restatement of
tests/test_motion_interp_cpu.py where the script cannot run; then everything built on it — tables, max_len crops, target heading, an env,
start-time draws — against the same quantities built from the fixture's already-extended clips.

Bounds: the export's arrays 1e-6 absolute (see test_motion_interp_cpu.py), the clip's own frames bit for bit.  Tables: both sides run the
same build kernel on inputs at most 1e-6 apart, with the per-quantity bounds of test_motion_build_matches_reference_fk.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.motion_interp import Interpolation
from pbhc_amd.motion_lib import MotionLib, load_motion_file, rebase_heading
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, build_hip_env, fixture_config
from tests.test_gpu_parity import angvel_tol, close, table_speed_floor
from tests.test_motion_interp_cpu import CASE_NAMES, SCRIPT_DEFAULT_POSE, TOL, load_cases, restate, skeleton23, trimmed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0


def skeleton29():
    return Skeleton.from_json(os.path.join(GOLDEN, "skeleton_g1_29dof_rev_1_0.json"))


def spec_of(c, D=23, names=None):
    rc = fixture_config("v1_g1_23dof_walk.yaml", 4).robot
    return Interpolation(num_dof=D, default_pose=c["default_pose"], start_frames=c["n"], end_frames=c["m"], clip_start=c["clip_start"],
                         clip_end=c["clip_end"], knee_modify=c["knee"], dof_names=list(rc.dof_names) if names is None else names)


def run_export(sk, clips, n, m, knee, default_pose, contact_fill=0.5, with_contact=True):
    """clips: [(pose_aa [F,Bx,3], trans [F,3], contact [F,2])] -> per clip (pose_aa, trans, contact or None) from ONE launch.  The outputs are
    allocated with 3 sentinel frames behind them: nothing may be written there."""
    Bx = sk.num_bodies_ext
    nf = [p.shape[0] for p, _, _ in clips]
    in_start = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
    out_start = np.concatenate([[0], np.cumsum([f + n + m for f in nf])]).astype(np.int32)
    tin, tout = int(in_start[-1]), int(out_start[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(np.float32))).to(DEV)
    d_pose, d_trans = up([p[:, :Bx] for p, _, _ in clips]), up([t for _, t, _ in clips])
    d_contact = up([c for _, _, c in clips]) if with_contact else None
    o_pose = torch.full((tout + 3, Bx, 3), SENTINEL, device=DEV)
    o_trans = torch.full((tout + 3, 3), SENTINEL, device=DEV)
    o_contact = torch.full((tout + 3, 2), SENTINEL, device=DEV) if with_contact else None
    d_dof = torch.from_numpy(np.asarray(default_pose[7:], np.float32)).to(DEV)
    p = _lib.PbhcMotionExtend()
    p.start_frames, p.end_frames, p.knee_modify, p.default_height, p.contact_fill = n, m, int(knee), float(default_pose[2]), contact_fill
    for k in range(4):
        p.default_quat_xyzw[k] = float(default_pose[3 + k])
    p.default_dof = C.c_void_p(d_dof.data_ptr())
    csk = sk.to_c()
    d_in, d_out = torch.from_numpy(in_start).to(DEV), torch.from_numpy(out_start).to(DEV)
    _lib.check(_lib.lib().pbhc_motion_extend_batch(C.byref(csk), _lib.ptr(d_pose), _lib.ptr(d_trans), _lib.ptr(d_contact), tin, len(clips),
                                                   _lib.ptr(d_in), _lib.ptr(d_out), tout, p,
                                                   _lib.ptr(o_pose), _lib.ptr(o_trans), _lib.ptr(o_contact), _lib.current_stream()), "pbhc_motion_extend_batch")
    torch.cuda.synchronize()
    for o in (o_pose, o_trans) + ((o_contact,) if with_contact else ()):
        assert bool((o[tout:] == SENTINEL).all()), "the launch wrote behind its output"
        assert not bool((o[:tout] == SENTINEL).any()), "the launch left output frames unwritten"
    o_pose, o_trans = o_pose.cpu().numpy(), o_trans.cpu().numpy()
    o_contact = o_contact.cpu().numpy() if with_contact else None
    return [(o_pose[a:b], o_trans[a:b], None if o_contact is None else o_contact[a:b]) for a, b in zip(out_start[:-1], out_start[1:])]


def assert_extension(got, want, src, n, what):
    """got / want: (pose_aa, trans, contact or None) of one extended clip; src: the clip itself, whose frames must come through bit for bit"""
    F = src[0].shape[0]
    for name, a, b, s in zip(("pose_aa", "trans", "contact"), got, want, src):
        if b is None:
            assert a is None
            continue
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
        print(f"{what} {name}: max |kernel - expected| = {err:.3e}")
        assert err <= TOL, (what, name, err)
        assert np.array_equal(a[n:n + F].view(np.uint32), np.asarray(s, np.float32)[:, :a.shape[1]].view(np.uint32)), (what, name, "clip frames not bit for bit")


@pytest.mark.parametrize("case", CASE_NAMES)
def test_kernel_matches_the_reference_script(case):
    c = load_cases()[case]
    src = trimmed(c)
    got = run_export(skeleton23(), [src], c["n"], c["m"], c["knee"], c["default_pose"])[0]
    assert_extension(got, (c["pose_aa"], c["trans"], c["contact"]), src, c["n"], case)


def _clips(sk, robot):
    """3 clips of different lengths, one of a single frame, with a contact mask"""
    if robot == 23:
        c = load_cases()["walk_lin_30_30"]
        pose, trans = c["in_pose_aa"], c["in_trans"]
    else:
        clip = load_motion_file(os.path.join(GOLDEN, "clips", "g1_rig_Skeleton_Sequence_converted_processed_g1_29dof_rev_1_0.npz"))[0][1]
        pose, trans = np.asarray(clip["pose_aa"], np.float32), np.asarray(clip["root_trans_offset"], np.float32)
    assert pose.shape[1] == sk.num_bodies_ext
    out = []
    for a, b in ((3, 8), (50, 51), (70, 101)):
        F = b - a
        contact = np.stack([np.arange(F) % 2, (np.arange(F) // 2) % 2], axis=1).astype(np.float32)
        out.append((pose[a:b], trans[a:b], contact))
    return out


def _pose_for(D):
    pose = np.zeros(7 + D)
    pose[2], pose[3:7] = 0.77, [0.05, -0.08, 0.3, 0.95]
    pose[7:] = 0.3 * np.cos(0.7 * np.arange(D) + 0.2)
    return pose


@pytest.mark.parametrize("robot,n,m,knee,with_contact", [
    (23, 0, 1, False, True), (23, 2, 0, False, True), (23, 1, 1, False, False), (23, 0, 2, True, True), (23, 2, 3, True, True), (23, 6, 0, True, False),
    (29, 1, 2, False, True), (29, 2, 0, False, False), (29, 6, 7, True, True)])
def test_batch_edges_against_the_restatement(robot, n, m, knee, with_contact):
    """Bx = 27 and 33, three clips of 5 / 1 / 31 frames in one launch (frames per workgroup: 4, so clip boundaries fall inside workgroups),
    n, m in {0, 1, 2}, knee_modify with h in {1, 3}, a library without contact masks (NULL in, NULL out)."""
    sk = skeleton23() if robot == 23 else skeleton29()
    clips = _clips(sk, robot)
    pose0 = _pose_for(sk.num_dof)
    got = run_export(sk, clips, n, m, knee, pose0, contact_fill=0.25, with_contact=with_contact)
    for i, (src, g) in enumerate(zip(clips, got)):
        want = restate(sk.dof_axis, src[0], src[1], src[2] if with_contact else None, n, m, knee, pose0, contact_fill=0.25)
        assert g[0].shape[0] == src[0].shape[0] + n + m
        assert_extension(g, want, src if with_contact else (src[0], src[1], None), n, f"{robot}dof clip {i} ({n},{m}) knee={knee}")


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def _raw_clip(c, contact=True):
    clip = dict(pose_aa=c["in_pose_aa"], root_trans_offset=c["in_trans"], fps=30)
    if contact:
        clip["contact_mask"] = c["in_contact"]
    return clip


def _ext_clip(c, contact=True):
    clip = dict(pose_aa=c["pose_aa"], root_trans_offset=c["trans"], fps=30)
    if contact:
        clip["contact_mask"] = c["contact"]
    return clip


def assert_rows_close(sk, rows, ref, what, fps=30):
    """packed table rows built from inputs <= 1e-6 apart: the bounds of test_motion_build_matches_reference_fk, quantity by quantity"""
    D, Bx = sk.num_dof, sk.num_bodies_ext
    rows, ref = rows.cpu(), ref.cpu()
    assert rows.shape == ref.shape, (what, rows.shape, ref.shape)
    F, o = rows.shape[0], 2 * D + 2
    close(rows[:, :D], ref[:, :D], 2e-6, f"{what} dof_pos")
    close(rows[:, D:2 * D], ref[:, D:2 * D], 2e-5, f"{what} dof_vel")
    close(rows[:, 2 * D:o], ref[:, 2 * D:o], 1e-6, f"{what} contact")
    close(rows[:, o:o + 3 * Bx], ref[:, o:o + 3 * Bx], 3e-6, f"{what} gts_t")
    close(rows[:, o + 3 * Bx:o + 7 * Bx], ref[:, o + 3 * Bx:o + 7 * Bx], 3e-6, f"{what} grs_t")
    close(rows[:, o + 7 * Bx:o + 10 * Bx], ref[:, o + 7 * Bx:o + 10 * Bx], 5e-5, f"{what} gvs_t")
    gav, rav = rows[:, o + 10 * Bx:].view(F, Bx, 3), ref[:, o + 10 * Bx:].view(F, Bx, 3)
    close(gav, rav, angvel_tol(rav, 1.0 / fps, norm=table_speed_floor(rav)), f"{what} gavs_t")


def assert_same_meta(a, b):
    assert a.num_frames.tolist() == b.num_frames.tolist() and torch.equal(a._motion_lengths, b._motion_lengths)
    assert torch.equal(a.length_starts, b.length_starts) and torch.equal(a._motion_dt, b._motion_dt)
    assert (a.table.single_num_frames, a.table.single_dt, a.table.single_len, a.table.num_motions, a.table.row) == (
        b.table.single_num_frames, b.table.single_dt, b.table.single_len, b.table.num_motions, b.table.row)


@pytest.mark.parametrize("case", ["walk_lin_30_30", "horse_knee_6_7", "tilted_lin_30_30"])
def test_tables_equal_those_of_the_fixtures_extended_clip(case):
    c = load_cases()[case]
    sk = skeleton23()
    a = MotionLib(sk, [_raw_clip(c)], 4, DEV, interpolation=spec_of(c))           # clip_start / clip_end: the horse case is cut on the host
    b = MotionLib(sk, [_ext_clip(c)], 4, DEV)
    assert_same_meta(a, b)
    assert_rows_close(sk, a.frames, b.frames, case)
    got = a.extended_clips()[0]
    assert np.abs(got["pose_aa"] - c["pose_aa"]).max() <= TOL and np.abs(got["contact_mask"] - c["contact"]).max() <= TOL and got["fps"] == 30


def test_two_clip_library_and_a_library_without_contact_masks():
    cw, ch = load_cases()["walk_lin_30_30"], load_cases()["horse_lin_30_30"]
    sk = skeleton23()
    horse_cut = {k: (v[20:60] if isinstance(v, np.ndarray) else v) for k, v in _raw_clip(ch, contact=False).items()}
    a = MotionLib(sk, [_raw_clip(cw, contact=False), horse_cut], 4, DEV, interpolation=spec_of(cw))
    b = MotionLib(sk, [_ext_clip(cw, contact=False), _ext_clip(ch, contact=False)], 4, DEV)
    assert not a.has_contact_mask and a.num_frames.tolist() == [182, 100]
    assert_same_meta(a, b)
    assert_rows_close(sk, a.frames, b.frames, "walk + horse, no contact masks")


def test_max_len_crops_are_drawn_from_the_extended_clip():
    c = load_cases()["walk_lin_30_30"]
    sk = skeleton23()
    N, K = 5, 48
    starts = torch.tensor([0, 10, 29, 100, 182 - K])                              # inside the lead-in, across both seams, the last possible crop
    a = MotionLib(sk, [_raw_clip(c)], N, DEV, max_len=K, interpolation=spec_of(c))
    b = MotionLib(sk, [_ext_clip(c)], N, DEV, max_len=K)
    for ml in (a, b):
        ml.load_motions(random_sample=False, max_len=K, crop_starts=starts)
    assert a.max_len == K and a.num_frames.tolist() == b.num_frames.tolist() == [K] * N and torch.equal(a._motion_lengths, b._motion_lengths)
    assert_rows_close(sk, a.frames, b.frames, "crops")
    # a clip shorter than max_len that the extension makes long enough is cropped too
    short = dict(pose_aa=c["in_pose_aa"][:20], root_trans_offset=c["in_trans"][:20], fps=30)
    s = MotionLib(sk, [short], 2, DEV, max_len=K, interpolation=spec_of(c))
    s.load_motions(random_sample=False, max_len=K, crop_starts=torch.tensor([0, 32]))
    assert s.max_len == K and s.num_frames.tolist() == [K, K]


def test_target_heading_commutes_with_the_extension():
    """load_motions(target_heading) rebases the raw clips and extends again, in place: the tables must be those of "extend, then rebase" —
    the fixture's extended clip through rebase_heading — within the bounds of the existing target-heading test."""
    c = load_cases()["tilted_lin_30_30"]
    sk = skeleton23()
    heading = np.array([0.0, 0.0, np.sin(0.55), np.cos(0.55)])
    a = MotionLib(sk, [_raw_clip(c)], 4, DEV, interpolation=spec_of(c))
    ptr = a.frames.data_ptr()
    a.load_motions(random_sample=False, target_heading=heading)
    assert a.frames.data_ptr() == ptr and a.table.frames == ptr and a.num_frames.tolist() == [182]
    b = MotionLib(sk, [rebase_heading(_ext_clip(c), heading)], 4, DEV)
    rows, ref = a.frames.cpu(), b.frames.cpu()
    D, Bx = sk.num_dof, sk.num_bodies_ext
    o = 2 * D + 2
    close(rows[:, o:o + 3 * Bx], ref[:, o:o + 3 * Bx], 5e-6, "target heading gts_t")
    close(rows[:, o + 3 * Bx:o + 7 * Bx].abs(), ref[:, o + 3 * Bx:o + 7 * Bx].abs(), 5e-6, "target heading grs_t")
    close(rows[:, :D], ref[:, :D], 2e-6, "target heading dof_pos")
    close(rows[:, o + 7 * Bx:o + 10 * Bx], ref[:, o + 7 * Bx:o + 10 * Bx], 1e-4, "target heading gvs_t")
    close(rows[:, 2 * D:o], ref[:, 2 * D:o], 1e-6, "target heading contact")


def test_absent_key_and_zero_frames_leave_the_tables_byte_identical():
    c = load_cases()["walk_lin_30_30"]
    sk = skeleton23()
    plain = MotionLib(sk, [_raw_clip(c)], 4, DEV)
    none = MotionLib(sk, [_raw_clip(c)], 4, DEV, interpolation=None)
    zero = MotionLib(sk, [_raw_clip(c)], 4, DEV, interpolation=Interpolation(num_dof=23, default_pose=SCRIPT_DEFAULT_POSE, start_frames=0, end_frames=0))
    for ml in (none, zero):
        assert ml.interpolation is None and torch.equal(ml.frames.view(torch.int32), plain.frames.view(torch.int32))
        assert ml.num_frames.tolist() == [122]
    mcfg = fixture_config("v1_g1_23dof_walk.yaml", 4).robot.motion
    assert torch.equal(MotionLib.from_config(mcfg, sk, 4, DEV).frames.view(torch.int32), MotionLib(sk, [_raw_clip(c, contact=False)], 4, DEV).frames.view(torch.int32))


def test_start_time_draws_stay_below_the_extended_length():
    c = load_cases()["walk_lin_30_30"]
    N = 4096
    ml = MotionLib(skeleton23(), [_raw_clip(c)], N, DEV, interpolation=spec_of(c))
    ml.load_motions(random_sample=False)
    length = (122 + 60 - 1) / 30.0
    assert abs(float(ml.get_motion_length()[0]) - length) < 1e-6
    ml.init_start_sampling(16)
    start = torch.full((N,), -1.0, device=DEV)
    counter = torch.zeros(1, dtype=torch.float64, device=DEV)
    ml.draw_start_times_device(start, seed=11, counter_ptr=counter.data_ptr(), salt=3)
    torch.cuda.synchronize()
    assert float(start.min()) >= 0.0 and float(start.max()) < length
    assert float(start.max()) > 121 / 30.0 + 1.0                                   # and they reach into the lead-out: the law is over the extended clip
    t = ml.sample_time(torch.arange(N, device=DEV))
    assert float(t.max()) < length and float(t.max()) > 121 / 30.0 + 1.0


def test_env_runs_on_the_extended_clip_and_starts_near_the_default_pose():
    n = 30
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 16, overrides={"robot.motion.interpolation": {"start_frames": n, "end_frames": 30}})
    ml = env._motion_lib
    assert ml.interpolation is not None and ml.num_frames.tolist() == [182]
    assert abs(float(ml.get_motion_length()[0]) - (122 + 60 - 1) / 30.0) < 1e-6
    env.set_is_evaluating()                                                        # resets start at motion time 0
    env.reset_all()
    assert torch.allclose(env.motion_len, torch.full_like(env.motion_len, (122 + 60 - 1) / 30.0), atol=1e-6)
    for _ in range(3):
        obs, rew, reset, _ = env.step({"actions": torch.zeros(16, env.num_dof, device=DEV)})
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in obs.values()) and torch.isfinite(rew).all()
    # phase 0 of the reference: the default joints blended 1 / (n + 1) towards the clip's first frame
    clip = load_motion_file(os.path.join(GOLDEN, "clips", "g1_walk_45cms_23dof.npz"))[0][1]
    d = (np.asarray(clip["pose_aa"], np.float32)[0, 1:24] * env.skeleton.dof_axis).sum(-1).astype(np.float64)
    d0 = SCRIPT_DEFAULT_POSE[7:]
    ids = torch.zeros(1, dtype=torch.long, device=DEV)
    ref0 = ml.get_motion_state(ids, torch.zeros(1, device=DEV))
    close(ref0["dof_pos"][0], d0 + (d - d0) / (n + 1), 2e-6, "reference joints at phase 0")
    close(ref0["root_pos"][0, 2], 0.8, 2e-6, "reference root height at phase 0")
    # and a reset at start time 0 puts the robot on the reference at (0 + 1) dt, 0.6 of the way from frame 0 to frame 1
    env.motion_start_times.fill_(-1.0)
    env._reset_all_state()
    assert float(env.motion_start_times.abs().max()) == 0.0
    blend = (1.0 + env.dt * 30.0) / (n + 1)
    close(env.simulator.dof_pos, torch.from_numpy(d0 + (d - d0) * blend).float().expand(16, -1), 1e-5, "robot joints after a reset at phase 0")


def test_cli_writes_the_clips_the_trainer_sees(tmp_path):
    from tools import interpolate_motion

    out = str(tmp_path / "walk_extended.npz")
    assert interpolate_motion.main(["--config", os.path.join(GOLDEN, "configs", "v1_g1_23dof_walk.yaml"), "--out", out, "--start-frames", "30",
                                    "--end-frames", "30"]) == 0
    c = load_cases()["walk_lin_30_30"]
    got = load_motion_file(out)[0][1]
    assert got["fps"] == 30 and "contact_mask" not in got                          # the shipped walk clip has no contact mask: none is invented
    assert np.abs(got["pose_aa"] - c["pose_aa"]).max() <= TOL and np.abs(got["root_trans_offset"] - c["trans"]).max() <= TOL
