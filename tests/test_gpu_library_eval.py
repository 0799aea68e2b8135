"""Library evaluation: k_clip_track against float64 restatements, the error definitions, env.library_sweep end to end against the
test's own loop over a second env, and both agents' evaluate_library().

The track table is integer-only: its frames column, the retire array and untouched rows are compared exactly.  The error columns hold
sums of llrintf(e * 2^20); the bound of one frame is DERIVED: 2^-21 for the rounding to the grid plus (B + 8) * 2^-24 * e for the float32
evaluation of at most B norms and a mean — in grid units of 2^-20: 0.5 + (B + 8) * e / 16 — and a row's bound is the sum over its frames.
The expected errors are computed in float64 from the SAME float32 inputs the kernel forms them from: body positions by pbhc_sim_fk,
reference by pbhc_motion_state (k_clip_track runs the same two device functions, built with the same flags)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd import motion_lib as ML
from pbhc_amd.skeleton import Skeleton
from tests.helpers import GOLDEN, clip_from_env_golden, skel_from_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = 1048576.0                       # 2^20
ROBOTS = {"g1_23dof": "env_v1_walk.npz", "g1_29dof": "env_v2_teacher29.npz"}
KEYS = ("episodes", "failures", "success", "end_time_ratio", "episode_length", "frames", "E_gmpbpe", "E_mpbpe", "E_mpjpe",
        "success_rate", "E_gmpbpe_mean", "E_mpbpe_mean", "E_mpjpe_mean", "unfinished", "waves", "steps")


def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def frame_bound(B, e):
    """the derived bound of the module docstring for frames of error `e` (array), in grid units"""
    return 0.5 + (B + 8) * np.asarray(e, np.float64) / 16.0


# ---- the two reference device functions and the kernel under test ------------------------------------------------------------------
def device_fk(csk, root, dof_state):
    """pbhc_sim_fk on root [N,13] and the interleaved dof_state [N,D,2] -> body positions [N,B,3] float32"""
    N, B = root.shape[0], csk.num_bodies
    out = torch.empty(N, B, 13, device=DEV)
    _lib.check(_lib.lib().pbhc_sim_fk(C.byref(csk), root.data_ptr(), dof_state.data_ptr(), dof_state.data_ptr() + 4, 2, N, out.data_ptr(),
                                      _lib.current_stream()), "pbhc_sim_fk")
    return out[:, :, 0:3]


def device_reference(csk, table, ids, times, origins):
    """pbhc_motion_state -> (dof_pos [N,D], body positions [N,B,3]) float32"""
    N, D, Bx, B = ids.shape[0], csk.num_dof, csk.num_bodies_ext, csk.num_bodies
    out = torch.empty(N, table.row, device=DEV)
    _lib.check(_lib.lib().pbhc_motion_state(C.byref(table), Bx, D, ids.data_ptr(), times.data_ptr(), origins.data_ptr(), N, out.data_ptr(),
                                            _lib.current_stream()), "pbhc_motion_state")
    return out[:, :D], out[:, 2 * D + 2:2 * D + 2 + 3 * Bx].view(N, Bx, 3)[:, :B]


def errors64(p, r, q, qref):
    """(e_g, e_l, e_j) [N] float64 of eval_accuracy's per-frame definitions from float32 device tensors"""
    p, r, q, qref = (x.double().cpu().numpy() for x in (p, r, q, qref))
    e_g = np.linalg.norm(p - r, axis=-1).mean(axis=-1)
    e_l = np.linalg.norm((p - p[:, :1]) - (r - r[:, :1]), axis=-1).mean(axis=-1)
    return e_g, e_l, np.linalg.norm(q - qref, axis=-1)


def clip_track(csk, table, root, dof_state, times, origins, ids, reset, slot, retire, M, window):
    _lib.check(_lib.lib().pbhc_clip_track(C.byref(csk), C.byref(table), root.data_ptr(), dof_state.data_ptr(), times.data_ptr(), origins.data_ptr(),
                                          ids.data_ptr(), reset.data_ptr(), slot.data_ptr(), None if retire is None else retire.data_ptr(),
                                          root.shape[0], M, window.data_ptr(), _lib.current_stream()), "pbhc_clip_track")
    torch.cuda.synchronize()


_LIBS, _INPUTS = {}, {}


def library(robot):
    """(skeleton, C skeleton, MotionLib) of a golden clip: one table entry for g1_23dof, three (a synthetic library of it) for g1_29dof"""
    if robot not in _LIBS:
        import bench

        s = skel_from_golden(robot)
        sk = Skeleton(s["body_names"], s["body_names_ext"], s["parents"], s["offsets"], s["local_rot_wxyz"], s["dof_axis"])
        clip = clip_from_env_golden(dict(np.load(os.path.join(GOLDEN, ROBOTS[robot]))))
        clips = [clip] if robot == "g1_23dof" else bench.synth_library({k: (v[:60] if k != "fps" else v) for k, v in clip.items()}, 3, seed=3)
        _LIBS[robot] = (sk, sk.to_c(), ML.MotionLib(sk, clips, 1, DEV))
    return _LIBS[robot]


def inputs(robot, N):
    """random in-range states of N envs and their float64 errors (computed once per robot and N, never modified)"""
    if (robot, N) not in _INPUTS:
        sk, csk, ml = library(robot)
        rng = np.random.default_rng(1000 * N + csk.num_dof)
        D, E = csk.num_dof, ml.table.num_motions
        ids = tg(rng.integers(0, E, N).astype(np.int64))
        times = (tg(rng.uniform(-0.05, 1.1, N).astype(np.float32)) * ml._motion_lengths[ids]).contiguous()     # incl. t < 0 and t > len
        origins = tg((2.0 * rng.standard_normal((N, 3))).astype(np.float32))
        qref, r = device_reference(csk, ml.table, ids, times, origins)
        root = torch.zeros(N, 13, device=DEV)
        root[:, 0:3] = r[:, 0] + tg((0.2 * rng.standard_normal((N, 3))).astype(np.float32))
        quat = rng.standard_normal((N, 4))
        root[:, 3:7] = tg((quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32))
        root[:, 7:13] = tg(rng.standard_normal((N, 6)).astype(np.float32))
        q = (qref + tg((0.3 * rng.standard_normal((N, D))).astype(np.float32))).clamp(-2.0, 2.0)
        dof_state = torch.stack([q, tg(rng.standard_normal((N, D)).astype(np.float32))], dim=-1).contiguous()
        e = errors64(device_fk(csk, root, dof_state), r, q, qref)
        _INPUTS[(robot, N)] = dict(ids=ids, times=times, origins=origins, root=root, dof_state=dof_state, e=e)
    return _INPUTS[(robot, N)]


def expected_call(table, bounds, slot, reset, e, M, B, alias):
    """one launch restated: adds onto `table` [M,4] float64 (frames, sums of e * 2^20) and `bounds` [M,3]; -> slot after the launch"""
    slot = slot.copy()
    for i in range(len(slot)):
        c = int(slot[i])
        if not 0 <= c < M:
            continue
        if reset[i] != 0:
            if alias:
                slot[i] = -1
            continue
        table[c, 0] += 1
        for k in range(3):
            table[c, 1 + k] += e[k][i] * GRID
            bounds[c, k] += frame_bound(B, e[k][i])
    return slot


def check_table(window, table, bounds, what):
    got = window.cpu().numpy()
    assert np.array_equal(got[:, 0], table[:, 0].astype(np.int64)), what + ": frames"
    assert not got[table[:, 0] == 0].any(), what + ": rows of untouched clips"
    diff = np.abs(got[:, 1:].astype(np.float64) - table[:, 1:])
    print(f"{what}: worst error / bound {float((diff / np.maximum(bounds, 0.5)).max()):.3f}")
    assert (diff <= bounds).all(), f"{what}: {diff.max()} grid units, bounds {bounds[diff > bounds]}"


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 70])
@pytest.mark.parametrize("N", [1, 9, 67, 259])
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_kernel_equals_float64_and_accumulates(robot, N, M):
    """N: a partly filled last workgroup (4 envs each) and odd counts; reset masks all-zero, all-one and random; slot_clip with -1, M and
    2^40; retire NULL and aliased to slot_clip; two launches into one table (the sum, not an overwrite)."""
    sk, csk, ml = library(robot)
    x = inputs(robot, N)
    rng = np.random.default_rng(7 * N + M)
    slot0 = rng.integers(0, M, N).astype(np.int64)
    strays = {1: (), 9: (2, 5, 7)}.get(N, (5, 9, 11))
    for i, v in zip(strays, (-1, M, 2**40)):
        slot0[i] = v
    reset_b = (rng.random(N) < 0.5).astype(np.int64)
    for mode in ("zeros", "ones", "random"):
        reset_a = {"zeros": np.zeros(N, np.int64), "ones": np.ones(N, np.int64), "random": (rng.random(N) < 0.5).astype(np.int64)}[mode]
        for alias in (False, True):
            what = f"{robot} N {N} M {M} {mode} {'aliased' if alias else 'NULL'}"
            window = torch.zeros(M, 4, dtype=torch.int64, device=DEV)
            slot = tg(slot0)
            table, bounds = np.zeros((M, 4)), np.zeros((M, 3))
            want = slot0
            for reset in (reset_a, reset_b):
                clip_track(csk, ml.table, x["root"], x["dof_state"], x["times"], x["origins"], x["ids"], tg(reset), slot, slot if alias else None, M, window)
                want = expected_call(table, bounds, want, reset, x["e"], M, csk.num_bodies, alias)
                # -1 exactly on the active envs that reset; everything else — strays included — untouched
                assert np.array_equal(slot.cpu().numpy(), want), what + ": retire"
            if not alias:
                assert np.array_equal(want, slot0)
            check_table(window, table, bounds, what)
    if N > 1:
        assert table[:, 0].sum() > 0


def test_a_frame_with_a_nan_joint_angle_is_not_counted():
    robot, N, M = "g1_23dof", 9, 3
    sk, csk, ml = library(robot)
    x = inputs(robot, N)
    dof_state = x["dof_state"].clone()
    dof_state[4, 3, 0] = float("nan")
    slot = np.arange(N, dtype=np.int64) % M
    window = torch.zeros(M, 4, dtype=torch.int64, device=DEV)
    clip_track(csk, ml.table, x["root"], dof_state, x["times"], x["origins"], x["ids"], tg(np.zeros(N, np.int64)), tg(slot), None, M, window)
    table, bounds = np.zeros((M, 4)), np.zeros((M, 3))
    reset = np.zeros(N, np.int64)
    reset[4] = 1                                           # restated as "env 4 adds nothing"
    expected_call(table, bounds, slot, reset, x["e"], M, csk.num_bodies, False)
    assert table[:, 0].sum() == N - 1
    check_table(window, table, bounds, "nan joint")


# ---- 2. the definitions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_definitions_on_a_translated_root_and_an_offset_joint(robot):
    """State = the reference itself (root pose and joint angles of the table at frame times), then the root translated by a known vector /
    one joint offset by delta.  Tolerance: twice the largest distance between pbhc_sim_fk's positions of the untranslated state and the
    table's positions (the reference path, not the code under test).  Measured on an MI355X: 2.083e-07 m (g1_23dof), 2.731e-07 m
    (g1_29dof), i.e. tolerances of 4.2e-07 / 5.5e-07.  That is below the table's 2^-21 rounding, so the known vector's
    length and delta are chosen ON the 2^-20 grid: the rounding then adds nothing to what is compared."""
    sk, csk, ml = library(robot)
    N, D, B = 9, csk.num_dof, csk.num_bodies
    ids = tg(np.arange(N, dtype=np.int64) % ml.table.num_motions)
    times = (torch.arange(N, device=DEV) * 3).float() * ml._motion_dt[ids]                   # frame times
    origins = tg(np.zeros((N, 3), np.float32))
    out = torch.empty(N, ml.table.row, device=DEV)
    Bx = csk.num_bodies_ext
    _lib.check(_lib.lib().pbhc_motion_state(C.byref(ml.table), Bx, D, ids.data_ptr(), times.data_ptr(), origins.data_ptr(), N, out.data_ptr(),
                                            _lib.current_stream()), "pbhc_motion_state")
    o_pos = 2 * D + 2
    qref, r = out[:, :D], out[:, o_pos:o_pos + 3 * Bx].view(N, Bx, 3)[:, :B]
    root = torch.zeros(N, 13, device=DEV)
    root[:, 0:3], root[:, 3:7] = r[:, 0], out[:, o_pos + 3 * Bx:o_pos + 3 * Bx + 4]
    dof_state = torch.stack([qref, torch.zeros_like(qref)], dim=-1).contiguous()
    measured = float((device_fk(csk, root, dof_state).double() - r.double()).norm(dim=-1).max())
    tol = 2.0 * measured
    print(f"{robot}: |pbhc_sim_fk - table| max {measured:.3e} m, tolerance {tol:.3e}")
    assert measured < 1e-3
    zeros, slot = tg(np.zeros(N, np.int64)), tg(np.arange(N, dtype=np.int64))

    def run(root, dof_state):
        window = torch.zeros(N, 4, dtype=torch.int64, device=DEV)
        clip_track(csk, ml.table, root, dof_state, times, origins, ids, zeros, slot, None, N, window)
        w = window.cpu().numpy()
        assert (w[:, 0] == 1).all()
        return w[:, 1:].astype(np.float64) / GRID

    v = torch.tensor([0.36, -0.48, 0.8], device=DEV)                # |v| = 1 m and delta below: multiples of the table's 2^-20 grid
    moved = root.clone()
    moved[:, 0:3] += v
    e = run(moved, dof_state)
    assert np.abs(e[:, 0] - float(v.double().norm())).max() <= tol, e[:, 0]
    assert e[:, 1].max() <= tol and e[:, 2].max() <= tol, e
    delta = 0.25
    bent = dof_state.clone()
    bent[:, 5, 0] += delta
    e = run(root, bent)
    assert np.abs(e[:, 2] - delta).max() <= tol, e[:, 2]


# ---- 3. the sweep end to end -------------------------------------------------------------------------------------------------------
SWEEP_N, SWEEP_M, SWEEP_FAIL, SWEEP_SYNC = 8, 19, (2, 9, 17), 8


def _sweep_library():
    import bench

    g = dict(np.load(os.path.join(GOLDEN, "env_v2_teacher29.npz")))
    base = {k: (v[:26] if k != "fps" else v) for k, v in clip_from_env_golden(g).items()}       # 25 frame intervals at 30 fps < 42 control steps
    return bench.synth_library(base, SWEEP_M, seed=3)


def _sweep_env(clips, seed=7):
    from tests.helpers import build_hip_env

    torch.manual_seed(seed)
    np.random.seed(seed)
    orig = ML.load_motion_file
    ML.load_motion_file = lambda path: [(f"c{i}", c) for i, c in enumerate(clips)]
    try:
        return build_hip_env("v2_g1_29dof_teacher.yaml", SWEEP_N, general=True, overrides={"domain_rand.push_robots": False, "env.config.clip_statistics": True})[1]
    finally:
        ML.load_motion_file = orig


def _installer(env, oml, skel, T=56):
    """before_wave: a synth_replay window of the wave's clips from motion time 0; the root of the SWEEP_FAIL clips 1 m up from frame 5 on"""
    from tests.helpers import synth_replay

    def install(w, clip_ids):
        N = env.num_envs
        ids = env._motion_lib.slot_clip.cpu()
        assert torch.equal(torch.where(clip_ids.cpu() >= 0, clip_ids.cpu(), ids), ids)           # the wave's clips, idle envs wrapped around
        zero = torch.zeros(N)
        root, qp, qv, cf = synth_replay(oml, skel, N, T, zero, zero.long(), env.dt, env.env_origins.cpu(), 40 + w, env.feet_indices.cpu(), ids=ids)
        for i, c in enumerate(clip_ids.tolist()):
            if c in SWEEP_FAIL:
                root[5:, i, 2] += 1.0
        env.simulator.set_replay(root.to(DEV), qp.to(DEV), qv.to(DEV), cf.to(DEV))
    return install


def _warm(env):
    """reset_all, then one collector launch over every env: the training window is not empty when the sweep starts"""
    env.reset_all()
    env.reset_buf.fill_(1)
    env._launch_clip_stats(_lib.current_stream())


def _act(obs):
    return 0.1 * torch.tanh(obs["actor_obs"][:, :29]).contiguous()


def test_sweep_scores_every_clip_once_and_equals_the_tests_own_loop():
    from oracle.motion_lib import MotionLib as OML

    clips = _sweep_library()
    skel = skel_from_golden("g1_29dof")
    oml = OML(skel, clips)
    N, M = SWEEP_N, SWEEP_M
    # -- the sweep
    env = _sweep_env(clips)
    _warm(env)
    slot_before, window_before, interval = env._motion_lib.slot_clip.clone(), env._clip_window.clone(), env.resample_time_interval
    assert int(window_before[:, 0].sum()) > 0 and slot_before.tolist() == [i % M for i in range(N)]
    out = env.library_sweep(_act, sync_every=SWEEP_SYNC, before_wave=_installer(env, oml, skel))
    torch.cuda.synchronize()
    assert set(KEYS) <= set(out) and out["waves"] == 3 and out["unfinished"] == []
    assert out["episodes"].tolist() == [1] * M
    assert [c for c in range(M) if not bool(out["success"][c])] == list(SWEEP_FAIL)
    assert abs(out["success_rate"] - (M - len(SWEEP_FAIL)) / M) < 1e-12
    assert torch.equal(env._motion_lib.slot_clip, slot_before) and torch.equal(env._clip_window, window_before)
    assert env.resample_time_interval == interval and env._finalize_stream is None and env.is_evaluating
    assert int(env.episode_length_buf.abs().sum()) == 0                                      # every env is reset afterwards
    # -- the same waves driven from here on a second env of the same seed
    ref = _sweep_env(clips)
    _warm(ref)
    ref.set_is_evaluating()
    csk, ml, B = ref.simulator._csk, ref._motion_lib, ref.num_bodies
    install = _installer(ref, oml, skel)
    epi, frames = np.zeros((M, 4), np.int64), np.zeros(M, np.int64)
    esum, bound = np.zeros((M, 3)), np.zeros((M, 3))
    steps = 0
    for w in range(3):
        ml.load_motions(random_sample=False, start_idx=w * N, max_len=ref.max_len)
        clip_ids = np.where(np.arange(N) + w * N < M, np.arange(N) + w * N, -1)
        install(w, torch.from_numpy(clip_ids))
        ref._reset_all_state()
        cap = int(np.ceil(float(ref.motion_len[:int((clip_ids >= 0).sum())].max()) / ref.dt)) + 8
        first = clip_ids >= 0                                                                # still in its first episode
        obs = None
        for k in range(cap):
            obs = ref.step({"actions": torch.zeros(N, ref.num_dof, device=DEV) if k == 0 else _act(obs)})[0]
            steps += 1
            torch.cuda.synchronize()
            reset = ref.reset_buf.cpu().numpy()
            qref, r = device_reference(csk, ml.table, ref._slot_clip, ref._ref_time, ref.env_origins)
            e = errors64(device_fk(csk, ref.simulator.robot_root_states, ref.simulator.dof_state), r, ref.simulator.dof_pos, qref)
            tout, ratio, length = ref.time_out_buf.cpu().numpy(), ref.end_time_ratio_buf.cpu().numpy(), ref.last_episode_length_buf.cpu().numpy()
            for i in np.nonzero(first)[0]:
                c = clip_ids[i]
                if reset[i]:
                    epi[c] += (1, int(tout[i] == 0), int(np.rint(np.float32(ratio[i]) * np.float32(16777216.0))), int(length[i]))
                    first[i] = False
                else:
                    frames[c] += 1
                    for j in range(3):
                        esum[c, j] += e[j][i]
                        bound[c, j] += frame_bound(B, e[j][i])
            if (k + 1) % SWEEP_SYNC == 0 and not first.any():
                break
        assert not first.any()
    assert out["steps"] == steps
    n = np.maximum(epi[:, 0], 1).astype(np.float64)
    assert np.array_equal(out["episodes"].cpu().numpy(), epi[:, 0]) and np.array_equal(out["failures"].cpu().numpy(), epi[:, 1])
    assert np.array_equal(out["end_time_ratio"].cpu().numpy(), epi[:, 2].astype(np.float64) / 16777216.0 / n)
    assert np.array_equal(out["episode_length"].cpu().numpy(), epi[:, 3].astype(np.float64) / n)
    assert np.array_equal(out["frames"].cpu().numpy(), frames) and frames.min() >= 3
    for j, key in enumerate(("E_gmpbpe", "E_mpbpe", "E_mpjpe")):
        got = out[key].cpu().numpy() * frames * GRID                                         # the table's integer sum again
        diff = np.abs(got - esum[:, j] * GRID)
        print(f"sweep {key}: mean {float(out[key].mean()):.4e}, worst error / bound {float((diff / bound[:, j]).max()):.3f}")
        assert (diff <= bound[:, j] + 1e-6).all(), (key, diff, bound[:, j])                  # (1e-6 grid units: this test's own float64 arithmetic)
    fail = list(SWEEP_FAIL)
    assert (out["end_time_ratio"].cpu().numpy()[fail] < 0.5).all() and (np.delete(out["end_time_ratio"].cpu().numpy(), fail) > 0.9).all()


# ---- 4. both agents ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload,num_clips", [("v1_walk", 1), ("v2_student23", 5)])
def test_agents_evaluate_library(workload, num_clips):
    import bench

    orig = ML.load_motion_file
    if num_clips > 1:                                      # (a short base clip: the sweep plays every clip to its end)
        ML.load_motion_file = lambda path: [(n, {k: (v[:40] if k != "fps" else v) for k, v in c.items()}) for n, c in orig(path)]
    try:
        cfg, env, Algo = bench.build(4, DEV, 3, workload, num_clips=num_clips)
    finally:
        ML.load_motion_file = orig
    M = env._motion_lib._num_unique_motions
    assert M == num_clips
    algo = Algo(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
    algo.setup()
    ml = env._motion_lib

    def before_wave(w, clip_ids):
        """the wave's replay window from motion time 0 (without one the stub holds a stale state and every episode ends in its first
        step, which is not scored).  make_replay_on_device reads the episode clock: put it where the reset that follows will."""
        env._episode_length_buf.zero_()
        env.motion_start_times.zero_()
        env.motion_len.copy_(ml.get_motion_length(env.motion_ids))
        env.simulator.set_replay(*bench.make_replay_on_device(env, int(float(env.motion_len.max()) / env.dt) + 12, seed=5 + w))

    out = algo.evaluate_library(sync_every=16, before_wave=before_wave)
    torch.cuda.synchronize()
    assert algo.library_metrics is out and set(KEYS) <= set(out)
    assert out["waves"] == -(-M // 4) and out["unfinished"] == [] and out["steps"] > 0
    assert out["episodes"].tolist() == [1] * M and int(out["frames"].min()) > 0
    for k in ("end_time_ratio", "episode_length", "E_gmpbpe", "E_mpbpe", "E_mpjpe"):
        assert out[k].shape == (M,) and bool(torch.isfinite(out[k]).all()), k
    for k in ("success_rate", "E_gmpbpe_mean", "E_mpbpe_mean", "E_mpjpe_mean"):
        assert isinstance(out[k], float) and np.isfinite(out[k]), k
    assert not torch.is_grad_enabled() or all(not t.requires_grad for t in out.values() if torch.is_tensor(t))
