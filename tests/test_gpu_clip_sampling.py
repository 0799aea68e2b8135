"""Per-clip episode statistics (k_clip_stats), the fold into the motion library's sampling hooks (k_clip_sampling_update) and the device
slot draw (k_clip_sample_slots) against numpy restatements in this file; then the env, the rollout graph and two ranks.

The window is integer-only, so every comparison of it is exact.  Tolerances of the update (used by tests 2, 4 and 6): E, F and
_success_rate are the same IEEE double operations as numpy's, cast to float32 once (the library is built with -ffp-contract=off) -> bit-equal;
_sampling_prob differs only by the ORDER of the double sum over r (relative error <= M * 2^-53), which can flip the final rounding to
float32 and no more -> within 1 ulp of float32."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pbhc_amd import _lib
from tests.helpers import GOLDEN, _philox4x32_7, build_hip_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = dict(decay=0.5, prior=1.0, floor=0.1)


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------
def ref_window(reset, tout, ratio, length, slot, M):
    w = np.zeros((M, 4), np.int64)
    ok = (reset != 0) & (slot >= 0) & (slot < M)
    c = slot[ok]
    fixed = np.rint(ratio[ok].astype(np.float32) * np.float32(16777216.0)).astype(np.int64)
    for col, v in enumerate((np.ones(c.shape, np.int64), (tout[ok] == 0).astype(np.int64), fixed, length[ok].astype(np.int64))):
        np.add.at(w[:, col], c, v)
    return w


def ref_update(E, F, e, f, decay, prior, floor):
    """-> E', F', success, p (float32) from float32 E, F and int64 e, f"""
    M = len(E)
    E2 = (decay * E.astype(np.float64) + e.astype(np.float64)).astype(np.float32)
    F2 = (decay * F.astype(np.float64) + f.astype(np.float64)).astype(np.float32)
    Ed, Fd = E2.astype(np.float64), F2.astype(np.float64)
    r = (Fd + prior) / (Ed + prior)
    succ = np.where(E2 > 0, (1.0 - Fd / np.where(E2 > 0, Ed, 1.0)).astype(np.float32), np.float32(0))
    p = ((1.0 - floor) * r / r.sum() + floor / M).astype(np.float32)
    return E2, F2, succ, p


def ref_draw(p, seed, draw_index, N):
    """-> (clip [N], near [N]): the reference draw and which slots lie within 1e-9 of a boundary of the reference CDF"""
    M = len(p)
    cdf = np.cumsum(p.astype(np.float64))
    w0 = _philox4x32_7(int(seed), np.arange(N, dtype=np.int64), int(draw_index), 20, 0)[0]
    u = (w0 >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    target = u.astype(np.float64) * cdf[-1]
    clip = np.minimum(np.searchsorted(cdf, target, side="right"), M - 1)
    near = (np.abs(target[:, None] - cdf[None, :]) < 1e-9).any(axis=1)
    return clip.astype(np.int64), near


def within_one_ulp32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all())


def check_update(dev, ref, what=""):
    """dev / ref: (E, F, success, p) — the tolerances of the module docstring"""
    for name, d, r in zip(("E", "F", "success"), dev[:3], ref[:3]):
        assert np.array_equal(np.asarray(d, np.float32).view(np.uint32), np.asarray(r, np.float32).view(np.uint32)), what + name
    assert within_one_ulp32(dev[3], ref[3]), what + "p"


# ---- device calls ------------------------------------------------------------------------------------------------------------------
def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def collect(reset, tout, ratio, length, slot, window):
    """numpy episode arrays -> k_clip_stats into the device tensor `window` [M,4]"""
    t = [tg(reset.astype(np.int64)), tg(tout.astype(np.uint8)), tg(ratio.astype(np.float32)), tg(length.astype(np.int64)), tg(slot.astype(np.int64))]
    _lib.check(_lib.lib().pbhc_clip_stats(*[x.data_ptr() for x in t], len(reset), window.shape[0], window.data_ptr(), _lib.current_stream()),
               "pbhc_clip_stats")
    torch.cuda.synchronize()


def synth_episodes(N, M, mode, seed, stray=False):
    rng = np.random.default_rng(seed)
    reset = {"zeros": np.zeros(N, np.int64), "ones": np.ones(N, np.int64), "random": (rng.random(N) < 0.5).astype(np.int64)}[mode]
    tout = ((reset != 0) & (rng.random(N) < 0.4)).astype(np.uint8)                   # a subset of the resets
    special = np.array([0.0, 1e-9, 0.5, 1.05], np.float32)
    ratio = np.where(rng.random(N) < 0.5, special[rng.integers(0, 4, N)], rng.uniform(0.0, 1.1, N).astype(np.float32)).astype(np.float32)
    ratio[:min(N, 4)] = special[:min(N, 4)]
    length = rng.integers(0, 2**31, N, endpoint=True).astype(np.int64)
    length[N - 1] = 2**31
    slot = rng.integers(0, M, N).astype(np.int64)
    if stray == "sorted":                                                            # whole waves of one clip, a workgroup with several
        slot = np.sort(slot)
    elif stray:                                                                      # skipped, never used as an index
        slot[5], slot[9], slot[11] = -1, M, 2**40
    return reset, tout, ratio, length, slot


# ---- 1. the collector alone --------------------------------------------------------------------------------------------------------
# (the collector's workgroup is 1024 threads = 16 waves: 1100 and 2050 cross it, with one clip, with waves of one clip each but several per
# workgroup (slots sorted), and with mixed waves)
@pytest.mark.parametrize("N,M,stray", [(1, 1, False), (67, 1, False), (67, 3, False), (67, 3, True), (259, 70, False), (1100, 1, False),
                                       (1100, 3, False), (2050, 70, False), (2050, 2, "sorted")])
@pytest.mark.parametrize("mode", ["zeros", "ones", "random"])
def test_collector_equals_numpy_and_accumulates(N, M, stray, mode):
    a = synth_episodes(N, M, mode, seed=100 + N + M, stray=stray)
    b = synth_episodes(N, M, "random", seed=200 + N + M, stray=stray)
    window = torch.zeros(M, 4, dtype=torch.int64, device=DEV)
    collect(*a, window)
    wa = ref_window(*a, M)
    assert torch.equal(window.cpu(), torch.from_numpy(wa))
    if mode == "ones" and not stray:
        assert int(wa[:, 0].sum()) == N and int(wa[:, 3].sum()) >= 2**31
    collect(*b, window)                                                              # the sum, not an overwrite
    assert torch.equal(window.cpu(), torch.from_numpy(wa + ref_window(*b, M)))


# ---- 2. the update alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 257, 1025])
def test_update_equals_the_numpy_rule(M):
    rng = np.random.default_rng(M)
    lib = _lib.lib()
    E, F, S, P = (torch.zeros(M, device=DEV) for _ in range(4))
    cdf = torch.zeros(M, dtype=torch.float64, device=DEV)
    Eh, Fh = np.zeros(M, np.float32), np.zeros(M, np.float32)
    for rnd in range(2):                                                             # the second time with non-zero E, F
        e = rng.integers(0, 50, M).astype(np.int64)
        e[rng.random(M) < 0.3] = 0                                                   # clips without an episode
        if M > 1 and rnd == 0:
            e[0] = 0
        f = (e * rng.random(M)).astype(np.int64)
        w = np.stack([e, f, rng.integers(0, 2**30, M), rng.integers(0, 2**20, M)], axis=1).astype(np.int64)
        window = tg(w)
        _lib.check(lib.pbhc_clip_sampling_update(window.data_ptr(), E.data_ptr(), F.data_ptr(), S.data_ptr(), P.data_ptr(), cdf.data_ptr(), M,
                                                 DEFAULTS["decay"], DEFAULTS["prior"], DEFAULTS["floor"], _lib.current_stream()), "update")
        torch.cuda.synchronize()
        ref = ref_update(Eh, Fh, e, f, **DEFAULTS)
        check_update((E.cpu().numpy(), F.cpu().numpy(), S.cpu().numpy(), P.cpu().numpy()), ref, f"M {M} round {rnd}: ")
        Eh, Fh = ref[0], ref[1]
        assert int(window.abs().sum()) == 0                                          # the window is cleared
        c = cdf.cpu().numpy()
        assert abs(c[-1] - 1.0) <= M * 2.0**-24
        assert (np.diff(c) > 0).all() and np.abs(c - np.cumsum(P.cpu().numpy().astype(np.float64))).max() < 1e-12


# ---- 3. the slot draw alone --------------------------------------------------------------------------------------------------------
def _pick_seed(p, draw_index, N, base):
    """a seed (with high key bits) for which the REFERENCE leaves no slot out: chosen on the CPU, before the device is asked"""
    for k in range(64):
        seed = base + k
        if not ref_draw(p, seed, draw_index, N)[1].any():
            return seed
    raise AssertionError("no seed without a near-boundary slot")


def device_draw(p, seed, draw_index, N):
    M = len(p)
    slots = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    cdf = torch.cumsum(tg(p.astype(np.float32)).double(), 0).contiguous()       # (the product's own scan: tests 2 and 4)
    _lib.check(_lib.lib().pbhc_clip_sample_slots(cdf.data_ptr(), M, seed, draw_index, slots.data_ptr(), N, _lib.current_stream()),
               "pbhc_clip_sample_slots")
    torch.cuda.synchronize()
    return slots.cpu().numpy()


def check_draw(got, p, seed, draw_index, max_out):
    clip, near = ref_draw(p, seed, draw_index, len(got))
    assert int(near.sum()) <= max_out
    assert np.array_equal(got[~near], clip[~near])
    assert got.min() >= 0 and got.max() < len(p)


@pytest.mark.parametrize("M", [1, 3, 257, 1025])
@pytest.mark.parametrize("N", [13, 4096])
def test_slot_draw_equals_searchsorted(M, N):
    rng = np.random.default_rng(1000 + M)
    p = rng.random(M).astype(np.float32)
    if M > 3:
        p[rng.random(M) < 0.1] = 0.0
    p = (p / p.sum(dtype=np.float64)).astype(np.float32)
    seen = []
    for draw_index in (0, 5):
        seed = _pick_seed(p, draw_index, N, (0x1234 << 32) + 77 * M)
        got = device_draw(p, seed, draw_index, N)
        check_draw(got, p, seed, draw_index, max_out=N // 100)
        assert not (got[p[got] == 0]).size                                           # a clip of probability 0 is never drawn
        seen.append((seed, got))
    if M > 1 and N == 4096 and seen[0][0] == seen[1][0]:
        assert not np.array_equal(seen[0][1], seen[1][1])                            # the draw index keys the stream


def test_slot_draw_frequencies_and_zero_probability():
    p, N = np.array([0.5, 0.25, 0.25, 0.0], np.float32), 4096
    seed = _pick_seed(p, 1, N, 2024)
    got = device_draw(p, seed, 1, N)
    check_draw(got, p, seed, 1, max_out=0)
    counts = np.bincount(got, minlength=4)
    assert counts[3] == 0
    for i in range(3):                                   # deterministic for the seed: this cannot flake
        assert abs(counts[i] - N * p[i]) <= 5.0 * np.sqrt(N * p[i] * (1.0 - p[i])), counts


# ---- 4. the env --------------------------------------------------------------------------------------------------------------------
def _teacher_env(n, overrides):
    import bench
    from pbhc_amd import motion_lib as ML
    from tests.helpers import clip_from_env_golden

    g = dict(np.load(os.path.join(GOLDEN, "env_v2_teacher29.npz")))
    clips = bench.synth_library(clip_from_env_golden(g), 3, seed=3)
    orig = ML.load_motion_file
    ML.load_motion_file = lambda path: [(f"c{i}", c) for i, c in enumerate(clips)]
    try:
        return build_hip_env("v2_g1_29dof_teacher.yaml", n, general=True, overrides=dict({"domain_rand.push_robots": False}, **overrides))
    finally:
        ML.load_motion_file = orig


def _read_episodes(env):
    torch.cuda.synchronize()
    return (env.reset_buf.cpu().numpy().copy(), env.time_out_buf.cpu().numpy().astype(np.uint8), env.end_time_ratio_buf.cpu().numpy().copy(),
            env.last_episode_length_buf.cpu().numpy().copy(), env._motion_lib.slot_clip.cpu().numpy().copy())


def test_env_collects_per_clip_and_resamples_by_failure():
    import bench

    N, M = 13, 3
    cfg, env = _teacher_env(N, {"env.config.resample_time_interval_s": 0.02 * 6, "env.config.clip_sampling": {"enable": True}})
    assert env.resample_time_interval == 6 and env._clip["sampling"] and env._clip["statistics"]
    table = np.zeros((M, 4), np.int64)
    env.reset_all()                                                                  # step 1
    table += ref_window(*_read_episodes(env), M)
    fail_envs, tout_envs = [7, 8], [3, 4]
    env.motion_start_times[tout_envs] = env.motion_len[tout_envs] - 1.5 * env.dt     # time-outs
    root, qp, qv, cf = bench.make_replay_on_device(env, 12, seed=5)
    root[1, fail_envs, 2] += 1.0                                                     # failures: the root 1 m above its reference in one frame
    env.simulator.set_replay(root, qp, qv, cf)
    act = torch.zeros(N, env.num_dof, device=DEV)
    for step in range(2, 6):                                                         # steps 2..5
        env.step({"actions": act})
        table += ref_window(*_read_episodes(env), M)
    st = env.clip_statistics()
    assert torch.equal(env._clip_window.cpu(), torch.from_numpy(table))
    assert torch.equal(st["episodes"].cpu(), torch.from_numpy(table[:, 0])) and torch.equal(st["failures"].cpu(), torch.from_numpy(table[:, 1]))
    n = np.maximum(table[:, 0], 1).astype(np.float64)
    assert np.array_equal(st["end_time_ratio_mean"].cpu().numpy(), table[:, 2].astype(np.float64) / 16777216.0 / n)
    assert np.array_equal(st["episode_length_mean"].cpu().numpy(), table[:, 3].astype(np.float64) / n)
    # the run shows something: a failure, a time-out episode, episodes on two clips
    assert table[:, 1].sum() >= 1 and (table[:, 0] - table[:, 1]).sum() >= 1 and (table[:, 0] > 0).sum() >= 2, table
    log = env.read_log()
    assert log["clip_episodes"] == table[:, 0].sum()
    assert abs(log["clip_success_rate"] - (1.0 - table[:, 1].sum() / table[:, 0].sum())) < 1e-12
    assert abs(log["clip_sampling_concentration"] - 1.0) < 1e-6                      # still uniform
    slot_before = env._motion_lib.slot_clip.cpu().numpy().copy()
    assert slot_before.tolist() == [i % 3 for i in range(N)]
    obs, _, _, _ = env.step({"actions": act})                                        # step 6 -> update, draw, reset of every env
    reset6, tout6, _, len6, slot_after = _read_episodes(env)                          # (reset_buf / time_out_buf stay the step's own)
    table += ref_window(reset6, tout6, np.zeros(N, np.float32), len6, slot_before, M)
    ml, c = env._motion_lib, env._clip
    ref = ref_update(np.zeros(M, np.float32), np.zeros(M, np.float32), table[:, 0], table[:, 1], c["decay"], c["prior_episodes"], c["uniform_floor"])
    p_dev = ml._sampling_prob.cpu().numpy()
    check_update((ml._sampling_history.cpu().numpy(), ml._termination_history.cpu().numpy(), ml._success_rate.cpu().numpy(), p_dev), ref, "env: ")
    assert len(set(p_dev.tolist())) > 1                                              # the clips no longer weigh the same
    check_draw(slot_after, p_dev, env._seed, 0, max_out=1)
    assert int(env.episode_length_buf.abs().sum()) == 0                              # every env is reset
    assert int(env._clip_window.abs().sum()) == 0 and int(env.clip_statistics()["episodes"].sum()) == 0
    assert torch.allclose(env.motion_len, ml._motion_lengths[ml.slot_clip])
    obs, _, _, _ = env.step({"actions": act})
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in obs.values())
    assert env.read_log()["clip_sampling_concentration"] > 1.0


def test_statistics_only_with_a_finalize_stream_across_the_periodic_resample():
    """clip_statistics without clip_sampling, the step's reduction and the collector on a finalize stream, and the periodic resample inside
    step(): the slot -> clip table is redrawn (torch.multinomial, on the stepping stream) only after the collector of that step has read the
    old one.  Every finished episode of the resample step lands in the row of the clip it was run on."""
    import bench

    N, M = 64, 3
    cfg, env = _teacher_env(N, {"env.config.resample_time_interval_s": 0.02 * 4, "env.config.clip_statistics": True})
    assert env.resample_time_interval == 4 and env._clip["statistics"] and not env._clip["sampling"]
    env.reset_all()                                                                  # step 1
    env.clear_clip_statistics()
    root, qp, qv, cf = bench.make_replay_on_device(env, 8, seed=5)
    root[2, :, 2] += 1.0                                                             # every env fails in the resample step (third frame)
    env.simulator.set_replay(root, qp, qv, cf)
    env._motion_lib._sampling_prob.copy_(torch.tensor([0.0, 0.0, 1.0], device=DEV))  # the redraw moves every slot to clip 2
    side = torch.cuda.Stream()
    env.set_finalize_stream(side)
    act = torch.zeros(N, env.num_dof, device=DEV)
    table = np.zeros((M, 4), np.int64)
    try:
        for step in (2, 3):
            env.step({"actions": act})
            env.wait_finalize()
            table += ref_window(*_read_episodes(env), M)
        slot_before = env._motion_lib.slot_clip.cpu().numpy().copy()
        assert slot_before.tolist() == [i % 3 for i in range(N)]
        env.step({"actions": act})                                                   # step 4: collector on the side stream, then the resample
        env.wait_finalize()
        reset4, tout4, _, len4, slot_after = _read_episodes(env)
    finally:
        env.set_finalize_stream(None)
    assert slot_after.tolist() == [2] * N and int(reset4.sum()) >= N // 2            # the resample happened; the step finished episodes
    step4 = ref_window(reset4, tout4, np.zeros(N, np.float32), len4, slot_before, M)
    got = env._clip_window.cpu().numpy()
    assert (step4[:, 0] > 0).sum() == 3
    for col in (0, 1, 3):                            # (the resample's reset overwrote end_time_ratio_buf: column 2 is checked up to step 3)
        assert np.array_equal(got[:, col], table[:, col] + step4[:, col]), col
    assert (got[:, 2] >= table[:, 2]).all()


def test_off_means_no_window_and_no_log_keys():
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 4)
    assert env._clip == dict(statistics=False, sampling=False, decay=0.5, prior_episodes=1.0, uniform_floor=0.1) and env._clip_window is None
    env.reset_all()
    assert not any(k.startswith("clip_") for k in env.read_log())
    for call in (env.clip_statistics, env.clear_clip_statistics, env.update_clip_sampling):
        with pytest.raises(_lib.PbhcError, match="clip_statistics"):
            call()


def test_one_clip_env_counts_every_reset_on_one_row():
    """v1 has one clip: M = 1, every lane of a wave adds to the same row"""
    N = 67
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", N, overrides={"env.config.clip_statistics": True})
    assert env._clip_window.shape == (1, 4)
    env.reset_all()
    table = ref_window(*_read_episodes(env), 1)
    env.reset_buf.fill_(1)                               # what a reset of every env leaves: N adds onto one row
    env.time_out_buf.zero_()
    eps = _read_episodes(env)
    env._launch_clip_stats(_lib.current_stream())
    table += ref_window(*eps, 1)
    assert int(table[0, 0]) >= N and torch.equal(env._clip_window.cpu(), torch.from_numpy(table))
    env.clear_clip_statistics()
    assert int(env._clip_window.abs().sum()) == 0


# ---- 5. rollout graph = eager loop -------------------------------------------------------------------------------------------------
_ROLLOUTS = {}


def _rollouts(split, graph):
    if (split, graph) in _ROLLOUTS:
        return _ROLLOUTS[(split, graph)]
    import bench
    from pbhc_amd.agents.mh_ppo import MHPPO

    os.environ["PBHC_ROLLOUT_GRAPH"], os.environ["PBHC_ROLLOUT_SPLIT"] = str(int(graph)), str(int(split))
    try:
        torch.manual_seed(11)
        np.random.seed(11)
        cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 64, noise_off=False, overrides={"env.config.clip_statistics": True})
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
        algo.setup()
        algo._train_mode()
        obs = env.reset_all()
        env.simulator.set_replay(*bench.make_replay_on_device(env, 4 * algo.num_steps_per_env + 2, seed=5))
        used, out = [], {}
        for r in range(4):
            algo.storage.clear()
            obs = algo._rollout_step(obs)
            used.append(bool(getattr(algo, "_rollout_used_graph", False)))
            if r == 1:                                   # the window is read and cleared between two replays of the same graph
                out["clip_window_before_clear"] = env._clip_window.clone()
                env.clear_clip_statistics()
        torch.cuda.synchronize()
        out.update({k: getattr(algo.storage, k).clone() for k in algo.storage.stored_keys})
        out["globals"] = env.globals.clone()
        out["clip_window"] = env._clip_window.clone()
        out["episodes"] = env.clip_statistics()["episodes"]
        _ROLLOUTS[(split, graph)] = (out, used)
        return out, used
    finally:
        os.environ.pop("PBHC_ROLLOUT_GRAPH", None)
        os.environ.pop("PBHC_ROLLOUT_SPLIT", None)


@pytest.mark.parametrize("split", [1, 0])
def test_clip_table_of_the_graph_rollout_equals_the_eager_loop(split):
    """split = 1: the collector inside the captured rollout (on the finalize stream) is a schedule, not arithmetic — the integer table (also
    the one read and cleared between two replays) and the rollout buffers are bit-identical to the eager loop.  split = 0: no graph is
    ever captured (the rollout graph needs the split streams), so that case is NOT a graph <-> eager identity: it runs the one-stream
    placement of the launch twice, with PBHC_ROLLOUT_GRAPH set and unset, and checks that the switch changes nothing there."""
    (a, used_a), (b, used_b) = _rollouts(split, 1), _rollouts(split, 0)
    assert used_a == ([False, True, True, True] if split else [False] * 4) and not any(used_b)     # (the graph needs the split streams)
    assert int(a["episodes"].sum()) > 0 and int(a["clip_window_before_clear"][:, 0].sum()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 6. two ranks ------------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _clip_rank_main(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        N, M = 13, 3
        cfg, env = _teacher_env(N, {"env.config.clip_sampling": {"enable": True}})
        rows = []
        for rnd in range(2):
            collect(*synth_episodes(67, M, "random", seed=10 * rnd + rank), env._clip_window)
            env.update_clip_sampling()
            torch.cuda.synchronize()
            ml = env._motion_lib
            rows.append(dict(E=ml._sampling_history.cpu().numpy(), F=ml._termination_history.cpu().numpy(), S=ml._success_rate.cpu().numpy(),
                             p=ml._sampling_prob.cpu().numpy(), window=env._clip_window.cpu().numpy()))
        torch.save(rows, out_path + f".{rank}")
    finally:
        dist.destroy_process_group()


def test_two_ranks_fold_the_summed_windows(tmp_path):
    world, M = 2, 3
    out = str(tmp_path / "clip.pt")
    mp.spawn(_clip_rank_main, args=(world, _free_port(), out), nprocs=world, join=True)
    rows = [torch.load(out + f".{rank}", weights_only=False) for rank in range(world)]
    E, F = np.zeros(M, np.float32), np.zeros(M, np.float32)
    for rnd in range(2):
        w = sum(ref_window(*synth_episodes(67, M, "random", seed=10 * rnd + rank), M) for rank in range(world))
        assert w[:, 0].sum() > 0
        ref = ref_update(E, F, w[:, 0], w[:, 1], 0.5, 1.0, 0.1)
        for rank in range(world):
            r = rows[rank][rnd]
            check_update((r["E"], r["F"], r["S"], r["p"]), ref, f"rank {rank} round {rnd}: ")
            assert not r["window"].any()
        assert np.array_equal(rows[0][rnd]["p"], rows[1][rnd]["p"])                  # every rank holds the same probabilities
        E, F = ref[0], ref[1]
