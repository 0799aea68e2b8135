"""The rollout's rider form (agents/rollout.py): the env step's one-workgroup reduction and the done / episode-statistics kernel of control step
t - 1 run as extra workgroups of the policy launch of step t (`PbhcRider`, `pbhc_mlp_fwd_*_riders`), so that step -> policy -> step stays on
one queue.  That is a schedule, not arithmetic: everything a rollout leaves is held bit for bit to the branch form (`PBHC_ROLLOUT_RIDERS=0`),
the captured loop to the eager one, and the 512-thread reduction workgroup to `k_env_finalize` on the same partial rows.

Shapes: T = 4 steps per rollout, three rollouts, v1 walk config.  N = 40 is no multiple of 16 (a partial last policy workgroup and a partial
last book-keeping rider); N = 272 leaves 2 * 68 = 136 > 8 * 16 partial rows, so both the unrolled and the tail part of the reduction's loop run.
Episodes are shortened (staggered episode lengths just below the limit, before every rollout) so that resets and time-outs fall inside it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.helpers import build_hip_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 4
CFG = "v1_g1_23dof_walk.yaml"


def _rollouts(N, riders, graph=False, rollouts=3, overrides=None):
    """`rollouts` rollouts of MHPPO on the v1 walk config from fixed seeds -> everything they leave, + which form / whether a graph ran"""
    import bench
    from pbhc_amd.agents.mh_ppo import MHPPO

    os.environ["PBHC_ROLLOUT_RIDERS"] = "1" if riders else "0"
    os.environ["PBHC_ROLLOUT_GRAPH"] = "1" if graph else "0"
    try:
        torch.manual_seed(11)
        np.random.seed(11)
        cfg, env = build_hip_env(CFG, N, noise_off=False, overrides=overrides)
        cfg.algo.config.num_steps_per_env = T
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
        algo.setup()
        algo._train_mode()
        obs = env.reset_all()
        env.simulator.set_replay(*bench.make_replay_on_device(env, rollouts * T + 2, seed=5))
        forms, used = [], []
        for _ in range(rollouts):
            # env i times out at step i % T of this rollout (set again every rollout: terminate_when_dof_far resets EVERY env at once, which
            # would wipe a pattern laid out once over the whole window)
            env._episode_length_buf.copy_(int(env.max_episode_length) - (torch.arange(N, device=DEV) % T))
            algo.storage.clear()
            obs = algo._rollout_step(obs)
            forms.append(algo._rollout_form)
            used.append(bool(algo._rollout_used_graph))
        torch.cuda.synchronize()
        st = algo.storage
        out = {k: getattr(st, k).clone() for k in st.stored_keys}
        out.update({"obs." + k: v.clone() for k, v in obs.items()})
        out.update(time_outs=algo._time_outs.clone(), cur_reward_sum=algo.cur_reward_sum.clone(), cur_episode_length=algo.cur_episode_length.clone(),
                   globals=env.globals.clone(), frame_cursor=env.simulator.frame_cursor.clone(), episode_sums=env._episode_sums.clone())
        info = dict(forms=forms, used=used, ep_stats=algo._ep_stats.clone(), rows=env.finalize_rider().num_partial_rows, owed=env.finalize_owed,
                    log=env.read_log())
        return out, info
    finally:
        os.environ.pop("PBHC_ROLLOUT_RIDERS", None)
        os.environ.pop("PBHC_ROLLOUT_GRAPH", None)


_cache = {}


def _cached(N, riders, graph=False):
    """(a reference run is computed once and shared; nothing modifies what it returned)"""
    key = (N, riders, graph)
    if key not in _cache:
        _cache[key] = _rollouts(N, riders, graph)
    return _cache[key]


def _log_equal(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def _same(a, b, ia, ib):
    for run, info in ((a, ia), (b, ib)):
        assert bool(run["dones"].any()) and bool(run["time_outs"].any()), "no reset / time-out inside the window: the comparison proves nothing"
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    ea, eb = ia["ep_stats"], ib["ep_stats"]
    assert float(ea[2]) == float(eb[2]) and float(ea[2]) > 0                    # count: exact
    assert torch.allclose(ea[:2], eb[:2], rtol=1e-12, atol=0.0)                  # the two sums: double atomics, no fixed order in either form


@pytest.mark.parametrize("N", [40, 272])
def test_rider_form_equals_branch_form(N):
    """1. rider form against branch form, both eager: every rollout-buffer key, dones, stored time-outs, the running episode sums, the env's
    globals (sigma, EMA, curricula, step counter, log block), the frame cursor and the observations returned are bit-identical"""
    a, ia = _cached(N, True)
    b, ib = _cached(N, False)
    assert ia["forms"] == ["riders"] * 3 and ib["forms"] == ["branch"] * 3 and not any(ia["used"]) and not any(ib["used"])
    assert ia["rows"] == 2 * ((N + 3) // 4) and (N != 272 or ia["rows"] > 8 * 16) and (N != 40 or N % 16 != 0)
    assert not ia["owed"]
    _same(a, b, ia, ib)
    assert _log_equal(ia["log"], ib["log"])                                                # read_log() / log_dict see the last step's reduction


@pytest.mark.parametrize("N", [40, 272])
def test_rider_form_captured_equals_rider_form_eager(N):
    """2. the rider form as ONE hipGraph (rollouts 2 and 3 replay it) against the rider form step by step"""
    a, ia = _rollouts(N, True, graph=True)
    b, ib = _cached(N, True)
    assert ia["forms"] == ["riders"] * 3 and ia["used"] == [False, True, True] and not any(ib["used"])
    _same(a, b, ia, ib)


def _one_row_stack():
    """a one-layer 16 -> 8 stack for a one-row launch of k_mlp_fwd: (input, weight arrays for the C ABI, things to keep alive)"""
    from pbhc_amd import _lib

    lib = _lib.lib()
    g = torch.Generator().manual_seed(3)
    W, b, x = torch.randn(8, 16, generator=g).to(DEV), torch.randn(8, generator=g).to(DEV), torch.randn(1, 16, generator=g).to(DEV)
    packed = torch.empty(lib.pbhc_mlp_packed_floats(8, 16), device=DEV)
    _lib.check(lib.pbhc_mlp_pack(W.data_ptr(), 8, 16, packed.data_ptr(), _lib.current_stream()), "pbhc_mlp_pack")
    inp = _lib.PbhcMlpInput()
    inp.x[0], inp.ld[0], inp.width[0], inp.nseg = x.data_ptr(), 16, 16, 1
    return inp, (C.c_void_p * 1)(packed.data_ptr()), (C.c_void_p * 1)(b.data_ptr()), (C.c_int * 2)(16, 8), (W, b, x, packed)


@pytest.mark.parametrize("rows", [2, 129, 200, 700])
def test_rider_reduction_equals_k_env_finalize(rows):
    """3. the reduction body alone: a one-row policy launch that carries only the finalize rider (512 threads, two chunks per wave) against
    `k_env_finalize` (1024 threads) on the same random partial rows, twice in a row: globals and cursor equal bit for bit.  v1 walk config:
    adaptive sigma on, penalty / limit / motion-far curricula on (the partial rows hold resets, so the curricula's branch runs).  700 rows: the
    512-thread caller's joint loop over a wave's two chunks (16 loads in flight each) runs twice, then the 8-load loop, then the tail."""
    from pbhc_amd import _lib

    lib = _lib.lib()
    cfg, env = build_hip_env(CFG, 16)
    env.reset_all()
    assert env._c.adaptive_sigma and env._c.penalty_curriculum and env._c.motion_far_curriculum
    NP = _lib.K["PBHC_NUM_TOTALS"]
    partials = (torch.rand(rows, NP, generator=torch.Generator().manual_seed(rows)) * 3.0).to(DEV)
    inp, w, b, dims, keep = _one_row_stack()
    y0, y1 = torch.zeros(1, 8, device=DEV), torch.zeros(1, 8, device=DEV)
    _lib.check(lib.pbhc_mlp_fwd_cat(C.byref(inp), w, b, dims, 1, 0, y0.data_ptr(), 8, 1, None, _lib.current_stream()), "pbhc_mlp_fwd_cat")
    torch.cuda.synchronize()
    res = []
    for form in ("kernel", "rider"):
        glob, cursor = env.globals.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
        r = env.finalize_rider()
        r.globals, r.partials, r.frame_cursor, r.num_partial_rows, r.num_frames = glob.data_ptr(), partials.data_ptr(), cursor.data_ptr(), rows, 7
        assert r.has_finalize == 1 and r.has_post == 0
        for _ in range(2):
            if form == "kernel":
                _lib.check(lib.pbhc_debug_env_finalize(C.byref(r), _lib.current_stream()), "pbhc_debug_env_finalize")
            else:
                _lib.check(lib.pbhc_mlp_fwd_cat_riders(C.byref(inp), w, b, dims, 1, 0, y1.data_ptr(), 8, 1, None, C.byref(r), _lib.current_stream()),
                           "pbhc_mlp_fwd_cat_riders")
        torch.cuda.synchronize()
        res.append((glob, cursor))
    (ga, ca), (gb, cb) = res
    assert torch.equal(ga, gb) and torch.equal(ca, cb) and int(ca) == 2
    c = _lib.K["PBHC_G_STEP_COUNTER"]
    assert float(ga[c]) == float(env.globals[c]) + 2.0
    s0, e0 = _lib.K["PBHC_G_SIGMA"], _lib.K["PBHC_G_EMA"]
    assert not torch.equal(ga[e0:e0 + _lib.K["PBHC_NUM_SIGMA"]], env.globals[e0:e0 + _lib.K["PBHC_NUM_SIGMA"]])      # the EMA chains ran
    a0 = _lib.K["PBHC_G_AVG_EP_LEN"]
    assert float(ga[a0]) != float(env.globals[a0])                               # ... and the chain the curricula are keyed on
    assert torch.isfinite(ga).all() and torch.isfinite(ga[s0:s0 + _lib.K["PBHC_NUM_SIGMA"]]).all()
    assert torch.equal(y0, y1)                                                   # the stack's own workgroup is what it was


def test_book_keeping_rider_equals_rollout_post2():
    """the book-keeping riders alone (16 envs per workgroup, N = 40: a partial last one) against `pbhc_rollout_post2` (8 per workgroup)"""
    from pbhc_amd import _lib

    lib = _lib.lib()
    N, R, gamma = 40, 3, 0.99
    g = torch.Generator().manual_seed(7)
    rew = torch.randn(N, R, generator=g).to(DEV)
    reset = (torch.rand(N, generator=g) < 0.3).to(torch.int64).to(DEV)
    tout = ((torch.rand(N, generator=g) < 0.5) & (reset.cpu() > 0)).to(torch.uint8).to(DEV)
    inp, w, b, dims, keep = _one_row_stack()
    y = torch.zeros(1, 8, device=DEV)
    res = []
    for form in ("kernel", "rider"):
        out = dict(rewards=torch.zeros(N, R, device=DEV), dones=torch.zeros(N, dtype=torch.uint8, device=DEV), touts=torch.zeros(N, dtype=torch.uint8, device=DEV),
                   cur_rew=torch.arange(N, device=DEV, dtype=torch.float32) * 0.25, cur_len=torch.arange(N, device=DEV, dtype=torch.float32),
                   ep=torch.zeros(3, dtype=torch.float64, device=DEV))
        P = lambda k: out[k].data_ptr()
        if form == "kernel":
            _lib.check(lib.pbhc_rollout_post2(rew.data_ptr(), None, reset.data_ptr(), tout.data_ptr(), N, R, gamma, P("rewards"), P("dones"), P("cur_rew"),
                                              P("cur_len"), P("ep"), P("touts"), _lib.current_stream()), "pbhc_rollout_post2")
        else:
            r = _lib.PbhcRider()
            r.rew, r.values, r.reset_buf, r.time_outs = rew.data_ptr(), None, reset.data_ptr(), tout.data_ptr()
            r.rewards_out, r.dones_out, r.cur_reward_sum, r.cur_episode_length, r.ep_stats, r.time_outs_out = (P(k) for k in ("rewards", "dones", "cur_rew", "cur_len", "ep", "touts"))
            r.N, r.R, r.gamma, r.has_post = N, R, gamma, 1
            _lib.check(lib.pbhc_mlp_fwd_cat_riders(C.byref(inp), w, b, dims, 1, 0, y.data_ptr(), 8, 1, None, C.byref(r), _lib.current_stream()),
                       "pbhc_mlp_fwd_cat_riders")
        torch.cuda.synchronize()
        res.append(out)
    a, b_ = res
    assert bool(a["dones"].any()) and bool(a["touts"].any())
    for k in ("rewards", "dones", "touts", "cur_rew", "cur_len"):
        assert torch.equal(a[k], b_[k]), k
    assert float(a["ep"][2]) == float(b_["ep"][2]) > 0 and torch.allclose(a["ep"][:2], b_["ep"][:2], rtol=1e-12, atol=0.0)


def test_collectors_fall_back_to_the_branch_form():
    """4a. with clip_statistics on (its collector lives behind the reduction on the finalize stream) the agent reports the branch form whatever
    the switch says, and leaves what the branch form leaves"""
    ov = {"env.config.clip_statistics": True}
    a, ia = _rollouts(40, True, overrides=ov)
    b, ib = _rollouts(40, False, overrides=ov)
    assert ia["forms"] == ["branch"] * 3 and ib["forms"] == ["branch"] * 3
    _same(a, b, ia, ib)


def test_owed_reduction_is_flushed_by_the_next_step_and_by_readers():
    """4b, 4c. a step that leaves its reduction owed and untaken: the next eager step launches it first (the globals equal two ordinary
    steps'), and a reader of the globals (wait_finalize(): sync_globals, read_log / log_dict) sees it"""
    from pbhc_amd import _lib

    res = []
    for deferred in (False, True):
        torch.manual_seed(5)
        cfg, env = build_hip_env(CFG, 40)
        env.reset_all()
        act = {"actions": torch.zeros(40, env.num_dof, device=DEV)}
        env.set_finalize_deferred(deferred)
        env.step(act)
        assert env.finalize_owed == deferred
        env.sync_globals()                                   # (one process: nothing to exchange)
        log1 = env.read_log()                                # flushes: the log block is this step's
        assert not env.finalize_owed
        g1 = env.globals.clone()
        env.step(act)
        assert env.finalize_owed == deferred
        env.step(act)                                        # finds one owed and untaken
        if deferred:
            assert env.finalize_owed
            with pytest.raises(_lib.PbhcError):
                env.set_finalize_stream(torch.cuda.Stream())
            env.set_finalize_deferred(False)
        assert not env.finalize_owed
        torch.cuda.synchronize()
        res.append((g1, log1, env.globals.clone(), env.simulator.frame_cursor.clone()))
    c = _lib.K["PBHC_G_STEP_COUNTER"]
    assert float(res[1][2][c]) == float(res[0][2][c]) and float(res[1][0][c]) + 2.0 == float(res[1][2][c])
    assert torch.equal(res[0][0], res[1][0]) and _log_equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])
