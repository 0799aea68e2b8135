"""The paired launches of MHPPO's optimiser step (`pbhc_linear_act_fwd_out_pair`, `pbhc_linear_dgrad_act_pair`: two independent problems of
one kernel instantiation on a shared grid) and the joint driver that issues them (fused_mlp.forward_pair).

A pair runs the single entry's tile code on the single entry's tiles, so every comparison with two single calls is bit for bit
(`torch.equal` on every output buffer, guard-filled so that a store beyond a problem's rows / columns shows); the single calls' results are
held, besides, to the fp64 bound of tests/test_gpu_gemm.py (3e-5 absolute on O(1) outputs), so that the equality is not one of two empty
results."""
import ctypes as C
import gc

import pytest
import torch

from tests.test_gpu_gemm import TOL, _act_grad_ref, _act_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = -12345.0


_KEPT = []


@pytest.fixture(autouse=True, scope="module")
def _ordinary_graph_rng_state():
    """Not about the paired launches; about this module's place in a run.  torch creates the device generator's graph-time seed / offset
    tensors when the first live graph registers and drops them with the last one.  The rollout captures inside torch.inference_mode(), so
    whenever that state is born in a rollout and some agent's graphs are still alive (dropped agents live until the collector runs), a later
    capture OUTSIDE inference mode — tests/test_gpu_update_tail.py captures an optimiser step — fails in capture_begin ("Inplace update to
    inference tensor outside InferenceMode").  Whether that happens depends on when the collector ran, and the agents this module builds and
    drops move that: with these tests added, and no other change, that capture failed in a gpu-only run.  The order dependence is the
    suite's and the cause is the rollout's; until the rollout itself sees to it, this module leaves the state behind as ordinary tensors,
    which both modes may update: everything collectable is collected, then one one-kernel graph is captured outside inference mode and kept."""
    if not _KEPT:
        gc.collect()
        t = torch.zeros(1, device=DEV)
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        try:
            with torch.cuda.graph(g, stream=side):
                t.add_(1.0)
            _KEPT.append((g, t))
        except RuntimeError:                                   # (a live holder of rollout-born state: nothing here can change it)
            pass
        torch.cuda.current_stream().wait_stream(side)
    yield


def _L():
    from pbhc_amd import _lib

    return _lib, _lib.lib()


def _guard(*shape):
    return torch.full(shape, GUARD, device=DEV)


def _p(t):
    return None if t is None else t.data_ptr()


# ---- forward of the 128-column layer with the output layer riding ----------------------------------------------------------------------
def _fwd_problem(seed, M, K, NO):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return dict(x=torch.randn(M, K, device=DEV, generator=g), w=torch.randn(128, K, device=DEV, generator=g) / K ** 0.5,
                b=torch.randn(128, device=DEV, generator=g), wo=torch.randn(NO, 128, device=DEV, generator=g) / 128 ** 0.5,
                bo=torch.randn(NO, device=DEV, generator=g), M=M, K=K, NO=NO)


def _fwd_bufs(p, pad=3):
    """y / pre / out with `pad` guard rows behind the problem's M (the kernels' rows are contiguous: a column overrun lands in the next row)"""
    return dict(y=_guard(p["M"] + pad, 128), pre=_guard(p["M"] + pad, 128), out=_guard(p["M"] + pad, p["NO"]))


def _fwd_args(p, o, act):
    return (p["x"].data_ptr(), p["w"].data_ptr(), p["b"].data_ptr(), o["y"].data_ptr(), o["pre"].data_ptr() if act == 2 else None, p["M"], 128, p["K"], act,
            p["wo"].data_ptr(), p["bo"].data_ptr(), p["NO"], o["out"].data_ptr())


@pytest.mark.parametrize("act", [1, 3], ids=["elu", "relu"])
@pytest.mark.parametrize("NOs", [(23, 20), (1, 32)])
@pytest.mark.parametrize("Ks", [(256, 512), (36, 30)])
@pytest.mark.parametrize("Ms", [(1, 1), (33, 200), (200, 33)])
def test_fwd_out_pair_equals_two_single_calls(Ms, Ks, NOs, act):
    L, lib = _L()
    ps = [_fwd_problem(11 + j + Ms[j] + Ks[j] + NOs[j], Ms[j], Ks[j], NOs[j]) for j in (0, 1)]
    single = [_fwd_bufs(p) for p in ps]
    for p, o in zip(ps, single):
        L.check(lib.pbhc_linear_act_fwd_out(*_fwd_args(p, o, act), L.current_stream()), "pbhc_linear_act_fwd_out")
    pair = [_fwd_bufs(p) for p in ps]
    L.check(lib.pbhc_linear_act_fwd_out_pair(*_fwd_args(ps[0], pair[0], act), *_fwd_args(ps[1], pair[1], act), L.current_stream()), "pbhc_linear_act_fwd_out_pair")
    torch.cuda.synchronize()
    for j, p in enumerate(ps):
        for k in ("y", "pre", "out"):                                  # (`pre`: ELU / ReLU write none — the buffer must still be all guard)
            assert torch.equal(pair[j][k], single[j][k]), (j, k)
            assert bool((pair[j][k][p["M"]:] == GUARD).all()), (j, k, "rows beyond M")
        assert bool((pair[j]["pre"] == GUARD).all())
        # and the single call is what it should be (so the equality is not two empty results)
        z = p["x"].double() @ p["w"].double().t() + p["b"].double()
        yr = _act_ref(act, z)
        assert (pair[j]["y"][:p["M"]].double() - yr).abs().max().item() < TOL
        assert (pair[j]["out"][:p["M"]].double() - (yr @ p["wo"].double().t() + p["bo"].double())).abs().max().item() < TOL


def test_fwd_out_pair_with_pre_activation_output():
    """SiLU writes `pre`: the second output image of the same epilogue, paired"""
    L, lib = _L()
    ps = [_fwd_problem(5, 33, 36, 23), _fwd_problem(6, 200, 256, 20)]
    single, pair = [_fwd_bufs(p) for p in ps], [_fwd_bufs(p) for p in ps]
    for p, o in zip(ps, single):
        L.check(lib.pbhc_linear_act_fwd_out(*_fwd_args(p, o, 2), L.current_stream()), "pbhc_linear_act_fwd_out")
    L.check(lib.pbhc_linear_act_fwd_out_pair(*_fwd_args(ps[0], pair[0], 2), *_fwd_args(ps[1], pair[1], 2), L.current_stream()), "pbhc_linear_act_fwd_out_pair")
    torch.cuda.synchronize()
    for j in (0, 1):
        for k in ("y", "pre", "out"):
            assert torch.equal(pair[j][k], single[j][k]), (j, k)
        assert not bool((pair[j]["pre"][:ps[j]["M"]] == GUARD).any())


def test_pair_entries_refuse_what_the_single_entries_would_not_run_on_these_tiles():
    L, lib = _L()
    p, q = _fwd_problem(1, 8, 36, 4), _fwd_problem(2, 8, 36, 4)
    o, r = _fwd_bufs(p), _fwd_bufs(q)
    bad = list(_fwd_args(q, r, 1))
    bad[11] = 33                                                       # NO > 32
    assert lib.pbhc_linear_act_fwd_out_pair(*_fwd_args(p, o, 1), *bad, L.current_stream()) != 0
    bad = list(_fwd_args(q, r, 1))
    bad[6] = 64                                                        # N != 128
    assert lib.pbhc_linear_act_fwd_out_pair(*bad, *_fwd_args(p, o, 1), L.current_stream()) != 0
    t = torch.zeros(64, 256, device=DEV)
    ok = (t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None, 8, 8, 128, 1)
    for bad in ((t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None, 8, 8, 132, 1),      # K = out_features > 128: not a 32 x 128 launch
                (t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None, None, 8, 6, 128, 1)):     # N % 4 != 0: the register-staged kernel
        assert lib.pbhc_linear_dgrad_act_pair(*ok, *bad, L.current_stream()) != 0
        assert lib.pbhc_linear_dgrad_act_pair(*bad, *ok, L.current_stream()) != 0
    torch.cuda.synchronize()
    # the library's own answer to "does pbhc_linear_dgrad_act run this on 32 x 128 tiles": the rows of pick_shape()'s range, K <= 128, N % 4 == 0
    q = lib.pbhc_linear_dgrad_act_pairable
    assert q(24576, 512, 128) == 1 and q(12288, 256, 128) == 1 and q(8192, 8, 23) == 1 and q(32768, 256, 128) == 1
    assert q(8191, 512, 128) == 0 and q(32769, 512, 128) == 0 and q(24576, 512, 256) == 0 and q(24576, 510, 128) == 0 and q(24576, 512, 3) == 0
    lib.pbhc_gemm_debug_force_shape(2)
    try:
        assert q(24576, 512, 128) == 0                                 # a forced tile shape / diagnosis setting: the single entries alone
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    assert q(24576, 512, 128) == 1


# ---- input gradient of the 128-column layer ----------------------------------------------------------------------------------------------
def _dgrad_problem(seed, M, N, K, act):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dy = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    zpre = torch.randn(M, N, device=DEV, generator=g)
    return dict(dy=dy, w=w, zpre=zpre, saved=_act_ref(act, zpre) if act else None, M=M, N=N, K=K)


def _dgrad_bufs(p):
    MAXB = _L()[0].K["PBHC_ACT_MAX_BLOCKS"]
    return dict(dx=_guard(p["M"] + 3, p["N"]), part=_guard(MAXB * p["N"]), nb=C.c_int(0))


def _dgrad_args(p, o, act):
    return (p["dy"].data_ptr(), p["w"].data_ptr(), _p(p["saved"]), o["dx"].data_ptr(), o["part"].data_ptr(), C.byref(o["nb"]), p["M"], p["N"], p["K"], act)


@pytest.mark.parametrize("act", [1, 3, 0], ids=["elu", "relu", "none"])
@pytest.mark.parametrize("Ms", [(33, 200), (200, 33)])
@pytest.mark.parametrize("Ns", [(256, 512), (8, 132)])
def test_dgrad_pair_equals_two_single_calls_on_32_row_tiles(Ns, Ms, act):
    L, lib = _L()
    ps = [_dgrad_problem(21 + j + Ms[j] + Ns[j], Ms[j], Ns[j], 128, act) for j in (0, 1)]
    single = [_dgrad_bufs(p) for p in ps]
    lib.pbhc_gemm_debug_force_shape(4)
    try:
        for p, o in zip(ps, single):
            L.check(lib.pbhc_linear_dgrad_act(*_dgrad_args(p, o, act), L.current_stream()), "pbhc_linear_dgrad_act")
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    pair = [_dgrad_bufs(p) for p in ps]
    L.check(lib.pbhc_linear_dgrad_act_pair(*_dgrad_args(ps[0], pair[0], act), *_dgrad_args(ps[1], pair[1], act), L.current_stream()), "pbhc_linear_dgrad_act_pair")
    torch.cuda.synchronize()
    for j, p in enumerate(ps):
        assert pair[j]["nb"].value == single[j]["nb"].value == (p["M"] + 31) // 32
        assert torch.equal(pair[j]["dx"], single[j]["dx"]) and torch.equal(pair[j]["part"], single[j]["part"]), j
        assert bool((pair[j]["dx"][p["M"]:] == GUARD).all()) and bool((pair[j]["part"][pair[j]["nb"].value * p["N"]:] == GUARD).all())
        ref = (p["dy"].double() @ p["w"].double()) * (_act_grad_ref(act, p["zpre"].double()) if act else 1.0)
        assert (pair[j]["dx"][:p["M"]].double() - ref).abs().max().item() < TOL


# ---- MHPPO ----------------------------------------------------------------------------------------------------------------------------
STATE = ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step")


def _two_steps(monkeypatch, num_envs, overrides):
    """Two optimiser steps on one minibatch of a walk rollout with PBHC_PAIR_TAILS=1 and =0 from the same state -> per setting
    (flat parameters, Adam moments, learning rates, step counts, the loss scalars of each step, the form each step took, the kinds of the
    paired launches issued)"""
    import bench
    from pbhc_amd.agents import fused_mlp
    from pbhc_amd.agents.mh_ppo import MHPPO
    from tests.helpers import build_hip_env

    paired = []
    issue_pair = fused_mlp._issue_pair
    monkeypatch.setattr(fused_mlp, "_issue_pair", lambda kind, a0, a1: (paired.append(kind), issue_pair(kind, a0, a1))[1])

    torch.manual_seed(7)
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", num_envs, noise_off=False, overrides=overrides)
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
    algo.setup()
    algo._train_mode()
    obs = env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, algo.num_steps_per_env + 2, seed=7))
    algo._rollout_step(obs)
    n = algo.storage.num_envs * algo.storage.num_transitions_per_env
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    batch = next(iter(algo.storage.mini_batch_generator(algo.num_mini_batches, 1, keys=algo.UPDATE_KEYS, indices=perm)))
    batch = {k: v.clone() for k, v in batch.items()}
    start = {k: getattr(algo, k).clone() for k in STATE}
    out = {}
    for setting in ("1", "0"):
        monkeypatch.setenv("PBHC_PAIR_TAILS", setting)
        for k in STATE:
            getattr(algo, k).copy_(start[k])
        algo._gflat.zero_()
        algo._gflat_clean = False
        loss = {k: torch.zeros((), device=DEV) for k in algo.METERS}
        scalars, forms = [], []
        del paired[:]
        for _ in range(2):
            algo._update_ppo(batch, loss)
            scalars.append(algo._loss_scalars.clone())
            forms.append(algo._update_form)
        torch.cuda.synchronize()
        res = {k: getattr(algo, k).clone() for k in STATE}
        res["scalars"] = torch.stack(scalars)
        res["losses"] = torch.stack([loss[k] for k in ("Value", "Surrogate", "Entropy")])
        out[setting] = (res, forms, batch["actor_obs"].shape[0], list(paired))
    assert not torch.equal(out["1"][0]["_pflat"], start["_pflat"])
    return out


def _same(out):
    for k in out["1"][0]:
        assert torch.equal(out["1"][0][k], out["0"][0][k]), k


def test_mhppo_paired_steps_equal_per_stack_steps(monkeypatch):
    """512 envs x 24 steps in one minibatch (12 288 rows: the smallest that reaches the paired path)"""
    out = _two_steps(monkeypatch, 512, {"algo.config.num_mini_batches": 1})
    assert out["1"][2] == 12288
    assert out["1"][1] == ["paired", "paired"] and out["0"][1] == ["per-stack", "per-stack"]
    assert out["1"][3] == ["fwd_out", "dgrad"] * 2 and out["0"][3] == []      # one forward and one input-gradient pair per step, none with the switch off
    _same(out)


def test_small_minibatch_takes_the_per_stack_path(monkeypatch):
    out = _two_steps(monkeypatch, 64, {"algo.config.num_mini_batches": 1})
    assert out["1"][2] == 1536
    assert out["1"][1] == ["per-stack", "per-stack"] and out["1"][3] == []            # no paired launch was issued


def test_narrow_last_hidden_layer_takes_the_per_stack_path(monkeypatch):
    out = _two_steps(monkeypatch, 512, {"algo.config.num_mini_batches": 1, "algo.config.module_dict.actor.layer_config.hidden_dims": [512, 256, 64]})
    assert out["1"][2] == 12288
    assert out["1"][1] == ["per-stack", "per-stack"] and out["1"][3] == []
