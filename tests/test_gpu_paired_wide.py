"""The paired launch of the WIDE layers' forwards in MHPPO's optimiser step (`pbhc_linear_act_fwd_pair`: two independent problems of
k_gemm2<0, 1, 4, 2, 1, 32, 2> — 64 x 128 tiles — on a shared grid) and the joint driver that issues it (fused_mlp._run_joint,
`PBHC_PAIR_WIDE`).

As in tests/test_gpu_paired_tails.py a pair runs the single entry's tile code on the single entry's tiles, so every comparison with two
single calls is bit for bit (`torch.equal` on every output buffer, guard rows behind each so that a store beyond a problem's rows / columns
shows), and the results are held, besides, to the fp64 bound of tests/test_gpu_gemm.py (3e-5 absolute on O(1) outputs).

How the pair entry sees "both single entries on 64 x 128 tiles": the shapes here are small, and `pick_shape` would send them to 64 x 64
tiles, so the shape is forced with `pbhc_gemm_debug_force_shape(2)` around the single calls AND the pair call — the force is honoured by
`pbhc_linear_act_fwd_pairable`, because it is what the single entry runs.

The same pair for the wide layers' INPUT GRADIENTS was built and held to the same tests (bit for bit, 24 cases), and deleted again because
it measured slower in the update (profiles/update_paired_wide.txt §2, §5): nothing of it is left to test."""
import pytest
import torch

from tests.test_gpu_gemm import TOL, _act_ref
from tests.test_gpu_paired_tails import _ordinary_graph_rng_state  # noqa: F401  (module fixture: see there; this module builds agents too)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = -12345.0
PAD = 3


def _L():
    from pbhc_amd import _lib

    return _lib, _lib.lib()


def _guard(*shape):
    return torch.full(shape, GUARD, device=DEV)


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
def _fwd_problem(seed, M, N, K):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return dict(x=torch.randn(M, K, device=DEV, generator=g), w=torch.randn(N, K, device=DEV, generator=g) / K ** 0.5,
                b=torch.randn(N, device=DEV, generator=g), M=M, N=N, K=K)


def _fwd_bufs(p):
    return dict(y=_guard(p["M"] + PAD, p["N"]), pre=_guard(p["M"] + PAD, p["N"]))


def _fwd_args(p, o, act):
    return (p["x"].data_ptr(), p["w"].data_ptr(), p["b"].data_ptr(), o["y"].data_ptr(), o["pre"].data_ptr() if act == 2 else None, p["M"], p["N"], p["K"], act)


def _fwd_pair_against_singles(ps, act):
    L, lib = _L()
    single, pair = [_fwd_bufs(p) for p in ps], [_fwd_bufs(p) for p in ps]
    lib.pbhc_gemm_debug_force_shape(2)
    try:
        for p in ps:
            assert lib.pbhc_linear_act_fwd_pairable(p["M"], p["N"], p["K"]) == 1
        for p, o in zip(ps, single):
            L.check(lib.pbhc_linear_act_fwd(*_fwd_args(p, o, act), L.current_stream()), "pbhc_linear_act_fwd")
        L.check(lib.pbhc_linear_act_fwd_pair(*_fwd_args(ps[0], pair[0], act), *_fwd_args(ps[1], pair[1], act), L.current_stream()), "pbhc_linear_act_fwd_pair")
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    torch.cuda.synchronize()
    for j, p in enumerate(ps):
        for k in ("y", "pre"):
            assert torch.equal(pair[j][k], single[j][k]), (j, k)
            assert bool((pair[j][k][p["M"]:] == GUARD).all()), (j, k, "rows beyond M")
        z = p["x"].double() @ p["w"].double().t() + p["b"].double()
        err = (pair[j]["y"][:p["M"]].double() - _act_ref(act, z)).abs().max().item()
        assert err < TOL, (j, err)
        if act == 2:
            assert not bool((pair[j]["pre"][:p["M"]] == GUARD).any())
            assert (pair[j]["pre"][:p["M"]].double() - z).abs().max().item() < TOL
        else:
            assert bool((pair[j]["pre"] == GUARD).all())               # ELU / ReLU / none write no pre-activation


@pytest.mark.parametrize("act", [1, 3, 0], ids=["elu", "relu", "none"])
@pytest.mark.parametrize("Ks", [(380, 630), (36, 30)])
@pytest.mark.parametrize("Ns", [(256, 512), (132, 8), (130, 128)])
@pytest.mark.parametrize("Ms", [(1, 1), (65, 200), (200, 65)])
def test_fwd_pair_equals_two_single_calls_on_64_row_tiles(Ms, Ns, Ks, act):
    _fwd_pair_against_singles([_fwd_problem(11 + j + Ms[j] + Ns[j] + Ks[j], Ms[j], Ns[j], Ks[j]) for j in (0, 1)], act)


def test_fwd_pair_with_pre_activation_output():
    """SiLU writes `pre`: the second output image of the same epilogue, paired"""
    _fwd_pair_against_singles([_fwd_problem(5, 65, 132, 36), _fwd_problem(6, 200, 256, 380)], 2)


@pytest.mark.parametrize("M", [512, 200], ids=["8+8_tiles", "4+4_tiles"])
def test_fwd_pair_both_arms_of_the_xcd_remap(M):
    """(M 512, N 128): 8 tiles per problem, the tile order remapped over the XCDs; (M 200, N 128): 4 tiles, not remapped"""
    _fwd_pair_against_singles([_fwd_problem(31 + M, M, 128, 380), _fwd_problem(32 + M, M, 128, 36)], 1)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_fwd_pair_entry_refuses_what_the_single_entry_would_not_run_on_these_tiles():
    L, lib = _L()
    st = L.current_stream()
    q = lib.pbhc_linear_act_fwd_pairable
    # one problem on another shape: (16 384, 130, 4) is 512 tiles of 64 x 128 — pick_shape's own choice; (200, 130, 4) goes to 64 x 64 tiles
    ok, other = _fwd_problem(1, 16384, 130, 4), _fwd_problem(2, 200, 130, 4)
    o_ok, o_other = _fwd_bufs(ok), _fwd_bufs(other)
    assert q(16384, 130, 4) == 1 and q(200, 130, 4) == 0
    assert lib.pbhc_linear_act_fwd_pair(*_fwd_args(ok, o_ok, 1), *_fwd_args(other, o_other, 1), st) != 0
    assert lib.pbhc_linear_act_fwd_pair(*_fwd_args(other, o_other, 1), *_fwd_args(ok, o_ok, 1), st) != 0
    # K < 4: the register-staged kernel
    f_k = _fwd_problem(7, 16384, 130, 3)
    o_k = _fwd_bufs(f_k)
    assert q(16384, 130, 3) == 0
    assert lib.pbhc_linear_act_fwd_pair(*_fwd_args(ok, o_ok, 1), *_fwd_args(f_k, o_k, 1), st) != 0
    assert lib.pbhc_linear_act_fwd_pair(*_fwd_args(f_k, o_k, 1), *_fwd_args(ok, o_ok, 1), st) != 0
    # a diagnosis setting (K-loop ablation flags, staging variant) changes what the single entry runs
    for setting in (0xff | (1 << 8), 2 | (1 << 8), 0xff | (2 << 16)):
        lib.pbhc_gemm_debug_force_shape(setting)
        try:
            assert q(16384, 130, 4) == 0
            assert lib.pbhc_linear_act_fwd_pair(*_fwd_args(ok, o_ok, 1), *_fwd_args(ok, o_ok, 1), st) != 0
        finally:
            lib.pbhc_gemm_debug_force_shape(-1)
    torch.cuda.synchronize()
    for o in (o_ok, o_other, o_k):                                     # a refusal launches nothing
        assert bool((o["y"] == GUARD).all()) and bool((o["pre"] == GUARD).all())
    # the query at the edges of pick_shape's range (the actor's 512 -> 256 forward): 64 x 64 tiles below 512 tiles of 64 x 128
    assert q(12288, 256, 512) == 0 and q(16384, 256, 512) == 1
    assert q(12288, 512, 380) == 1 and q(24576, 768, 630) == 1
    assert q(24576, 128, 256) == 0                                     # the 128-column layer: 32 x 128 tiles
    assert q(0, 256, 512) == 0
    # ... and the input gradient's 32-row query keeps its meaning
    assert lib.pbhc_linear_dgrad_act_pairable(24576, 512, 256) == 0 and lib.pbhc_linear_dgrad_act_pairable(24576, 512, 128) == 1


# ---- MHPPO -----------------------------------------------------------------------------------------------------------------------------
STATE = ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step")


def _two_steps(monkeypatch, num_envs, overrides):
    """Two optimiser steps on one minibatch of a walk rollout with PBHC_PAIR_WIDE=1 and =0 from the same state (the helper pattern of
    tests/test_gpu_paired_tails.py) -> per setting (state and loss scalars, the form each step took, rows, the wide pairs each step recorded,
    the kinds `_issue_pair` — the 32-row pairs — was called with)"""
    import bench
    from pbhc_amd.agents import fused_mlp
    from pbhc_amd.agents.mh_ppo import MHPPO
    from tests.helpers import build_hip_env

    tails = []
    issue_pair = fused_mlp._issue_pair
    monkeypatch.setattr(fused_mlp, "_issue_pair", lambda kind, a0, a1: (tails.append(kind), issue_pair(kind, a0, a1))[1])
    monkeypatch.delenv("PBHC_PAIR_TAILS", raising=False)

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
        monkeypatch.setenv("PBHC_PAIR_WIDE", setting)
        for k in STATE:
            getattr(algo, k).copy_(start[k])
        algo._gflat.zero_()
        algo._gflat_clean = False
        loss = {k: torch.zeros((), device=DEV) for k in algo.METERS}
        scalars, forms, pairs = [], [], []
        del tails[:]
        for _ in range(2):
            algo._update_ppo(batch, loss)
            scalars.append(algo._loss_scalars.clone())
            forms.append(algo._update_form)
            pairs.append(list(algo._update_pairs))
        torch.cuda.synchronize()
        res = {k: getattr(algo, k).clone() for k in STATE}
        res["scalars"] = torch.stack(scalars)
        res["losses"] = torch.stack([loss[k] for k in ("Value", "Surrogate", "Entropy")])
        out[setting] = (res, forms, batch["actor_obs"].shape[0], pairs, list(tails))
    assert not torch.equal(out["1"][0]["_pflat"], start["_pflat"])
    return out


def _check(out, rows, pairs):
    for s in ("1", "0"):
        assert out[s][2] == rows
        assert out[s][1] == ["paired", "paired"]
        assert out[s][4] == ["fwd_out", "dgrad"] * 2                  # the 32-row pairs form with either setting
    assert out["1"][3] == [pairs, pairs] and out["0"][3] == [[], []]
    for k in out["1"][0]:
        assert torch.equal(out["1"][0][k], out["0"][0][k]), k


def test_mhppo_both_wide_forward_pairs_equal_per_stack_launches(monkeypatch):
    """1 024 envs x 16 steps in one minibatch: 16 384 rows, the smallest at which pick_shape sends all four wide forwards to 64 x 128 tiles
    (the actor's 512 -> 256 forward is 512 tiles there)"""
    out = _two_steps(monkeypatch, 1024, {"algo.config.num_mini_batches": 1, "algo.config.num_steps_per_env": 16})
    _check(out, 16384, ["fwd", "fwd"])


def test_mhppo_mixed_wide_pairs_at_12288_rows(monkeypatch):
    """512 envs x 24 steps: the L1 forwards pair; the actor's L2 forward runs on 64 x 64 tiles, so the L2 forwards go through their own
    entries"""
    out = _two_steps(monkeypatch, 512, {"algo.config.num_mini_batches": 1})
    _check(out, 12288, ["fwd"])
