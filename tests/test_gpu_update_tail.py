"""The tail of MHPPO's optimiser step: the loss's first stage alone (`pbhc_ppo_loss_partials`) and its second stage as one more workgroup of the
backward's finishing launch (`pbhc_colsum_final_ppo_reduce`, csrc/pbhc_ppo.hip), as MHPPO._update_ppo now runs them.

The first stage is pbhc_ppo_loss's own kernel on the same grid and the second stage keeps that reduce's order of additions (256 threads with four
columns each instead of 1024 with one), so everything is compared bit for bit with `pbhc_ppo_loss`; grad_std, scalars[4] and the learning-rate
rule are held, besides, to the float64 restatement and the error rule of tests/test_gpu_ppo_kernels.py (err <= 4 * err32 + 1e-6) with that file's
helpers, inputs and cases."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_ppo_kernels import (CLIP, DEV, ENTROPY_COEF, LOSS_SHAPES, LR_CASES, VALUE_COEF, _LOSS_KEYS, _check, _guarded, _lib, _loss_inputs, _loss_refs,
                                        _oracle, _rule, _run_loss, _tail_ok)

pytestmark = pytest.mark.gpu


def _run_tail(shape, clipped, kl_form, adapt, desired_kl=0.01, lr=(1e-3, 5e-4), acc=None, jobs_n=(3, 700)):
    """pbhc_ppo_loss_partials, then pbhc_colsum_final_ppo_reduce with len(jobs_n) column-sum jobs of its own (random partial rows); every
    output lies in a sentinel-padded buffer"""
    L, lib = _lib()
    B, A, R = shape
    inp = {k: v.to(DEV) for k, v in _loss_inputs(B, A, R)[0].items()}
    out = dict(grad_mu=_guarded(B * A), grad_value=_guarded(B * R), grad_std=_guarded(A), scalars=_guarded(4), lr=_guarded(2))
    sizes = dict(grad_mu=B * A, grad_value=B * R, grad_std=A, scalars=4, lr=2, acc=4)
    out["lr"][:2] = torch.tensor(lr, dtype=torch.float32)
    if acc is not None:
        out["acc"] = _guarded(4)
        out["acc"][:4] = torch.tensor(acc, dtype=torch.float32)
    scratch = torch.zeros(lib.pbhc_ppo_loss_scratch_floats(B), device=DEV)
    npart = C.c_int(0)
    L.check(lib.pbhc_ppo_loss_partials(*[inp[k].data_ptr() for k in _LOSS_KEYS], B, A, R, CLIP, VALUE_COEF, int(clipped), kl_form - 1, out["grad_mu"].data_ptr(),
                                       out["grad_value"].data_ptr(), scratch.data_ptr(), C.byref(npart), L.current_stream()), "pbhc_ppo_loss_partials")
    assert npart.value == min((B + 7) // 8, 512)
    g = torch.Generator().manual_seed(B + 17)
    jobs = (L.PbhcColsumJob * L.K["PBHC_MAX_COLSUM_JOBS"])()
    parts, sums = [], []
    for j, n in zip(jobs, jobs_n):
        part = torch.randn(37, n, generator=g).to(DEV)
        o = _guarded(n)
        j.part, j.out, j.num_row_blocks, j.n = part.data_ptr(), o.data_ptr(), 37, n
        parts.append(part)
        sums.append(o)
    red = L.PbhcPpoReduce()
    red.scratch, red.std, red.grad_std, red.scalars, red.lr = scratch.data_ptr(), inp["std"].data_ptr(), out["grad_std"].data_ptr(), out["scalars"].data_ptr(), out["lr"].data_ptr()
    red.scalars_acc = out["acc"].data_ptr() if acc is not None else None
    red.num_partials, red.B, red.A, red.adapt_lr, red.entropy_coef, red.desired_kl = npart.value, B, A, adapt, ENTROPY_COEF, float(desired_kl)
    L.check(lib.pbhc_colsum_final_ppo_reduce(jobs, len(jobs_n), C.byref(red), L.current_stream()), "pbhc_colsum_final_ppo_reduce")
    torch.cuda.synchronize()
    for k, buf in out.items():
        assert _tail_ok(buf, sizes[k]), f"{k}: written beyond its {sizes[k]} floats"
    # the launch's own column-sum jobs: what pbhc_colsum_final makes of them
    for part, o, n in zip(parts, sums, jobs_n):
        assert _tail_ok(o, n)
        want = _guarded(n)
        one = (L.PbhcColsumJob * L.K["PBHC_MAX_COLSUM_JOBS"])()
        one[0].part, one[0].out, one[0].num_row_blocks, one[0].n = part.data_ptr(), want.data_ptr(), 37, n
        L.check(lib.pbhc_colsum_final(one, 1, L.current_stream()), "pbhc_colsum_final")
        torch.cuda.synchronize()
        assert torch.equal(o, want)
    return {k: buf[:sizes[k]].cpu() for k, buf in out.items()}


@pytest.mark.parametrize("kl_form", [1, 2])
@pytest.mark.parametrize("clipped", [0, 1])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_tail_equals_ppo_loss_and_matches_fp64_autograd(shape, clipped, kl_form):
    """grad_mu, grad_value, grad_std, scalars[4] and scalars_acc: the bits of pbhc_ppo_loss, and within the bound of
    test_ppo_loss_matches_fp64_autograd of oracle.ppo.losses in float64 under autograd; adapt_lr clear: lr bit-identical"""
    ref64, ref32 = _loss_refs(*shape, clipped, kl_form)
    lr = (1.2345e-3, 6.789e-4)
    old = (3.5, -1.25, 100.0, 0.015625)
    out = _run_tail(shape, clipped, kl_form, 0, lr=lr, acc=old)
    pair = _run_loss(shape, clipped, (kl_form - 1) << 1, lr=lr, acc=old)
    assert torch.equal(out["lr"], torch.tensor(lr, dtype=torch.float32))
    for k in ("grad_mu", "grad_value", "grad_std", "scalars"):
        _check(f"tail {shape} clipped={clipped} kl_form={kl_form} {k}", out[k], ref64[k], ref32[k])
    for k in ("grad_mu", "grad_value", "grad_std", "scalars", "acc"):
        assert torch.equal(out[k], pair[k]), k


def test_tail_reduce_alone_in_its_launch():
    """no column-sum job: the launch is the reduce's one workgroup"""
    shape = (4100, 23, 21)
    out = _run_tail(shape, 1, 1, 0, jobs_n=())
    pair = _run_loss(shape, 1, 0)
    for k in ("grad_std", "scalars"):
        assert torch.equal(out[k], pair[k]), k


@pytest.mark.parametrize("kl_form", [1, 2])
@pytest.mark.parametrize("case", LR_CASES, ids=[c[0] for c in LR_CASES])
@pytest.mark.parametrize("shape", [(13, 32, 32), (4100, 23, 21)])
def test_tail_learning_rate_rule(shape, case, kl_form):
    """the cases of test_ppo_loss_learning_rate_rule: KL mean 4 x, 0.25 x and 1 x desired_kl (one on each side of both thresholds), both
    clamps, each rate from its own value — and the bits of pbhc_ppo_loss"""
    _, kl_over_desired, lr = case
    kl64 = float(_loss_refs(*shape, 1, kl_form)[0]["scalars"][3])
    assert kl64 > 0.0
    desired = kl64 / kl_over_desired
    out = _run_tail(shape, 1, kl_form, 1, desired_kl=desired, lr=lr)
    want = [_rule(float(np.float32(x)), kl64, desired) for x in lr]
    assert want[0] != want[1]
    for i in range(2):
        assert abs(float(out["lr"][i]) - want[i]) <= 1e-6 * want[i], (i, out["lr"], want)
    if "clamp" in case[0]:
        assert float(out["lr"][0 if case[0] == "down_clamp" else 1]) == float(np.float32(1e-5 if case[0] == "down_clamp" else 1e-2))
    if case[0] == "keep":
        assert torch.equal(out["lr"], torch.tensor(lr, dtype=torch.float32))
    pair = _run_loss(shape, 1, ((kl_form - 1) << 1) | 1, desired_kl=desired, lr=lr)
    assert torch.equal(out["lr"], pair["lr"]) and torch.equal(out["scalars"], pair["scalars"])


def test_mhppo_step_equals_the_two_launch_loss_and_captures(monkeypatch):
    """One MHPPO optimiser step at 64 envs x 24 steps from fixed weights and one minibatch: every gradient (std included), the loss scalars and
    the updated flat buffers equal, bit for bit, a step that runs pbhc_ppo_loss (both stages, two launches) before the backward; grad_std and the
    scalars lie within the bound above of float64 autograd on the step's own (mu, value); captured into a graph and replayed, the step equals the
    eager one bit for bit."""
    import bench
    from pbhc_amd import _lib as L
    from pbhc_amd.agents.mh_ppo import MHPPO
    from tests.helpers import build_hip_env

    torch.manual_seed(5)
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 64, noise_off=False)
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
    algo.setup()
    algo._train_mode()
    algo.clip_param, algo.value_loss_coef, algo.entropy_coef = CLIP, VALUE_COEF, ENTROPY_COEF
    obs = env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, algo.num_steps_per_env + 2, seed=5))
    algo._rollout_step(obs)
    n = algo.storage.num_envs * algo.storage.num_transitions_per_env
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    batch = next(iter(algo.storage.mini_batch_generator(algo.num_mini_batches, 1, keys=algo.UPDATE_KEYS, indices=perm)))
    batch = {k: v.clone() for k, v in batch.items()}
    state = ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step")
    start = {k: getattr(algo, k).clone() for k in state}
    na, nc = algo._n_actor, algo._n_critic
    so, sn = algo._std_slice
    seen = {}
    adam = algo._adam2

    def adam_keeping_grads(zero_grad):
        seen["grads"] = algo._gflat[:na + nc].clone()
        adam(zero_grad)

    monkeypatch.setattr(algo, "_adam2", adam_keeping_grads)

    def reset():
        for k in state:
            getattr(algo, k).copy_(start[k])
        algo._gflat.zero_()
        algo._gflat_clean = False

    def result():
        torch.cuda.synchronize()
        out = {k: getattr(algo, k).clone() for k in state}
        out["grads"], out["scalars"] = seen["grads"].clone(), algo._loss_scalars.clone()
        return out

    def step(capture=False):
        reset()
        loss = {k: torch.zeros((), device=DEV) for k in algo.METERS}
        if capture:
            g = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(g, stream=side):
                algo._update_ppo(batch, loss)
            for k in state:                                  # (the capture ran nothing: the replay starts from the same state)
                assert torch.equal(getattr(algo, k), start[k]), k
            g.replay()
        else:
            algo._update_ppo(batch, loss)
        return result()

    def step_with_the_two_launch_loss():
        reset()
        mu = algo.actor.actor_module(batch["actor_obs"])
        value = algo.critic.critic_module(batch["critic_obs"])
        algo._zero_grads()
        B = mu.shape[0]
        L.check(L.lib().pbhc_ppo_loss(mu.data_ptr(), algo.actor.std.data_ptr(), value.data_ptr(), batch["actions"].data_ptr(), batch["actions_log_prob"].data_ptr(),
                                      batch["action_mean"].data_ptr(), batch["action_sigma"].data_ptr(), batch["advantages"].data_ptr(), batch["returns"].data_ptr(),
                                      batch["values"].data_ptr(), B, algo.num_act, algo.num_rew_fn, float(algo.clip_param), float(algo.value_loss_coef),
                                      float(algo.entropy_coef), int(algo.use_clipped_value_loss), float(algo.desired_kl or 0.0),
                                      int(algo.desired_kl is not None and algo.schedule == "adaptive"), algo._grad_mu.data_ptr(), algo._grad_value.data_ptr(),
                                      algo._gflat[so:so + sn].data_ptr(), algo._loss_scalars.data_ptr(), None, algo._lr.data_ptr(), algo._loss_scratch.data_ptr(),
                                      L.current_stream()), "pbhc_ppo_loss")
        algo._backward_both(mu, value, None)
        algo._adam2(zero_grad=1)
        return result(), mu.detach().clone(), value.detach().clone()

    a = step()
    b, mu, value = step_with_the_two_launch_loss()
    assert bool((a["grads"] != 0).any()) and not torch.equal(a["_pflat"], start["_pflat"])
    for k in a:
        assert torch.equal(a[k], b[k]), k
    inp = dict(mu=mu, std=start["_pflat"][so:so + sn].clone(), value=value, actions=batch["actions"], old_logp=batch["actions_log_prob"].reshape(-1),
               old_mu=batch["action_mean"], old_sigma=batch["action_sigma"], adv=batch["advantages"].reshape(-1), returns=batch["returns"], old_values=batch["values"])
    inp = {k: v.detach().cpu() for k, v in inp.items()}
    clipped = int(algo.use_clipped_value_loss)
    ref64, ref32 = _oracle(inp, torch.float64, clipped, 1), _oracle(inp, torch.float32, clipped, 1)
    _check("mhppo step grad_std", a["grads"][so:so + sn], ref64["grad_std"], ref32["grad_std"])
    _check("mhppo step scalars", a["scalars"], ref64["scalars"], ref32["scalars"])
    c = step(capture=True)
    for k in a:
        assert torch.equal(a[k], c[k]), k
