"""The small kernels that decide what the optimiser does — `pbhc_ppo_loss`, `pbhc_kl_lr_rule`, `pbhc_adam_clip` / `pbhc_adam_clip2` (csrc/pbhc_ppo.hip),
`pbhc_gae` (csrc/pbhc_kernels.hip), `pbhc_policy_sample`, `pbhc_rollout_post` / `pbhc_rollout_post2` — through the C ABI against float64 references
of the same operation: `oracle.ppo.losses` under autograd (the function tests/test_oracle_ppo*.py pin against the reference project's goldens),
`clip_grad_norm_` + `torch.optim.Adam` / `AdamW`, `oracle.ppo.compute_returns`, and the host Philox model of tests/helpers.py.

Error rule.  For an output tensor x with float64 reference r:  err = max |x - r| / (|r| + mean |r|); the yardstick err32 is the SAME reference
function evaluated by torch in float32 on the same inputs; the kernel must satisfy  err <= 4 * err32 + 1e-6  (4: another summation order and
another expf / logf; 1e-6 = 8 fp32 ulp, for the tiny shapes where err32 is 0).  The loss's `scalars[4]` is one such tensor.  A reference that is
all zeros demands an output that is all zeros.  Every test prints `err / err32` per output before it asserts.

Measured on an MI355X (max over the flag combinations of a shape; `err / err32`, and err where err32 is 0):
  pbhc_ppo_loss (B, A, R)     grad_mu   grad_value   grad_std   scalars
    (1, 1, 1)                 exact 0   1.00         1.00       2.04
    (5, 23, 21)               0.60      0.82         0.47       1.06
    (13, 32, 32)              0.99      1.67         1.09       1.01
    (4096, 23, 21)            0.77      1.00         0.88       2.65
    (4100, 23, 21)            0.64      1.06         1.23       1.14
    (12300, 29, 1)            0.97      1.26         0.51       0.48
    (12300, 23, 21)           0.94      1.33         1.01       0.61
  pbhc_adam_clip n            param     exp_avg      exp_avg_sq norm      grad
    1                         1.00      1.00         1.00       exact     1.00
    3                         1.98      3.17         1.63       1.00      1.00     (err 2e-8: all below the 1e-6 floor)
    5                         3.28      0.30         0.79       1.00      1.00     (likewise)
    1027                      1.50      0.95         0.63       1.00      0.43
    1048576 + 4099            1.04      0.01         0.01       0.00      0.01     (torch's float32 norm is off by 7e-6 here)
  pbhc_adam_clip2 (n0, n1)
    (1, 1)                    1.00      1.00         1.00       exact     1.00
    (3, 5)                    1.98      3.17         1.63       1.00      1.00
    (1027, 4098)              1.50      1.08         1.00       1.00      0.51
    (1048576 + 5, 300001)     1.20      1.11         1.00       0.03      0.03
  pbhc_gae (T, N, R)          returns   advantages
    (1, 1, 1)                 exact     NaN, as torch.std of one element
    (1, 300, 21)              1.00      1.20
    (24, 13, 21)              1.00      0.85
    (24, 130, 1)              1.00      1.00
    (7, 37, 32)               1.00      0.89
    (24, 4096, 21)            1.00      0.96
  pbhc_policy_sample (N, A, R)  logp    max |z - z_philox| (bound 2e-5)
    (1, 1, 1)                 1.18      3e-8
    (13, 32, 32)              1.32      1.1e-6
    (4099, 23, 21)            0.82      9.5e-6
Neutralised share of the loss inputs (asserted <= 1 % each): rows 0 / 0 / 0 / 0.024 / 0.024 / 0.016 / 0.024 %, value elements 0 / 0.95 (one of 105) /
0.24 / 0.15 / 0.11 / 0.09 / 0.14 %, in the order of the shapes above; 15 - 20 % of the rows lie inside the clip range, 38 - 41 % of the value elements
outside +- clip.
"""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest
import torch

from oracle import ppo
from tests import helpers

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -777.25                     # sentinel behind every output: exactly representable, never produced
PAD = 67                           # sentinel floats behind an output
CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 0.7, 0.01
MARGIN = 1e-4                      # ~100 x the fp32 rounding of an O(1) ratio through expf of a 32-term sum


def _lib():
    from pbhc_amd import _lib as L

    return L, L.lib()


def _err(x, ref):
    x, ref = x.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert x.shape == ref.shape
    if not ref.any():
        return 0.0 if not x.any() else math.inf
    return ((x - ref).abs() / (ref.abs() + ref.abs().mean())).max().item()


def _check(name, x, ref64, ref32):
    e, e32 = _err(x, ref64), _err(ref32, ref64)
    print(f"ERR {name}: err {e:.3e} err32 {e32:.3e} err/err32 {e / e32 if e32 > 0 else float('nan'):.3f}")
    assert e <= 4.0 * e32 + 1e-6, (name, e, e32)


def _sent(t):
    return SENT if t.dtype.is_floating_point else 0xA5


def _guarded(n, dtype=torch.float32, pad=PAD):
    """device buffer of n elements followed by `pad` sentinels, all pre-filled with the sentinel"""
    t = torch.empty(n + pad, dtype=dtype, device=DEV)
    return t.fill_(_sent(t))


def _tail_ok(buf, n=0):
    return bool((buf[n:] == _sent(buf)).all())


# ================================================================================================================================================
#  1. pbhc_ppo_loss
# ================================================================================================================================================
LOSS_SHAPES = [(1, 1, 1), (5, 23, 21), (13, 32, 32), (4096, 23, 21), (4100, 23, 21), (12300, 29, 1), (12300, 23, 21)]
_LOSS_KEYS = ("mu", "std", "value", "actions", "old_logp", "old_mu", "old_sigma", "adv", "returns", "old_values")


def _oracle(inp, dtype, clipped, kl_form):
    """oracle.ppo.losses under autograd on mu, std and value -> the kernel's outputs"""
    t = {k: v.to(dtype) for k, v in inp.items()}
    mu, std, value = (t[k].clone().requires_grad_(True) for k in ("mu", "std", "value"))
    cfg = types.SimpleNamespace(clip_param=CLIP, value_loss_coef=VALUE_COEF, entropy_coef=ENTROPY_COEF, use_clipped_value_loss=bool(clipped))
    b = dict(actions=t["actions"], actions_log_prob=t["old_logp"].unsqueeze(-1), action_mean=t["old_mu"], action_sigma=t["old_sigma"],
             advantages=t["adv"].unsqueeze(-1), values=t["old_values"], returns=t["returns"])
    actor_loss, critic_loss, scalars = ppo.losses(mu, mu * 0.0 + std, value, b, cfg, kl_form)
    actor_loss.backward()
    critic_loss.backward()
    return dict(grad_mu=mu.grad, grad_value=value.grad, grad_std=std.grad, scalars=torch.stack([s.detach() for s in scalars]))


@functools.lru_cache(maxsize=None)
def _loss_inputs(B, A, R):
    """the recipe of the module's issue, float64 -> float32, then the branch points neutralised from ONE float64 evaluation.
    Returns (inputs (float32, CPU), share of neutralised rows, share of neutralised value elements)."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * A + R)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    std = 0.3 + 0.9 * torch.rand(A, generator=g, dtype=torch.float64)
    old_sigma = (std * (1.0 + 0.1 * rn(B, A))).clamp(min=0.05)
    old_mu = rn(B, A)
    mu = old_mu + 0.1 * std * rn(B, A)
    actions = old_mu + old_sigma * rn(B, A)
    old_logp = ppo.gaussian_log_prob(actions, old_mu, old_sigma)
    adv = rn(B)
    adv[::7] = 0.0
    old_values = rn(B, R)
    value = old_values + 0.3 * rn(B, R)
    value[::5] = old_values[::5]
    returns = old_values + 0.5 * rn(B, R)
    loc = dict(locals())
    inp = {k: loc[k].float() for k in _LOSS_KEYS}
    d = {k: v.double() for k, v in inp.items()}
    ratio = torch.exp(ppo.gaussian_log_prob(d["actions"], d["mu"], d["mu"] * 0.0 + d["std"]) - d["old_logp"])
    rows = ((ratio - (1.0 - CLIP)).abs() < MARGIN) | ((ratio - (1.0 + CLIP)).abs() < MARGIN)
    dv = d["value"] - d["old_values"]
    l1 = (d["value"] - d["returns"]).pow(2)
    l2 = (d["old_values"] + dv.clamp(-CLIP, CLIP) - d["returns"]).pow(2)
    elems = ((dv.abs() - CLIP).abs() < MARGIN) | ((dv.abs() > CLIP) & ((l1 - l2).abs() < MARGIN))
    inp["adv"][rows] = 0.0
    inp["value"][elems] = inp["old_values"][elems]
    stats = dict(in_clip=float(((ratio >= 1.0 - CLIP) & (ratio <= 1.0 + CLIP)).double().mean()), value_out=float((dv.abs() > CLIP).double().mean()))
    return inp, float(rows.double().mean()), float(elems.double().mean()), stats


@functools.lru_cache(maxsize=None)
def _loss_refs(B, A, R, clipped, kl_form):
    inp = _loss_inputs(B, A, R)[0]
    return _oracle(inp, torch.float64, clipped, kl_form), _oracle(inp, torch.float32, clipped, kl_form)


def _run_loss(shape, clipped, adapt_lr, desired_kl=0.01, lr=(1e-3, 5e-4), acc=None, calls=1):
    """one (or `calls`) pbhc_ppo_loss launch on the shape's inputs; every output lies in a sentinel-padded buffer"""
    L, lib = _lib()
    B, A, R = shape
    inp = {k: v.to(DEV) for k, v in _loss_inputs(B, A, R)[0].items()}
    out = dict(grad_mu=_guarded(B * A), grad_value=_guarded(B * R), grad_std=_guarded(A), scalars=_guarded(4), lr=_guarded(2))
    out["lr"][:2] = torch.tensor(lr, dtype=torch.float32)
    if acc is not None:
        out["acc"] = _guarded(4)
        out["acc"][:4] = torch.tensor(acc, dtype=torch.float32)
    scratch = torch.zeros(lib.pbhc_ppo_loss_scratch_floats(B), device=DEV)
    for _ in range(calls):
        L.check(lib.pbhc_ppo_loss(*[inp[k].data_ptr() for k in _LOSS_KEYS], B, A, R, CLIP, VALUE_COEF, ENTROPY_COEF, int(clipped), float(desired_kl), adapt_lr,
                                  out["grad_mu"].data_ptr(), out["grad_value"].data_ptr(), out["grad_std"].data_ptr(), out["scalars"].data_ptr(),
                                  out["acc"].data_ptr() if acc is not None else None, out["lr"].data_ptr(), scratch.data_ptr(), L.current_stream()), "pbhc_ppo_loss")
    torch.cuda.synchronize()
    sizes = dict(grad_mu=B * A, grad_value=B * R, grad_std=A, scalars=4, lr=2, acc=4)
    for k, buf in out.items():
        assert _tail_ok(buf, sizes[k]), f"{k}: written beyond its {sizes[k]} floats"
    return {k: buf[:sizes[k]].cpu() for k, buf in out.items()}


@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_ppo_loss_inputs_keep_the_branch_points_rare(shape):
    """the neutralised share (rows within 1e-4 of ratio = 1 +- clip; value elements within 1e-4 of |dv| = clip or of l1 = l2 out of range) is a
    condition on the inputs: at most 1 % each (measured: the table at the top of this file)"""
    _, rows, elems, stats = _loss_inputs(*shape)
    print(f"NEUTRALISED {shape}: rows {100 * rows:.4f} % elements {100 * elems:.4f} %  (in clip range {100 * stats['in_clip']:.1f} %, |dv| > clip {100 * stats['value_out']:.1f} %)")
    assert rows <= 0.01 and elems <= 0.01


@pytest.mark.parametrize("kl_form", [1, 2])
@pytest.mark.parametrize("clipped", [0, 1])
@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_ppo_loss_matches_fp64_autograd(shape, clipped, kl_form):
    """grad_mu, grad_value, grad_std and scalars[4] against oracle.ppo.losses in float64 under autograd; adapt_lr bit 0 clear: lr bit-identical;
    scalars_acc NULL; nothing written beyond B*A, B*R, A, 4 floats."""
    ref64, ref32 = _loss_refs(*shape, clipped, kl_form)
    lr = (1.2345e-3, 6.789e-4)
    out = _run_loss(shape, clipped, (kl_form - 1) << 1, lr=lr)
    assert torch.equal(out["lr"], torch.tensor(lr, dtype=torch.float32))
    for k in ("grad_mu", "grad_value", "grad_std", "scalars"):
        _check(f"loss {shape} clipped={clipped} kl_form={kl_form} {k}", out[k], ref64[k], ref32[k])


@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_ppo_loss_scalars_acc_accumulates(shape):
    """scalars_acc[i] += scalars[i]: two calls into a buffer of known non-zero values give old + 2 * scalars.  The kernel adds in fp32: two
    roundings, each at most 2^-24 of a partial sum no larger than |old| + 2 |s|."""
    old = (3.5, -1.25, 100.0, 0.015625)
    out = _run_loss(shape, 1, 0, acc=old, calls=2)
    ref64 = _loss_refs(*shape, 1, 1)[0]
    s, acc, o = out["scalars"].double(), out["acc"].double(), torch.tensor(old, dtype=torch.float64)
    assert ((acc - (o + 2.0 * s)).abs() <= 2.0 * 2.0 ** -24 * (o.abs() + 2.0 * s.abs())).all(), (acc, o + 2.0 * s)
    _check(f"loss {shape} scalars after two calls", out["scalars"], ref64["scalars"], _loss_refs(*shape, 1, 1)[1]["scalars"])


def _rule(lr, kl, desired):
    if kl > desired * 2.0:
        return max(1e-5, lr / 1.5)
    if kl < desired / 2.0 and kl > 0.0:
        return min(1e-2, lr * 1.5)
    return lr


LR_CASES = [("down", 4.0, (1e-3, 5e-4)), ("up", 0.25, (1e-3, 5e-4)), ("keep", 1.0, (1e-3, 5e-4)),
            ("down_clamp", 4.0, (1.2e-5, 8e-3)), ("up_clamp", 0.25, (1.2e-5, 8e-3))]


@pytest.mark.parametrize("kl_form", [1, 2])
@pytest.mark.parametrize("case", LR_CASES, ids=[c[0] for c in LR_CASES])
@pytest.mark.parametrize("shape", [(13, 32, 32), (4100, 23, 21)])
def test_ppo_loss_learning_rate_rule(shape, case, kl_form):
    """adapt_lr bit 0: lr[0] and lr[1] each from its own value — KL mean 4 x, 0.25 x and 1 x desired_kl (far from the 2 x and 0.5 x thresholds),
    both clamps — and pbhc_kl_lr_rule on the kernel's own KL mean gives the same bits."""
    L, lib = _lib()
    _, kl_over_desired, lr = case
    kl64 = float(_loss_refs(*shape, 1, kl_form)[0]["scalars"][3])
    assert kl64 > 0.0
    desired = kl64 / kl_over_desired
    out = _run_loss(shape, 1, ((kl_form - 1) << 1) | 1, desired_kl=desired, lr=lr)
    want = [_rule(float(np.float32(x)), kl64, desired) for x in lr]
    assert want[0] != want[1]
    for i in range(2):
        assert abs(float(out["lr"][i]) - want[i]) <= 1e-6 * want[i], (i, out["lr"], want)
    if "clamp" in case[0]:
        assert float(out["lr"][0 if case[0] == "down_clamp" else 1]) == float(np.float32(1e-5 if case[0] == "down_clamp" else 1e-2))
    if case[0] == "keep":
        assert torch.equal(out["lr"], torch.tensor(lr, dtype=torch.float32))
    lr2 = _guarded(2)
    lr2[:2] = torch.tensor(lr, dtype=torch.float32)
    kl_dev = out["scalars"][3:4].to(DEV)
    L.check(lib.pbhc_kl_lr_rule(lr2.data_ptr(), 2, kl_dev.data_ptr(), float(desired), L.current_stream()), "pbhc_kl_lr_rule")
    torch.cuda.synchronize()
    assert torch.equal(lr2[:2].cpu(), out["lr"]) and _tail_ok(lr2, 2)


@pytest.mark.parametrize("n", [1, 2, 64])
def test_kl_lr_rule(n):
    """pbhc_kl_lr_rule on n rates: the three branches, both clamps, a KL mean of exactly 0 and a negative one (both leave lr unchanged), and a
    sentinel behind lr[n-1]."""
    L, lib = _lib()
    desired = 0.01
    start = torch.tensor(([1.2e-5, 8e-3, 1e-3, 5e-4] * 16)[:n], dtype=torch.float32)
    for kl in (0.04, 0.0025, 0.01, 0.0, -0.003):
        lr = _guarded(n)
        lr[:n] = start
        klt = torch.tensor([kl], dtype=torch.float32, device=DEV)
        L.check(lib.pbhc_kl_lr_rule(lr.data_ptr(), n, klt.data_ptr(), desired, L.current_stream()), "pbhc_kl_lr_rule")
        torch.cuda.synchronize()
        got = lr[:n].cpu()
        assert _tail_ok(lr, n)
        if kl in (0.01, 0.0, -0.003):
            assert torch.equal(got, start), kl
        else:
            want = torch.tensor([_rule(float(x), kl, desired) for x in start], dtype=torch.float64)
            assert ((got.double() - want).abs() <= 1e-6 * want).all(), (kl, got, want)
            assert float(got[0]) == float(np.float32(1e-5)) if kl == 0.04 else n < 2 or float(got[1]) == float(np.float32(1e-2))
    assert lib.pbhc_kl_lr_rule(lr.data_ptr(), 0, klt.data_ptr(), desired, None) == L.K["PBHC_EINVAL"]
    assert lib.pbhc_kl_lr_rule(lr.data_ptr(), 65, klt.data_ptr(), desired, None) == L.K["PBHC_EINVAL"]


@pytest.mark.parametrize("bad", [(13, 33, 21), (13, 23, 0), (0, 23, 21)], ids=["A33", "R0", "B0"])
def test_ppo_loss_rejects_bad_sizes_and_launches_nothing(bad):
    L, lib = _lib()
    B, A, R = bad
    inp = {k: torch.zeros(13 * 33, device=DEV) + 0.5 for k in _LOSS_KEYS}
    outs = [_guarded(13 * 33, pad=0) for _ in range(6)]
    scratch = torch.zeros(lib.pbhc_ppo_loss_scratch_floats(16), device=DEV)
    rc = lib.pbhc_ppo_loss(*[inp[k].data_ptr() for k in _LOSS_KEYS], B, A, R, CLIP, VALUE_COEF, ENTROPY_COEF, 1, 0.01, 1, *[o.data_ptr() for o in outs], scratch.data_ptr(),
                           L.current_stream())
    torch.cuda.synchronize()
    assert rc == L.K["PBHC_EINVAL"]
    assert all(bool((o == SENT).all()) for o in outs) and not scratch.any()


# ================================================================================================================================================
#  2. pbhc_adam_clip / pbhc_adam_clip2
# ================================================================================================================================================
# The entries take their hyper-parameters as C floats and the learning rate as a device float: the references run at exactly those values (the
# float32 roundings of 0.9, 0.999, 1e-8, 0.01, 1e-2 and 3e-3 as doubles), like every other input.  At the decimal 0.999 instead, exp_avg_sq differs
# by 1.3e-5 relative — 1 - float32(0.999) is 0.99998713e-3 — which is the rounding of the argument, not of the kernel's arithmetic.
_f32 = lambda x: float(np.float32(x))
MAX_NORM, B1, B2, EPS = 1.0, _f32(0.9), _f32(0.999), _f32(1e-8)
WEIGHT_DECAYS = [0.0, _f32(0.01)]
ADAM_STEPS = 3
SEG_LR, SEG_STEP0 = (_f32(1e-2), _f32(3e-3)), (0, 3)
# gradient norms per step, per segment: on opposite sides of max_norm in every launch, and each segment on both sides over the steps
SEG_NORMS = ((3.0, 0.3), (0.5, 2.0), (3.0, 0.3))


@functools.lru_cache(maxsize=4)
def _adam_data(n, k):
    """segment k's start state (float32 values) and its three gradients"""
    g = torch.Generator().manual_seed(77 * n + k)
    p = torch.randn(n, generator=g)
    if SEG_STEP0[k]:
        m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g) + 1e-4
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    grads = []
    for it in range(ADAM_STEPS):
        gr = torch.randn(n, generator=g).double()
        if float(gr.norm()) == 0.0:
            gr += 1.0
        grads.append((gr * (SEG_NORMS[it][k] / gr.norm())).float())
    return p, m, v, grads


def _adam_reference(n, k, wd, dtype):
    """clip_grad_norm_ + torch.optim.Adam / AdamW on one segment -> per step (param, exp_avg, exp_avg_sq, clipped grad, norm)"""
    p0, m0, v0, grads = _adam_data(n, k)
    p = torch.nn.Parameter(p0.to(dtype).clone())
    kw = dict(lr=SEG_LR[k], betas=(B1, B2), eps=EPS)
    opt = torch.optim.AdamW([p], weight_decay=wd, **kw) if wd else torch.optim.Adam([p], **kw)
    opt.state[p] = {"step": torch.tensor(float(SEG_STEP0[k])), "exp_avg": m0.to(dtype).clone(), "exp_avg_sq": v0.to(dtype).clone()}
    out = []
    for gr in grads:
        p.grad = gr.to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_([p], MAX_NORM)
        opt.step()
        st = opt.state[p]
        out.append(dict(param=p.detach().clone(), exp_avg=st["exp_avg"].clone(), exp_avg_sq=st["exp_avg_sq"].clone(), grad=p.grad.clone(), norm=norm.detach().reshape(1).clone()))
    assert float(opt.state[p]["step"]) == SEG_STEP0[k] + ADAM_STEPS
    return out


class _Flat:
    """the four flat buffers of n floats, each with sentinels behind it, plus lr / step / norm / scratch"""

    def __init__(self, segs):
        self.n = sum(n for n, _ in segs)
        self.buf = {k: _guarded(self.n) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
        o = 0
        for n, k in segs:
            p, m, v, _ = _adam_data(n, k)
            self.buf["param"][o:o + n], self.buf["exp_avg"][o:o + n], self.buf["exp_avg_sq"][o:o + n] = p, m, v
            o += n
        self.lr = torch.tensor([SEG_LR[k] for _, k in segs], device=DEV)
        self.step = torch.tensor([float(SEG_STEP0[k]) for _, k in segs], device=DEV)
        self.norm = _guarded(len(segs))
        self.scratch = torch.zeros(512 * len(segs), dtype=torch.float64, device=DEV)

    def ptrs(self, off=0):
        return [self.buf[k][off:].data_ptr() for k in ("param", "grad", "exp_avg", "exp_avg_sq")]

    def tails_ok(self):
        return all(_tail_ok(b, self.n) for b in self.buf.values())


def _compare_segment(tag, f, off, n, idx, ref64, ref32, zero_grad):
    for key in ("param", "exp_avg", "exp_avg_sq"):
        _check(f"{tag} {key}", f.buf[key][off:off + n], ref64[key], ref32[key])
    _check(f"{tag} norm", f.norm[idx:idx + 1], ref64["norm"], ref32["norm"])
    if zero_grad:
        assert not f.buf["grad"][off:off + n].view(torch.int32).any(), f"{tag}: grad not zeroed bit for bit"
    else:
        _check(f"{tag} grad", f.buf["grad"][off:off + n], ref64["grad"], ref32["grad"])


@pytest.mark.parametrize("wd", WEIGHT_DECAYS, ids=["adam", "adamw"])
@pytest.mark.parametrize("n", [1, 3, 5, 1027, 1_048_576 + 4099])
def test_adam_clip_single_segment(n, wd):
    """the scalar tail alone (n < 4), a tail behind vector quads, and both kernels grid-striding with a tail (n above 512 x 2048 and 1024 x 1024)"""
    L, lib = _lib()
    ref64, ref32 = _adam_reference(n, 0, wd, torch.float64), _adam_reference(n, 0, wd, torch.float32)
    f = _Flat([(n, 0)])
    for it in range(ADAM_STEPS):
        f.buf["grad"][:n] = _adam_data(n, 0)[3][it]
        L.check(lib.pbhc_adam_clip(*f.ptrs(), n, f.lr.data_ptr(), f.step.data_ptr(), MAX_NORM, B1, B2, EPS, wd, f.scratch.data_ptr(), f.norm.data_ptr(), L.current_stream()),
                "pbhc_adam_clip")
        torch.cuda.synchronize()
        _compare_segment(f"adam n={n} wd={wd} step {it}", f, 0, n, 0, ref64[it], ref32[it], 0)
        assert float(f.step[0]) == it + 1 and f.tails_ok() and _tail_ok(f.norm, 1)


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("wd", WEIGHT_DECAYS, ids=["adam", "adamw"])
@pytest.mark.parametrize("sizes", [(1, 1), (3, 5), (1027, 4098), (1_048_576 + 5, 300_001)])
def test_adam_clip2_two_segments(sizes, wd, zero_grad):
    """two segments in one launch pair, the second only 4-byte aligned (n0 odd): their own learning rates, step counts (0 and 3) and norms — one
    clipped, one not, in every launch; each against its float64 torch optimiser, and bit-identical to two pbhc_adam_clip calls on the halves."""
    L, lib = _lib()
    n0, n1 = sizes
    segs = [(n0, 0), (n1, 1)]
    refs = [(_adam_reference(n, k, wd, torch.float64), _adam_reference(n, k, wd, torch.float32)) for n, k in segs]
    f, h = _Flat(segs), _Flat(segs)
    for it in range(ADAM_STEPS):
        gr = torch.cat([_adam_data(n, k)[3][it] for n, k in segs])
        f.buf["grad"][:n0 + n1] = gr
        h.buf["grad"][:n0 + n1] = gr
        L.check(lib.pbhc_adam_clip2(*f.ptrs(), n0, n1, f.lr.data_ptr(), f.step.data_ptr(), MAX_NORM, B1, B2, EPS, wd, zero_grad, f.scratch.data_ptr(), f.norm.data_ptr(),
                                    L.current_stream()), "pbhc_adam_clip2")
        for idx, (off, n) in enumerate(((0, n0), (n0, n1))):
            L.check(lib.pbhc_adam_clip(*h.ptrs(off), n, h.lr[idx:].data_ptr(), h.step[idx:].data_ptr(), MAX_NORM, B1, B2, EPS, wd, h.scratch[512 * idx:].data_ptr(),
                                       h.norm[idx:].data_ptr(), L.current_stream()), "pbhc_adam_clip")
        torch.cuda.synchronize()
        for idx, (off, n) in enumerate(((0, n0), (n0, n1))):
            _compare_segment(f"adam2 {sizes} wd={wd} zero_grad={zero_grad} step {it} segment {idx}", f, off, n, idx, refs[idx][0][it], refs[idx][1][it], zero_grad)
            want_clipped = SEG_NORMS[it][idx] > MAX_NORM
            got_norm = float(f.norm[idx])
            assert (got_norm > MAX_NORM) == want_clipped
        assert f.step.tolist() == [SEG_STEP0[0] + it + 1.0, SEG_STEP0[1] + it + 1.0]
        for key in ("param", "exp_avg", "exp_avg_sq") + (() if zero_grad else ("grad",)):
            assert torch.equal(f.buf[key], h.buf[key]), f"{key}: clip2 differs from two pbhc_adam_clip calls"
        assert torch.equal(f.norm, h.norm) and torch.equal(f.step, h.step)
        assert f.tails_ok() and h.tails_ok() and _tail_ok(f.norm, 2)


# ================================================================================================================================================
#  3. pbhc_gae
# ================================================================================================================================================
GAE_SHAPES = [(1, 1, 1), (1, 300, 21), (24, 13, 21), (24, 130, 1), (7, 37, 32), (24, 4096, 21)]
GAMMA, LAM = 0.99, 0.95


@pytest.mark.parametrize("shape", GAE_SHAPES)
def test_gae_matches_fp64(shape):
    """returns, normalised advantages and the moments behind the block partials (stats[2 nb], stats[2 nb + 1]) against oracle.ppo.compute_returns in
    float64.  dones: 10 % random, an env done at every step, one never done, one done at the last step; encoded as the bytes 1 and 255."""
    L, lib = _lib()
    T, N, R = shape
    g = torch.Generator().manual_seed(31 * T + 7 * N + R)
    rewards, values, last = torch.randn(T, N, R, generator=g), torch.randn(T, N, R, generator=g), torch.randn(N, R, generator=g)
    done = torch.rand(T, N, generator=g) < 0.1
    done[:, 0] = True
    if N > 1:
        done[:, 1] = False
    if N > 2:
        done[T - 1, 2] = True
    d8 = torch.where(done, torch.where(torch.rand(T, N, generator=g) < 0.5, 1, 255), 0).to(torch.uint8)
    assert set(d8.unique().tolist()) <= {0, 1, 255} and (T * N < 100 or {1, 255} <= set(d8.unique().tolist()))
    nb = (T * N + 255) // 256
    ret, adv = _guarded(T * N * R), _guarded(T * N)
    stats = _guarded(2 * nb + 2, dtype=torch.float64)
    dev = [t.to(DEV) for t in (rewards, values, d8, last)]
    L.check(lib.pbhc_gae(*[t.data_ptr() for t in dev], T, N, R, GAMMA, LAM, ret.data_ptr(), adv.data_ptr(), stats.data_ptr(), L.current_stream()), "pbhc_gae")
    torch.cuda.synchronize()
    assert _tail_ok(ret, T * N * R) and _tail_ok(adv, T * N) and _tail_ok(stats, 2 * nb + 2)
    ref = {}
    for dt in (torch.float64, torch.float32):
        r, a = ppo.compute_returns(rewards.to(dt), values.to(dt), done.unsqueeze(-1), last.to(dt), GAMMA, LAM)
        ref[dt] = (r, a.squeeze(-1))
    r64 = ref[torch.float64][0]
    tot = (r64 - values.double()).sum(-1)
    _check(f"gae {shape} returns", ret[:T * N * R].view(T, N, R), r64, ref[torch.float32][0])
    mean, sd = float(stats[2 * nb]), float(stats[2 * nb + 1])
    assert abs(mean - float(tot.mean())) <= 1e-6 * max(abs(float(tot.mean())), float(tot.abs().mean()))
    if T * N == 1:
        assert math.isnan(sd) and torch.isnan(adv[:1]).all() and torch.isnan(ref[torch.float64][1]).all()      # torch.std of one element
        return
    assert abs(sd - float(tot.std())) <= 1e-6 * float(tot.std())
    _check(f"gae {shape} advantages", adv[:T * N].view(T, N), ref[torch.float64][1], ref[torch.float32][1])


# ================================================================================================================================================
#  4. pbhc_policy_sample, pbhc_rollout_post, pbhc_rollout_post2
# ================================================================================================================================================
SEED = 0x9E3779B97F4A7C15          # both 32-bit halves non-zero


@pytest.mark.parametrize("counter", [7, 2 ** 24 + 3])
@pytest.mark.parametrize("shape", [(1, 1, 1), (13, 32, 32), (4099, 23, 21)])
def test_policy_sample_draws_are_the_philox_model(shape, counter):
    """every draw against the host Philox model — key (seed lo, seed hi), counter words (row, uint32(counter[0]), 0x5A4D, lane), u1 = ((o0 >> 8) + 0.5)
    / 2^24, u2 = (o1 >> 8) / 2^24, Box-Muller in float64.  z = (action - mu) / std within 2e-5: sqrt(-2 ln u1) <= 5.9 and the fp32 rounding of
    2 pi u2 moves cosf's argument by up to 4e-7 (~5e-7 with cosf's own few ulp): 6e-6, times 3."""
    L, lib = _lib()
    N, A, R = shape
    g = torch.Generator().manual_seed(N + A + R)
    mu, std, value = torch.randn(N, A, generator=g), 0.3 + 0.9 * torch.rand(A, generator=g), torch.randn(N, R, generator=g)
    ctr = torch.tensor([float(counter)], dtype=torch.float64, device=DEV)
    mu_d, std_d, value_d = mu.to(DEV), std.to(DEV), value.to(DEV)
    rows = N + 3                                                    # sentinel rows behind row N-1
    for with_value in (True, False):
        act, am, asg = (torch.full((rows, A), SENT, device=DEV) for _ in range(3))
        lp, vout = torch.full((rows,), SENT, device=DEV), torch.full((rows, R), SENT, device=DEV)
        L.check(lib.pbhc_policy_sample(mu_d.data_ptr(), std_d.data_ptr(), value_d.data_ptr() if with_value else None, N, A, R, SEED, ctr.data_ptr(), act.data_ptr(),
                                       am.data_ptr(), asg.data_ptr(), lp.data_ptr(), vout.data_ptr() if with_value else None, L.current_stream()), "pbhc_policy_sample")
        torch.cuda.synchronize()
        for t in (act, am, asg, lp, vout):
            assert bool((t[N:] == SENT).all())
        assert torch.equal(am[:N].cpu(), mu) and torch.equal(asg[:N].cpu(), std.expand(N, A))
        assert torch.equal(vout[:N].cpu(), value) if with_value else bool((vout == SENT).all())
        o = helpers._philox4x32_7(SEED, np.arange(N)[:, None], counter & 0xFFFFFFFF, 0x5A4D, np.arange(A)[None, :])
        u1 = ((o[0] >> np.uint64(8)).astype(np.float64) + 0.5) / 2.0 ** 24
        u2 = (o[1] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        z_want = torch.from_numpy(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
        z = (act[:N].cpu().double() - mu.double()) / std.double()
        dz = (z - z_want).abs().max().item()
        print(f"ERR sample {shape} counter={counter}: max |z - z_philox| {dz:.3e}")
        assert dz <= 2e-5
        a64 = act[:N].cpu().double()
        sig = mu * 0.0 + std
        _check(f"sample {shape} counter={counter} logp", lp[:N], ppo.gaussian_log_prob(a64, mu.double(), sig.double()), ppo.gaussian_log_prob(act[:N].cpu(), mu, sig))


@pytest.mark.parametrize("R", [1, 21, 32])
@pytest.mark.parametrize("N", [1, 13, 4099])
def test_rollout_post_bookkeeping(N, R):
    """bootstrap or pass-through of the rewards, dones, the time-out copy, the running episode sums and the ep_stats accumulator (two calls onto a
    non-zero start; a call in which no env finishes leaves it bit-identical); sentinels behind every output."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(1000 * N + R)
    values = torch.randn(N, R, generator=g)
    start = torch.tensor([12.5, 300.0, 4.0], dtype=torch.float64)
    ep = _guarded(3, dtype=torch.float64)
    ep[:3] = start
    cur_r, cur_l = _guarded(N), _guarded(N)
    cur_r[:N], cur_l[:N] = torch.rand(N, generator=g), torch.randint(0, 50, (N,), generator=g).float()
    want = start.clone()
    # call 0: post2, values NULL + time-out copy; call 1: post2 with values, no copy; call 2: pbhc_rollout_post; call 3: nobody finishes
    for call in range(4):
        rew = torch.randn(N, R, generator=g)
        reset = (torch.rand(N, generator=g) < 0.3).long() * torch.randint(1, 5, (N,), generator=g)
        if call == 0:
            reset[0] = 3                                            # (N = 1: one finished episode at least)
        if call == 3:
            reset.zero_()
        tout = (torch.rand(N, generator=g) < 0.5) & (reset > 0)
        cr0, cl0 = cur_r[:N].cpu(), cur_l[:N].cpu()
        out_r, dones, tcopy = _guarded(N * R), _guarded(N, dtype=torch.uint8), _guarded(N, dtype=torch.uint8)
        ep_before = ep.clone()
        args = [rew.to(DEV), values.to(DEV), reset.to(DEV), tout.to(DEV)]
        vptr = None if call == 0 else args[1].data_ptr()
        tail = [N, R, GAMMA, out_r.data_ptr(), dones.data_ptr(), cur_r.data_ptr(), cur_l.data_ptr(), ep.data_ptr()]
        if call == 2:
            assert lib.pbhc_rollout_post(args[0].data_ptr(), None, args[2].data_ptr(), args[3].data_ptr(), *tail, L.current_stream()) == L.K["PBHC_EINVAL"]
            torch.cuda.synchronize()
            assert bool((out_r == SENT).all()) and torch.equal(ep, ep_before)
            L.check(lib.pbhc_rollout_post(args[0].data_ptr(), vptr, args[2].data_ptr(), args[3].data_ptr(), *tail, L.current_stream()), "pbhc_rollout_post")
        else:
            L.check(lib.pbhc_rollout_post2(args[0].data_ptr(), vptr, args[2].data_ptr(), args[3].data_ptr(), *tail, tcopy.data_ptr() if call == 0 else None,
                                           L.current_stream()), "pbhc_rollout_post2")
        torch.cuda.synchronize()
        for buf, n in ((out_r, N * R), (dones, N), (tcopy, N), (cur_r, N), (cur_l, N), (ep, 3)):
            assert _tail_ok(buf, n)
        got_r = out_r[:N * R].view(N, R).cpu()
        if call == 0:
            assert torch.equal(got_r, rew)                          # pass-through, bit-exact
            assert torch.equal(tcopy[:N].cpu(), tout.to(torch.uint8))
        else:
            assert (got_r.double() - (rew.double() + GAMMA * values.double() * tout.unsqueeze(1))).abs().max().item() <= 1e-6
            assert _tail_ok(tcopy)                      # no copy requested: nothing written
        d = reset > 0
        assert torch.equal(dones[:N].cpu(), d.to(torch.uint8))
        nr, nl = cr0.double() + rew.double().sum(-1), cl0 + 1.0
        assert (cur_r[:N].cpu().double() - torch.where(d, torch.zeros_like(nr), nr)).abs().max().item() <= 1e-5
        assert torch.equal(cur_l[:N].cpu(), torch.where(d, torch.zeros_like(nl), nl))
        if call == 3:
            assert torch.equal(ep, ep_before)                       # nobody finished: bit for bit
        else:
            want += torch.stack([nr[d].sum(), nl[d].double().sum(), d.double().sum()])
            assert ((ep[:3].cpu() - want).abs() <= 1e-6 * want.abs()).all(), (ep[:3], want)
    assert float(want[2]) > float(start[2])
