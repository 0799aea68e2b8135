"""The rollout's inference kernels (`pbhc_mlp_fwd*`, `pbhc_conv_encoder_fwd`, csrc/pbhc_mlp.hip) through the C ABI, pinned against what they
do to memory AROUND their operands.  Every operand sits in an arena (tests/arena.py): inputs in NaN — margins and inter-row padding, which
the contract says a kernel must not depend on — outputs in an exactly representable sentinel.  Every test asserts that the result is finite,
that it matches a float64 reference of the same operation, and that every sentinel outside the output's logical elements is untouched,
the columns between N and the row pitch included.  The margins keep even a wrong kernel inside the buffers.

Tolerances are the project's: stack outputs 3e-5 at O(1) (tests/test_gpu_gemm.py); the encoder 2e-5 * max(1, max |ref|)
(test_conv_encoder_no_grad_path_matches_conv1d); logp and the draws by the rule of tests/test_gpu_ppo_kernels.py (err <= 4 * err32 + 1e-6,
max |z - z_philox| <= 2e-5).  Every test prints `err / bound` before it asserts.

A NaN that the one-launch encoder lets in does not come out as NaN: layer 1's ReLU (`v > 0 ? v : 0`) turns it into 0, the last time step's
hidden row is lost, and the embedding is finite and wrong.  With the fragment mask of `enc_job` taken out, the five encoder cases with
d % 16 != 0 below measure err / bound = 4 025, 4 025, 6 807, 21 323 and 7 490 — finite every time; only the comparison with float64 sees
it.  Not only the last time step reaches the padding: with d < 16 the k-step of every step t with t d + 16 > T d does (the d = 1 and d = 4
cases; a mask on the last step alone measured err / bound = 8 372 at d = 1).

Measured on an MI355X (`err / bound`; the three sampling entries agree bit for bit, so one line each):
  pbhc_conv_encoder_fwd (M, T, d, H, conv 1, conv 2, E, act, ldx slack, x offset)
    (33, 20, 58, 60, (40, 6, 2), (20, 4, 2), 128, 2, 0, 0)    0.018        (1, 5, 1, 20, (20, 2, 1), (10, 2, 1), 7, 3, 0, 1)      0.003
    (33, 20, 58, 60, (40, 6, 2), (20, 4, 2), 128, 2, 26, 2)   0.018        (5, 10, 13, 30, (20, 4, 2), (10, 2, 1), 19, 1, 5, 3)   0.008
    (16, 4, 16, 12, (20, 4, 1), (9, 1, 1), 5, 2, 0, 0)        0.006        (17, 6, 128, 22, (12, 3, 2), (7, 2, 1), 33, 3 / 1)     0.010 / 0.014
    (5, 5, 4, 20, (20, 2, 1), (10, 2, 1), 7, 2, 0, 0)         0.006
  pbhc_mlp_fwd = pbhc_mlp_fwd_cat (M, dims)
    (1, [5, 7]) 0.004    (17, [1, 1]) 0.009    (1, [1, 1]) 0.000    (33, [37, 50, 19, 3]) offset 1: 0.012, offset 4: 0.012, no biases: 0.007
    (18, [19, 33, 5]) three segments 0.009 on both paths    (35, [15, 20, 6]) 0.014    (16, [64, 64]) 0.023    (17, [2528, 16]) 0.141
  sampling epilogue (M, dims)         max |z - z_philox| / 2e-5     logp err / (4 err32 + 1e-6)    (logp err, err32)
    (33, [8, 64, 23])                 0.044                         0.054                          6.8e-8, 6.9e-8
    (17, [8, 64, 32])                 0.035                         0.072                          8.7e-8, 5.0e-8
    (33, [40, 23])                    0.047                         0.055                          6.9e-8, 6.4e-8
    (1, [5, 4])                       0.006                         0.087                          9.5e-8, 2.4e-8
    (17, [16, 32])                    0.035                         0.115                          1.4e-7, 5.0e-8
    (33, [3, 1])                      0.017                         0.039                          4.6e-8, 4.6e-8
    (17, [12, 40, 24, 1])             0.013                         0.041                          4.9e-8, 4.3e-8
    (1, [12, 40, 24, 4])              0.004                         0.023                          2.5e-8, 2.5e-8
    (33, [30, 64, 48, 32, 23])        0.044                         0.072                          9.1e-8, 6.5e-8
    (17, [30, 64, 48, 32, 32])        0.035                         0.094                          1.2e-7, 6.4e-8
  the Python guards: encoder 0.001 (both paths), stack 0.002 (all four results)
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import ppo
from tests import helpers
from tests.arena import SENT, act64, arena, conv_encoder_ref
from tests.test_gpu_ppo_kernels import _err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 3e-5
NAN = float("nan")
SEED = 0x9E3779B97F4A7C15          # both 32-bit halves non-zero


def _lib():
    from pbhc_amd import _lib as L

    return L, L.lib()


def _pack(lib, L, w):
    """pbhc_mlp_pack of a row-major [N, K] matrix (the packed copy is an operand layout of its own: 16-byte aligned, no arena)"""
    w = w.contiguous()
    pk = torch.empty(lib.pbhc_mlp_packed_floats(w.shape[0], w.shape[1]), device=DEV)
    L.check(lib.pbhc_mlp_pack(w.data_ptr(), w.shape[0], w.shape[1], pk.data_ptr(), L.current_stream()), "pbhc_mlp_pack")
    return pk


def _in(data, pitch=None, offset=0):
    """an input operand: data inside, NaN in the margins and the row padding"""
    data = data if data.dim() == 2 else data.reshape(1, -1)
    return arena(data.shape[0], data.shape[1], pitch, offset, NAN, data, DEV)


def _out(rows, cols, pitch=None, offset=0):
    return arena(rows, cols, pitch, offset, SENT, None, DEV)


# ================================================================================================================================================
#  1. pbhc_conv_encoder_fwd
# ================================================================================================================================================
# (M, T, d, H, (O1, k1, s1), (O2, k2, s2), E, act, ldx beyond (T - 1) d + ceil16(d), x float offset)
ENC_CASES = [
    (33, 20, 58, 60, (40, 6, 2), (20, 4, 2), 128, 2, 0, 0),       # the production shape, pitch at its minimum: 6 floats of over-read
    (33, 20, 58, 60, (40, 6, 2), (20, 4, 2), 128, 2, 26, 2),      # ... on a wider slab, rows 4-byte aligned only
    (1, 5, 1, 20, (20, 2, 1), (10, 2, 1), 7, 3, 0, 1),            # d = 1: 15 floats of over-read, one k-step: EVERY step's read reaches the padding
    (5, 5, 4, 20, (20, 2, 1), (10, 2, 1), 7, 2, 0, 0),            # d = 4: the k-steps of steps 2, 3 and 4 reach it
    (5, 10, 13, 30, (20, 4, 2), (10, 2, 1), 19, 1, 5, 3),         # d = 13: 3 floats
    (16, 4, 16, 12, (20, 4, 1), (9, 1, 1), 5, 2, 0, 0),           # d = 16: none; T == k1 and L1 == k2: one position per layer
    (17, 6, 128, 22, (12, 3, 2), (7, 2, 1), 33, 3, 0, 0),         # d = 128: the entry's limit, 8 k-steps; a (k, s) pair outside _CONV_TABLE
    (17, 6, 128, 22, (12, 3, 2), (7, 2, 1), 33, 1, 4, 1),
]


def _encoder(lib, L, M, T, d, H, c1, c2, E, act, seed):
    """random raw matrices in the ABI's layout (float32, on the device) + the filled PbhcConvEncoder"""
    (O1, k1, s1), (O2, k2, s2) = c1, c2
    L1 = (T - k1) // s1 + 1
    L2 = (L1 - k2) // s2 + 1
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    mats = dict(w1=rn(H, d) / d ** 0.5, wc1=rn(O1, k1 * H) / (k1 * H) ** 0.5, wc2=rn(O2, k2 * O1) / (k2 * O1) ** 0.5, wo=rn(E, max(L2, 1) * O2) / (max(L2, 1) * O2) ** 0.5)
    bias = dict(b1=0.3 * rn(H), bc1=0.3 * rn(O1), bc2=0.3 * rn(O2), bo=0.3 * rn(E))
    bias_a = {k: _in(v, offset=1 + i) for i, (k, v) in enumerate(bias.items())}           # biases: 4-byte aligned only, NaN around them
    packed = {k: _pack(lib, L, v) for k, v in mats.items()}
    e = L.PbhcConvEncoder()
    e.w1, e.wc1, e.wc2, e.wo = (packed[k].data_ptr() for k in ("w1", "wc1", "wc2", "wo"))
    e.b1, e.bc1, e.bc2, e.bo = (bias_a[k].ptr() for k in ("b1", "bc1", "bc2", "bo"))
    e.T, e.d, e.H, e.E, e.O1, e.k1, e.s1, e.O2, e.k2, e.s2, e.act = T, d, H, E, O1, k1, s1, O2, k2, s2, act
    x = rn(M, T * d)
    return e, x, mats, bias, (packed, bias_a)


@pytest.mark.parametrize("case", ENC_CASES)
def test_conv_encoder_fwd_ignores_padding_and_stays_inside_its_output(case):
    L, lib = _lib()
    M, T, d, H, c1, c2, E, act, extra, xoff = case
    e, x, mats, bias, keep = _encoder(lib, L, M, T, d, H, c1, c2, E, act, sum(case[:4]) + act)
    ldx = (T - 1) * d + (d + 15) // 16 * 16 + extra
    assert int(lib.pbhc_conv_encoder_lds_bytes(C.byref(e))) <= 160 * 1024
    xa = _in(x, ldx, xoff)
    ya = _out(M, E, E + 3, 1)
    L.check(lib.pbhc_conv_encoder_fwd(xa.ptr(), ldx, C.byref(e), ya.ptr(), E + 3, M, L.current_stream()), "pbhc_conv_encoder_fwd")
    torch.cuda.synchronize()
    dd = lambda t: t.double().cpu()
    ref = conv_encoder_ref(dd(x), dd(mats["w1"]), dd(bias["b1"]), dd(mats["wc1"]), dd(bias["bc1"]), dd(mats["wc2"]), dd(bias["bc2"]), dd(mats["wo"]), dd(bias["bo"]),
                           T, d, c1[1], c1[2], c2[1], c2[2], act)
    got = dd(ya.view)
    bound = 2e-5 * max(1.0, ref.abs().max().item())
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() if finite else float("inf")
    print(f"ERR encoder {case}: finite {finite} err/bound {err / bound:.3f}")
    assert finite
    assert err < bound
    assert ya.intact() and xa.intact()


def test_conv_encoder_fwd_refusals_write_nothing():
    """d over the limit, a window start that is not 16-byte aligned, ldx one too small, ldy < E, an LDS need above 160 KB: PBHC_EINVAL, output untouched"""
    L, lib = _lib()
    EINVAL = L.K["PBHC_EINVAL"]
    good = (5, 10, 13, 30, (20, 4, 2), (10, 2, 1), 19, 1)
    # (case, ldx - minimum, ldy - E)
    bad = [((5, 10, 129, 30, (20, 4, 2), (10, 2, 1), 19, 1), 0, 3),
           ((5, 10, 130, 30, (20, 4, 2), (10, 2, 1), 19, 1), 0, 3),
           ((5, 10, 13, 30, (20, 4, 1), (10, 2, 1), 19, 1), 0, 3),             # s1 * H = 30
           ((5, 10, 13, 32, (21, 4, 2), (10, 2, 1), 19, 1), 0, 3),             # s2 * O1 = 21
           (good, -1, 3),
           (good, 0, -1),
           ((5, 20, 13, 128, (40, 6, 2), (20, 4, 2), 19, 1), 0, 3)]            # image h alone: 16 rows x 2 580 floats
    for case, dldx, dldy in bad:
        M, T, d, H, c1, c2, E, act = case
        e, x, mats, bias, keep = _encoder(lib, L, M, T, d, H, c1, c2, E, act, 5)
        ldx_min = (T - 1) * d + (d + 15) // 16 * 16
        xa = _in(x, ldx_min + 1, 0)
        ya = _out(M, E, E + 3, 0)
        if case[3] == 128:
            assert int(lib.pbhc_conv_encoder_lds_bytes(C.byref(e))) > 160 * 1024
        assert lib.pbhc_conv_encoder_fwd(xa.ptr(), ldx_min + dldx, C.byref(e), ya.ptr(), E + dldy, M, L.current_stream()) == EINVAL, (case, dldx, dldy)
        torch.cuda.synchronize()
        assert ya.untouched(), (case, dldx, dldy)
    # (the same call with nothing wrong is taken)
    M, T, d, H, c1, c2, E, act = good
    e, x, mats, bias, keep = _encoder(lib, L, M, T, d, H, c1, c2, E, act, 5)
    ldx_min = (T - 1) * d + (d + 15) // 16 * 16
    xa, ya = _in(x, ldx_min, 0), _out(M, E, E, 0)
    assert lib.pbhc_conv_encoder_fwd(xa.ptr(), ldx_min, C.byref(e), ya.ptr(), E, M, L.current_stream()) == 0
    torch.cuda.synchronize()
    assert ya.intact() and bool(torch.isfinite(ya.view).all())


# ================================================================================================================================================
#  2. pbhc_mlp_fwd / pbhc_mlp_fwd_cat
# ================================================================================================================================================
class _Stack:
    """random Linear stack `dims` in float32 on the device: packed weights, biases in NaN arenas (or NULL), the ctypes arrays, the fp64 forward"""

    def __init__(self, lib, L, dims, seed, with_bias=True):
        g = torch.Generator(device=DEV).manual_seed(seed)
        n = len(dims) - 1
        self.dims, self.n = dims, n
        self.Ws = [torch.randn(dims[i + 1], dims[i], device=DEV, generator=g) / dims[i] ** 0.5 for i in range(n)]
        self.bs = [0.1 * torch.randn(dims[i + 1], device=DEV, generator=g) for i in range(n)] if with_bias else None
        self.packed = [_pack(lib, L, w) for w in self.Ws]
        self.bias_a = [_in(b, offset=1 + (i & 3)) for i, b in enumerate(self.bs)] if with_bias else None
        self.w = (C.c_void_p * n)(*[t.data_ptr() for t in self.packed])
        self.b = (C.c_void_p * n)(*([a.ptr() for a in self.bias_a] if with_bias else [None] * n))
        self.d = (C.c_int * (n + 1))(*dims)
        self.gen = g

    def ref(self, x, act):
        h = x.double().cpu()
        for i in range(self.n):
            h = h @ self.Ws[i].double().cpu().t() + (self.bs[i].double().cpu() if self.bs is not None else 0.0)
            if i < self.n - 1:
                h = act64(act, h)
        return h


def _segments(L, arenas):
    inp = L.PbhcMlpInput()
    for i, a in enumerate(arenas):
        inp.x[i], inp.ld[i], inp.width[i] = a.ptr(), a.view.stride(0), a.view.shape[1]
    inp.nseg = len(arenas)
    return inp


# (M, dims, [(width, pitch, float offset) per segment], biases, act)
MLP_CASES = [
    (1, [5, 7], [(5, 5, 0)], True, 1),                            # one row, one layer
    (17, [1, 1], [(1, 1, 0)], True, 2),                           # dims [1, 1]
    (1, [1, 1], [(1, 4, 4)], False, 3),
    (33, [37, 50, 19, 3], [(37, 40, 1)], True, 1),                # ld % 4 == 0, base 4 bytes behind a 16-byte boundary: the element path by alignment alone
    (33, [37, 50, 19, 3], [(37, 40, 4)], True, 1),                # ... 16 bytes behind a 512-byte boundary: the 16-byte path on a shifted base
    (33, [37, 50, 19, 3], [(37, 40, 4)], False, 2),               # NULL biases
    (18, [19, 33, 5], [(8, 8, 0), (4, 12, 4), (7, 8, 8)], True, 3),        # three segments, 16-byte path: the last piece straddles the row's end into NaN
    (18, [19, 33, 5], [(8, 9, 0), (4, 12, 4), (7, 8, 8)], True, 3),        # ... an odd pitch: the element path
    (35, [15, 20, 6], [(5, 8, 1), (3, 3, 2), (7, 11, 3)], True, 2),        # three odd segments
    (16, [64, 64], [(64, 64, 0)], True, 1),                       # whole tiles, no padding at all
]


@pytest.mark.parametrize("case", MLP_CASES)
def test_mlp_fwd_ignores_padding_and_stays_inside_its_output(case):
    L, lib = _lib()
    M, dims, segs, with_bias, act = case
    st = _Stack(lib, L, dims, 13 * M + sum(dims) + act, with_bias)
    assert sum(s[0] for s in segs) == dims[0]
    xs = [torch.randn(M, w, device=DEV, generator=st.gen) for w, _, _ in segs]
    xa = [_in(x, p, o) for x, (_, p, o) in zip(xs, segs)]
    ref = st.ref(torch.cat(xs, -1), act)
    N = dims[-1]
    outs = []
    if len(segs) == 1:
        ya = _out(M, N, N + 3, 1)
        L.check(lib.pbhc_mlp_fwd(xa[0].ptr(), segs[0][1], st.w, st.b, st.d, st.n, act, ya.ptr(), N + 3, M, L.current_stream()), "pbhc_mlp_fwd")
        outs.append(("fwd", ya))
    inp = _segments(L, xa)
    ya = _out(M, N, N + 5, 2)
    L.check(lib.pbhc_mlp_fwd_cat(C.byref(inp), st.w, st.b, st.d, st.n, act, ya.ptr(), N + 5, M, None, L.current_stream()), "pbhc_mlp_fwd_cat")
    outs.append(("cat", ya))
    torch.cuda.synchronize()
    for name, ya in outs:
        got = ya.view.double().cpu()
        finite = bool(torch.isfinite(got).all())
        err = (got - ref).abs().max().item() if finite else float("inf")
        print(f"ERR mlp {name} {case}: finite {finite} err/bound {err / TOL:.3f}")
        assert finite
        assert err < TOL
        assert ya.intact()
    assert torch.equal(outs[0][1].view, outs[-1][1].view)                 # one kernel, one summation order
    assert all(a.intact() for a in xa)


def test_mlp_fwd_widest_stack_runs_and_the_next_wider_is_refused():
    """16 rows x (pitch0 + pitch1) floats of LDS: [2528, 16] needs 16 * (2532 + 20) * 4 = 163 328 bytes, the most a stack can need under
    160 KB (the pitches are 4 mod 16); [2529, 16] rounds its input row up to 2544: 164 352 bytes, refused with nothing written.  The two
    production stacks keep the need they had: 16 * (388 + 516) * 4 and 16 * (644 + 772) * 4."""
    L, lib = _lib()
    lds = lambda dims: int(lib.pbhc_mlp_fwd_lds_bytes((C.c_int * len(dims))(*dims), len(dims) - 1))
    assert lds([380, 512, 256, 128, 23]) == 57856 and lds([630, 768, 512, 128, 21]) == 90624
    assert lds([2528, 16]) == 163328 <= 160 * 1024 < lds([2529, 16]) == 164352
    # the image the last layer writes holds a row of the output: one layer, and two layers behind a narrow input
    assert lds([40, 23]) == 16 * (52 + 36) * 4 and lds([8, 64, 23]) == 16 * (36 + 68) * 4 and lds([5, 4]) == 16 * (20 + 20) * 4
    M = 17
    for dims, ok in (([2528, 16], True), ([2529, 16], False)):
        st = _Stack(lib, L, dims, 3)
        x = torch.randn(M, dims[0], device=DEV, generator=st.gen)
        xa, ya = _in(x, dims[0] + 4 - dims[0] % 4, 0), _out(M, 16, 19, 1)
        rc = lib.pbhc_mlp_fwd(xa.ptr(), xa.view.stride(0), st.w, st.b, st.d, 1, 1, ya.ptr(), 19, M, L.current_stream())
        torch.cuda.synchronize()
        if ok:
            assert rc == 0
            got = ya.view.double().cpu()
            err = (got - st.ref(x, 1)).abs().max().item()
            print(f"ERR mlp widest {dims}: err/bound {err / TOL:.3f}")
            assert bool(torch.isfinite(got).all()) and err < TOL and ya.intact()
        else:
            assert rc == L.K["PBHC_EINVAL"] and ya.untouched()


# ================================================================================================================================================
#  3. the sampling epilogue: pbhc_mlp_fwd_sample, pbhc_mlp_fwd_cat with `sample`
# ================================================================================================================================================
# (M, dims, x pitch, x float offset): A in {1, 4, 23, 32}, 1 to 4 layers, M in {1, 17, 33}.  One layer: the log-prob terms go to an image no
# layer's input sizes; [8, 64, A]: to the image of the 8-wide input
SAMPLE_CASES = [
    (33, [8, 64, 23], 8, 0), (17, [8, 64, 32], 12, 4), (33, [40, 23], 40, 0), (1, [5, 4], 8, 0), (17, [16, 32], 16, 1), (33, [3, 1], 3, 0),
    (17, [12, 40, 24, 1], 12, 0), (1, [12, 40, 24, 4], 16, 0), (33, [30, 64, 48, 32, 23], 32, 0), (17, [30, 64, 48, 32, 32], 31, 1),
]


def _sample_outs(M, A):
    return dict(actions=_out(M, A, offset=1), action_mean=_out(M, A, offset=2), action_sigma=_out(M, A, offset=3), logp=_out(1, M, offset=1))


def _sample_struct(L, outs, std_a, ctr, offset):
    smp = L.PbhcMlpSample()
    smp.std, smp.counter, smp.seed, smp.counter_offset = std_a.ptr(), ctr.data_ptr(), SEED, offset
    smp.actions, smp.action_mean, smp.action_sigma, smp.logp = (outs[k].ptr() for k in ("actions", "action_mean", "action_sigma", "logp"))
    return smp


@pytest.mark.parametrize("case", SAMPLE_CASES)
def test_mlp_fwd_sample_epilogue(case):
    """action_mean == pbhc_mlp_fwd's output bit for bit; action_sigma == std; (actions - mean) / std == the host Philox model (key (seed lo,
    seed hi), counter words (row, uint32(counter[0]) + counter_offset, 0x5A4D, column), Box-Muller in float64); logp == the fp64 Normal
    log-density of the returned action; the three entries agree bit for bit; sentinels behind all four outputs (and y) intact."""
    L, lib = _lib()
    M, dims, pitch, xoff = case
    A = dims[-1]
    st = _Stack(lib, L, dims, 7 * M + sum(dims))
    x = torch.randn(M, dims[0], device=DEV, generator=st.gen)
    std = 0.3 + 0.9 * torch.rand(A, device=DEV, generator=st.gen)
    xa, std_a = _in(x, pitch, xoff), _in(std, offset=3)
    counter, coff = 2 ** 24 + 3, 5
    ctr = torch.tensor([float(counter)], dtype=torch.float64, device=DEV)
    act = 1 + (M + A) % 3
    ya = _out(M, A, A + 3, 1)
    L.check(lib.pbhc_mlp_fwd(xa.ptr(), pitch, st.w, st.b, st.d, st.n, act, ya.ptr(), A + 3, M, L.current_stream()), "pbhc_mlp_fwd")
    inp = _segments(L, [xa])
    runs = []
    o = _sample_outs(M, A)
    smp = _sample_struct(L, o, std_a, ctr, coff)
    L.check(lib.pbhc_mlp_fwd_sample(xa.ptr(), pitch, st.w, st.b, st.d, st.n, act, M, C.byref(smp), L.current_stream()), "pbhc_mlp_fwd_sample")
    runs.append(("sample", o, None))
    o = _sample_outs(M, A)
    smp = _sample_struct(L, o, std_a, ctr, coff)
    L.check(lib.pbhc_mlp_fwd_cat(C.byref(inp), st.w, st.b, st.d, st.n, act, None, 0, M, C.byref(smp), L.current_stream()), "pbhc_mlp_fwd_cat")
    runs.append(("cat", o, None))
    o = _sample_outs(M, A)
    smp = _sample_struct(L, o, std_a, ctr, coff)
    y2 = _out(M, A, A + 1, 3)
    L.check(lib.pbhc_mlp_fwd_cat(C.byref(inp), st.w, st.b, st.d, st.n, act, y2.ptr(), A + 1, M, C.byref(smp), L.current_stream()), "pbhc_mlp_fwd_cat")
    runs.append(("cat+y", o, y2))
    torch.cuda.synchronize()

    mean = ya.view.cpu()
    ref = st.ref(x, act)
    err = (mean.double() - ref).abs().max().item()
    print(f"ERR sample {case} mean: err/bound {err / TOL:.3f}")
    assert bool(torch.isfinite(mean).all()) and err < TOL and ya.intact()
    ph = helpers._philox4x32_7(SEED, np.arange(M)[:, None], (counter + coff) & 0xFFFFFFFF, 0x5A4D, np.arange(A)[None, :])
    u1 = ((ph[0] >> np.uint64(8)).astype(np.float64) + 0.5) / 2.0 ** 24
    u2 = (ph[1] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    z_want = torch.from_numpy(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    std_c = std.cpu()
    sig = mean * 0.0 + std_c
    for name, o, y in runs:
        for k, a in o.items():
            assert a.intact(), (name, k)
            assert bool(torch.isfinite(a.view).all()), (name, k)
        assert torch.equal(o["action_mean"].view.cpu(), mean), name
        assert torch.equal(o["action_sigma"].view.cpu(), std_c.expand(M, A)), name
        if y is not None:
            assert y.intact() and torch.equal(y.view.cpu(), mean)
        actions, logp = o["actions"].view.cpu(), o["logp"].view.cpu().reshape(M)
        dz = ((actions.double() - mean.double()) / std_c.double() - z_want).abs().max().item()
        lp64 = ppo.gaussian_log_prob(actions.double(), mean.double(), sig.double())
        lp32 = ppo.gaussian_log_prob(actions, mean, sig)
        e, e32 = _err(logp, lp64), _err(lp32, lp64)
        print(f"ERR sample {case} {name}: max |z - z_philox| / 2e-5 {dz / 2e-5:.3f}  logp err {e:.3e} err32 {e32:.3e} err/bound {e / (4.0 * e32 + 1e-6):.3f}")
        assert dz <= 2e-5, name
        assert e <= 4.0 * e32 + 1e-6, (name, e, e32)
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k].view, runs[1][1][k].view) and torch.equal(runs[0][1][k].view, runs[2][1][k].view), k
    assert xa.intact() and std_a.intact()


@pytest.mark.parametrize("dims", [[8, 64, 33], [40, 33], [30, 64, 48, 32, 48]])
def test_mlp_fwd_sample_refuses_more_than_32_actions(dims):
    """the sampling epilogue is sized for an action row of up to 32: PBHC_EINVAL from every entry, nothing written; without `sample` the same stack runs"""
    L, lib = _lib()
    M, A = 17, dims[-1]
    st = _Stack(lib, L, dims, 11)
    x = torch.randn(M, dims[0], device=DEV, generator=st.gen)
    xa, std_a = _in(x), _in(torch.ones(A, device=DEV))
    ctr = torch.tensor([7.0], dtype=torch.float64, device=DEV)
    o = _sample_outs(M, A)
    smp = _sample_struct(L, o, std_a, ctr, 0)
    inp = _segments(L, [xa])
    ya = _out(M, A, A + 3, 1)
    EINVAL = L.K["PBHC_EINVAL"]
    assert lib.pbhc_mlp_fwd_sample(xa.ptr(), dims[0], st.w, st.b, st.d, st.n, 1, M, C.byref(smp), L.current_stream()) == EINVAL
    assert lib.pbhc_mlp_fwd_cat(C.byref(inp), st.w, st.b, st.d, st.n, 1, None, 0, M, C.byref(smp), L.current_stream()) == EINVAL
    assert lib.pbhc_mlp_fwd_cat(C.byref(inp), st.w, st.b, st.d, st.n, 1, ya.ptr(), A + 3, M, C.byref(smp), L.current_stream()) == EINVAL
    torch.cuda.synchronize()
    assert ya.untouched() and all(a.untouched() for a in o.values())
    L.check(lib.pbhc_mlp_fwd_cat(C.byref(inp), st.w, st.b, st.d, st.n, 1, ya.ptr(), A + 3, M, None, L.current_stream()), "pbhc_mlp_fwd_cat")
    torch.cuda.synchronize()
    err = (ya.view.double().cpu() - st.ref(x, 1)).abs().max().item()
    assert err < TOL and ya.intact()


# ================================================================================================================================================
#  4. the Python guards: a view whose last row ends where its storage ends takes the fallback
# ================================================================================================================================================
class _Spy:
    """wraps entries of the loaded library so that a test sees which were called (and with what); restores them on exit"""

    def __init__(self, lib, names):
        self.lib, self.names, self.calls = lib, names, []

    def __enter__(self):
        self.orig = {n: getattr(self.lib, n) for n in self.names}
        for n, fn in self.orig.items():
            setattr(self.lib, n, (lambda n, fn: lambda *a: (self.calls.append((n, a)), fn(*a))[1])(n, fn))
        return self

    def __exit__(self, *exc):
        for n, fn in self.orig.items():
            setattr(self.lib, n, fn)

    def count(self, name):
        return sum(1 for n, _ in self.calls if n == name)


def _ends_with_its_storage(B, cols, pitch):
    """[B, cols] view, rows `pitch` apart, whose last element is the last of its storage; the storage's byte count leaves >= 64 bytes before
    the next multiple of 512 (the allocator's granule: a read of a few floats past the end would still be inside the block)"""
    n = (B - 1) * pitch + cols
    assert 64 <= 512 - (4 * n) % 512 < 512
    buf = torch.randn(n, device=DEV)
    return buf.as_strided((B, cols), (pitch, 1))


def test_conv_encoder_takes_the_per_layer_path_when_the_over_read_would_leave_the_storage():
    L, lib = _lib()
    from pbhc_amd.agents import agent_modules as am

    T, d, H, E, B = 5, 13, 20, 16, 3
    torch.manual_seed(1)
    cfg = {"input_dim": ["x"], "hidden_dim": H, "output_dim": E, "layer_config": {"type": "Conv1d", "activation": "SiLU"}}
    enc = am.ConvEncoder({"x": d}, cfg, T).to(DEV)
    ref = am.ConvEncoder({"x": d}, cfg, T).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in enc.state_dict().items()})
    ref.unfold_gemm = False
    pitch = 72                                                   # >= (T - 1) d + ceil16(d) = 68: the pitch alone allows the one-launch encoder
    x_end = _ends_with_its_storage(B, T * d, pitch)              # ... whose last row would be read 3 floats past the storage
    slab = torch.randn(B, pitch, device=DEV)
    x_in = slab[:, :T * d]                                       # the same pitch with the padding inside the storage
    with torch.no_grad():
        enc.prepare_inference()
        assert enc._enc_c is not None
        with _Spy(lib, ["pbhc_conv_encoder_fwd", "pbhc_linear_act_fwd_strided"]) as spy:
            got_end = enc(x_end)
            assert spy.count("pbhc_conv_encoder_fwd") == 0 and spy.count("pbhc_linear_act_fwd_strided") == 3
            got_in = enc(x_in)
            assert spy.count("pbhc_conv_encoder_fwd") == 1 and spy.count("pbhc_linear_act_fwd_strided") == 3
        enc.release_inference()
        for got, x in ((got_end, x_end), (got_in, x_in)):
            want = ref(x.double().cpu())
            err, bound = (got.double().cpu() - want).abs().max().item(), 2e-5 * max(1.0, want.abs().max().item())
            print(f"ERR encoder guard: err/bound {err / bound:.3f}")
            assert err < bound


def test_stack_entries_fall_back_when_the_16_byte_piece_would_leave_the_storage():
    L, lib = _lib()
    from pbhc_amd.agents import fused_mlp

    torch.manual_seed(2)
    B, K, A = 5, 13, 3
    seq = nn.Sequential(nn.Linear(K, 8), nn.ELU(), nn.Linear(8, A)).to(DEV)
    x_end = _ends_with_its_storage(B, K, 16)                     # 16-byte aligned, pitch % 4 == 0: the 16-byte path, whose last piece would end 3 floats past the storage
    assert x_end.data_ptr() % 16 == 0
    slab = torch.randn(B, 16, device=DEV)
    x_in = slab[:, :K]
    std = torch.full((A,), 0.5, device=DEV)
    ctr = torch.tensor([3.0], dtype=torch.float64, device=DEV)
    mk = lambda: dict(actions=torch.zeros(B, A, device=DEV), action_mean=torch.zeros(B, A, device=DEV), action_sigma=torch.zeros(B, A, device=DEV),
                      logp=torch.zeros(B, 1, device=DEV))
    names = ["pbhc_mlp_fwd", "pbhc_mlp_fwd_sample", "pbhc_mlp_fwd_cat"]
    with torch.no_grad():
        assert fused_mlp.pack_stack(seq)
        try:
            with _Spy(lib, names) as spy:
                got_end = fused_mlp.forward_inference(seq, x_end)
                assert spy.count("pbhc_mlp_fwd") == 1 and spy.calls[-1][1][1] == K             # a contiguous copy: row pitch K, the element path
                kw = mk()
                assert fused_mlp.forward_sample(seq, x_end, std, 1, ctr.data_ptr(), 0, **kw) is False
                assert fused_mlp.forward_cat_inference(seq, [x_end]) is False
                assert fused_mlp.forward_cat_inference(seq, [x_in[:, :8], x_end[:, 8:]]) is False
                assert spy.count("pbhc_mlp_fwd_sample") == 0 and spy.count("pbhc_mlp_fwd_cat") == 0 and not any(v.any() for v in kw.values())
                # the same pitch with the padding inside the storage: read in place
                got_in = fused_mlp.forward_inference(seq, x_in)
                assert spy.count("pbhc_mlp_fwd") == 2 and spy.calls[-1][1][1] == 16
                kw = mk()
                assert fused_mlp.forward_sample(seq, x_in, std, 1, ctr.data_ptr(), 0, **kw) is True
                got_cat = fused_mlp.forward_cat_inference(seq, [x_in])
                assert spy.count("pbhc_mlp_fwd_sample") == 1 and spy.count("pbhc_mlp_fwd_cat") == 1
        finally:
            fused_mlp.release_stack(seq)
    torch.cuda.synchronize()
    seq64 = nn.Sequential(nn.Linear(K, 8), nn.ELU(), nn.Linear(8, A)).double()
    seq64.load_state_dict({k: v.double().cpu() for k, v in seq.state_dict().items()})
    with torch.no_grad():
        for got, x in ((got_end, x_end), (got_in, x_in), (got_cat, x_in), (kw["action_mean"], x_in)):
            err = (got.double().cpu() - seq64(x.double().cpu())).abs().max().item()
            print(f"ERR stack guard: err/bound {err / TOL:.3f}")
            assert err < TOL
