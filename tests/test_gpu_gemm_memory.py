"""The single-problem fused GEMM entries (`pbhc_linear_act_fwd`, `_fwd_out`, `_fwd_strided`, `pbhc_linear_dgrad_act`, `pbhc_linear_wgrad`,
csrc/pbhc_gemm.hip; `pbhc_linear_out_bwd`, csrc/pbhc_ppo.hip) through the C ABI, pinned against what they do to memory AROUND their operands.
tests/test_gpu_gemm.py holds their values to float64 on exactly-sized, 512-byte aligned tensors; here every operand sits in an arena
(tests/arena.py).  Inputs: NaN margins, base pointers 0, 1, 2 and 3 floats behind a 16-byte boundary — the header promises "rows need
4-byte alignment only" — so a read outside an operand that reaches a result makes it non-finite.  Outputs — y, pre, out, dx, dh, dw and every
scratch / partial area at exactly the size the header asks for — in an exactly representable sentinel, so a ragged tile that stores a few
floats past its operand, or a partial row past the count the entry reports, is found.  Shapes: the small ragged ones of tests/test_gpu_gemm.py
under every pbhc_gemm_debug_force_shape value that file loops over; values against float64 with that file's tolerances.  Every test prints
`err / bound` before it asserts.

Measured on an MI355X (`err / bound`, the largest over the four offsets and the six forced shapes of a case):
  pbhc_linear_act_fwd (M, N, K)            pre     y       no bias
    (200, 130, 37)                         0.065   0.065   0.040
    (97, 23, 630)                          0.168   0.164   0.087
    (1, 1, 5)                              0.001   0.001   0.001
    (130, 257, 3)                          0.022   0.026   0.025
    (64, 128, 1)                           0.023   0.021   0.020
  pbhc_linear_act_fwd_out (M, K, NO)       pre     y       out
    (33, 37, 1)                            0.098   0.056   0.019
    (1, 4, 29)                             0.019   0.019   0.019
    (100, 64, 23)                          0.104   0.104   0.046
  pbhc_linear_act_fwd_strided              pre     y
    (33, 13, 20, 5, 13, 7, 3)              0.025   0.028
    (70, 58, 60, 6, 58, 10, 5)             0.073   0.061
    (17, 4, 130, 3, 4, 1, 2)               0.017   0.025
    (37, 80, 10, 4, 40, 3, 1)              0.075   0.075
    (130, 120, 20, 3, 30, 6, 4)            0.109   0.109
    (1, 7, 5, 2, 7, 1, 1)                  0.011   0.011
  pbhc_linear_dgrad_act (M, N, K)          dx      column sums
    (200, 132, 37)                         0.035   0.016
    (97, 128, 1)                           0.032   0.014
    (130, 256, 3)                          0.024   0.021
    (77, 130, 40)                          0.038   0.018
  pbhc_linear_wgrad (M, N, K)              dw
    (640, 4, 5) 0.173    (384, 72, 630) 0.161    (512, 128, 37) 0.174    (32, 4, 4) 0.081
  pbhc_linear_out_bwd (M, A, K)            dh      dw      db      column sums
    (37, 1, 64)                            0.002   0.004   0.002   0.001
    (5, 9, 128)                            0.005   0.011   0.005   0.002
    (100, 32, 256)                         0.013   0.019   0.011   0.004
    (33, 23, 192)                          0.012   0.015   0.008   0.004
No entry stored outside its outputs or let a NaN from around an input into a result.
"""
import ctypes as C

import pytest
import torch

from tests.arena import SENT, act64, arena

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 3e-5
NAN = float("nan")
FORCED = (-1, 0, 1, 2, 0x10000 | 0xff, 0x20000 | 2)            # automatic; each tile shape; register-staged version; BK 16 x 3 stages
OFFSETS = [0, 1, 2, 3]


def _lib():
    from pbhc_amd import _lib as L

    return L, L.lib()


def _in(data, offset, pitch=None):
    data = data if data.dim() == 2 else data.reshape(1, -1)
    return arena(data.shape[0], data.shape[1], pitch, offset, NAN, data, DEV)


def _out(rows, cols, pitch=None):
    return arena(rows, cols, pitch, 0, SENT, None, DEV)


def _act_grad64(act, z):
    z = z.detach().clone().requires_grad_(True)
    act64(act, z).sum().backward()
    return z.grad


def _close(name, got, ref, bound):
    got = got.double().cpu()
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() if finite else float("inf")
    print(f"ERR {name}: finite {finite} err/bound {err / bound:.3f}")
    assert finite, name
    assert err < bound, (name, err, bound)


def _rows_behind_untouched(a, nb):
    """a partial area [PBHC_ACT_MAX_BLOCKS, n]: rows [nb, ...) and everything around the area still hold the sentinel"""
    return a.intact() and bool((a.view[nb:] == SENT).all())


@pytest.fixture
def forced_shape():
    L, lib = _lib()
    yield lib.pbhc_gemm_debug_force_shape
    lib.pbhc_gemm_debug_force_shape(-1)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", [(200, 130, 37), (97, 23, 630), (1, 1, 5), (130, 257, 3), (64, 128, 1)])
def test_linear_act_fwd_memory(shape, off, forced_shape):
    L, lib = _lib()
    M, N, K = shape
    act = (off + M) % 4
    g = torch.Generator(device=DEV).manual_seed(1000 * off + M + N + K)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    xa, wa, ba = _in(x, off), _in(w, (off + 1) & 3), _in(b, (off + 2) & 3)
    z = x.double().cpu() @ w.double().cpu().t() + b.double().cpu()
    for forced in FORCED:
        forced_shape(forced)
        ya, pa = _out(M, N), _out(M, N)
        L.check(lib.pbhc_linear_act_fwd(xa.ptr(), wa.ptr(), ba.ptr(), ya.ptr(), pa.ptr(), M, N, K, act, L.current_stream()), "fwd")
        torch.cuda.synchronize()
        _close(f"fwd {shape} off {off} forced {forced:#x} pre", pa.view, z, TOL)
        _close(f"fwd {shape} off {off} forced {forced:#x} y", ya.view, act64(act, z), TOL)
        assert ya.intact() and pa.intact(), forced
    forced_shape(-1)
    ya = _out(M, N)                                                 # no bias, no pre-activation output
    L.check(lib.pbhc_linear_act_fwd(xa.ptr(), wa.ptr(), None, ya.ptr(), None, M, N, K, act, L.current_stream()), "fwd")
    torch.cuda.synchronize()
    _close(f"fwd {shape} off {off} no bias", ya.view, act64(act, z - b.double().cpu()), TOL)
    assert ya.intact() and xa.intact() and wa.intact() and ba.intact()


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("act", [1, 2, 3])
@pytest.mark.parametrize("shape", [(33, 37, 1), (1, 4, 29), (100, 64, 23)])
def test_linear_act_fwd_out_memory(shape, act, off):
    L, lib = _lib()
    M, K, NO = shape
    g = torch.Generator(device=DEV).manual_seed(31 * act + M + K + NO + off)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(128, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(128, device=DEV, generator=g)
    wo = torch.randn(NO, 128, device=DEV, generator=g) / 128 ** 0.5
    bo = torch.randn(NO, device=DEV, generator=g)
    xa, wa, ba, woa, boa = _in(x, off), _in(w, (off + 1) & 3), _in(b, (off + 2) & 3), _in(wo, (off + 3) & 3), _in(bo, (off + 1) & 3)
    dd = lambda t: t.double().cpu()
    for with_bias in (True, False):
        ya, pa, oa = _out(M, 128), _out(M, 128), _out(M, NO)
        L.check(lib.pbhc_linear_act_fwd_out(xa.ptr(), wa.ptr(), ba.ptr() if with_bias else None, ya.ptr(), pa.ptr(), M, 128, K, act, woa.ptr(),
                                            boa.ptr() if with_bias else None, NO, oa.ptr(), L.current_stream()), "fwd_out")
        torch.cuda.synchronize()
        z = dd(x) @ dd(w).t() + (dd(b) if with_bias else 0.0)
        h = act64(act, z)
        name = f"fwd_out {shape} act {act} off {off} bias {with_bias}"
        _close(name + " pre", pa.view, z, TOL)
        _close(name + " y", ya.view, h, TOL)
        _close(name + " out", oa.view, h @ dd(wo).t() + (dd(bo) if with_bias else 0.0), TOL)
        assert ya.intact() and pa.intact() and oa.intact()
    assert all(a.intact() for a in (xa, wa, ba, woa, boa))


# pbhc_linear_act_fwd_strided as the one-launch encoder's per-layer fallback calls it (agents/agent_modules.ConvEncoder._forward_infer):
# (M, K, N, batches, x batch stride, lda - row width, ldc - row width).  The per-step Linear: batch t reads the d floats of time step t of a
# padded slab row, writes H columns of [M, T, H]; a Conv1d window: batch l reads k * C floats at l * s * C
STRIDED = [(33, 13, 20, 5, 13, 7, 3), (70, 58, 60, 6, 58, 10, 5), (17, 4, 130, 3, 4, 1, 2), (37, 80, 10, 4, 40, 3, 1), (130, 120, 20, 3, 30, 6, 4), (1, 7, 5, 2, 7, 1, 1)]


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("case", STRIDED)
def test_linear_act_fwd_strided_memory(case, off, forced_shape):
    L, lib = _lib()
    M, K, N, nb, xs, padx, pady = case
    act = 1 + (off + M) % 3
    g = torch.Generator(device=DEV).manual_seed(17 * off + sum(case))
    wx, wy = (nb - 1) * xs + K, nb * N                            # the row's logical widths
    lda, ldc = wx + padx, wy + pady
    x = torch.randn(M, wx, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    xa, wa, ba = _in(x, off, lda), _in(w, (off + 1) & 3), _in(b, (off + 2) & 3)
    dd = lambda t: t.double().cpu()
    z = torch.cat([dd(x)[:, t * xs:t * xs + K] @ dd(w).t() + dd(b) for t in range(nb)], dim=1)
    for forced in FORCED:
        forced_shape(forced)
        ya, pa = _out(M, wy, ldc), _out(M, wy, ldc)
        L.check(lib.pbhc_linear_act_fwd_strided(xa.ptr(), lda, xs, wa.ptr(), ba.ptr(), ya.ptr(), pa.ptr(), ldc, N, nb, M, N, K, act, L.current_stream()), "strided")
        torch.cuda.synchronize()
        _close(f"strided {case} off {off} forced {forced:#x} pre", pa.view, z, TOL)
        _close(f"strided {case} off {off} forced {forced:#x} y", ya.view, act64(act, z), TOL)
        assert ya.intact() and pa.intact(), forced
    assert xa.intact() and wa.intact() and ba.intact()


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", [(200, 132, 37), (97, 128, 1), (130, 256, 3), (77, 130, 40)])
def test_linear_dgrad_act_memory(shape, off, forced_shape):
    L, lib = _lib()
    M, N, K = shape
    act = (off + M) % 4
    g = torch.Generator(device=DEV).manual_seed(7000 * off + M + N + K)
    dy = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    zpre = torch.randn(M, N, device=DEV, generator=g)
    saved = zpre if act == 2 else act64(act, zpre)                        # SiLU: pre-activation; ELU / ReLU: the activation output
    dya, wa, sa = _in(dy, off), _in(w, (off + 1) & 3), _in(saved, (off + 2) & 3)
    ref = (dy.double().cpu() @ w.double().cpu()) * (_act_grad64(act, zpre.double().cpu()) if act else 1.0)
    MAXB = L.K["PBHC_ACT_MAX_BLOCKS"]
    for forced in FORCED:
        forced_shape(forced)
        dxa, parta = _out(M, N), _out(MAXB, N)
        nb = C.c_int(0)
        L.check(lib.pbhc_linear_dgrad_act(dya.ptr(), wa.ptr(), sa.ptr() if act else None, dxa.ptr(), parta.ptr(), C.byref(nb), M, N, K, act, L.current_stream()), "dgrad")
        torch.cuda.synchronize()
        assert 1 <= nb.value <= MAXB
        _close(f"dgrad {shape} off {off} forced {forced:#x} dx", dxa.view, ref, TOL)
        _close(f"dgrad {shape} off {off} forced {forced:#x} colsum", parta.view[:nb.value].double().sum(0), ref.sum(0), TOL * max(1.0, M ** 0.5))
        assert dxa.intact() and _rows_behind_untouched(parta, nb.value), forced
    forced_shape(-1)
    dxa = _out(M, N)                                                      # no column sums requested
    L.check(lib.pbhc_linear_dgrad_act(dya.ptr(), wa.ptr(), sa.ptr() if act else None, dxa.ptr(), None, None, M, N, K, act, L.current_stream()), "dgrad")
    torch.cuda.synchronize()
    _close(f"dgrad {shape} off {off} no colsum", dxa.view, ref, TOL)
    assert dxa.intact() and dya.intact() and wa.intact() and sa.intact()


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("shape", [(640, 4, 5), (384, 72, 630), (512, 128, 37), (32, 4, 4)])
def test_linear_wgrad_memory(shape, off):
    L, lib = _lib()
    M, N, K = shape
    g = torch.Generator(device=DEV).manual_seed(M + N + K + off)
    dy = torch.randn(M, N, device=DEV, generator=g)
    x = torch.randn(M, K, device=DEV, generator=g)
    dya, xa = _in(dy, off), _in(x, (off + 1) & 3)
    P = lib.pbhc_linear_wgrad_parts(M, N, K)
    assert 1 <= P <= max(1, (M // 32) // 4)
    dwa, scratch = _out(N, K), _out(P, N * K)                             # scratch: parts * N * K floats, as the header asks
    L.check(lib.pbhc_linear_wgrad(dya.ptr(), xa.ptr(), dwa.ptr(), scratch.ptr(), M, N, K, L.current_stream()), "wgrad")
    torch.cuda.synchronize()
    ref = dy.double().cpu().t() @ x.double().cpu()
    _close(f"wgrad {shape} off {off}", dwa.view, ref, 2e-6 * max(1.0, (M / 1024) ** 0.5) * ref.abs().max().item())
    assert dwa.intact() and scratch.intact() and dya.intact() and xa.intact()


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("mfma", [1, 0])
@pytest.mark.parametrize("shape", [(37, 1, 64), (5, 9, 128), (100, 32, 256), (33, 23, 192)])
def test_linear_out_bwd_memory(shape, mfma, off):
    L, lib = _lib()
    M, A, K = shape
    act = 1 + (off + M) % 3
    g = torch.Generator(device=DEV).manual_seed(31 * off + M + A + K)
    z = torch.randn(M, K, device=DEV, generator=g)                   # pre-activation of the layer below
    h = act64(act, z)
    dy = torch.randn(M, A, device=DEV, generator=g)
    w = torch.randn(A, K, device=DEV, generator=g) / K ** 0.5
    dya, ha, wa = _in(dy, off), _in(h, (off + 1) & 3), _in(w, (off + 2) & 3)
    sa = _in(z, (off + 3) & 3) if act == 2 else None                 # ELU / ReLU: derivative from the output (= h)
    MAXB = L.K["PBHC_ACT_MAX_BLOCKS"]
    dha, pdw, pdb, pcs = _out(M, K), _out(MAXB, A * K), _out(MAXB, A), _out(MAXB, K)
    nb = C.c_int(0)
    lib.pbhc_debug_out_bwd_variant(mfma)        # 1 (default): K = 128 / 256 on the matrix cores; 0: the streaming form for every shape
    try:
        L.check(lib.pbhc_linear_out_bwd(dya.ptr(), ha.ptr(), None if sa is None else sa.ptr(), wa.ptr(), M, A, K, act, dha.ptr(), pdw.ptr(), pdb.ptr(), pcs.ptr(),
                                        C.byref(nb), L.current_stream()), "pbhc_linear_out_bwd")
    finally:
        lib.pbhc_debug_out_bwd_variant(1)
    torch.cuda.synchronize()
    assert 1 <= nb.value <= MAXB
    dd = lambda t: t.double().cpu()
    ref_dh = (dd(dy) @ dd(w)) * _act_grad64(act, dd(z))
    scale = max(1.0, M ** 0.5)
    name = f"out_bwd {shape} mfma {mfma} off {off}"
    _close(name + " dh", dha.view, ref_dh, TOL)
    _close(name + " dw", pdw.view[:nb.value].double().sum(0).view(A, K), dd(dy).t() @ dd(h), TOL * scale)
    _close(name + " db", pdb.view[:nb.value].double().sum(0), dd(dy).sum(0), TOL * scale)
    _close(name + " colsum", pcs.view[:nb.value].double().sum(0), ref_dh.sum(0), TOL * scale)
    assert dha.intact() and all(_rows_behind_untouched(a, nb.value) for a in (pdw, pdb, pcs))
    assert all(a.intact() for a in (dya, ha, wa)) and (sa is None or sa.intact())
