"""The K loop of the LDS-DMA GEMM tile code (`gemm2_tile`, csrc/pbhc_gemm.hip): the two-slot ring under load and at ragged shapes.

Written with a re-placement of the loop's LDS-DMA pieces and barrier (profiles/gemm_kloop_handover.txt: measured, not kept); what does not
depend on that re-placement stays, because it checks the ring itself: a piece written into a slot that is still being read, or read
before it was waited for, makes runs of a launch that fills every CU differ from each other."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 3e-5          # tests/test_gpu_gemm.py: TOL, the bound of these entries against fp64 (column sums: TOL * max(1, sqrt(M)), as there)


def _lib_():
    from pbhc_amd import _lib

    return _lib, _lib.lib()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _fwd(x, w, b, M, N, K, act, setting):
    _lib, lib = _lib_()
    y, pre = _nan(M, N), _nan(M, N)
    lib.pbhc_gemm_debug_force_shape(setting)
    try:
        _lib.check(lib.pbhc_linear_act_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), pre.data_ptr(), M, N, K, act, _lib.current_stream()), "fwd")
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    return y, pre


def _dgrad(dy, w, saved, M, N, K, act, setting):
    _lib, lib = _lib_()
    dx, part, nb = _nan(M, N), _nan(_lib.K["PBHC_ACT_MAX_BLOCKS"] * N), C.c_int(0)
    lib.pbhc_gemm_debug_force_shape(setting)
    try:
        _lib.check(lib.pbhc_linear_dgrad_act(dy.data_ptr(), w.data_ptr(), saved.data_ptr() if act else None, dx.data_ptr(), part.data_ptr(), C.byref(nb),
                                             M, N, K, act, _lib.current_stream()), "dgrad")
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    return dx, part[:nb.value * N].clone(), nb.value


def _fwd_out(x, w, b, wo, bo, M, K, NO, act):
    _lib, lib = _lib_()
    y, pre, out = _nan(M, 128), _nan(M, 128), _nan(M, NO)
    _lib.check(lib.pbhc_linear_act_fwd_out(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), pre.data_ptr(), M, 128, K, act, wo.data_ptr(), bo.data_ptr(),
                                           NO, out.data_ptr(), _lib.current_stream()), "fwd_out")
    return y, pre, out


@pytest.mark.parametrize("mode", [0, 1])
def test_full_chip_runs_agree_with_each_other(mode):
    """768 tiles of 64 x 128, three workgroups on every CU, 24 stages: three runs write the same bits (`y`, `pre` / `dx`, column-sum rows, row-block
    count).  A determinism check on correct code; nothing is provoked."""
    M, N, K = 12288, 512, 768
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(M, K, device="cuda", generator=g)
    if mode == 0:
        w, b = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5, torch.randn(N, device="cuda", generator=g)
        run = lambda: _fwd(x, w, b, M, N, K, 1, 2)
    else:
        w, z = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5, torch.randn(M, N, device="cuda", generator=g)
        run = lambda: _dgrad(x, w, z, M, N, K, 2, 2)
    want = run()
    for t in want:
        assert not (torch.is_tensor(t) and torch.isnan(t).any().item())
    for rep in range(2):
        for i, (p, q) in enumerate(zip(run(), want)):
            assert torch.equal(p, q) if torch.is_tensor(p) else p == q, (mode, rep, i)


# (M, N, K): ragged rows and columns; 2, 20 and 3 stages of 32 with K % 4 = 1, 2, 1 (the straddling chunk's rotate pass) and a partial last stage
@pytest.mark.parametrize("shape", [(200, 132, 37), (97, 260, 630), (130, 4, 65)])
def test_ragged_shapes_match_fp64(shape):
    """forward, input gradient with its column sums, and the forward with the fused output layer against float64 on everything they write"""
    M, N, K = shape
    g = torch.Generator(device="cuda").manual_seed(600 + K)
    x = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(max(N, 128), K, device="cuda", generator=g) / K ** 0.5
    b = torch.randn(max(N, 128), device="cuda", generator=g)
    wt = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
    z = torch.randn(M, N, device="cuda", generator=g)
    wo, bo = torch.randn(23, 128, device="cuda", generator=g) / 128 ** 0.5, torch.randn(23, device="cuda", generator=g)
    for act in (0, 1, 2, 3):
        f = {0: lambda t: t, 1: F.elu, 2: F.silu, 3: F.relu}[act]
        y, pre = _fwd(x, w[:N], b[:N], M, N, K, act, -1)
        zr = x.double() @ w[:N].double().t() + b[:N].double()
        assert (pre.double() - zr).abs().max().item() < TOL and (y.double() - f(zr)).abs().max().item() < TOL

        zd = z.double().clone().requires_grad_(True)
        f(zd).sum().backward()
        ref = (x.double() @ wt.double()) * (zd.grad if act else 1.0)
        dx, part, nb = _dgrad(x, wt, z if act == 2 else f(z), M, N, K, act, -1)
        assert (dx.double() - ref).abs().max().item() < TOL
        assert nb >= 1 and (part.view(nb, N).double().sum(0) - ref.sum(0)).abs().max().item() < TOL * max(1.0, M ** 0.5)

        y, pre, out = _fwd_out(x, w[:128], b[:128], wo, bo, M, K, 23, act)
        zr = x.double() @ w[:128].double().t() + b[:128].double()
        assert (pre.double() - zr).abs().max().item() < TOL and (y.double() - f(zr)).abs().max().item() < TOL
        assert (out.double() - (f(zr) @ wo.double().t() + bo.double())).abs().max().item() < TOL
