"""The weight-stationary input gradient (k_dgrad_ws in pbhc_gemm.hip): `dx = (dy[M, 128] . W[128, N]) * act'(saved)` with the 128 x 128 slice
of W held in LDS by a persistent workgroup whose two four-wave teams take alternate 32-row tiles.

It runs the ring kernel's (k_gemm2<1, 1, 4, 1, 1, 32, 2>) arithmetic per tile, so every comparison with the ring path — kept reachable as
staging variant 4 of `pbhc_gemm_debug_force_shape` — is bit for bit: `torch.equal` on guard-filled dx and column-sum buffers and on the
row-block count.  Three cases are also held to float64 at the bound of tests/test_gpu_gemm.py, so that the equality is not one of two empty
results.  M 224 / 229 are seven row tiles / seven and a ragged eighth: with 1-3 workgroups a team runs several tiles (the steady state of the
role alternation and its drain) and the teams run different counts; M 1-33 are the row edges, N 4 / 132 the column edges, N 256 / 512
several column slices."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_gemm import TOL, _act_grad_ref, _act_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = -12345.0
RING = 4 << 16                                                         # staging variant 4: the K = 128 input gradients stay on the ring kernel
WGS = (0, 1, 2, 3, 5)                                                  # workgroups of the stationary kernel: automatic, and forced


def _L():
    from pbhc_amd import _lib

    return _lib, _lib.lib()


def _problem(seed, M, N, K):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dy = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(K, N, device=DEV, generator=g) / K ** 0.5
    zpre = torch.randn(M, N, device=DEV, generator=g)
    saved = {0: None, 1: _act_ref(1, zpre), 2: zpre, 3: _act_ref(3, zpre)}     # SiLU: the pre-activation; ELU / ReLU: the activation's output
    return dict(dy=dy, w=w, zpre=zpre, saved=saved, M=M, N=N, K=K)


def _bufs(p, scratch=True):
    MAXB = _L()[0].K["PBHC_ACT_MAX_BLOCKS"]
    return dict(dx=torch.full((p["M"] + 3, p["N"]), GUARD, device=DEV), part=torch.full((MAXB * p["N"],), GUARD, device=DEV) if scratch else None, nb=C.c_int(-1))


def _args(p, o, act):
    s = p["saved"][act]
    return (p["dy"].data_ptr(), p["w"].data_ptr(), None if s is None else s.data_ptr(), o["dx"].data_ptr(), None if o["part"] is None else o["part"].data_ptr(),
            C.byref(o["nb"]), p["M"], p["N"], p["K"], act)


def _single(p, act, setting, scratch=True):
    """pbhc_linear_dgrad_act on 32 x 128 tiles under a diagnosis setting (bits 16-23 staging variant, 24-30 workgroup count)"""
    L, lib = _L()
    o = _bufs(p, scratch)
    lib.pbhc_gemm_debug_force_shape(4 | setting)
    try:
        L.check(lib.pbhc_linear_dgrad_act(*_args(p, o, act), L.current_stream()), "pbhc_linear_dgrad_act")
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    return o


def _pair(ps, act, setting=None):
    L, lib = _L()
    os_ = [_bufs(p) for p in ps]
    if setting is not None:
        lib.pbhc_gemm_debug_force_shape(0xff | setting)
    try:
        L.check(lib.pbhc_linear_dgrad_act_pair(*_args(ps[0], os_[0], act), *_args(ps[1], os_[1], act), L.current_stream()), "pbhc_linear_dgrad_act_pair")
    finally:
        lib.pbhc_gemm_debug_force_shape(-1)
    return os_


def _assert_same(p, got, want, what):
    nb = (p["M"] + 31) // 32
    assert got["nb"].value == want["nb"].value == nb, what
    assert torch.equal(got["dx"], want["dx"]), what
    assert bool((got["dx"][p["M"]:] == GUARD).all()) and not bool((got["dx"][:p["M"]] == GUARD).any()), what
    if got["part"] is not None:
        assert torch.equal(got["part"], want["part"]), what
        assert bool((got["part"][nb * p["N"]:] == GUARD).all()) and not bool((got["part"][:nb * p["N"]] == GUARD).any()), what


@pytest.mark.parametrize("N", [4, 128, 132, 256, 512])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 224, 229])
def test_stationary_equals_ring_bit_for_bit(M, N):
    """every activation (0 with saved == NULL), with and without the column sums, every workgroup count"""
    p = _problem(1000 * M + N, M, N, 128)
    for act in (0, 1, 2, 3):
        for scratch in (True, False):
            ring = _single(p, act, RING, scratch)
            for wgs in WGS:
                _assert_same(p, _single(p, act, wgs << 24, scratch), ring, (act, scratch, wgs))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shapes", [((229, 512), (33, 256)), ((33, 256), (229, 512)), ((229, 256), (33, 256)), ((33, 256), (229, 256)),
                                    ((224, 132), (224, 132))], ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
@pytest.mark.parametrize("act", [1, 0], ids=["elu", "none"])
def test_pair_equals_two_single_calls(shapes, act):
    """the larger problem goes first in the grid (equal N: the first given), so both orders; against ring singles, under every workgroup count"""
    ps = [_problem(77 + 13 * j + m + n, m, n, 128) for j, (m, n) in enumerate(shapes)]
    ring = [_single(p, act, RING) for p in ps]
    for wgs in WGS:
        for j, o in enumerate(_pair(ps, act, (wgs << 24) if wgs else None)):
            _assert_same(ps[j], o, ring[j], (wgs, j))
    for j, o in enumerate(_pair(ps, act, RING)):                       # and the ring pair is still there behind the variant
        _assert_same(ps[j], o, ring[j], ("ring pair", j))
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,act,wgs", [(229, 512, 1, 0), (224, 132, 2, 2), (33, 4, 3, 1)])
def test_stationary_against_float64(M, N, act, wgs):
    """dx against dy.double() @ W.double() * act', the partial rows against the float64 column sums of each 32-row block"""
    p = _problem(5 + M + N, M, N, 128)
    o = _single(p, act, wgs << 24)
    torch.cuda.synchronize()
    ref = (p["dy"].double() @ p["w"].double()) * _act_grad_ref(act, p["zpre"].double())
    err = (o["dx"][:M].double() - ref).abs().max().item()
    nb = o["nb"].value
    pad = torch.zeros(nb * 32, N, device=DEV, dtype=torch.float64)
    pad[:M] = ref
    perr = (o["part"][:nb * N].view(nb, N).double() - pad.view(nb, 32, N).sum(1)).abs().max().item()
    print(f"M {M} N {N} act {act}: dx err {err:.3e}, column-sum err {perr:.3e} (bound {TOL:.0e})")
    assert nb == (M + 31) // 32
    assert err < TOL and perr < TOL


@pytest.mark.parametrize("K", [36, 64])
def test_other_reductions_stay_on_the_ring_kernel(K):
    """K != 128: the automatic choice (with a workgroup count forced for the stationary kernel, which must not matter) equals the ring path
    through both entries — the variant that pins the ring kernel changes nothing for them"""
    ps = [_problem(300 + K, 229, 512, K), _problem(301 + K, 33, 256, K)]
    for act in (1, 0):
        ring = [_single(p, act, RING) for p in ps]
        for j, p in enumerate(ps):
            _assert_same(p, _single(p, act, 0), ring[j], ("single", j))
            _assert_same(p, _single(p, act, 2 << 24), ring[j], ("single, 2 workgroups", j))
        for setting in (None, 2 << 24, RING):
            for j, o in enumerate(_pair(ps, act, setting)):
                _assert_same(ps[j], o, ring[j], ("pair", setting, j))
        ref = (ps[0]["dy"].double() @ ps[0]["w"].double()) * (_act_grad_ref(act, ps[0]["zpre"].double()) if act else 1.0)
        assert (ring[0]["dx"][:229].double() - ref).abs().max().item() < TOL
    torch.cuda.synchronize()
