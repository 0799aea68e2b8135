"""Failure-weighted start-time sampling: the per-bin collector (k_start_stats), the fold (k_start_sampling_update) and the start-time draw
(k_start_draw) against numpy restatements in this file; then the env, the rollout graph and two ranks.

The window is integer-only and the collector's phases are the same IEEE double operations as numpy's (the library is built with
-ffp-contract=off), so every comparison of the window is exact.  Tolerances of the update — the ones tests/test_gpu_clip_sampling.py applies
to the clip rule: V and F are double operations cast to float32 once -> bit-equal; the look-ahead weights are formed in the same order ->
prob differs only by the ORDER of the double sum over the bins (relative error <= K * 2^-53), which can flip the final rounding to float32
and no more -> within 1 ulp of float32.  The draw is handed the SAME double CDF as the restatement: bins and start times are bit-equal."""
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
RULE = dict(decay=0.9, prior=1.0, floor=0.1, lam=0.8)
DT = 0.02
U_MAX = np.float32(16777215.0 / 16777216.0)                       # the largest value u01 returns


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------
def ref_window(reset, tout, ratio, length, slot, clip_len, dt, M, K):
    w = np.zeros((M, K, 2), np.int64)
    ok = (reset != 0) & (slot >= 0) & (slot < M)
    c = slot[ok]
    pe = ratio[ok].astype(np.float32).astype(np.float64)
    ps = pe - (length[ok].astype(np.float64) * float(dt)) / clip_len.astype(np.float32)[c].astype(np.float64)
    fin = np.isfinite(pe) & np.isfinite(ps)
    c, pe, ps, fail = c[fin], pe[fin], ps[fin], (tout[ok][fin] == 0).astype(np.int64)
    e = np.clip(np.floor(pe * K), 0, K - 1).astype(np.int64)
    s = np.minimum(np.clip(np.floor(ps * K), 0, K - 1).astype(np.int64), e)
    np.add.at(w[:, :, 0], (c, s), 1)
    stop = e + 1 < K
    np.add.at(w[:, :, 0], (c[stop], e[stop] + 1), -1)
    np.add.at(w[:, :, 1], (c, e), fail)
    return w


def ref_update(V, F, window, decay, prior, floor, H, lam):
    """-> V', F', p (float32 [M,K]), cdf (double) from float32 V, F and the int64 window"""
    M, K = V.shape
    v, f = np.cumsum(window[:, :, 0], axis=1), window[:, :, 1]
    V2 = (decay * V.astype(np.float64) + v.astype(np.float64)).astype(np.float32)
    F2 = (decay * F.astype(np.float64) + f.astype(np.float64)).astype(np.float32)
    r = (F2.astype(np.float64) + prior) / (V2.astype(np.float64) + prior)
    w, pw = np.zeros((M, K)), 1.0
    for u in range(H):                                                               # no wrap-around
        w[:, :K - u] += pw * r[:, u:]
        pw *= lam
    p = ((1.0 - floor) * w / w.sum(axis=1, keepdims=True) + floor / K).astype(np.float32)
    return V2, F2, p, np.cumsum(p.astype(np.float64), axis=1)


def ref_draw(cdf, clip_len, slot, seed, counter, salt, u=None):
    """-> (bin, start_time float32, near): `near` marks envs whose target lies within 1e-9 of an edge of its clip's CDF"""
    N, K = len(slot), cdf.shape[1]
    if u is None:
        o = _philox4x32_7(int(seed), np.arange(N, dtype=np.int64), int(counter), 21, int(salt))
        u = np.stack([(o[k] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0) for k in (0, 1)], axis=1)
    rows = cdf[slot]
    target = u[:, 0].astype(np.float64) * rows[:, K - 1]
    b = np.minimum((rows <= target[:, None]).sum(axis=1), K - 1)                     # rows are non-decreasing: the first index past the target
    near = (np.abs(target[:, None] - rows) < 1e-9).any(axis=1)
    length = clip_len.astype(np.float32)[slot]
    t = (((b.astype(np.float64) + u[:, 1].astype(np.float64)) / K) * length.astype(np.float64)).astype(np.float32)
    return b, np.minimum(t, np.nextafter(length, np.float32(0.0))), near


def within_one_ulp32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all())


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check_update(dev, ref, what=""):
    """dev / ref: (V, F, p, cdf) — the tolerances of the module docstring"""
    assert bits_equal(dev[0], ref[0]), what + "V"
    assert bits_equal(dev[1], ref[1]), what + "F"
    assert within_one_ulp32(dev[2], ref[2]), what + "p"
    K = dev[2].shape[1]
    c = np.asarray(dev[3])
    assert np.abs(c[:, -1] - 1.0).max() <= K * 2.0**-24, what + "cdf total"
    assert (np.diff(c, axis=1) > 0).all() and np.abs(c - np.cumsum(np.asarray(dev[2]).astype(np.float64), axis=1)).max() < 1e-12, what + "cdf"


# ---- device calls ------------------------------------------------------------------------------------------------------------------
def tg(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def collect(reset, tout, ratio, length, slot, clip_len, dt, window):
    """numpy episode arrays -> k_start_stats into the device tensor `window` [M,K,2]"""
    t = [tg(reset.astype(np.int64)), tg(tout.astype(np.uint8)), tg(ratio.astype(np.float32)), tg(length.astype(np.int64)), tg(slot.astype(np.int64)),
         tg(clip_len.astype(np.float32))]
    _lib.check(_lib.lib().pbhc_start_stats(*[x.data_ptr() for x in t], float(dt), len(reset), window.shape[0], window.shape[1], window.data_ptr(),
                                           _lib.current_stream()), "pbhc_start_stats")
    torch.cuda.synchronize()


def synth_episodes(N, M, K, mode, seed, stray=False):
    """-> reset, tout, ratio, length, slot, clip_len.  Random phases lie at least 1e-4 from a bin edge (start and end); the first entries are
    exactly representable edge phases (0, 0.5, 1, 1.25 with length 0: start == end), then non-finite ratios."""
    rng = np.random.default_rng(seed)
    reset = {"zeros": np.zeros(N, np.int64), "ones": np.ones(N, np.int64), "random": (rng.random(N) < 0.5).astype(np.int64)}[mode]
    tout = ((reset != 0) & (rng.random(N) < 0.4)).astype(np.uint8)
    clip_len = rng.uniform(2.0, 60.0, M).astype(np.float32)
    slot = rng.integers(0, M, N).astype(np.int64)
    ratio, length = np.zeros(N, np.float32), np.zeros(N, np.int64)
    todo = np.arange(N)
    for _ in range(200):
        r = rng.uniform(0.0, 1.1, len(todo)).astype(np.float32)
        steps_to_end = np.floor(r.astype(np.float64) * clip_len[slot[todo]].astype(np.float64) / DT)
        ln = (rng.random(len(todo)) * (steps_to_end + 1)).astype(np.int64)
        pe = r.astype(np.float64)
        ps = pe - (ln.astype(np.float64) * DT) / clip_len[slot[todo]].astype(np.float64)
        far = lambda x: np.abs(x * K - np.rint(x * K)) >= 1e-4 * K
        good = far(pe) & far(ps)
        ratio[todo[good]], length[todo[good]] = r[good], ln[good]
        todo = todo[~good]
        if len(todo) == 0:
            break
    assert len(todo) == 0
    special = np.array([0.0, 0.5, 1.0, 1.25, np.nan, np.inf, -np.inf], np.float32)
    n = min(N, len(special))
    ratio[:n], length[:n] = special[:n], 0
    if stray:                                                                        # skipped, never used as an index
        slot[5], slot[9], slot[11] = -1, M, 2**40
    return reset, tout, ratio, length, slot, clip_len


# ---- 1. the collector alone --------------------------------------------------------------------------------------------------------
# (the collector's workgroup is 256 threads: 259, 1100 and 4099 cross it; M = 1 sends every add through the LDS histogram, M = 70 nearly
# every add straight to memory, M = 3 mixes the two)
@pytest.mark.parametrize("N,M,K,stray", [(1, 1, 1, False), (67, 1, 8, False), (67, 3, 5, False), (67, 3, 5, True), (259, 70, 32, False),
                                         (1100, 1, 64, False), (4099, 3, 128, False)])
@pytest.mark.parametrize("mode", ["zeros", "ones", "random"])
def test_collector_equals_numpy_and_accumulates(N, M, K, stray, mode):
    a = synth_episodes(N, M, K, mode, seed=100 + N + M, stray=stray)
    b = synth_episodes(N, M, K, "random", seed=200 + N + M, stray=stray)
    b = b[:5] + (a[5],)                                                              # the same clips
    window = torch.zeros(M, K, 2, dtype=torch.int64, device=DEV)
    collect(*a, DT, window)
    wa = ref_window(*a, DT, M, K)
    assert torch.equal(window.cpu(), torch.from_numpy(wa))
    finite = int((np.isfinite(a[2]) & (a[0] != 0) & (a[4] >= 0) & (a[4] < M)).sum())
    visits = np.cumsum(wa[:, :, 0], axis=1)
    assert (visits >= 0).all() and (visits >= wa[:, :, 1]).all()                     # a failure lies in a bin its episode visited
    if mode == "zeros":
        assert not wa.any()
    if mode == "ones":
        assert int(visits.max(axis=1).sum()) <= finite and int(wa[:, :, 0].clip(min=0).sum()) >= (finite > 0)
    collect(*b, DT, window)                                                          # the sum, not an overwrite
    assert torch.equal(window.cpu(), torch.from_numpy(wa + ref_window(*b, DT, M, K)))


def test_collector_edge_phases_by_hand():
    """dt 0.25 and an 8 s clip: length / 32 is exact.  K = 8."""
    K = 8
    #                 end phase, length -> start phase            bins (s, e)
    rows = [(0.0, 0),            # 0                              (0, 0)
            (0.0, 4),            # -0.125: clamped                (0, 0)
            (0.5, 0),            # 0.5: the edge belongs to bin 4 (4, 4)
            (0.5, 16),           # 0                              (0, 4)
            (1.0, 0),            # 1: clamped to the last bin     (7, 7)
            (1.0, 4),            # 0.875                          (7, 7)
            (1.25, 8),           # 1 -> both clamped              (7, 7)
            (0.375, 1)]          # 0.34375                        (2, 3)
    ratio, length = np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int64)
    N = len(rows)
    tout = np.array([0, 1, 0, 0, 1, 0, 0, 0], np.uint8)
    want = np.zeros((1, K, 2), np.int64)
    for (s, e), to in zip([(0, 0), (0, 0), (4, 4), (0, 4), (7, 7), (7, 7), (7, 7), (2, 3)], tout):
        want[0, s, 0] += 1
        if e + 1 < K:
            want[0, e + 1, 0] -= 1
        want[0, e, 1] += int(to == 0)
    args = (np.ones(N, np.int64), tout, ratio, length, np.zeros(N, np.int64), np.array([8.0], np.float32))
    assert np.array_equal(ref_window(*args, 0.25, 1, K), want)                       # the restatement says what the hand says
    window = torch.zeros(1, K, 2, dtype=torch.int64, device=DEV)
    collect(*args, 0.25, window)
    assert torch.equal(window.cpu(), torch.from_numpy(want))
    assert np.cumsum(want[0, :, 0]).tolist() == [3, 1, 2, 2, 2, 0, 0, 3]


# ---- 2. the update alone -----------------------------------------------------------------------------------------------------------
def synth_window(M, K, rng, episodes=40):
    w = np.zeros((M, K, 2), np.int64)
    n = M * episodes
    c = rng.integers(0, M, n)
    e = rng.integers(0, K, n)
    s = (rng.random(n) * (e + 1)).astype(np.int64)
    np.add.at(w[:, :, 0], (c, s), 1)
    stop = e + 1 < K
    np.add.at(w[:, :, 0], (c[stop], e[stop] + 1), -1)
    np.add.at(w[:, :, 1], (c, e), (rng.random(n) < 0.6).astype(np.int64))
    if M > 1:
        w[0] = 0                                                                     # a clip nobody played: stays uniform
    return w


def device_update(window, V, F, P, cdf, H, rule=RULE):
    M, K = P.shape
    _lib.check(_lib.lib().pbhc_start_sampling_update(window.data_ptr(), V.data_ptr(), F.data_ptr(), P.data_ptr(), cdf.data_ptr(), M, K, rule["decay"],
                                                     rule["prior"], rule["floor"], H, rule["lam"], _lib.current_stream()), "update")
    torch.cuda.synchronize()


@pytest.mark.parametrize("M", [1, 3, 257])
@pytest.mark.parametrize("K,H", [(1, 1), (5, 1), (5, 4), (5, 5), (128, 1), (128, 4), (128, 128)])
def test_update_equals_the_numpy_rule(M, K, H):
    rng = np.random.default_rng(1000 * M + K + H)
    V, F, P = (torch.zeros(M, K, device=DEV) for _ in range(3))
    cdf = torch.zeros(M, K, dtype=torch.float64, device=DEV)
    Vh, Fh = np.zeros((M, K), np.float32), np.zeros((M, K), np.float32)
    for rnd in range(2):                                                             # the second time with non-zero V, F
        w = synth_window(M, K, rng)
        window = tg(w)
        device_update(window, V, F, P, cdf, H)
        ref = ref_update(Vh, Fh, w, RULE["decay"], RULE["prior"], RULE["floor"], H, RULE["lam"])
        check_update((V.cpu().numpy(), F.cpu().numpy(), P.cpu().numpy(), cdf.cpu().numpy()), ref, f"M {M} K {K} H {H} round {rnd}: ")
        Vh, Fh = ref[0], ref[1]
        assert int(window.abs().sum()) == 0                                          # the window is cleared
        if M > 1 and rnd == 0 and H == 1:                                            # an unseen clip: r = 1 in every bin, a uniform law
            assert len(set(P[0].cpu().numpy().tolist())) == 1


def test_update_every_episode_fails_in_the_last_bin():
    """K = 6, H = 4, a hundred episodes from bin 0 that all fail in bin 5: r_5 = 1, r_b = 1 / 101 below.  The look-ahead credits the bins
    that lead into the failure, the closer the more: p_5 > p_4 > p_3 > p_2 > p_1 = p_0."""
    K, H, n = 6, 4, 100
    w = np.zeros((1, K, 2), np.int64)
    w[0, 0, 0], w[0, 5, 1] = n, n
    V, F, P = (torch.zeros(1, K, device=DEV) for _ in range(3))
    cdf = torch.zeros(1, K, dtype=torch.float64, device=DEV)
    device_update(tg(w), V, F, P, cdf, H)
    ref = ref_update(np.zeros((1, K), np.float32), np.zeros((1, K), np.float32), w, RULE["decay"], RULE["prior"], RULE["floor"], H, RULE["lam"])
    check_update((V.cpu().numpy(), F.cpu().numpy(), P.cpu().numpy(), cdf.cpu().numpy()), ref)
    assert V[0].tolist() == [float(n)] * K and F[0].tolist() == [0.0] * 5 + [float(n)]
    p = P[0].cpu().numpy().astype(np.float64)
    assert p[5] > p[4] > p[3] > p[2] > p[1] and abs(p[1] - p[0]) < 1e-7
    q, lam = 1.0 / (n + 1.0), RULE["lam"]
    wb = np.array([q * (1 + lam + lam**2 + lam**3)] * 2 + [q * (1 + lam + lam**2) + lam**3, q * (1 + lam) + lam**2, q + lam, 1.0])
    assert np.abs(p - ((1 - RULE["floor"]) * wb / wb.sum() + RULE["floor"] / K)).max() < 1e-7


# ---- 3. the draw alone -------------------------------------------------------------------------------------------------------------
def synth_law(M, K, rng, zeros=True):
    """-> (cdf [M,K] double, clip_len [M] float32) of a random law with bins of probability 0"""
    p = rng.random((M, K)).astype(np.float32)
    if zeros and K > 3:
        p[rng.random((M, K)) < 0.2] = 0.0
        p[:, 1] = 0.5                                                                # (no empty row)
        p[:, 0] = 0.0                                                                # a leading and a trailing bin nobody may get
        p[:, K - 1] = 0.0
    p = (p / p.sum(axis=1, dtype=np.float64, keepdims=True)).astype(np.float32)
    return np.cumsum(p.astype(np.float64), axis=1), rng.uniform(2.0, 60.0, M).astype(np.float32), p


def device_draw(cdf, clip_len, slot, seed, counter, salt, reset=None, u=None, start=None):
    N, (M, K) = len(slot), cdf.shape
    start = torch.full((N,), -7.0, device=DEV) if start is None else start
    t = [tg(cdf.astype(np.float64)), tg(clip_len.astype(np.float32)), tg(slot.astype(np.int64)), None if reset is None else tg(reset.astype(np.int64)),
         None if u is None else tg(u.astype(np.float32)), torch.tensor([float(counter), -1.0], dtype=torch.float64, device=DEV)]
    P = lambda x: None if x is None else x.data_ptr()
    _lib.check(_lib.lib().pbhc_start_draw(P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), N, M, K, int(seed), P(t[5]), int(salt), start.data_ptr(),
                                          _lib.current_stream()), "pbhc_start_draw")
    torch.cuda.synchronize()
    return start.cpu().numpy()


def _pick_seed(cdf, clip_len, slot, counter, salt, base):
    """a seed (with high key bits) for which the REFERENCE leaves no env near a CDF edge: chosen on the CPU, before the device is asked"""
    for k in range(64):
        if not ref_draw(cdf, clip_len, slot, base + k, counter, salt)[2].any():
            return base + k
    raise AssertionError("no seed without a near-edge env")


@pytest.mark.parametrize("M,K", [(1, 1), (1, 8), (3, 5), (70, 32), (3, 128)])
@pytest.mark.parametrize("N", [13, 4096])
def test_draw_equals_the_restatement(M, K, N):
    rng = np.random.default_rng(7 * M + K + N)
    cdf, clip_len, p = synth_law(M, K, rng)
    slot = rng.integers(0, M, N).astype(np.int64)
    seen = {}
    for counter, salt in ((3, 0), (4, 0), (3, 1)):
        seed = _pick_seed(cdf, clip_len, slot, counter, salt, (0x1234 << 32) + 77 * M + K)
        got = device_draw(cdf, clip_len, slot, seed, counter, salt)
        b, want, near = ref_draw(cdf, clip_len, slot, seed, counter, salt)
        assert not near.any() and bits_equal(got, want)                              # every env, bit for bit
        assert (got >= 0).all() and (got < clip_len[slot]).all()
        assert not (p[slot, b] == 0).any()                                           # the restated bins: never one of probability 0
        seen[(counter, salt)] = (seed, got)
        # the bins themselves: the same u1 with u2 = 0.5 puts every start in the middle of its bin
        o = _philox4x32_7(int(seed), np.arange(N, dtype=np.int64), counter, 21, salt)[0]
        u = np.stack([(o >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0), np.full(N, 0.5, np.float32)], axis=1)
        mid = device_draw(cdf, clip_len, slot, seed, counter, salt, u=u)
        got_bin = np.floor(mid.astype(np.float64) / clip_len[slot].astype(np.float64) * K).astype(np.int64)
        assert np.array_equal(got_bin, b) and bits_equal(mid, ref_draw(cdf, clip_len, slot, seed, counter, salt, u=u)[1])
    if K > 1 and N == 4096:                                                          # the counter and the salt key the stream
        for other in ((4, 0), (3, 1)):
            if seen[other][0] == seen[(3, 0)][0]:
                assert not np.array_equal(seen[other][1], seen[(3, 0)][1])


def test_draw_stays_below_the_clip_length_at_the_largest_u2():
    """(K - 1 + u2) / K * len rounds to len in float32 for the largest u2: the result is the largest float below len instead"""
    K = 128
    clip_len = np.array([60.0, 3.3, 2.0, 17.123456], np.float32)
    M = len(clip_len)
    cdf = np.cumsum(np.full((M, K), 1.0 / K), axis=1)
    slot = np.arange(4 * M, dtype=np.int64) % M
    u = np.stack([np.full(len(slot), U_MAX), np.full(len(slot), U_MAX)], axis=1)
    u[M:2 * M, 1] = np.float32(0.999999)                                             # also below the rounding edge
    got = device_draw(cdf, clip_len, slot, 1, 0, 0, u=u)
    b, want, _ = ref_draw(cdf, clip_len, slot, 1, 0, 0, u=u)
    assert (b == K - 1).all() and bits_equal(got, want) and (got < clip_len[slot]).all()
    unclamped = (((K - 1 + u[:, 1].astype(np.float64)) / K) * clip_len[slot].astype(np.float64)).astype(np.float32)
    assert (unclamped >= clip_len[slot]).any()                                       # the case exists: without the clamp this test fails
    assert bits_equal(got[:M], np.nextafter(clip_len, np.float32(0)))


def test_draw_with_reset_buf_leaves_the_other_envs_alone_and_skips_stray_clips():
    M, K, N = 3, 8, 259
    rng = np.random.default_rng(5)
    cdf, clip_len, p = synth_law(M, K, rng)
    slot = rng.integers(0, M, N).astype(np.int64)
    slot[5], slot[9], slot[11] = -1, M, 2**40
    reset = (rng.random(N) < 0.5).astype(np.int64)
    reset[[5, 9, 11]] = 1
    held = rng.uniform(0, 1, N).astype(np.float32)
    got = device_draw(cdf, clip_len, slot, 99, 12, 0, reset=reset, start=tg(held))
    ok = (reset != 0) & (slot >= 0) & (slot < M)
    want = ref_draw(cdf, clip_len, np.where(ok, slot, 0), 99, 12, 0)[1]
    assert ok.sum() > 50 and (~ok).sum() > 50
    assert bits_equal(got[ok], want[ok]) and bits_equal(got[~ok], held[~ok])


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
            env.last_episode_length_buf.cpu().numpy().copy(), env._motion_lib.slot_clip.cpu().numpy().copy(),
            env._motion_lib._motion_lengths.cpu().numpy().copy())


def _counter(env):
    return int(env.globals[_lib.K["PBHC_G_STEP_COUNTER"]].item())


def _walk(env, M, K, steps=12):
    """reset_all + `steps` control steps with the buffers read back after each: the window against the restatement of what the steps left, the
    start times the resets took against the buffer before the step, the buffer after the step against the restated draw"""
    import bench

    N = env.num_envs
    assert env._start["sampling"] and env._start_window.shape == (M, K, 2) and env._start_time.shape == (N,)
    assert env._io.ovr_start_time == env._start_time.data_ptr()
    ml = env._motion_lib
    cdf, clip_len = ml._start_cdf.cpu().numpy(), ml._motion_lengths.cpu().numpy()
    assert np.abs(cdf - np.arange(1, K + 1) / K).max() < 1e-6                        # a fresh table is uniform
    table = np.zeros((M, K, 2), np.int64)
    env.reset_all()                                                                  # (every env takes its buffered start time) + step 1
    torch.cuda.synchronize()
    table += ref_window(*_read_episodes(env), env.dt, M, K)
    tout_envs = [40, 41]
    env.motion_start_times[tout_envs] = env.motion_len[tout_envs] - 2.5 * env.dt     # time-outs
    root, qp, qv, cf = bench.make_replay_on_device(env, steps + 2, seed=5)
    for k in range(1, steps, 2):                                                     # failures: a few roots 1 m above the reference, every other frame
        root[k, [(3 * k + j) % N for j in range(5)], 2] += 1.0
    env.simulator.set_replay(root, qp, qv, cf)
    act = torch.zeros(N, env.num_dof, device=DEV)
    resets = touts = 0
    for step in range(steps):
        torch.cuda.synchronize()
        before = env._start_time.cpu().numpy().copy()
        env.step({"actions": act})
        torch.cuda.synchronize()
        eps = _read_episodes(env)
        table += ref_window(*eps, env.dt, M, K)
        r = eps[0] != 0
        resets += int(r.sum())
        touts += int((r & (eps[1] != 0)).sum())
        assert torch.equal(env._start_window.cpu(), torch.from_numpy(table)), step
        assert bits_equal(env.motion_start_times.cpu().numpy()[r], before[r]), step  # the reset path took the buffered start time
        after = env._start_time.cpu().numpy()
        want = ref_draw(cdf, clip_len, eps[4], env._seed, _counter(env), 0)[1]
        assert bits_equal(after[r], want[r]) and bits_equal(after[~r], before[~r]), step
        assert (after >= 0).all() and (after < clip_len[eps[4]]).all()
    visits = np.cumsum(table[:, :, 0], axis=1)
    assert resets > 0 and table[:, :, 1].sum() >= 1 and visits.max() >= 1 and (visits >= table[:, :, 1]).all(), table
    assert touts >= 1                                                                # a time-out as well
    st = env.start_statistics()
    assert torch.equal(st["visits"].cpu(), torch.from_numpy(visits)) and torch.equal(st["failures"].cpu(), torch.from_numpy(table[:, :, 1]))
    log = env.read_log()
    assert abs(log["start_sampling_concentration"] - 1.0) < 1e-5                     # still uniform
    f = table[:, :, 1].sum(axis=0)
    assert abs(log["start_failure_bin_mean"] - (f * np.arange(K)).sum() / f.sum()) < 1e-9
    # the fold: the numpy rule on that table, a fresh start time for every env
    c = env._start
    assert env.update_start_sampling() is True
    torch.cuda.synchronize()
    zero = np.zeros((M, K), np.float32)
    ref = ref_update(zero, zero, table, c["decay"], c["prior_episodes"], c["uniform_floor"], c["lookahead_bins"], c["lookahead_decay"])
    check_update((ml._start_visits.cpu().numpy(), ml._start_failures.cpu().numpy(), ml._start_prob.cpu().numpy(), ml._start_cdf.cpu().numpy()), ref, "env: ")
    assert int(env._start_window.abs().sum()) == 0 and env.read_log()["start_sampling_concentration"] > 1.0
    want = ref_draw(ml._start_cdf.cpu().numpy(), clip_len, eps[4], env._seed, _counter(env), env._start_redraws)[1]
    assert env._start_redraws >= 2 and bits_equal(env._start_time.cpu().numpy(), want)
    obs, _, _, _ = env.step({"actions": act})
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() for v in obs.values())


def test_env_v1_walk_collects_and_resets_from_the_buffer():
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 67, overrides={"env.config.start_sampling": {"enable": True, "bins": 8}})
    _walk(env, 1, 8)


def test_env_v2_teacher_three_clips_collects_and_resets_from_the_buffer():
    cfg, env = _teacher_env(67, {"env.config.start_sampling": {"enable": True, "bins": 8}})
    _walk(env, 3, 8)


# ---- 5. rollout graph = eager loop -------------------------------------------------------------------------------------------------
_ROLLOUTS = {}


def _rollouts(graph):
    if graph in _ROLLOUTS:
        return _ROLLOUTS[graph]
    import bench
    from pbhc_amd.agents.mh_ppo import MHPPO

    os.environ["PBHC_ROLLOUT_GRAPH"], os.environ["PBHC_ROLLOUT_SPLIT"] = str(int(graph)), "1"
    try:
        torch.manual_seed(11)
        np.random.seed(11)
        cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 64, noise_off=False, overrides={"env.config.start_sampling": {"enable": True, "bins": 8}})
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
        algo.setup()
        algo._train_mode()
        obs = env.reset_all()
        env.simulator.set_replay(*bench.make_replay_on_device(env, 4 * algo.num_steps_per_env + 2, seed=5))
        used, out = [], {}
        ml = env._motion_lib
        for r in range(4):
            algo.storage.clear()
            obs = algo._rollout_step(obs)                # (ends with the fold: update_every_rollouts = 1)
            used.append(bool(getattr(algo, "_rollout_used_graph", False)))
            out[f"prob_after_rollout_{r}"] = ml._start_prob.clone()
            out[f"start_time_after_rollout_{r}"] = env._start_time.clone()
        torch.cuda.synchronize()
        out.update({k: getattr(algo.storage, k).clone() for k in algo.storage.stored_keys})
        out.update(globals=env.globals.clone(), window=env._start_window.clone(), start_time=env._start_time.clone(), prob=ml._start_prob.clone(),
                   visits=ml._start_visits.clone(), failures=ml._start_failures.clone(), cdf=ml._start_cdf.clone(),
                   motion_start_times=env.motion_start_times.clone())
        out["redraws"] = torch.tensor(env._start_redraws)
        _ROLLOUTS[graph] = (out, used)
        return out, used
    finally:
        os.environ.pop("PBHC_ROLLOUT_GRAPH", None)
        os.environ.pop("PBHC_ROLLOUT_SPLIT", None)


def test_start_tables_of_the_graph_rollout_equal_the_eager_loop():
    """the collector and the draw inside the captured rollout (on the finalize stream) are a schedule, not arithmetic: the integer window,
    the start-time buffer, the tables of every fold between two replays and the rollout buffers are bit-identical to the eager loop"""
    (a, used_a), (b, used_b) = _rollouts(1), _rollouts(0)
    assert used_a == [False, True, True, True] and not any(used_b)
    assert float(a["visits"].sum()) > 0                                              # episodes ended, and were folded
    assert not torch.equal(a["prob_after_rollout_3"], torch.full_like(a["prob"], 1.0 / 8))
    assert int(a["window"].abs().sum()) == 0                                         # (the last rollout ended with a fold)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 6. off is off; suspended, not refused -----------------------------------------------------------------------------------------
def test_off_means_no_buffers_no_pointer_and_no_log_keys():
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", 4)
    assert env._start["statistics"] is False and env._start["sampling"] is False
    assert env._start_window is None and env._start_time is None and not env._io.ovr_start_time
    ml = env._motion_lib
    assert ml._start_visits is None and ml._start_failures is None and ml._start_prob is None and ml._start_cdf is None
    env.reset_all()
    env.step({"actions": torch.zeros(4, env.num_dof, device=DEV)})
    assert not env._io.ovr_start_time and not any(k.startswith("start_") for k in env.read_log())
    for call in (env.start_statistics, env.clear_start_statistics, env.update_start_sampling):
        with pytest.raises(_lib.PbhcError, match="start_statistics"):
            call()


def test_statistics_only_collects_without_a_buffer():
    N = 8
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", N, overrides={"env.config.start_statistics": True})
    assert env._start["statistics"] and not env._start["sampling"] and env._start_time is None and not env._io.ovr_start_time
    assert env._start_window.shape == (1, 32, 2)
    env.reset_all()
    torch.cuda.synchronize()
    table = ref_window(*_read_episodes(env), env.dt, 1, 32)
    assert torch.equal(env._start_window.cpu(), torch.from_numpy(table))
    assert "start_failure_bin_mean" in env.read_log()
    env.clear_start_statistics()
    assert int(env._start_window.abs().sum()) == 0


def _tables(env):
    ml = env._motion_lib
    return [t.clone() for t in (env._start_window, env._start_time, ml._start_visits, ml._start_failures, ml._start_prob, ml._start_cdf)]


def test_evaluation_and_library_sweep_suspend_and_leave_the_tables_alone():
    N = 4
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", N, overrides={"env.config.start_sampling": {"enable": True, "bins": 8}})
    env.reset_all()
    env.reset_buf.fill_(1)                                                           # a window that is not empty, a law that is not uniform
    env._launch_start_sampling(_lib.current_stream())
    env.update_start_sampling()
    env._launch_start_sampling(_lib.current_stream())
    torch.cuda.synchronize()
    live = env._start_time.data_ptr()
    assert env._io.ovr_start_time == live and int(env._start_window.abs().sum()) > 0
    act = torch.zeros(N, env.num_dof, device=DEV)
    # injected start times win while set; clearing them re-points the buffer
    inj = torch.zeros(N, device=DEV)
    env.set_injected_draws(start_time=inj)
    assert env._io.ovr_start_time == inj.data_ptr()
    env.set_injected_draws()
    assert env._io.ovr_start_time == live
    # evaluation
    before, epoch = _tables(env), env._io_epoch
    env.set_is_evaluating()
    assert not env._io.ovr_start_time and env._io_epoch > epoch
    for _ in range(3):
        env.reset_buf.fill_(1)
        env.step({"actions": act})
    assert env.update_start_sampling() is False
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, _tables(env)))
    env.is_evaluating = False
    assert env._io.ovr_start_time == live                                            # the pointer is back
    # the sweep (it leaves the env evaluating, as before: the pointer returns with the flag)
    env.library_sweep(lambda obs: act, max_steps=4, sync_every=2)
    torch.cuda.synchronize()
    assert env.is_evaluating and not env._io.ovr_start_time and not env._start_suspended
    assert all(torch.equal(a, b) for a, b in zip(before, _tables(env)))
    env.is_evaluating = False
    assert env._io.ovr_start_time == live
    env.step({"actions": act})
    torch.cuda.synchronize()


# ---- 7. two ranks ------------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


TWO_RANK_K = 8


def _two_rank_episodes(rnd, rank, clip_len):
    return synth_episodes(67, 3, TWO_RANK_K, "random", seed=10 * rnd + rank)[:5] + (clip_len,)


def _start_rank_main(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        N = 13
        cfg, env = _teacher_env(N, {"env.config.start_sampling": {"enable": True, "bins": TWO_RANK_K}})
        ml = env._motion_lib
        clip_len = ml._motion_lengths.cpu().numpy()
        rows = []
        for rnd in range(2):
            collect(*_two_rank_episodes(rnd, rank, clip_len), DT, env._start_window)
            env.update_start_sampling()
            torch.cuda.synchronize()
            rows.append(dict(V=ml._start_visits.cpu().numpy(), F=ml._start_failures.cpu().numpy(), p=ml._start_prob.cpu().numpy(),
                             cdf=ml._start_cdf.cpu().numpy(), window=env._start_window.cpu().numpy(), clip_len=clip_len))
        torch.save(rows, out_path + f".{rank}")
    finally:
        dist.destroy_process_group()


def test_two_ranks_fold_the_summed_windows(tmp_path):
    world, M, K = 2, 3, TWO_RANK_K
    out = str(tmp_path / "start.pt")
    mp.spawn(_start_rank_main, args=(world, _free_port(), out), nprocs=world, join=True)
    rows = [torch.load(out + f".{rank}", weights_only=False) for rank in range(world)]
    clip_len = rows[0][0]["clip_len"]
    assert np.array_equal(clip_len, rows[1][0]["clip_len"])
    V, F = np.zeros((M, K), np.float32), np.zeros((M, K), np.float32)
    for rnd in range(2):
        w = sum(ref_window(*_two_rank_episodes(rnd, rank, clip_len), DT, M, K) for rank in range(world))
        assert w[:, :, 1].sum() > 0
        ref = ref_update(V, F, w, 0.9, 1.0, 0.1, 4, 0.8)
        for rank in range(world):
            r = rows[rank][rnd]
            check_update((r["V"], r["F"], r["p"], r["cdf"]), ref, f"rank {rank} round {rnd}: ")
            assert not r["window"].any()
        assert np.array_equal(rows[0][rnd]["p"], rows[1][rnd]["p"])                  # every rank holds the same law
        V, F = ref[0], ref[1]
