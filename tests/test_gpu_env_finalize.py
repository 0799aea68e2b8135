"""The env step's one-workgroup reduction (csrc/pbhc_env_finalize.h) against a plain model of it (tests/finalize_model.py, held to the
reference's own traces by tests/test_env_finalize_model_cpu.py): `k_env_finalize` (1024 threads, through `pbhc_debug_env_finalize`), the rider
workgroup of `k_mlp_fwd` (512 threads, through a one-row `pbhc_mlp_fwd_cat_riders`) and the data-parallel apply (`pbhc_env_finalize`), each on
partial rows / totals, globals and a cursor of the test's choice.

What is compared how:
  * every global slot, the log block included, BIT FOR BIT with the model.  The partial rows hold m * 2**-10 with integer m < 2**20 (every row and
    column distinct and positive): any float64 summation order is exact, the expected totals are `math.fsum`; the scalar chains are IEEE double
    (and, for the average episode length and the batch error mean, fp32) operations in the model's order, the library is built with
    -ffp-contract=off, and double division is correctly rounded on the device;
  * except `end_time_ratio_std`, the one `sqrt`: within 2 ulp of float64 (the device library specifies its double sqrt to 1 ulp).

The partial rows lie in a larger buffer whose other rows hold other positive numbers: a loop that runs one row too far counts them.
Deliberate differences from the reference: see tests/finalize_model.py (one env's `end_time_ratio_std` is 0, not NaN)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests.helpers import SIGMA_MEAN_OVERRIDES, SIGMA_SCALE_OVERRIDES, SOFT_LIMIT_OVERRIDES, TERM_NOISE_OVERRIDES, V2_SIGMA_OVERRIDES, build_hip_env
from tests.test_gpu_reset_options import DOF_FAR
from tests.test_gpu_rollout_riders import _one_row_stack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WALK, STUDENT = "v1_g1_23dof_walk.yaml", "v2_g1_23dof_student.yaml"
CONFIGS = {
    "walk": (WALK, None, False),                                                              # as shipped: sigma "origin", penalty and motion-far curricula
    "walk_curricula": (WALK, dict(SOFT_LIMIT_OVERRIDES, **TERM_NOISE_OVERRIDES, **DOF_FAR), False),     # + noise, soft-limit and dof-far curricula
    "walk_sigmamean": (WALK, SIGMA_MEAN_OVERRIDES, False),
    "walk_sigmascale": (WALK, SIGMA_SCALE_OVERRIDES, False),
    "student_sigma": (STUDENT, dict(V2_SIGMA_OVERRIDES, **{"domain_rand.push_robots": False}), True),   # general tracking: its columns, adaptive_type 3
}
ROWS = [1, 2, 15, 16, 17, 31, 112, 113, 128, 129, 248, 249, 250, 256, 257, 264, 504, 505, 513, 700, 2048]
PAD_ROWS = 272                                       # rows behind the ones handed to the kernel (more than one trip of either unrolled loop)
_envs = {}
_stack = []                                          # the one-row policy stack that carries the rider, made once


def _env(name):
    """(env, cfg mapping read back from the device config): a 16-env env per config, built once per module; nothing modifies it"""
    from pbhc_amd import _lib
    from tests.finalize_model import cfg_from_struct

    if name not in _envs:
        cfgname, overrides, general = CONFIGS[name]
        old = os.environ.get("PBHC_SPECIALISE")
        os.environ["PBHC_SPECIALISE"] = "off"        # (no step runs on these envs: no step kernel to specialise)
        try:
            _, env = build_hip_env(cfgname, 16, overrides=overrides, general=general)
        finally:
            os.environ.pop("PBHC_SPECIALISE") if old is None else os.environ.__setitem__("PBHC_SPECIALISE", old)
        env.reset_all()
        torch.cuda.synchronize()
        c = _lib.PbhcEnvConfig()
        _lib.check(_lib.lib().pbhc_env_get_config(env._env, C.byref(c)), "pbhc_env_get_config")
        _envs[name] = (env, cfg_from_struct(c))
    return _envs[name]


def _K():
    from pbhc_amd import _lib
    return _lib.K


def _G(name):
    return _K()["PBHC_G_" + name]


def _L(name):
    return _K()["PBHC_G_LOG"] + _K()["PBHC_L_" + name]


def _grid_rows(rows, seed=0):
    """[rows + PAD_ROWS, 64] fp32: entry m * 2**-10, m < 2**20 distinct over the whole buffer and positive"""
    NP = _K()["PBHC_NUM_TOTALS"]
    idx = torch.arange((rows + PAD_ROWS) * NP, dtype=torch.int64) + seed * 131
    m = 1 + (idx * 7919) % 1048573                   # 1048573 is prime and > (2048 + PAD_ROWS) * 64: distinct, in [1, 2**20)
    assert int(m.max()) < 2 ** 20 and m.unique().numel() == m.numel()
    return (m.double() * 2.0 ** -10).float().view(rows + PAD_ROWS, NP)


def _totals(buf, rows):
    return np.array([math.fsum(col) for col in buf[:rows].double().T.tolist()])


def _launch(env, form, buf, rows, glob0, num_frames, launches=2, cursor0=0):
    """`launches` reductions in a row of buf[:rows] from the globals `glob0` -> (globals, cursor) as numpy / int"""
    from pbhc_amd import _lib

    lib = _lib.lib()
    glob = torch.as_tensor(glob0, dtype=torch.float64).to(DEV).contiguous()
    cursor = torch.full((1,), cursor0, dtype=torch.int32, device=DEV)
    dbuf = buf.to(DEV).contiguous()
    r = env.finalize_rider()
    r.globals, r.partials, r.frame_cursor, r.num_partial_rows, r.num_frames = glob.data_ptr(), dbuf.data_ptr(), cursor.data_ptr(), rows, num_frames
    assert r.has_finalize == 1 and r.has_post == 0 and 1 <= rows <= dbuf.shape[0] - PAD_ROWS
    if form == "rider":
        if not _stack:
            _stack.append(_one_row_stack() + (torch.zeros(1, 8, device=DEV),))
        inp, w, b, dims, keep, y = _stack[0]
    for _ in range(launches):
        if form == "kernel":
            _lib.check(lib.pbhc_debug_env_finalize(C.byref(r), _lib.current_stream()), "pbhc_debug_env_finalize")
        else:
            _lib.check(lib.pbhc_mlp_fwd_cat_riders(C.byref(inp), w, b, dims, 1, 0, y.data_ptr(), 8, 1, None, C.byref(r), _lib.current_stream()),
                       "pbhc_mlp_fwd_cat_riders")
    torch.cuda.synchronize()
    return glob.cpu().numpy(), int(cursor)


def _ulps(a, b):
    a, b = np.float64(a), np.float64(b)
    assert a >= 0 and b >= 0 and np.isfinite(a) and np.isfinite(b), (a, b)
    return abs(int(a.view(np.int64)) - int(b.view(np.int64)))


def _assert_equals_model(got, want, what):
    """every slot bit for bit, end_time_ratio_std within 2 ulp"""
    std = _L("END_TIME_RATIO_STD")
    d = _ulps(got[std], want[std])
    print(f"{what}: end_time_ratio_std {got[std]!r} vs model {want[std]!r}: {d} ulp")
    assert d <= 2, (what, "end_time_ratio_std", got[std], want[std], d)
    a, b = got.copy(), want.copy()
    a[std] = b[std] = 0.0
    bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
    assert bad.size == 0, (what, [(int(i), float(got[i]), float(want[i])) for i in bad[:8]])


def _model(tot, cfg, glob0, num_frames, launches=2, n=None, cursor0=0, advance=True):
    from tests.finalize_model import finalize_model

    g, cur = np.array(glob0, np.float64), cursor0
    for _ in range(launches):
        g, cur = finalize_model(tot, cfg, g, cur, num_frames, cfg["num_envs"] if n is None else n, advance=advance)
    return g, cur


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS)
def test_column_sums_equal_exact_sums(rows):
    """both callers' hand-unrolled column sums against exact sums, on both sides of every loop's entry and exit condition (512 threads: the
    joint 2 x 16-load loop needs 249 + wave rows, its 8-load loop 113 + chunk; 1024 threads: the 8-load loop needs 113 + wave), two launches in
    a row, with 7 frames and with 1 frame in the replay window; v1 with every curriculum on, and general tracking (its own columns)"""
    buf = _grid_rows(rows, seed=rows)
    tot = _totals(buf, rows)
    for name in ("walk_curricula", "student_sigma"):
        env, cfg = _env(name)
        glob0 = env.globals.cpu().numpy()
        for num_frames in (7, 1):
            want, wcur = _model(tot, cfg, glob0, num_frames)
            assert wcur == 2 % num_frames and want[_G("STEP_COUNTER")] == glob0[_G("STEP_COUNTER")] + 2.0
            for form in ("kernel", "rider"):
                got, cur = _launch(env, form, buf, rows, glob0, num_frames)
                w = f"{name} {form} rows {rows} frames {num_frames}"
                assert cur == 2 % num_frames, w
                assert got[_G("STEP_COUNTER")] == glob0[_G("STEP_COUNTER")] + 2.0, w
                _assert_equals_model(got, want, w)
                assert got[_L("REW_MEAN")] != glob0[_L("REW_MEAN")] and got[_G("AVG_EP_LEN")] != glob0[_G("AVG_EP_LEN")], w     # (the chains ran)


# ---------------------------------------------------------------------------------------------------------------------------------------
CHAIN_ROWS = 129


def _chain_rows(tot):
    """CHAIN_ROWS partial rows whose column totals are `tot` (multiples of 2**-10 below 1024 each: exact in fp32): split over rows 5 and 128, the other
    rows zero, the pad rows positive"""
    NP = _K()["PBHC_NUM_TOTALS"]
    t = torch.as_tensor(np.asarray(tot, np.float64))
    assert bool((t * 1024 == (t * 1024).round()).all()) and bool((t >= 0).all()) and bool((t < 1024).all())
    buf = torch.ones(CHAIN_ROWS + PAD_ROWS, NP, dtype=torch.float64)
    buf[:CHAIN_ROWS] = 0.0
    a = (t * 1024 / 3).floor() / 1024
    buf[5], buf[128] = a, t - a
    buf = buf.float()
    assert np.array_equal(_totals(buf, CHAIN_ROWS), t.numpy())
    return buf


def _base_totals(cfg, nreset=2.0):
    """plausible totals of a step of cfg['num_envs'] envs of which `nreset` were reset"""
    from tests.finalize_model import P

    n = float(cfg["num_envs"])
    tot = np.zeros(_K()["PBHC_NUM_TOTALS"])
    q = lambda x: round(x * 1024) / 1024
    for i in range(_K()["PBHC_NUM_SIGMA"]):
        tot[P["P_ERR"] + i] = q(n * (0.02 + 0.013 * i))
    for j, col in enumerate(("P_UPPER_NORM", "P_LOWER_NORM", "P_VR_NORM", "P_JOINT_NORM", "P_KEY_NORM", "P_LUP_NORM", "P_LLO_NORM", "P_LVR_NORM", "P_LKEY_NORM")):
        tot[P[col]] = q(n * (0.11 + 0.07 * j))
    tot[P["P_CLIP_CNT"]], tot[P["P_REW_SUM"]] = 5.0, q(n * 0.37)
    tot[P["P_RESET_CNT"]], tot[P["P_RESET_EPLEN"]] = nreset, q(nreset * 37.5)
    for j, col in enumerate(("P_TERM_GRAVITY", "P_TERM_FAR", "P_TERM_TIMEOUT", "P_TERM_END", "P_TERM_REFZ", "P_TERM_REFORI", "P_TERM_BODYZ", "P_TERM_CONTACT",
                             "P_TERM_LOWH", "P_TERM_POSLIM", "P_TERM_VELLIM", "P_TERM_TAULIM")):
        tot[P[col]] = float((j % 3) if nreset else 0)
    etr = np.round((0.1 + 0.8 * np.arange(int(n)) / n) * 1024) / 1024            # a spread of end-time ratios: a positive variance
    tot[P["P_ETR_SUM"]], tot[P["P_ETR_SQ"]] = q(float(etr.sum())), q(float((etr * etr).sum()))
    return tot


def _both_forms(env, cfg, tot, glob0, what, launches=1):
    """one launch of each form from `glob0` on rows that add up to `tot`: both equal the model -> the globals they left"""
    buf = _chain_rows(tot)
    want, _ = _model(tot, cfg, glob0, 7, launches=launches)
    for form in ("kernel", "rider"):
        got, cur = _launch(env, form, buf, CHAIN_ROWS, glob0, 7, launches=launches)
        assert cur == launches % 7
        _assert_equals_model(got, want, f"{what} {form}")
    return got


@pytest.mark.parametrize("name,kind", [("walk", 0), ("walk_sigmamean", 1), ("walk_sigmascale", 2), ("student_sigma", 3)])
def test_sigma_chain_of_every_type(name, kind):
    """the four adaptive_type values: active slots whose EMA lands above the current sigma, below it, and (x 1.1) above it but below it once
    scaled by 0.8; an inactive slot with a non-zero error total stays what it was"""
    env, cfg = _env(name)
    assert cfg["adaptive_sigma"] == 1 and cfg["adaptive_type"] == kind
    NS = _K()["PBHC_NUM_SIGMA"]
    active = [i for i in range(NS) if cfg["sigma_active"][i]]
    idle = [i for i in range(NS) if not cfg["sigma_active"][i]]
    assert len(active) >= 4 and idle
    glob0 = env.globals.cpu().numpy()
    tot = _base_totals(cfg)
    from tests.finalize_model import P

    factors = (1.5, 0.5, 1.1, 0.9)
    for j, i in enumerate(active):
        glob0[_G("SIGMA") + i] = 0.25 + 0.125 * j
        glob0[_G("EMA") + i] = glob0[_G("SIGMA") + i] * factors[j % 4]
        tot[P["P_ERR"] + i] = round(cfg["num_envs"] * glob0[_G("EMA") + i] * 1.01 * 1024) / 1024        # the batch mean: 1 % beyond the EMA
    for i in idle:
        glob0[_G("SIGMA") + i], glob0[_G("EMA") + i] = 0.75, 1.25
    got = _both_forms(env, cfg, tot, glob0, name)
    s, e = got[_G("SIGMA"):_G("SIGMA") + NS], got[_G("EMA"):_G("EMA") + NS]
    s0 = glob0[_G("SIGMA"):_G("SIGMA") + NS]
    for i in idle:
        assert s[i] == 0.75 and e[i] == 1.25
    for j, i in enumerate(active):                     # the case is what it says, and the rule is the type's (motion_tracking.py:1039-1048, general_tracking.py:977-991)
        f = factors[j % 4]
        assert (e[i] > s0[i]) == (f > 1.0) and e[i] != glob0[_G("EMA") + i]
        want = {0: min(e[i], s0[i]), 1: (min(e[i], s0[i]) + e[i]) / 2, 2: min(e[i] * cfg["adaptive_scale"], s0[i]), 3: e[i]}[kind]
        assert s[i] == want, (i, f, s[i], want)
    if kind == 2:
        assert abs(cfg["adaptive_scale"] - 0.8) < 1e-6 and any(s[i] < s0[i] < e[i] for i in active)     # the x 1.1 slots: only "scale" lowers sigma there


def _curricula(cfg):
    """(slot, down, up, degree, min, max, widens when episodes are short) of every curriculum the config has on"""
    out = []
    if cfg["penalty_curriculum"]:
        out.append(("PENALTY_SCALE", cfg["penalty_down"], cfg["penalty_up"], cfg["penalty_degree"], cfg["penalty_min"], cfg["penalty_max"], False))
    for q, (on, slot) in enumerate((("soft_pos_curriculum", "SOFT_POS_VAL"), ("soft_vel_curriculum", "SOFT_VEL_VAL"), ("soft_tau_curriculum", "SOFT_TAU_VAL"))):
        if cfg[on]:
            out.append((slot,) + tuple(cfg[k][q] for k in ("soft_cur_down", "soft_cur_up", "soft_cur_degree", "soft_cur_min", "soft_cur_max")) + (True,))
    if cfg["noise_curriculum"]:
        out.append(("NOISE_CURRICULUM", cfg["noise_down"], cfg["noise_up"], cfg["noise_degree"], cfg["noise_min"], cfg["noise_max"], False))
    if cfg["terminate_when_motion_far"] and cfg["motion_far_curriculum"]:
        out.append(("MOTION_FAR_THR",) + tuple(cfg["motion_far_" + k] for k in ("down", "up", "degree", "min", "max")) + (True,))
    if cfg["terminate_when_dof_far"] and cfg["dof_far_curriculum"]:
        out.append(("DOF_FAR_THR",) + tuple(cfg["dof_far_" + k] for k in ("down", "up", "degree", "min", "max")) + (True,))
    return out


@pytest.mark.parametrize("name,slots", [("walk", {"PENALTY_SCALE", "SOFT_POS_VAL", "SOFT_VEL_VAL", "SOFT_TAU_VAL", "MOTION_FAR_THR"}),     # (soft limits: on, pinned by min == max)
                                        ("walk_curricula", {"PENALTY_SCALE", "SOFT_POS_VAL", "SOFT_VEL_VAL", "SOFT_TAU_VAL", "NOISE_CURRICULUM", "MOTION_FAR_THR", "DOF_FAR_THR"}),
                                        ("student_sigma", None)])
def test_every_curriculum_branch_and_clamp(name, slots):
    """each curriculum the config has on, with the average episode length below `down`, strictly between the thresholds, above `up`, and from a
    start value that the move pushes through the min / the max clamp.  Two resets of 10000 (num_compute_average_epl) move the average by
    2e-4 of its distance to this step's lengths: it stays on the side of the thresholds where the case put it."""
    env, cfg = _env(name)
    cur = _curricula(cfg)
    assert slots is None or {c[0] for c in cur} == slots
    assert cfg["num_compute_average_epl"] >= 1000
    tot = _base_totals(cfg)
    for slot, down, up, degree, lo, hi, widen in cur:
        assert down + 1.0 < up and 0.0 <= degree < 1.0 and lo <= hi
        mid = 0.5 * (lo + hi)
        short, long_ = down - 3.0, up + 3.0
        cases = [("below", short, mid), ("between", 0.5 * (down + up), mid), ("above", long_, mid),
                 ("clamp min", long_ if widen else short, lo), ("clamp max", short if widen else long_, hi)]
        for what, avg0, v0 in cases:
            glob0 = env.globals.cpu().numpy()
            glob0[_G("AVG_EP_LEN")], glob0[_G(slot)] = avg0, v0
            got = _both_forms(env, cfg, tot, glob0, f"{name} {slot} {what}")
            v, avg = got[_G(slot)], got[_G("AVG_EP_LEN")]
            w = (name, slot, what, v0, v)
            assert avg != avg0 and (avg < down) == (avg0 < down) and (avg > up) == (avg0 > up), w
            if what == "between":
                assert v == v0, w
            elif what == "clamp min":
                assert v == lo, w
            elif what == "clamp max":
                assert v == hi, w
            elif lo < hi:                              # a free move: up when (short episodes and it widens) or (long episodes and it does not)
                grows = (what == "below") == widen
                assert v == min(max(v0 * (1.0 + degree if grows else 1.0 - degree), lo), hi) and (v > v0) == grows, w


@pytest.mark.parametrize("name", ["walk_curricula", "student_sigma"])
def test_step_without_a_reset_keeps_the_reset_chains(name):
    """no reset in the batch: the per-cause means are what the reference's `/ (mean(reset_buf) + 1e-15)` gives, and the average-length chain, the
    curricula and the end-time-ratio slots keep their old values"""
    from tests.finalize_model import P

    env, cfg = _env(name)
    tot = _base_totals(cfg, nreset=0.0)
    tot[P["P_TERM_GRAVITY"]], tot[P["P_TERM_TIMEOUT"]] = 3.0, 1.0      # (not a state a step leaves: the formula itself, at a zero reset fraction)
    glob0 = env.globals.cpu().numpy()
    keep = [_G(s) for s in ("AVG_EP_LEN", "PENALTY_SCALE", "SOFT_POS_VAL", "SOFT_VEL_VAL", "SOFT_TAU_VAL", "NOISE_CURRICULUM", "MOTION_FAR_THR", "DOF_FAR_THR")]
    keep += [_L("END_TIME_RATIO"), _L("END_TIME_RATIO_STD")]
    glob0[keep] = 0.5 + 0.0625 * np.arange(len(keep))
    glob0[_G("AVG_EP_LEN")] = 1.0                                       # (below every `down`: a curriculum that ran would move)
    got = _both_forms(env, cfg, tot, glob0, name + " no reset")
    assert np.array_equal(got[keep], glob0[keep])
    n = float(cfg["num_envs"])
    assert got[_L("TERM_GRAVITY")] == (3.0 / n) / 1e-15 and got[_L("TERM_TIME_OUT")] == (1.0 / n) / 1e-15 and got[_L("TERM_MOTION_FAR")] == 0.0
    assert got[_L("RESET_FRAC")] == 0.0 and got[_L("NUM_RESETS")] == 0.0
    assert got[_L("REW_MEAN")] == tot[P["P_REW_SUM"]] / n


def test_dof_far_flag_is_logged_and_cleared():
    """terminate_when_dof_far: the pre-pass's hit flag is the logged mean (over the reset fraction), the threshold logged is the one the step
    used, and the flag is cleared for the next step"""
    from tests.finalize_model import P

    env, cfg = _env("walk_curricula")
    assert cfg["terminate_when_dof_far"] == 1 and cfg["dof_far_curriculum"] == 1
    n = float(cfg["num_envs"])
    for hit in (1.0, 0.0):
        tot = _base_totals(cfg, nreset=n if hit else 2.0)              # a hit resets every env
        glob0 = env.globals.cpu().numpy()
        glob0[_G("DOF_FAR_HIT")], glob0[_G("DOF_FAR_THR")], glob0[_G("AVG_EP_LEN")] = hit, 1.75, 10.0
        got = _both_forms(env, cfg, tot, glob0, f"dof far hit {hit}")
        assert got[_L("TERM_DOF_FAR")] == hit / ((n if hit else 2.0) / n + 1e-15) and got[_G("DOF_FAR_HIT")] == 0.0
        assert got[_L("DOF_FAR_THR")] == 1.75 and got[_G("DOF_FAR_THR")] == 1.75 * (1.0 + cfg["dof_far_degree"])
        got2 = _both_forms(env, cfg, tot, glob0, f"dof far hit {hit}, two launches", launches=2)
        assert got2[_L("TERM_DOF_FAR")] == 0.0                         # the second launch saw the cleared flag


@pytest.mark.parametrize("name", ["walk_curricula", "student_sigma"])
def test_data_parallel_apply_equals_the_model(name):
    """`pbhc_env_finalize(env, totals, n_total)`: the apply half on totals summed over ranks equals the model at n = n_total and leaves the step
    counter (and the replay cursor: it is not even handed one) alone.  With one env in all, `end_time_ratio_std` is 0 where torch's std() of
    one element is NaN."""
    from pbhc_amd import _lib
    from tests.finalize_model import P

    env, cfg = _env(name)
    saved = env.globals.clone()
    cursor0 = env.simulator.frame_cursor.clone()
    try:
        for n_total, tot in ((3.0 * cfg["num_envs"], _base_totals(cfg, nreset=5.0)), (1.0, None)):
            if tot is None:                            # one env, reset, end-time ratio 0.5: variance estimate 0 / 0
                tot = np.zeros(_K()["PBHC_NUM_TOTALS"])
                tot[P["P_RESET_CNT"]], tot[P["P_RESET_EPLEN"]], tot[P["P_ETR_SUM"]], tot[P["P_ETR_SQ"]] = 1.0, 7.0, 0.5, 0.25
            glob0 = saved.cpu().numpy()
            glob0[_G("AVG_EP_LEN")], glob0[_L("END_TIME_RATIO_STD")] = 10.0, 0.375
            env.globals.copy_(torch.from_numpy(glob0).to(DEV))
            dtot = torch.from_numpy(tot).to(DEV)
            _lib.check(_lib.lib().pbhc_env_finalize(env._env, dtot.data_ptr(), n_total, _lib.current_stream()), "pbhc_env_finalize")
            torch.cuda.synchronize()
            got = env.globals.cpu().numpy()
            want, _ = _model(tot, cfg, glob0, 1, launches=1, n=n_total, advance=False)
            _assert_equals_model(got, want, f"{name} apply n_total {n_total}")
            assert got[_G("STEP_COUNTER")] == glob0[_G("STEP_COUNTER")] and torch.equal(env.simulator.frame_cursor, cursor0)
            assert got[_G("AVG_EP_LEN")] != 10.0 and got[_L("RESET_FRAC")] == tot[P["P_RESET_CNT"]] / n_total
            if n_total == 1.0:
                assert got[_L("END_TIME_RATIO")] == 0.5 and got[_L("END_TIME_RATIO_STD")] == 0.0
    finally:
        env.globals.copy_(saved)
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [13, 272])
def test_log_block_follows_from_the_steps_own_outputs(N):
    """no oracle: after a real step the log block is what the step's own per-env outputs imply.  Counts (resets, the reset fraction, the
    time-out share) exactly; `reward_mean` and `end_time_ratio` against the float64 mean of the returned fp32 values within 2**-22 * mean(|x|)
    (a workgroup pre-adds its four envs in fp32: three fp32 additions of relative error 2**-24 each, with a margin of 2; every later addition is
    a double one); the average-length chain and the curricula keyed on it through the model, exactly (sums of integers).  Scalar reward
    (use_vec_reward off), so that the returned value IS the summand.  N = 13: a partly filled last workgroup; N = 272: 136 partial rows, both
    unrolled loops and the tail.  Episode lengths are scripted as in tests/test_gpu_rollout_riders.py: env i times out at step i % 3."""
    import bench
    from tests.finalize_model import P, cfg_from_struct
    from pbhc_amd import _lib

    T = 3
    torch.manual_seed(11)
    np.random.seed(11)
    _, env = build_hip_env(WALK, N, overrides={"env.config.use_vec_reward": False})
    c = _lib.PbhcEnvConfig()
    _lib.check(_lib.lib().pbhc_env_get_config(env._env, C.byref(c)), "pbhc_env_get_config")
    cfg = cfg_from_struct(c)
    env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, T + 2, seed=5))
    gen = torch.Generator(device=DEV).manual_seed(3)
    assert env.finalize_rider().num_partial_rows == 2 * ((N + 3) // 4)
    for k in range(T):
        # env i times out at step i % T.  Laid out again before every step: an episode that long is far past the clip's end, where the
        # reference pose no longer matches the replay frame, so motion-far resets most envs in the first step and would wipe a pattern laid
        # out once
        env._episode_length_buf[k::T] = int(env.max_episode_length)
        env.wait_finalize()
        before = env.globals.cpu().numpy()
        obs, rew, reset, extras = env.step({"actions": 0.3 * torch.randn(N, env.num_dof, device=DEV, generator=gen)})
        env.wait_finalize()
        torch.cuda.synchronize()
        got = env.globals.cpu().numpy()
        w = f"N {N} step {k}: "
        rs = reset.bool().cpu()
        touts = extras["time_outs"].bool().cpu()
        nreset, ntout = int(rs.sum()), int(touts.sum())
        assert nreset > 0 and ntout > 0 and bool((rs | ~touts).all()), w + "the script left this step without a reset / a time-out"
        rfrac = nreset / float(N)
        assert got[_L("NUM_RESETS")] == float(nreset) and got[_L("RESET_FRAC")] == rfrac, w
        assert got[_L("TERM_TIME_OUT")] == (ntout / float(N)) / (rfrac + 1e-15), w
        assert rew.shape == (N,) and rew.dtype == torch.float32
        for slot, x in (("REW_MEAN", rew), ("END_TIME_RATIO", env.end_time_ratio_buf)):
            x = x.double().cpu()
            ref, tol = float(x.mean()), 2.0 ** -22 * float(x.abs().mean())
            print(f"{w}{slot} {got[_L(slot)]!r} vs {ref!r}: off by {abs(got[_L(slot)] - ref):.3e}, bound {tol:.3e}")
            assert ref != 0.0 and abs(got[_L(slot)] - ref) <= tol, w + slot
        assert env.read_log()["reward_mean"] == got[_L("REW_MEAN")] and env.read_log()["end_time_ratio"] == got[_L("END_TIME_RATIO")]
        # the average-length chain: totals that are sums of integers -> through the model, exactly
        tot = np.zeros(_K()["PBHC_NUM_TOTALS"])
        tot[P["P_RESET_CNT"]] = float(nreset)
        tot[P["P_RESET_EPLEN"]] = float(env.last_episode_length_buf.cpu()[rs].sum())
        want, _ = _model(tot, cfg, before, T + 2, launches=1)
        for slot in ("AVG_EP_LEN", "PENALTY_SCALE", "MOTION_FAR_THR", "SOFT_POS_VAL", "SOFT_VEL_VAL", "SOFT_TAU_VAL", "STEP_COUNTER"):
            assert got[_G(slot)] == want[_G(slot)], w + f"{slot}: {got[_G(slot)]!r} vs the model's {want[_G(slot)]!r}"
        assert got[_G("AVG_EP_LEN")] != before[_G("AVG_EP_LEN")] and got[_G("PENALTY_SCALE")] != before[_G("PENALTY_SCALE")], w
