"""FloatingBaseSim's per-env randomisation without a GPU (pbhc_amd/simulator/floating_sim.py, `domain_rand`): the config section and its
refusals, the per-env inertial table, the stability screen at the corner of the ranges, the new fields of the ABI and their argument checks,
and the calibration of the GPU tests' bound on the float32 restatement of the per-env models (tests/test_gpu_floating_dr.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.simulator import floating_sim as fsim
from pbhc_amd.skeleton import Skeleton
from tests import floating_dr_inputs as di
from tests import floating_model as fm
from tests.helpers import GOLDEN, fixture_config
from tests.test_floating_sim_cpu import G1, GAMMA, H, LAW, POINTS, TREE, WALK, _construct, _good

FLAGS = ("link_mass", "base_com", "friction", "push")
NEW_FIELDS = ("env_inertial", "env_friction", "push_counter", "push_interval", "push_vel", "u_push", "push_lo", "push_hi", "max_push_vel_xy",
              "push_fixed")


# ---- the config section ---------------------------------------------------------------------------------------------------------------------
def test_the_section_is_accepted_and_an_unknown_sub_key_is_refused_by_name():
    """(on a simulator without the feature `domain_rand` itself is an unknown key)"""
    for spec in ({}, dict.fromkeys(FLAGS, False), dict(base_com=True), dict(link_mass=True, base_com=True, push=True)):
        with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
            _construct(_good(domain_rand=spec))
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):             # all four, at a slip velocity that passes the corner
        _construct(_good(slip_velocity=0.6, domain_rand=dict.fromkeys(FLAGS, True)))
    with pytest.raises(_lib.PbhcError, match=r"floating_sim\.domain_rand\.link_inertia: unknown key \(known: link_mass, base_com, friction, push\)"):
        _construct(_good(domain_rand=dict(link_mass=True, link_inertia=True)))
    with pytest.raises(_lib.PbhcError, match=r"floating_sim\.domain_rand\.push: expected true or false, got 1"):
        _construct(_good(domain_rand=dict(push=1)))
    with pytest.raises(_lib.PbhcError, match=r"floating_sim\.domain_rand: expected a mapping"):
        _construct(_good(domain_rand=True))
    assert fsim.FloatingBaseSim.parse_domain_rand(None) == dict.fromkeys(FLAGS, False)
    assert fsim.FloatingBaseSim.parse_domain_rand(dict(friction=True)) == dict(link_mass=False, base_com=False, friction=True, push=False)


# ---- the inertial table -----------------------------------------------------------------------------------------------------------------
def test_inertial_table():
    g1, tree = Skeleton.from_mjcf(os.path.join(GOLDEN, G1)), Skeleton.from_mjcf(TREE)
    table_of = fsim.FloatingBaseSim.inertial_table
    N = 5
    rng = np.random.default_rng(3)
    for sk in (g1, tree):
        B, names_all = sk.num_bodies, list(sk.body_names)
        names = [names_all[b] for b in (0, 2, B - 1)]
        scale = rng.uniform(0.5, 2.0, (N, 3)).astype(np.float32)
        bias = rng.uniform(-0.05, 0.05, (N, 3)).astype(np.float32)
        t = table_of(sk, names, scale, bias)
        assert isinstance(t, np.ndarray) and t.dtype == np.float32 and t.shape == (N, 32, 4)
        assert not t[:, B:].any(), "rows >= B must be zero"
        mass, com = np.asarray(sk.body_mass, np.float32)[:B], np.asarray(sk.body_com, np.float32)[:B]
        want = np.tile(mass, (N, 1))
        for i, b in enumerate((0, 2, B - 1)):
            want[:, b] = mass[b] * scale[:, i]
        assert np.array_equal(t[:, :B, 0], want), "named bodies scaled, all others as they are"
        where = names_all.index("torso_link") if "torso_link" in names_all else 0
        assert (where != 0) == (sk is g1) and (sk is g1 or "torso_link" not in names_all)
        wc = np.tile(com, (N, 1, 1))
        wc[:, where] = com[where] + bias
        assert np.array_equal(t[:, :B, 1:], wc), "the bias lands on torso_link (G1); on the root link of the tree, which has neither torso_link nor pelvis"
        # torch in = numpy in; one of the two operands alone; the identity
        assert np.array_equal(table_of(sk, names, torch.from_numpy(scale), torch.from_numpy(bias)), t)
        assert np.array_equal(table_of(sk, names, scale, None)[:, :B, 1:], np.tile(com, (N, 1, 1)))
        assert np.array_equal(table_of(sk, [], None, bias)[:, :B, 0], np.tile(mass, (N, 1)))
        ident = table_of(sk, names, np.ones((N, 3), np.float32), np.zeros((N, 3), np.float32))
        assert np.array_equal(ident[:, :B, 0], np.tile(mass, (N, 1))) and np.array_equal(ident[:, :B, 1:], np.tile(com, (N, 1, 1)))
    # a skeleton WITHOUT torso_link whose pelvis is not body 0: the bias lands on the body named pelvis, not on the root
    B = g1.num_bodies
    other = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    names = list(other.body_names)
    at_torso, at_new = names.index("torso_link"), 5
    names[0], names[at_torso], names[at_new] = "base_link", "chest_link", "pelvis"
    other.body_names = names
    bias = rng.uniform(-0.05, 0.05, (N, 3)).astype(np.float32)
    t = table_of(other, [], None, bias)
    com = np.asarray(other.body_com, np.float32)[:B]
    wc = np.tile(com, (N, 1, 1))
    wc[:, at_new] = com[at_new] + bias
    assert at_new not in (0, at_torso) and np.array_equal(t[:, :B, 1:], wc), "without torso_link the bias belongs on the body NAMED pelvis"
    # ... and with neither name it lands on the root link, body 0 (the documented fallback; the hand-written tree above)
    names[at_new] = "hip_link"
    wc = np.tile(com, (N, 1, 1))
    wc[:, 0] = com[0] + bias
    assert np.array_equal(table_of(other, [], None, bias)[:, :B, 1:], wc)
    assert list(g1.body_names)[0] == "pelvis"
    bad = np.ones((N, 1), np.float32)
    bad[3, 0] = 0.0
    with pytest.raises(_lib.PbhcError, match=r"floating_sim\.domain_rand\.link_mass: the root link 'pelvis' has no mass in env 3"):
        table_of(g1, ["pelvis"], bad, None)
    bad[3, 0] = -0.5
    with pytest.raises(_lib.PbhcError, match=r"floating_sim\.domain_rand\.link_mass: the mass of 'torso_link' in env 3 is negative"):
        table_of(g1, ["torso_link"], bad, None)
    with pytest.raises(_lib.PbhcError, match=r"randomize_link_body_names: 'left_foot' is no body of the skeleton"):
        table_of(g1, ["left_foot"], np.ones((N, 1), np.float32), None)
    with pytest.raises(_lib.PbhcError, match=r"mass_scale: expected \[5, 2\]"):
        table_of(g1, ["pelvis", "torso_link"], np.ones((N, 3), np.float32), None)


# ---- the screen at the corner ---------------------------------------------------------------------------------------------------------------
def test_the_screen_is_taken_at_the_corner_of_the_ranges():
    """the shipped walk config at the section's defaults passes nominally (tests/test_floating_sim_cpu.py) and with the flags whose ranges
    it survives; at friction_range[1] = 1.2 the default slip velocity of 0.4 m/s does not pass and the refusal names the corner and the
    remedies; a link_mass_range that reaches down to a tenth makes the PD's and the contact's margins fail at ITS low end.  The margins are
    the hand-computable ones: the slope scales with friction x weight, 1 / Ht with the low masses."""
    cfg = fixture_config(WALK, 4, {"robot.motion.asset.assetFileName": G1})
    g1 = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    pts = fsim.FloatingBaseSim.parse_points(POINTS, g1)
    args = (cfg.env.config, g1, np.full(23, 0.02), pts, 10000.0, 100.0, 0.8)
    g = np.array([0.0, 0.0, -9.81])
    check = fsim.FloatingBaseSim.check_model
    nominal = check(*args, 0.4, g)
    assert check(*args, 0.4, g, domain_rand=None) == nominal == check(*args, 0.4, g, domain_rand=dict.fromkeys(FLAGS, False))
    assert check(*args, 0.4, g, domain_rand=dict(base_com=True, push=True)) == nominal, "the COM bias and the push are left out of the screen"
    light = check(*args, 0.4, g, domain_rand=dict(link_mass=True))
    lo, hi = (float(x) for x in cfg.env.config.domain_rand.link_mass_range)
    named = [list(g1.body_names).index(n) for n in cfg.env.config.domain_rand.randomize_link_body_names]
    mass = np.asarray(g1.body_mass, np.float64)
    heavy = mass.copy(); heavy[named] *= hi
    assert abs(light["weight"] - heavy.sum() * 9.81) < 1e-9 * light["weight"] and light["weight"] > nominal["weight"]
    assert light["a_pd"] > nominal["a_pd"] and light["a_n"] > nominal["a_n"] and light["b_n"] > nominal["b_n"] and light["b_t"] > nominal["b_t"]
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the regularised friction is unstable .*stable needs b < 2, at domain_rand\.friction_range\[1\] = 1\.2 "
                                             r"\(raise simulator\.config\.sim\.fps or the slip_velocity"):
        check(*args, 0.4, g, domain_rand=dict(friction=True))
    with pytest.raises(_lib.PbhcError, match=r"at domain_rand\.friction_range\[1\] = 1\.2 and domain_rand\.link_mass_range\[1\] = 1\.1 and "
                                             r"domain_rand\.link_mass_range\[0\] = 0\.9 \(raise"):
        check(*args, 0.4, g, domain_rand=dict(friction=True, link_mass=True))
    both = check(*args, 0.6, g, domain_rand=dict(friction=True, link_mass=True))
    assert both["friction"] == 1.2 and both["b_t"] < 2.0
    # the slope is friction x weight / slip / points: from the nominal's by hand
    assert abs(both["tangential_slope"] - nominal["tangential_slope"] * (1.2 / 0.8) * (0.4 / 0.6) * light["weight"] / nominal["weight"]) < 1e-9 * both["tangential_slope"]
    # through the constructor, with the flag's switch off the screen is the nominal one
    with pytest.raises(_lib.PbhcError, match=r"regularised friction is unstable .*at domain_rand\.friction_range\[1\] = 1\.2"):
        _construct(_good(domain_rand=dict(friction=True)))
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct(_good(domain_rand=dict(friction=True)), {"domain_rand.randomize_friction": False})
    # a range that fails at its low end
    # (a normal damping of 160 N s / m and a slip velocity of 2 m / s: passes nominally and on the shipped range, b_n 1.56)
    damped = args[:5] + (160.0, 0.8)
    assert check(*damped, 2.0, g)["b_n"] < check(*damped, 2.0, g, domain_rand=dict(link_mass=True))["b_n"] < 2.0
    cfg.env.config.domain_rand.link_mass_range = [0.1, 1.1]
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the explicit contact is unstable .*stable needs b < 2 and a \+ 2 b < 4, at "
                                             r"domain_rand\.link_mass_range\[0\] = 0\.1 \(raise simulator\.config\.sim\.fps, lower the stiffness"):
        check(*damped, 2.0, g, domain_rand=dict(link_mass=True))
    with pytest.raises(_lib.PbhcError, match=r"regularised friction is unstable .*at domain_rand\.link_mass_range\[0\] = 0\.1 and "
                                             r"domain_rand\.link_mass_range\[1\] = 1\.1 \(raise"):
        check(*args, 0.4, g, domain_rand=dict(link_mass=True))
    cfg.env.config.domain_rand.link_mass_range = [-0.1, 1.1]
    with pytest.raises(_lib.PbhcError, match=r"domain_rand\.link_mass: at domain_rand\.link_mass_range\[0\] = -0\.1 a link mass is negative"):
        check(*args, 0.4, g, domain_rand=dict(link_mass=True))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_fields_of_the_abi():
    lib = _lib.lib()
    E = _lib.K["PBHC_EINVAL"]
    assert lib.pbhc_abi_version() == _lib.K["PBHC_ABI_VERSION"] >= 16          # (16 brought these fields)
    # PbhcEnvConfig has a layout version of its own, which does not move with every ABI change
    assert 1 <= _lib.K["PBHC_ENV_CONFIG_VERSION"] <= _lib.K["PBHC_ABI_VERSION"]
    have = [f for f, _ in _lib.PbhcFloatingParams._fields_]
    assert [f for f in NEW_FIELDS if f not in have] == []
    assert lib.pbhc_sizeof_floating_params() == C.sizeof(_lib.PbhcFloatingParams)
    sk = Skeleton.from_mjcf(TREE)
    csk = sk.to_c()
    keep = []

    def good(**kw):
        p, table = fsim.FloatingBaseSim.params(sk, 0.02, 0.0, fm.sample_points(sk), "cpu", stiffness=100.0, friction=0.5, **kw)
        keep.append(table)
        return p

    one = C.c_void_p(16)                                     # a non-NULL pointer that is never followed: every call below is refused first
    call = lambda p_, n=1: lib.pbhc_debug_floating_substeps(C.byref(csk), C.byref(p_), one, one, one, one, n, 1, 0.005, 0, None, one, one, one, one,
                                                            one, None)
    # every new pointer NULL: the params pass their checks — the call is refused by the LAST check in front of the launch, the size of n
    p = good()
    assert all(not getattr(p, f) for f in NEW_FIELDS)
    assert call(p, n=1 << 27) == E and b"(uint64_t)n" in lib.pbhc_last_error()
    # tables given through params(): the pointers are theirs; still accepted up to the same check
    tab, fr = torch.zeros(3, 32, 4), torch.full((3,), 0.5)
    keep += [tab, fr]
    p = good(env_inertial=tab, env_friction=fr)
    assert p.env_inertial == tab.data_ptr() and p.env_friction == fr.data_ptr() and tab.data_ptr() % 16 == 0
    assert call(p, n=1 << 27) == E and b"(uint64_t)n" in lib.pbhc_last_error()
    for off in (4, 8, 12):
        p.env_inertial = tab.data_ptr() + off
        assert call(p) == E and b"env_inertial" in lib.pbhc_last_error(), off
    p = good()
    p.env_friction = fr.data_ptr() + 2
    assert call(p) == E and b"env_friction" in lib.pbhc_last_error()
    for field in ("push_counter", "push_interval", "push_vel", "u_push"):      # the test-only export has no control step: no push
        p = good()
        setattr(p, field, 16)
        assert call(p) == E and b"push_counter" in lib.pbhc_last_error(), field
    with pytest.raises(_lib.PbhcError, match=r"env_inertial: expected a contiguous float32 \[N, 32, 4\] tensor"):
        good(env_inertial=torch.zeros(3, 31, 4))
    with pytest.raises(_lib.PbhcError, match=r"env_friction: expected a contiguous float32 \[N\] tensor"):
        good(env_friction=torch.zeros(3, 1))


# ---- the calibration of the GPU tests' bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mjcf", [TREE, os.path.join(GOLDEN, G1)])
def test_the_float32_restatement_of_the_per_env_models_sits_inside_a_quarter_of_the_bound(mjcf):
    """the inputs of the GPU sub-step test (N = 33, fm.random_states seed 5, the per-env tables of tests/floating_dr_inputs.py): every env's
    own model restated in float32 against itself in float64, [a_0, alpha_0, q''] and the points' forces at <= 0.25 of the bound with K = 16;
    no point within `clear` = 1e-3 m of the ground, so the GPU test skips no element"""
    N = 33
    sk = Skeleton.from_mjcf(mjcf)
    m = fm.model(sk, 0.02, 0.05, points=fm.sample_points(sk), **LAW)
    table, friction = di.tables(sk, N)
    assert table[:, 0, 0].min() > 0 and 0.2 <= friction.min() and friction.max() <= 1.2
    models = di.env_models(m, table, friction)
    root, q, v, tau = fm.random_states(m, N, 5, clear=1e-3)
    want, f, d = di.forward_each(models, root, q, v, tau, H)
    w32, f32_, _ = di.forward_each(models, root, q, v, tau, H, np.float32)
    assert np.abs(m["ground_height"] - d["z"]).min() >= 1e-3, "a point within `clear` of the ground: an element to skip"
    r = float((np.abs(w32 - want) / (GAMMA * d["terms"])).max())
    on = d["f_abs"] > 0
    rf = float((np.abs(f32_ - f)[on] / (GAMMA * d["f_abs"][on])).max())
    print(f"{os.path.basename(mjcf)}: per-env float32 restatement / bound: accelerations {r:.3f}, forces {rf:.3f}")
    assert r <= 0.25 and rf <= 0.25
    assert (np.abs(f32_ - f)[~on] == 0).all()
