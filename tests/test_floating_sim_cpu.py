"""FloatingBaseSim without a GPU: the float64 model (tests/floating_model.py) against the fixed-base model, against the product's host-side
inertia matrix and against momentum conservation, every refusal at construction, the contact stability screen on a hand-computable case, the
exports' argument checks, and the calibration of the GPU tests' bound on the model's float32 restatement."""
import ctypes as C
import os

import numpy as np
import pytest

from pbhc_amd import _lib
from pbhc_amd.simulator import floating_sim as fsim
from pbhc_amd.skeleton import Skeleton
from tests import articulated_model as am
from tests import floating_model as fm
from tests.helpers import GOLDEN, fixture_config

SIM = "pbhc_amd.simulator.floating_sim.FloatingBaseSim"
WALK = "v1_g1_23dof_walk.yaml"
TREE = os.path.join(GOLDEN, "mjcf", "articulated_tree.xml")
G1 = "mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml"
G1_29 = "mjcf/g1_29dof_rev_1_0.xml"
SOLES = [[0.132, 0.026, -0.035], [0.132, -0.026, -0.035], [-0.054, 0.026, -0.035], [-0.054, -0.026, -0.035]]
POINTS = {"left_ankle_roll_link": SOLES, "right_ankle_roll_link": SOLES}
EPS = 2.0 ** -24
K_ACC = 16                                                   # tests/test_gpu_floating_sim.py
GAMMA = K_ACC * EPS
H = 0.005
LAW = dict(stiffness=2000.0, normal_damping=400.0, friction=0.8, slip_velocity=0.1, ground_height=0.25)


def _construct(spec=None, extra=None, mjcf=True):
    ov = {"simulator._target_": SIM}
    if mjcf:
        ov["robot.motion.asset.assetFileName"] = G1
    if spec is not None:
        ov["simulator.config.floating_sim"] = spec
    ov.update(extra or {})
    cfg = fixture_config(WALK, 4, ov)
    return fsim.FloatingBaseSim(cfg.env.config, "cpu")


def _good(**kw):
    return dict({"armature": 0.02, "damping": 0.05, "contact_points": POINTS}, **kw)


# ---- the model against itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mjcf", [TREE, os.path.join(GOLDEN, G1), os.path.join(GOLDEN, G1_29)])
def test_the_model_is_consistent(mjcf):
    sk = Skeleton.from_mjcf(mjcf)
    D, N = sk.num_dof, 5
    m = fm.model(sk, 0.02, 0.05, points=fm.sample_points(sk), **LAW)
    root, q, v, tau = fm.random_states(m, N, 1)
    s = fm.state(root, q, v)
    acc, f, d = fm.forward(m, s, tau, H)
    assert np.abs(f).max() > 10.0 and np.abs(d["H"] - np.swapaxes(d["H"], 1, 2)).max() < 1e-12
    # the model's own solved (a_0, alpha_0) as a prescribed base of the fixed-base model, the points' forces as joint torques: the same q''
    base = dict(R0=d["R0"], w0=s["w0"], alpha0=acc[:, 3:6], a0g=acc[:, 0:3] - m["gravity"])
    tau_c = tau + np.einsum("nkid,nki->nd", d["J"], f)[:, 6:]
    qdd, _ = am.forward(m, q, v, tau_c, base, H)
    assert np.abs(qdd - acc[:, 6:]).max() <= 1e-9 * np.abs(qdd).max(), np.abs(qdd - acc[:, 6:]).max() / np.abs(qdd).max()
    # the product's host-side matrix (spatial inertias and motion subspaces) is the model's (Jacobians of the centres of mass)
    for n in range(N):
        Hp = fsim.floating_inertia(sk, q[n], d["R0"][n])
        assert Hp.shape == (6 + D, 6 + D) and np.abs(Hp - d["H"][n]).max() < 1e-6 * np.abs(d["H"][n]).max()
        x, J = fsim.point_jacobians(sk, q[n], d["R0"][n], m["points"])
        assert np.abs(J - d["J"][n]).max() < 1e-6
    # the inverse dynamics at the solved acceleration returns the generalised force
    dd = fm.dynamics(m, q, v, d["R0"], s["w0"], acc)
    back = np.einsum("nde,ne->nd", d["H"], acc) + dd["C"]
    back[:, 6:] += (m["armature"] + H * m["damping"]) * acc[:, 6:] + m["damping"] * v
    want = np.einsum("nkid,nki->nd", d["J"], f)
    want[:, 6:] += tau
    assert np.abs(back - want).max() < 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("mjcf", [TREE, os.path.join(GOLDEN, G1)])
def test_momentum_without_gravity_and_contact(mjcf):
    """with gravity and contact off, the links' net forces and moments of the Newton-Euler sweep at the solved acceleration — summed directly,
    not through the Jacobians — vanish: H [a; q''] + C has zero net force and zero net moment, whatever the joint torques"""
    sk = Skeleton.from_mjcf(mjcf)
    m = fm.model(sk, 0.0, 0.0, gravity=(0.0, 0.0, 0.0), points=fm.sample_points(sk))
    root, q, v, tau = fm.random_states(m, 6, 2)
    s = fm.state(root, q, v)
    acc, f, d = fm.forward(m, s, tau, 0.0, contact_on=False)
    dd = fm.dynamics(m, q, v, d["R0"], s["w0"], acc)
    net_f = dd["F"].sum(1)
    net_m = (dd["Nn"] + np.cross(dd["r"], dd["F"])).sum(1)
    scale = np.abs(dd["F"]).max()
    assert scale > 10.0 and np.abs(net_f).max() < 1e-10 * scale and np.abs(net_m).max() < 1e-10 * scale
    # and the root rows of H acc + C are those sums
    rows = (np.einsum("nde,ne->nd", d["H"], acc) + dd["C"])[:, :6]
    assert np.abs(rows).max() < 1e-10 * scale


# ---- refusals, by name ----------------------------------------------------------------------------------------------------------------
def test_a_valid_config_gets_as_far_as_the_gpu_check():
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct(_good())
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct(_good(gravity=[0, 0, -3.7], enforce_limits=False, stiffness=5000.0, normal_damping=50.0, friction=0.5, slip_velocity=0.5,
                         ground_height=0.1, contact_points=dict(POINTS, pelvis=[[0.0, 0.0, -0.1]])))


def test_refusals_by_name():
    R = lambda pat: pytest.raises(_lib.PbhcError, match=pat)
    with R(r"floating_sim\.contact_force: unknown key"):
        _construct(_good(contact_force=300.0))
    with R(r"floating_sim\.base_acceleration: unknown key"):
        _construct(_good(base_acceleration=True))
    with R(r'floating_sim: robot\.control\.control_type "V"'):
        _construct(_good(), {"robot.control.control_type": "V"})
    with R(r"floating_sim\.armature: a list must have one entry per dof \(23\), got 22"):
        _construct(_good(armature=[0.02] * 22))
    with R(r"floating_sim: armature and damping must not be negative"):
        _construct(_good(damping=-0.1))
    with R(r"floating_sim\.gravity: expected a list of 3 numbers"):
        _construct(_good(gravity=[0, -9.81]))
    with R(r"floating_sim\.contact_points: missing or empty"):
        _construct({"armature": 0.02})
    with R(r"floating_sim\.contact_points: missing or empty"):
        _construct(_good(contact_points={}))
    with R(r"floating_sim\.contact_points\.left_foot: unknown body"):
        _construct(_good(contact_points={"left_foot": SOLES}))
    with R(r"floating_sim\.contact_points\.pelvis: 5 points; a body carries at most 4"):
        _construct(_good(contact_points={"pelvis": SOLES + [[0.0, 0.0, 0.0]]}))
    with R(r"floating_sim\.contact_points\.pelvis: expected a non-empty list of \[x, y, z\] points"):
        _construct(_good(contact_points={"pelvis": [[0.0, 0.0]]}))
    with R(r"floating_sim: stiffness, normal_damping and friction must not be negative"):
        _construct(_good(stiffness=-1.0))
    with R(r"floating_sim: stiffness, normal_damping and friction must not be negative"):
        _construct(_good(friction=-0.1))
    with R(r"floating_sim\.slip_velocity: must be positive"):
        _construct(_good(slip_velocity=0.0))
    with R(r"floating_sim\.stiffness: expected a number"):
        _construct(_good(stiffness="stiff"))
    with R(r"floating_sim: the skeleton has no link masses and inertia tensors.*assetFileName = the \.xml"):
        _construct(_good(), mjcf=False)
    sim = fsim.FloatingBaseSim.__new__(fsim.FloatingBaseSim)
    with R("FloatingBaseSim.set_replay: the simulator writes its own"):
        sim.set_replay(None, None, None, None)


def test_a_skeleton_that_cannot_run_is_refused_by_name():
    cfg = fixture_config(WALK, 4, {"robot.motion.asset.assetFileName": G1})
    sk = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    pts = fsim.FloatingBaseSim.parse_points(POINTS, sk)
    assert [b for b, _ in pts] == [6] * 4 + [12] * 4
    check = lambda skel, arm=0.02, **kw: fsim.FloatingBaseSim.check_model(cfg.env.config, skel, np.full(23, arm), pts, **dict(
        dict(stiffness=10000.0, normal_damping=100.0, friction=0.8, slip_velocity=0.4, gravity=np.array([0.0, 0.0, -9.81])), **kw))
    big = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    big.body_names = list(big.body_names) + [f"x{i}" for i in range(40)]
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the robot has 64 bodies"):
        check(big)
    rootless = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    rootless.body_mass = rootless.body_mass.copy()
    rootless.body_mass[0] = 0.0
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the root link 'pelvis' has no mass"):
        check(rootless)
    light = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    light.body_mass = light.body_mass.copy(); light.body_inertia = light.body_inertia.copy()
    light.body_mass[6] = 0.0; light.body_inertia[6] = 0.0
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: H\(q_default\) \+ diag\(armature\) is not positive definite"):
        check(light, arm=0.0)
    out = check(sk)
    assert set(out) >= {"a_pd", "b_pd", "a_n", "b_n", "b_t", "weight"}


def test_the_stability_screen():
    """on the seven-body tree made rigid by an armature of 1e9 kg m^2, one contact point at the tree's centre of mass is one point mass of
    11 kg on one spring: a = h^2 k / m, b = h d / m, and h c / m for the friction's slope — by hand.  Then the G1 walk config: the defaults
    pass at the shipped 200 Hz, a stiffness of 1e6 N / m, a normal damping of 1e4 N s / m and a slip velocity of 0.05 m / s are refused with
    the numbers and the remedies."""
    sk = Skeleton.from_mjcf(TREE)
    D = sk.num_dof
    q0 = np.zeros(D)
    Ht = fsim.floating_inertia(sk, q0) + np.diag(np.r_[np.zeros(6), np.full(D, 1e9)])
    mass = float(sk.body_mass.sum())
    assert abs(mass - 11.0) < 1e-6
    first = Ht[3:6, 0:3]                                     # m [c]x of the whole tree about the root's origin
    com = np.array([first[2, 1], first[0, 2], first[1, 0]]) / mass
    x, J = fsim.point_jacobians(sk, q0, np.eye(3), [(0, com)])
    k, d, c, h = 3000.0, 40.0, 25.0, 0.005
    got = fsim.contact_stability_margins(h, Ht, J[:, 2, :], J[:, :2, :].reshape(-1, 6 + D), k, d, c)
    assert abs(got["a_n"] - h * h * k / mass) < 1e-6 * got["a_n"] and abs(got["b_n"] - h * d / mass) < 1e-6 * got["b_n"]
    assert abs(got["b_t"] - h * c / mass) < 1e-6 * got["b_t"]
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct(_good())
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the explicit contact is unstable at the physics sub-step h = 0\.005 s: a = .* \(raise "
                                             r"simulator\.config\.sim\.fps, lower the stiffness"):
        _construct(_good(stiffness=1e6))
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the explicit contact is unstable"):
        _construct(_good(normal_damping=1e4))
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the regularised friction is unstable .*raise simulator\.config\.sim\.fps or the slip_velocity"):
        _construct(_good(slip_velocity=0.05))
    with pytest.raises(_lib.PbhcError, match=r"floating_sim: the explicit PD is unstable"):
        _construct(_good(armature=0.0))
    # the margins table of DESIGN §8
    cfg = fixture_config(WALK, 4, {"robot.motion.asset.assetFileName": G1})
    g1 = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    pts = fsim.FloatingBaseSim.parse_points(POINTS, g1)
    weight = float(g1.body_mass.sum()) * 9.81
    for fps in (200, 400):
        cfg.simulator.config.sim.fps = fps
        for k_, d_, vs in ((5000.0, 50.0, 0.4), (10000.0, 100.0, 0.4), (20000.0, 200.0, 0.4), (10000.0, 100.0, 0.2)):
            try:
                out = fsim.FloatingBaseSim.check_model(cfg.env.config, g1, np.full(23, 0.02), pts, k_, d_, 0.8, vs, np.array([0.0, 0.0, -9.81]))
                verdict = "passes"
            except _lib.PbhcError as e:
                out, verdict = None, "refused: " + str(e)[30:80]
            line = "" if out is None else f"a_n {out['a_n']:.3f} b_n {out['b_n']:.3f} b_t {out['b_t']:.3f}"
            print(f"{fps} Hz, k {k_:.0f}, d {d_:.0f}, slip {vs}: {line} static sink {100 * weight / (8 * k_):.2f} cm, {verdict}")
    cfg.simulator.config.sim.fps = 200
    out = fsim.FloatingBaseSim.check_model(cfg.env.config, g1, np.full(23, 0.02), pts, 10000.0, 100.0, 0.8, 0.4, np.array([0.0, 0.0, -9.81]))
    assert out["b_n"] < 2 and out["a_n"] + 2 * out["b_n"] < 4 and out["b_t"] < 2 and weight / (8 * 10000.0) < 0.01


# ---- the exports -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_without_a_gpu():
    lib = _lib.lib()
    E = _lib.K["PBHC_EINVAL"]
    assert lib.pbhc_sizeof_floating_params() == C.sizeof(_lib.PbhcFloatingParams)
    assert lib.pbhc_floating_sim_step(None, None, None, None) == E
    io, p = _lib.PbhcStepIO(), _lib.PbhcFloatingParams()
    assert lib.pbhc_floating_sim_step(None, C.byref(io), C.byref(p), None) == E
    assert b"bad argument" in lib.pbhc_last_error()
    sk = Skeleton.from_mjcf(TREE)
    csk = sk.to_c()
    keep = []

    def good(**kw):
        p, table = fsim.FloatingBaseSim.params(sk, 0.02, 0.0, fm.sample_points(sk), "cpu", **dict(dict(stiffness=100.0, friction=0.5), **kw))
        keep.append(table)
        return p

    one = C.c_void_p(8)                                      # a non-NULL pointer that is never followed: every call below is refused first
    call = lambda csk_, p_, n=1, steps=1, h=0.005, lim=0, limits=None, q=one: lib.pbhc_debug_floating_substeps(
        C.byref(csk_) if csk_ is not None else None, C.byref(p_) if p_ is not None else None, one, q, one, one, n, steps, h, lim, limits, one, one, one,
        one, one, None)
    assert call(None, good()) == E and call(csk, None) == E and call(csk, good(), q=None) == E
    assert call(csk, good(), n=0) == E and call(csk, good(), steps=0) == E and call(csk, good(), steps=4097) == E and call(csk, good(), h=0.0) == E
    assert call(csk, good(), lim=1, limits=None) == E
    for field, idx in (("mass", 3), ("armature", 2), ("damping", 0)):
        p = good()
        getattr(p, field)[idx] = -1.0
        assert call(csk, p) == E, field
        assert field.encode() in lib.pbhc_last_error()
    for kw in (dict(stiffness=-1.0), dict(normal_damping=-1.0), dict(friction=-1.0), dict(slip_velocity=0.0)):
        assert call(csk, good(**kw)) == E, kw
        assert list(kw)[0].encode() in lib.pbhc_last_error()
    p = good()
    p.mass[0] = 0.0
    assert call(csk, p) == E and b"mass[0]" in lib.pbhc_last_error()
    p = good()
    p.points = None
    assert call(csk, p) == E and b"points" in lib.pbhc_last_error()
    p = good()
    p.num_points[2] = 5
    assert call(csk, p) == E and b"num_points" in lib.pbhc_last_error()
    p = good()
    p.num_points[7] = 1                                      # a point on a body the seven-body tree does not have
    assert call(csk, p) == E and b"num_points" in lib.pbhc_last_error()
    wide = _lib.PbhcSkeleton()
    wide.num_bodies = wide.num_bodies_ext = 33
    wide.num_dof, wide.max_depth = 32, 1
    assert call(wide, good()) == E


# ---- the calibration of the GPU tests' bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mjcf,N", [(TREE, 33), (os.path.join(GOLDEN, G1), 33), (os.path.join(GOLDEN, G1_29), 9)])
def test_the_float32_restatement_sits_inside_a_quarter_of_the_bound(mjcf, N):
    """one sub-step on the GPU test's own inputs (seeds 5 and 7): the model restated in float32 against the model, [a_0, alpha_0, q''] and the
    points' forces, at <= 0.25 of the bound with K = 16"""
    sk = Skeleton.from_mjcf(mjcf)
    m = fm.model(sk, 0.02, 0.05, points=fm.sample_points(sk), **LAW)
    for seed in (5, 7):
        root, q, v, tau = fm.random_states(m, N, seed)
        want, f, d = fm.forward(m, fm.state(root, q, v), tau, H)
        w32, f32_, _ = fm.forward(m, fm.state(root, q, v, np.float32), tau, H, np.float32)
        r = float((np.abs(w32 - want) / (GAMMA * d["terms"])).max())
        on = d["f_abs"] > 0
        rf = float((np.abs(f32_ - f)[on] / (GAMMA * d["f_abs"][on])).max())
        print(f"{os.path.basename(mjcf)} seed {seed}: float32 restatement / bound: accelerations {r:.3f}, forces {rf:.3f}")
        assert r <= 0.25 and rf <= 0.25
        assert (np.abs(f32_ - f)[~on] == 0).all()


def test_the_drop_keeps_the_float32_restatement_inside_the_bound():
    """the GPU drop test's release on the model alone: every robot reaches the ground, and after 100 sub-steps every (robot, element) of the
    float32 restatement is within a quarter of the carried bound — so the GPU test skips nothing"""
    sk = Skeleton.from_mjcf(TREE)
    N, steps = 8, 100
    m = fm.model(sk, 0.02, fm.DROP_DAMP, points=fm.drop_points(sk), **fm.DROP_LAW)
    root, q, v, tau = fm.drop_inputs(m, N)
    r = fm.transported_bound(m, fm.state(root, q, v), tau, H, steps, GAMMA, EPS)
    r32 = fm.substeps(m, fm.state(root, q, v, np.float32), lambda q_, v_: tau.astype(np.float32), H, steps, dtype=np.float32)
    err32 = fm.state_error({k: x.astype(np.float64) for k, x in r32["s"].items()}, r["s"], sk.num_dof)
    print(f"drop: float32 restatement / carried bound {float((err32 / r['E']).max()):.3f}; lowest point {r['zmin'].min() * 1e3:.2f} mm, final root speed "
          f"{np.abs(r['s']['v0']).max():.3f} m/s, final root height error bound {r['E'][:, 2].max():.2e} m")
    assert (r["zmin"] < 0).all() and (err32 <= 0.25 * r["E"]).all()
    assert np.abs(r["s"]["v0"]).max() < 0.2
