"""ArticulatedSim without a GPU: the MJCF's inertia tensors, the float64 model (tests/articulated_model.py) against itself and against the
product's host-side inertia matrix, every refusal at construction, the stability screen, the exports' argument checks, and the cap on what
the GPU test may skip, on the model alone."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pbhc_amd import _lib
from pbhc_amd.simulator import articulated_sim as asim
from pbhc_amd.skeleton import Skeleton
from tests import articulated_model as am
from tests.helpers import GOLDEN, fixture_config

SIM = "pbhc_amd.simulator.articulated_sim.ArticulatedSim"
WALK = "v1_g1_23dof_walk.yaml"
TREE = os.path.join(GOLDEN, "mjcf", "articulated_tree.xml")
G1 = "mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml"
G1_29 = "mjcf/g1_29dof_rev_1_0.xml"


def _construct(spec=None, extra=None, mjcf=True):
    ov = {"simulator._target_": SIM}
    if mjcf:
        ov["robot.motion.asset.assetFileName"] = G1
    if spec is not None:
        ov["simulator.config.articulated_sim"] = spec
    ov.update(extra or {})
    cfg = fixture_config(WALK, 4, ov)
    return asim.ArticulatedSim(cfg.env.config, "cpu")


# ---- the inertial data ---------------------------------------------------------------------------------------------------------------
def test_inertia_tensors_of_the_hand_written_tree(tmp_path):
    """tests/golden/mjcf/articulated_tree.xml, DFS order base a b c d e f, worked by hand:
      a  diaginertia 0.012 0.011 0.004, no quat                    -> diag(0.012, 0.011, 0.004)
      b  fullinertia xx yy zz xy xz yz = 0.02 0.03 0.04 0.001 -0.002 0.003
                                                                   -> [[0.02, 0.001, -0.002], [0.001, 0.03, 0.003], [-0.002, 0.003, 0.04]]
      c  diaginertia 0.01 0.02 0.03 with quat (cos 45, 0, 0, sin 45): the principal axes turned 90 degrees about z, R = [[0,-1,0],[1,0,0],[0,0,1]],
         R diag R^T swaps the first two moments                    -> diag(0.02, 0.01, 0.03)
      e  no <inertial>                                             -> mass 0, centre of mass 0, tensor 0
      total mass 5 + 2 + 1.5 + 0.5 + 0.8 + 0 + 1.2 = 11 kg; the centre of mass of b is (0.02, -0.1, 0.01)"""
    sk = Skeleton.from_mjcf(TREE)
    assert sk.body_names == ["base", "a", "b", "c", "d", "e", "f"] and list(sk.parents) == [-1, 0, 1, 2, 1, 0, 5]
    I = sk.body_inertia
    assert I.shape == (7, 3, 3)
    np.testing.assert_allclose(I[1], np.diag([0.012, 0.011, 0.004]), atol=1e-15)
    np.testing.assert_allclose(I[2], [[0.02, 0.001, -0.002], [0.001, 0.03, 0.003], [-0.002, 0.003, 0.04]], atol=1e-15)
    np.testing.assert_allclose(I[3], np.diag([0.02, 0.01, 0.03]), atol=1e-9)          # (the quaternion is written to 7 digits)
    assert not I[5].any() and sk.body_mass[5] == 0 and not sk.body_com[5].any()
    assert abs(float(sk.body_mass.sum()) - 11.0) < 1e-6
    np.testing.assert_allclose(sk.body_com[2], [0.02, -0.1, 0.01], atol=1e-8)
    for b in (1, 2, 3, 4, 6):
        assert np.linalg.eigvalsh(I[b]).min() > 0
    # the JSON round trip
    path = tmp_path / "tree.json"
    sk.to_json(path)
    back = Skeleton.from_json(path)
    assert np.array_equal(back.body_inertia, sk.body_inertia) and np.array_equal(back.body_mass, sk.body_mass)
    # a skeleton without inertias writes the file it always wrote
    bare = Skeleton(sk.body_names, sk.body_names_ext, sk.parents, sk.offsets, sk.local_rot_wxyz, sk.dof_axis)
    bare.to_json(path)
    assert set(json.load(open(path))) == {"body_names", "body_names_ext", "parents", "offsets", "local_rot_wxyz", "dof_axis"}
    assert Skeleton.from_json(path).body_inertia is None
    masses = Skeleton(sk.body_names, sk.body_names_ext, sk.parents, sk.offsets, sk.local_rot_wxyz, sk.dof_axis, body_mass=sk.body_mass, body_com=sk.body_com)
    masses.to_json(path)
    assert "body_inertia" not in json.load(open(path)) and "body_mass" in json.load(open(path))


def test_g1_orientation_numbers():
    """the figures DESIGN §8 quotes for the G1 MJCF: total mass, the range of diag M at the default pose"""
    sk = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    cfg = fixture_config(WALK, 4, {})
    q0 = np.array([float(cfg.robot.init_state.default_joint_angles[n]) for n in cfg.robot.dof_names])
    d = np.diag(asim.joint_space_inertia(sk, q0))
    print(f"G1 23 dof: total mass {float(sk.body_mass.sum()):.3f} kg, diag M at the default pose {d.min():.3g} .. {d.max():.3g} kg m^2")
    assert abs(float(sk.body_mass.sum()) - 31.69) < 0.01
    assert 3e-4 < d.min() < 5e-4 and 0.8 < d.max() < 1.0


# ---- the model against itself ---------------------------------------------------------------------------------------------------------
def _random_state(sk, N, seed, moving_base=True):
    rng = np.random.default_rng(seed)
    D = sk.num_dof
    q, v, tau = rng.uniform(-0.6, 0.6, (N, D)), 2.0 * rng.standard_normal((N, D)), 10.0 * rng.standard_normal((N, D))
    base = am.rest_base(N)
    if moving_base:
        base = dict(R0=am.quat_xyzw_to_matrix(rng.standard_normal((N, 4))), w0=rng.standard_normal((N, 3)), alpha0=3.0 * rng.standard_normal((N, 3)),
                    a0g=2.0 * rng.standard_normal((N, 3)) + np.array([0.0, 0.0, 9.81]))
    return q, v, tau, base


@pytest.mark.parametrize("mjcf", [TREE, os.path.join(GOLDEN, G1), os.path.join(GOLDEN, G1_29)])
def test_the_model_is_consistent(mjcf):
    sk = Skeleton.from_mjcf(mjcf)
    D, N, h = sk.num_dof, 5, 0.005
    m = am.model(sk, armature=0.02, damping=0.05)
    q, v, tau, base = _random_state(sk, N, 1)
    qdd, d = am.forward(m, q, v, tau, base, h)
    M = d["M"]
    # M is symmetric; with the armature it is positive definite (the tree's link e weighs nothing)
    assert np.abs(M - np.swapaxes(M, 1, 2)).max() == 0.0 or np.abs(M - np.swapaxes(M, 1, 2)).max() < 1e-15
    assert np.linalg.eigvalsh(am.mtilde(m, M)).min() > 0
    # the product's host-side matrix (composite-rigid-body method, pbhc_amd/simulator/articulated_sim.py) is the model's (Jacobians)
    for n in range(N):
        Mp = asim.joint_space_inertia(sk, q[n])
        assert np.abs(Mp - M[n]).max() < 1e-6 * np.abs(M[n]).max(), (n, np.abs(Mp - M[n]).max())
    # inverse dynamics of the forward dynamics returns tau:  ID(q, v, q'') + (armature + h b) q'' + b v = tau
    back = am.dynamics(m, q, v, base, qdd=qdd)["c"] + (m["armature"] + h * m["damping"]) * qdd + m["damping"] * v
    assert np.abs(back - tau).max() < 1e-9 * max(1.0, np.abs(tau).max()), np.abs(back - tau).max()
    # with tau = c(q, 0) and v = 0, q'' = 0
    z = np.zeros((N, D))
    hold = am.dynamics(m, q, z, base)["c"]
    assert np.abs(hold).max() > 1.0, "nothing to hold against"
    qdd0, _ = am.forward(m, q, z, hold, base, h)
    assert np.abs(qdd0).max() < 1e-9, np.abs(qdd0).max()


def _energy_deviation(m, q0, h, T):
    N = q0.shape[0]
    base = am.rest_base(N)
    q, v = q0.copy(), np.zeros_like(q0)
    arm = m["armature"]
    energy = lambda q, v: (lambda d: d["T"] + 0.5 * (arm * v * v).sum(1) + d["V"])(am.dynamics(m, q, v, base))
    e0 = energy(q, v)
    worst = np.zeros(N)
    for _ in range(int(round(T / h))):
        r = am.substeps(m, q, v, lambda q_, v_: np.zeros_like(q_), base, h, 1)
        q, v = r["q"], r["v"]
        worst = np.maximum(worst, np.abs(energy(q, v) - e0))
    return worst, np.abs(v).max()


def test_energy_drift_of_the_passive_tree_halves_with_the_step():
    """no torque, no damping, no limits, base at rest: the total energy (1/2 v^T (M + armature) v - sum m g.r) of the semi-implicit Euler
    trajectory deviates from its start by O(h).  Over 0.4 s the largest deviation at h = 1/400 is between 0.4 and 0.6 of the one at
    h = 1/200 — a wrong Coriolis or gravity term leaves a residue that does not shrink with h."""
    sk = Skeleton.from_mjcf(TREE)
    m = am.model(sk, armature=0.02, damping=0.0)
    q0 = np.random.default_rng(3).uniform(-0.6, 0.6, (3, sk.num_dof))
    e1, vmax = _energy_deviation(m, q0, 1 / 200, 0.4)
    e2, _ = _energy_deviation(m, q0, 1 / 400, 0.4)
    print("energy deviation at h, h/2:", e1, e2, "ratio", e2 / e1, "largest |v|", vmax)
    assert vmax > 1.0, "the tree hardly moved"
    assert ((e2 / e1 > 0.4) & (e2 / e1 < 0.6)).all(), e2 / e1


# ---- refusals, by name ----------------------------------------------------------------------------------------------------------------
def test_a_valid_config_gets_as_far_as_the_gpu_check():
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct({"armature": 0.02, "damping": 0.05})
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct({"armature": [0.02] * 23, "damping": [0.0] * 23, "gravity": [0, 0, -3.7], "base_acceleration": False, "contact_force": 100.0,
                    "foot_height_threshold": 0.05, "enforce_limits": False})


def test_refusals_by_name():
    R = lambda pat: pytest.raises(_lib.PbhcError, match=pat)
    with R(r"articulated_sim\.inertia: unknown key"):
        _construct({"armature": 0.02, "inertia": 0.1})
    with R(r'articulated_sim: robot\.control\.control_type "V"'):
        _construct({"armature": 0.02}, {"robot.control.control_type": "V"})
    for key in ("armature", "damping"):
        with R(rf"articulated_sim\.{key}: a list must have one entry per dof \(23\), got 22"):
            _construct({"armature": 0.02, key: [0.02] * 22})
    with R(r"articulated_sim: armature and damping must not be negative"):
        _construct({"armature": 0.02, "damping": -0.1})
    with R(r"articulated_sim: armature and damping must not be negative"):
        _construct({"armature": [0.02] * 22 + [-0.02]})
    with R(r"articulated_sim\.gravity: expected a list of 3 numbers"):
        _construct({"armature": 0.02, "gravity": [0, -9.81]})
    # the fixture's own skeleton is a JSON without masses: the message points at the MJCF
    with R(r"articulated_sim: the skeleton has no link masses and inertia tensors.*assetFileName = the \.xml"):
        _construct({"armature": 0.02}, mjcf=False)
    sim = asim.ArticulatedSim.__new__(asim.ArticulatedSim)
    with R("ArticulatedSim.set_replay: the simulator writes its own"):
        sim.set_replay(None, None, None, None)


def test_a_skeleton_that_cannot_run_is_refused_by_name():
    cfg = fixture_config(WALK, 4, {"robot.motion.asset.assetFileName": G1})
    sk = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    # more bodies than lanes
    big = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    big.body_names = list(big.body_names) + [f"x{i}" for i in range(40)]
    with pytest.raises(_lib.PbhcError, match=r"articulated_sim: the robot has 64 bodies"):
        asim.ArticulatedSim.check_model(cfg.env.config, big, np.full(23, 0.02))
    # a massless chain end without an armature: M is singular
    light = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    light.body_mass = light.body_mass.copy(); light.body_inertia = light.body_inertia.copy()
    light.body_mass[6] = 0.0; light.body_inertia[6] = 0.0          # left_ankle_roll_link: the last link of the left leg
    assert light.body_names[6] == "left_ankle_roll_link"
    with pytest.raises(_lib.PbhcError, match=r"articulated_sim: M\(q_default\) \+ diag\(armature\) is not positive definite"):
        asim.ArticulatedSim.check_model(cfg.env.config, light, np.zeros(23))
    Mt = asim.ArticulatedSim.check_model(cfg.env.config, sk, np.full(23, 0.02))
    assert Mt.shape == (23, 23)


def test_the_stability_screen_on_the_g1():
    """the walk config on the G1 MJCF at 200 Hz: refused at armature 0 (a + 2 b far above 4: diag M goes down to 3.9e-4 kg m^2 under gains of
    hundreds), accepted at 0.02"""
    with pytest.raises(_lib.PbhcError, match=r"articulated_sim: the explicit PD is unstable at the physics sub-step h = 0\.005 s"):
        _construct({"armature": 0.0})
    with pytest.raises(_lib.PbhcError, match=r"articulated_sim: the explicit PD is unstable"):
        _construct(None)                                   # the default armature is 0
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct({"armature": 0.02})
    with pytest.raises(_lib.PbhcError, match="runs on the GPU only"):
        _construct({"armature": 0.0}, {"robot.control.control_type": "T"})          # no feedback gain: nothing to screen
    cfg = fixture_config(WALK, 4, {"robot.motion.asset.assetFileName": G1})
    sk = Skeleton.from_mjcf(os.path.join(GOLDEN, G1))
    q0 = np.array([float(cfg.robot.init_state.default_joint_angles[n]) for n in cfg.robot.dof_names])
    K, Kd = asim.ArticulatedSim._top_gains(cfg.env.config)
    for arm in (0.0, 0.005, 0.01, 0.02):
        Mt = asim.joint_space_inertia(sk, q0) + arm * np.eye(23)
        a, b = asim.pd_stability_margins(1 / 200, K, Kd, Mt)
        print(f"armature {arm}: a = {a:.4g}, b = {b:.4g}, a + 2 b = {a + 2 * b:.4g}, cond(Mt) = {np.linalg.cond(Mt):.3g}")
    # the scalar rule on a diagonal matrix is JointSpaceSim's own
    a, b = asim.pd_stability_margins(0.005, [400.0, 100.0], [5.0, 2.0], np.diag([0.05, 0.1]))
    assert abs(a - 0.005 ** 2 * 400 / 0.05) < 1e-12 and abs(b - 0.005 * 5 / 0.05) < 1e-12


# ---- the exports -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_einval_without_a_gpu():
    lib = _lib.lib()
    E = _lib.K["PBHC_EINVAL"]
    assert lib.pbhc_sizeof_articulated_params() == C.sizeof(_lib.PbhcArticulatedParams)
    assert lib.pbhc_articulated_sim_step(None, None, None, None) == E
    io, p = _lib.PbhcStepIO(), _lib.PbhcArticulatedParams()
    assert lib.pbhc_articulated_sim_step(None, C.byref(io), C.byref(p), None) == E
    assert b"bad argument" in lib.pbhc_last_error()
    sk = Skeleton.from_mjcf(TREE)
    csk = sk.to_c()
    good = lambda: asim.ArticulatedSim.params(sk, 0.02, 0.0)
    one = C.c_void_p(8)                                      # a non-NULL pointer that is never followed: every call below is refused first
    call = lambda csk_, p_, n=1, steps=1, h=0.005, lim=0, limits=None, q=one: lib.pbhc_debug_articulated_substeps(
        C.byref(csk_) if csk_ is not None else None, C.byref(p_) if p_ is not None else None, one, q, one, one, n, steps, h, lim, limits, one, one, one, None)
    assert call(None, good()) == E and call(csk, None) == E and call(csk, good(), q=None) == E
    assert call(csk, good(), n=0) == E and call(csk, good(), steps=0) == E and call(csk, good(), steps=4097) == E and call(csk, good(), h=0.0) == E
    assert call(csk, good(), lim=1, limits=None) == E
    for field, idx in (("mass", 3), ("armature", 2), ("damping", 0)):
        p = good()
        getattr(p, field)[idx] = -1.0
        assert call(csk, p) == E, field
        assert field.encode() in lib.pbhc_last_error()
    # more bodies than lanes: B = 33
    wide = _lib.PbhcSkeleton()
    wide.num_bodies = wide.num_bodies_ext = 33
    wide.num_dof, wide.max_depth = 32, 1
    assert call(wide, good()) == E
    # a parent that comes after its child
    bad = sk.to_c()
    bad.parent[2] = 4
    assert call(bad, good()) == E


# ---- what the GPU test may skip ----------------------------------------------------------------------------------------------------------
def test_the_model_of_the_gpu_scenario_keeps_clear_of_the_limits():
    """tests/test_gpu_articulated_sim.py may skip an (env, step) pair only when the float64 model has a pre-clamp position within 1e-5 rad of a
    hard limit in one of its sub-steps: the velocity zeroing is discontinuous there and through the coupling it reaches every joint.  Here the
    model ALONE runs the committed scenario (the G1 walk case: N = 70, six steps, armature 0.02, damping 0.05, gravity on, the base at rest,
    nominal gains, joints started beyond a limit) and skips at most 1 % of the pairs — in fact none; the clamp and the torque clip both bind."""
    from tests import joint_sim_model as jm
    from tests.helpers import build_env_config
    from tests.test_gpu_articulated_sim import ARM, DAMP, LOWERED, WALK_CASE, case_overrides
    from tests.test_gpu_joint_sim import scenario

    cfgname, N, general = WALK_CASE
    _, sk, c, _ = build_env_config(cfgname, case_overrides(cfgname, sim=False), num_envs=N, seed=1, general=general, has_contact_mask=True)
    assert sk.body_inertia is not None
    D = c.skel.num_dof
    sc = scenario(N, D, float(c.action_clip_value))
    f = lambda a: np.array([a[d] for d in range(D)], np.float64)
    lim = np.array([[c.hard_dof_pos_limits[d][0], c.hard_dof_pos_limits[d][1]] for d in range(D)], np.float64)
    tl = f(c.torque_limits)
    assert all(tl[d] == 1.0 for d in LOWERED)
    P = dict(control_type=0, Kp=f(c.p_gains), Kd=f(c.d_gains), action_scale=f(c.action_scale), torque_limit=tl, default=f(c.default_dof_pos),
             kp=np.ones((N, D)), kd=np.ones((N, D)), rfi_scale=np.ones((N, D)), rao_scale=np.zeros((N, D)), u_rfi=None, rfi_lim=0.0, n_ps=None,
             ps_rfi_lim=0.0, use_rao=False, clip_torques=bool(c.clip_torques))
    m = am.model(sk, ARM, DAMP)
    q = np.tile(f(c.default_dof_pos), (N, 1))
    v = np.zeros((N, D))
    for e, d, side in sc["beyond_limit"]:
        q[e, d] = lim[d, side] + (0.05 if side else -0.05)
    base = am.rest_base(N)
    skipped = clamps = clips = 0
    for k in range(sc["steps"]):
        a_del = jm.delayed_action(sc["actions"][k], float(c.action_clip_value), None, None, False)
        clips += int((np.abs(jm.torque_terms(q, v, a_del, P)[3]) > tl).sum())
        r = am.substeps(m, q, v, lambda q_, v_: jm.torque(q_, v_, a_del, P), base, float(c.sim_dt), 4, lim[:, 0], lim[:, 1])
        q, v = r["q"], r["v"]
        assert np.isfinite(q).all() and np.isfinite(v).all()
        skipped += int((r["margin"].min(axis=1) < 1e-5).sum())
        clamps += int(((q == lim[:, 0]) | (q == lim[:, 1])).sum())
    print(f"model alone: {skipped} of {N * sc['steps']} (env, step) pairs within 1e-5 rad of a limit, {clamps} elements on a limit after a step, "
          f"{clips} first-sub-step torques clipped")
    assert skipped <= 0.01 * N * sc["steps"], skipped
    assert clamps > 0 and clips > 0
