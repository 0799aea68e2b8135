"""FloatingBaseSim on the GPU (pbhc_amd/simulator/floating_sim.py, csrc/pbhc_floating_sim.hip): the device function against the float64 model
of tests/floating_model.py (Jacobians with the six root columns, a classical Newton-Euler sweep and a dense solve against the kernel's
articulated-body algorithm with the root's 6 x 6 solved last) through the test-only export, against the fixed-base kernel, then through the
env one control step at a time, falling and the reset, graph = eager, resume.

Bounds.  Per element, float64, from magnitudes: a relative error gamma = K 2^-24 of every product that enters x = [a_0, alpha_0, q''] moves it
by at most
    gamma (|Ht^-1| (|Ht| |x| + |tau| + |b v| + sum |terms of C| + sum_k |J_k|^T f_abs_k))_i                       (floating_model.forward: terms)
with f_abs_k what the float32 error of a point's force scales with (stiffness x the operands of the cancelling sum in delta, normal_damping x
the terms of the point's velocity, the friction's direction); a force itself is held to gamma f_abs.  Over several sub-steps the bound is
carried as the state is integrated, the error of earlier sub-steps coming back through |d x / d state| (central differences of the model,
the contact spring and the torque law included), plus the roundings of the state itself, 4 eps per sub-step (floating_model.carried_bound).
K is not chosen by what the kernel gives: the model is re-run in numpy float32 on the same inputs and K set so that this restatement stays
at <= 0.25 of the bound (asserted in tests/test_floating_sim_cpu.py and again here, without the GPU's result).
    K = 16, the fixed-base simulator's; figures in DESIGN.md §8.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.simulator import articulated_sim as asim
from pbhc_amd.simulator import floating_sim as fsim
from pbhc_amd.skeleton import Skeleton
from tests import articulated_model as am
from tests import floating_model as fm
from tests import joint_sim_model as jm
from tests.helpers import GOLDEN
from tests.test_gpu_articulated_sim import (ARM, DAMP, G1, G1_29, STUDENT, TREE, WALK, _np, _prepare, _report, _tau_abs, _torque_params, case_overrides,
                                            scenario, _debug as _debug_fixed, _seed_all)
from tests.helpers import build_hip_env

pytestmark = pytest.mark.gpu

SIM = "pbhc_amd.simulator.floating_sim.FloatingBaseSim"
EPS = 2.0 ** -24
K_ACC = 16
GAMMA = K_ACC * EPS
DEV = "cuda:0"
H = 0.005
LAW = dict(stiffness=2000.0, normal_damping=400.0, friction=0.8, slip_velocity=0.1, ground_height=0.25)      # soft and damped: the clamp is live
SOLES = [[0.132, 0.026, -0.035], [0.132, -0.026, -0.035], [-0.054, 0.026, -0.035], [-0.054, -0.026, -0.035]]
G1_POINTS = {"left_ankle_roll_link": SOLES, "right_ankle_roll_link": SOLES}


def _sk(mjcf):
    return Skeleton.from_mjcf(os.path.join(GOLDEN, mjcf))


def _setup(mjcf, arm=ARM, damp=DAMP, law=LAW, gravity=(0.0, 0.0, -9.81), points=None):
    sk = _sk(mjcf)
    pts = fm.sample_points(sk) if points is None else points
    m = fm.model(sk, arm, damp, gravity, pts, **law)
    p, table = fsim.FloatingBaseSim.params(sk, arm, damp, pts, DEV, gravity=gravity, **law)
    return sk, m, p, table                                   # `table`: the device point table p.points names — the caller keeps it alive


def _debug(sk, p, root, q, v, tau, steps, h=H, limits=None, place=None):
    """pbhc_debug_floating_substeps on float32 copies of the inputs -> dict of float64 numpy arrays.  place(name, tensor) -> tensor: where
    every device operand goes (tests/test_gpu_step_memory.py: into arenas)"""
    place = place or (lambda name, x: x)
    t = lambda name, a: place(name, torch.as_tensor(np.asarray(a, np.float32)).to(DEV).contiguous())
    tr, tq, tv, tt = t("root", root), t("q", q), t("v", v), t("tau", tau)
    n, D = tq.shape
    B = sk.num_bodies
    o_root, o_q, o_v = place("out_root", torch.zeros_like(tr)), place("out_q", torch.zeros_like(tq)), place("out_v", torch.zeros_like(tq))
    o_acc, o_f = place("out_acc0", torch.zeros(n, 6 + D, device=DEV)), place("out_force", torch.zeros(n, B, 4, 3, device=DEV))
    lim = None if limits is None else np.ascontiguousarray(limits, np.float32)
    csk = sk.to_c()
    _lib.check(_lib.lib().pbhc_debug_floating_substeps(C.byref(csk), C.byref(p), tr.data_ptr(), tq.data_ptr(), tv.data_ptr(), tt.data_ptr(), n, steps, h,
                                                       int(limits is not None), None if lim is None else lim.ctypes.data, o_root.data_ptr(), o_q.data_ptr(),
                                                       o_v.data_ptr(), o_acc.data_ptr(), o_f.data_ptr(), _lib.current_stream()),
               "pbhc_debug_floating_substeps")
    torch.cuda.synchronize()
    return dict(root=_np(o_root), q=_np(o_q), v=_np(o_v), acc0=_np(o_acc), force=_np(o_f), s=fm.state(_np(o_root), _np(o_q), _np(o_v)))


def _by_point(m, force):
    """[n,B,4,3] -> [n,K,3] in the model's point order; everything else of the table must be 0"""
    out, seen, rest = [], {}, force.copy()
    for b, _ in m["points"]:
        k = seen.get(b, 0)
        seen[b] = k + 1
        out.append(force[:, b, k])
        rest[:, b, k] = 0.0
    assert not rest.any(), "a force on a point no body has"
    return np.stack(out, 1)


@pytest.mark.parametrize("mjcf,N", [(TREE, 33), (G1, 33), (G1_29, 9)])
def test_one_substep_equals_the_model(mjcf, N):
    """random tilted, spinning roots, poses, velocities and torques; about a third of the points under the ground, some moving up fast enough
    for the max(0, .) clamp, some sliding below and some above the slip velocity: [a_0, alpha_0, q''] and every point's force of ONE sub-step
    against the model, per element; the float32 restatement within a quarter of the bound; no element skipped"""
    sk, m, p, table = _setup(mjcf)
    root, q, v, tau = fm.random_states(m, N, 5)
    s = fm.state(root, q, v)
    want, f, d = fm.forward(m, s, tau, H)
    want32, f32_, _ = fm.forward(m, fm.state(root, q, v, np.float32), tau, H, np.float32)
    tol, tol_f = GAMMA * d["terms"], GAMMA * d["f_abs"]
    got = _debug(sk, p, root, q, v, tau, 1)
    gf = _by_point(m, got["force"])
    err, err32 = np.abs(got["acc0"] - want), np.abs(want32 - want)
    _report(f"{mjcf} [a_0, alpha_0, q''] (largest {np.abs(want).max():.0f})", err, tol, err32)
    on = f[..., 2] > 0
    ef, ef32 = np.abs(gf - f), np.abs(f32_ - f)
    print(f"{mjcf} forces: kernel worst residual / bound {float((ef[on] / tol_f[on]).max()):.3f}, float32 restatement {float((ef32[on] / tol_f[on]).max()):.3f}")
    under = (m["ground_height"] - d["z"]) > 0
    vt = np.linalg.norm(np.einsum("nkid,nd->nki", d["J"], np.concatenate([s["v0"], s["w0"], s["v"]], 1))[..., :2], axis=-1)
    print(f"{under.sum()} of {under.size} points under the ground, {int((under & ~on).sum())} with the clamp live, {int((on & (vt < m['slip_velocity'])).sum())} "
          f"sliding below the slip velocity, {int((on & (vt > m['slip_velocity'])).sum())} above")
    assert 0.2 * under.size < under.sum() < 0.5 * under.size and (under & ~on).any() and (on & (vt < m["slip_velocity"])).any() and (on & (vt > m["slip_velocity"])).any()
    assert (err32 <= 0.25 * tol).all() and (ef32 <= 0.25 * tol_f).all(), ("K is too small for the float32 restatement", float((err32 / tol).max()))
    assert (ef <= tol_f).all(), (float((ef[on] / tol_f[on]).max()), np.argwhere(ef > tol_f)[:5].tolist())
    assert (err <= tol).all(), (float((err / tol).max()), np.argwhere(err > tol)[:5].tolist())


@pytest.mark.parametrize("mjcf,N", [(TREE, 33), (G1, 33)])
def test_consistency_with_the_fixed_base_kernel(mjcf, N):
    """the floating kernel's own (a_0, alpha_0), R_0 and w_0 handed to pbhc_debug_articulated_substeps as a prescribed base, its points' forces
    as joint torques J^T f: the two kernels' q'' agree within the sum of their bounds"""
    sk, m, p, table = _setup(mjcf)
    root, q, v, tau = fm.random_states(m, N, 7)
    s = fm.state(root, q, v)
    want, f, d = fm.forward(m, s, tau, H)
    got = _debug(sk, p, root, q, v, tau, 1)
    gf = _by_point(m, got["force"])
    tau_c = fm.f32(tau + np.einsum("nkid,nki->nd", d["J"], gf)[:, 6:])
    b13 = fm.f32(np.concatenate([root[:, 3:7], root[:, 10:13], got["acc0"][:, 3:6], got["acc0"][:, 0:3]], 1))
    _, _, qdd_fixed = _debug_fixed(sk, asim.ArticulatedSim.params(sk, ARM, DAMP), b13, q, v, tau_c, 1)
    base = dict(R0=am.quat_xyzw_to_matrix(b13[:, 0:4]), w0=b13[:, 4:7], alpha0=b13[:, 7:10], a0g=b13[:, 10:13] - m["gravity"])
    am_m = am.model(sk, ARM, DAMP)
    wf, df = am.forward(am_m, q, v, tau_c, base, H)
    tau_abs = np.abs(tau) + np.einsum("nkid,nki->nd", np.abs(d["J"]), np.abs(gf))[:, 6:]
    tol = GAMMA * (d["terms"][:, 6:] + am.qdd_bound_terms(am_m, wf, tau_abs, v, df))
    err = np.abs(got["acc0"][:, 6:] - qdd_fixed)
    _report(f"{mjcf} q'' floating - fixed", err, tol)
    assert np.abs(gf).max() > 10.0 and (err <= tol).all(), float((err / tol).max())


@pytest.mark.parametrize("mjcf", [TREE, G1])
def test_columns_of_the_inverse_inertia_matrix(mjcf):
    """D + 7 right-hand sides at one state at rest: nothing, the D unit joint torques, and unit forces through ONE contact point — on the
    root in one launch, under the last link in another — with a stiffness and a penetration that give 1 N up (no normal damping), and with
    friction 1 and the root moving at the slip velocity 1 N along -x or -y on top.  x(rhs) - x(nothing) is (H + diag)^-1 times that generalised
    force: the D joint columns, and the six combinations of the root's columns a force at a point reaches."""
    sk0 = _sk(mjcf)
    D, B = sk0.num_dof, sk0.num_bodies
    law = dict(stiffness=100.0, normal_damping=0.0, friction=1.0, slip_velocity=0.1, ground_height=0.0)
    rng = np.random.default_rng(9)
    q1 = fm.f32(rng.uniform(-0.6, 0.6, (1, D)))
    quat = rng.standard_normal((1, 4)); quat = fm.f32(quat / np.linalg.norm(quat))
    worst = 0.0
    for body, r in ((0, [0.05, -0.02, -0.1]), (B - 1, [0.03, 0.01, -0.04])):
        sk, m, p, table = _setup(mjcf, law=law, points=[(body, r)])
        n = D + 4
        R, pp, _ = am.kinematics(m, q1, fm.quat_to_matrix(quat))
        xz = pp[0, body, 2] + (R[0, body] @ m["points"][0][1])[2]
        root = np.zeros((n, 13)); root[:, 3:7] = quat
        root[:, 2] = 5.0                                     # rows 0 .. D: far above the ground
        root[D + 1:, 2] = -0.01 - xz                         # delta = 1 N / stiffness
        root[D + 2, 7], root[D + 3, 8] = -0.1, -0.1
        root = fm.f32(root)
        q, v = np.repeat(q1, n, 0), np.zeros((n, D))
        tau = np.zeros((n, D)); tau[1:D + 1] = np.eye(D)
        want, f, d = fm.forward(m, fm.state(root, q, v), tau, H)
        assert np.abs(f[D + 1:, 0] - np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]])).max() < 1e-4, f[D + 1:, 0]
        got = _debug(sk, p, root, q, v, tau, 1)
        cols, wcols = got["acc0"][1:] - got["acc0"][0], want[1:] - want[0]
        tol = GAMMA * (d["terms"][1:] + d["terms"][0])
        err = np.abs(cols - wcols)
        worst = max(worst, _report(f"{mjcf} point on body {body}: columns", err, tol))
        Hi = np.linalg.inv(d["Ht"][0])
        assert np.abs(wcols[:D] - Hi[:, 6:].T).max() < 1e-9 * np.abs(Hi).max()
        assert (err <= tol).all(), float((err / tol).max())
        assert np.abs(Hi[:6, 6:]).max() > 0.1, "no coupling between the root and the joints to speak of"


def _free_states(m, N, seed):
    rng = np.random.default_rng(seed)
    D = m["D"]
    quat = rng.standard_normal((N, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    root = np.concatenate([rng.uniform(-1, 1, (N, 2)), np.full((N, 1), 50.0), quat, rng.standard_normal((N, 3)), 1.5 * rng.standard_normal((N, 3))], 1)
    return fm.f32(root), fm.f32(rng.uniform(-0.6, 0.6, (N, D))), fm.f32(rng.standard_normal((N, D)))


@pytest.mark.parametrize("gravity", [(0.0, 0.0, 0.0), (0.0, 0.0, -9.81)])
def test_a_hundred_substeps_of_free_flight(gravity):
    """the seven-body tree, no torque, no damping, limits off, far above the ground, 100 sub-steps in ONE launch: the final state against the
    model within the carried bound.  Total linear and angular momentum, from the kernel's state in float64, against the model's within the
    bound carried through their derivatives (central differences): without gravity they stay where they started up to the integrator's own
    O(h) deviation, which the model shows; with gravity the centre of mass accelerates at g."""
    N, steps = 8, 100
    sk, m, p, table = _setup(TREE, arm=ARM, damp=0.0, gravity=gravity)
    D = sk.num_dof
    root, q, v = _free_states(m, N, 3)
    tau = np.zeros((N, D))
    s0 = fm.state(root, q, v)
    r = fm.carried_bound(m, s0, lambda q_, v_: tau[:1] * 0, H, steps, GAMMA, EPS, contact_on=True)
    r32 = fm.substeps(m, fm.state(root, q, v, np.float32), lambda q_, v_: np.zeros_like(q_), H, steps, dtype=np.float32)
    got = _debug(sk, p, root, q, v, tau, steps)
    assert not got["force"].any()
    err, err32 = fm.state_error(got["s"], r["s"], D), fm.state_error({k: x.astype(np.float64) for k, x in r32["s"].items()}, r["s"], D)
    _report(f"free flight, gravity {gravity[2]}: state after {steps} sub-steps", err, r["E"], err32)
    assert (err32 <= 0.25 * r["E"]).all(), "K is too small for the float32 restatement"
    assert (err <= r["E"]).all(), (float((err / r["E"]).max()), np.argwhere(err > r["E"])[:5].tolist())
    # momentum: |dP/de| E by central differences along every error coordinate
    P1, L1, c1 = fm.momentum(m, r["s"])
    Pg, Lg, cg = fm.momentum(m, got["s"])
    P0, L0, c0 = fm.momentum(m, s0)
    tolP, tolL = np.zeros((N, 3)), np.zeros((N, 3))
    for i in range(12 + 2 * D):
        Pp, Lp, _ = fm.momentum(m, fm._perturbed(r["s"], i, 1e-6, D))
        Pn, Ln, _ = fm.momentum(m, fm._perturbed(r["s"], i, -1e-6, D))
        tolP += np.abs(Pp - Pn) / 2e-6 * r["E"][:, i:i + 1]
        tolL += np.abs(Lp - Ln) / 2e-6 * r["E"][:, i:i + 1]
    print(f"momentum: |kernel - model| / bound P {float((np.abs(Pg - P1) / tolP).max()):.3f} L {float((np.abs(Lg - L1) / tolL).max()):.3f}; "
          f"model's own drift P {np.abs(P1 - P0).max():.2e} L {np.abs(L1 - L0).max():.2e} of {np.abs(L0).max():.2f}")
    assert (np.abs(Pg - P1) <= tolP).all() and (np.abs(Lg - L1) <= tolL).all()
    T, mass = steps * H, float(m["mass"].sum())
    if gravity[2] == 0.0:
        assert (np.abs(Pg - P0) <= np.abs(P1 - P0) + tolP).all()
        # angular momentum about the world origin of a body whose centre of mass moves: L = L_com + c x P, conserved as a whole
        assert (np.abs(Lg - L0) <= np.abs(L1 - L0) + tolL).all()
        assert np.abs(P1 - P0).max() < 1e-2 * np.abs(P0).max() and np.abs(L1 - L0).max() < 1e-2 * np.abs(L0).max()
    else:
        acc = (Pg - P0) / (mass * T)
        print(f"centre of mass acceleration {acc.mean(0)}")
        assert (np.abs(acc - np.asarray(gravity)) <= np.abs((P1 - P0) / (mass * T) - np.asarray(gravity)) + tolP / (mass * T)).all()
        assert np.abs((P1 - P0) / (mass * T) - np.asarray(gravity)).max() < 1e-2 * 9.81


def test_drop_and_rest():
    """the seven-body tree with four points under each of its two feet (c, f), released 2 mm above the ground, 100 sub-steps.  The test-only
    export holds the torque constant, so the pose is held by the torque of the standing tree's statics and a passive joint damping of
    20 N m s / rad where a policy would run a PD.  The final state against the model within the carried bound wherever the float32
    restatement is inside it too — which is every (robot, element), asserted here and on the CPU (tests/test_floating_sim_cpu.py); no point
    deeper than the model's deepest plus the bound."""
    N, steps = 8, 100
    sk = _sk(TREE)
    pts = fm.drop_points(sk)
    sk, m, p, table = _setup(TREE, arm=ARM, damp=fm.DROP_DAMP, law=fm.DROP_LAW, points=pts)
    D = sk.num_dof
    root, q, v, tau = fm.drop_inputs(m, N)
    s0 = fm.state(root, q, v)
    r = fm.transported_bound(m, s0, tau, H, steps, GAMMA, EPS)
    r32 = fm.substeps(m, fm.state(root, q, v, np.float32), lambda q_, v_: tau.astype(np.float32), H, steps, dtype=np.float32)
    err32 = fm.state_error({k: x.astype(np.float64) for k, x in r32["s"].items()}, r["s"], D)
    assert (err32 <= 0.25 * r["E"]).all(), ("the release leaves the float32 restatement outside a quarter of the bound", float((err32 / r["E"]).max()))
    got = _debug(sk, p, root, q, v, tau, steps)
    err = fm.state_error(got["s"], r["s"], D)
    _report(f"drop and rest: state after {steps} sub-steps (lowest point of the model {r['zmin'].min() * 1e3:.2f} mm)", err, r["E"], err32)
    assert (err <= r["E"]).all(), (float((err / r["E"]).max()), np.argwhere(err > r["E"])[:5].tolist())
    assert r["zmin"].max() < 0.0, "a robot never reached the ground"
    # the kernel's final point heights, in float64 from its state
    R, pp, _ = am.kinematics(m, got["s"]["q"], fm.quat_to_matrix(got["s"]["quat"]))
    z = np.stack([got["s"]["p0"][:, 2] + pp[:, b, 2] + np.einsum("nij,j->ni", R[:, b], rr)[:, 2] for b, rr in m["points"]], 1)
    slack = r["E"][:, 2] + r["E"][:, 3:6].sum(1) * 0.5 + r["E"][:, 12:12 + D].sum(1) * 0.5      # levers under 0.5 m
    assert (z.min(axis=1) >= r["zmin"] - slack).all(), (z.min(axis=1), r["zmin"])
    assert np.abs(got["s"]["v0"]).max() < 0.2, "the tree did not come to rest"


# ---- through the env ---------------------------------------------------------------------------------------------------------------------
def _overrides(cfgname, dr=True, extra=None, spec=None):
    ov = case_overrides(cfgname, dr, extra, sim=False)
    ov["simulator._target_"] = SIM
    ov["simulator.config.floating_sim"] = dict({"armature": ARM, "damping": DAMP, "contact_points": G1_POINTS}, **(spec or {}))
    return ov


def _build(cfgname, N, general, dr=True, extra=None, seed=3, noise_off=True, spec=None):
    _seed_all(seed)
    return build_hip_env(cfgname, N, general=general, overrides=_overrides(cfgname, dr, extra, spec), noise_off=noise_off)


def _env_model(env):
    s = env.simulator
    return fm.model(env.skeleton, ARM, DAMP, s.gravity, s.points, stiffness=s.stiffness, normal_damping=s.normal_damping, friction=s.friction,
                    slip_velocity=s.slip_velocity, ground_height=s.ground_height)


def _model_step(m, root, q, v, a_del, P):
    """the control step's sub-steps on the model from the state the previous step left, with the carried bound"""
    N = q.shape[0]
    tiled = {}

    def tile_fn(k):
        tiled["P"] = {key: (np.tile(x, (k, 1)) if isinstance(x, np.ndarray) and x.ndim == 2 and x.shape[0] == N else x) for key, x in P.items()}
        tiled["a"] = np.tile(a_del, (k, 1))

    pick = lambda q_: (tiled["P"], tiled["a"]) if q_.shape[0] != N else (P, a_del)
    torque = lambda q_, v_: jm.torque(q_, v_, pick(q_)[1], pick(q_)[0])
    tabs = lambda q_, v_: _tau_abs(q_, v_, pick(q_)[1], pick(q_)[0])
    return fm.carried_bound(m, fm.state(root, q, v), torque, P["h"], P["decimation"], GAMMA, EPS, lo=P["lo"], hi=P["hi"], tau_abs_fn=tabs, tile_fn=tile_fn)


def _run_case(cfgname, N, general, steps=None, zero_actions=False, prepare=None, after_step=None):
    """prepare(env) / after_step(env, k): the hooks of tests/test_gpu_parity.py's _env_step_vs_oracle"""
    cfg, env = _build(cfgname, N, general)
    D = env.num_dof
    sc = scenario(N, D, float(env._c.action_clip_value))
    _prepare(env, sc)
    s = env.simulator
    s.set_debug_torques(True)
    if prepare is not None:
        prepare(env)
    m = _env_model(env)
    out = []
    for k in range(sc["steps"] if steps is None else steps):
        kk = k % sc["steps"]
        actions = np.zeros_like(sc["actions"][kk]) if zero_actions else sc["actions"][kk]
        env.set_injected_draws(u_rfi=torch.from_numpy(sc["u_rfi"][kk]).to(env.device))
        P = _torque_params(env, sc["u_rfi"][kk])
        pre = dict(q=_np(s.dof_pos), v=_np(s.dof_vel), root=_np(s.robot_root_states), queue=_np(env.action_queue), delay=env.action_delay_idx.cpu().numpy())
        a_del = jm.delayed_action(actions, float(env._c.action_clip_value), pre["queue"], pre["delay"], bool(env._c.randomize_ctrl_delay))
        env.step({"actions": torch.from_numpy(actions).to(env.device)})
        torch.cuda.synchronize()
        if after_step is not None:
            after_step(env, k)
        out.append(dict(P=P, pre=pre, a_del=a_del, reset=env.reset_buf.bool().cpu().numpy(), frame_q=_np(s.replay["dof_pos"][0]),
                        frame_v=_np(s.replay["dof_vel"][0]), frame_root=_np(s.replay["root"][0]), frame_contact=s.replay["contact"][0].clone(),
                        root=_np(s.robot_root_states), dof_pos=_np(s.dof_pos), tau0=s.tau0.clone(), torques=env.torques.clone()))
    return env, m, out


_RUNS = {}


def _case(*key):
    if key not in _RUNS:
        _RUNS[key] = _run_case(*key)
    return _RUNS[key]


def got_v(r):
    return r["frame_root"][:, 7:13]


def _compare_step(m, r, D):
    mm = _model_step(m, r["pre"]["root"], r["pre"]["q"], r["pre"]["v"], r["a_del"], r["P"])
    got = fm.state(r["frame_root"], r["frame_q"], r["frame_v"])
    err = fm.state_error(got, mm["s"], D)
    ok = (mm["margin"].min(axis=1) >= 1e-5) & (mm["touch"] >= 1e-6)
    return mm, err, ok


@pytest.mark.parametrize("cfgname,N,general", [(WALK, 70, False), (STUDENT, 33, True)])
def test_frame_equals_the_model_one_step_at_a_time(cfgname, N, general):
    """From the state step k - 1 left (root_states and dof_state, resets included), the queue peeked before step k and the DR scales, the
    model's root and joints after the sub-steps are the frame step k consumed, per element within the carried bound.  An (env, step) pair in
    which the model has a pre-clamp position within 1e-5 rad of a limit or a contact point within 1e-6 m of the ground at the start of a
    sub-step is skipped (both laws are discontinuous there); at most 1 % of the pairs.  tau0 is the step's `torques`, bit for bit, and the
    contact frame holds all three components on the bodies that own points and nothing elsewhere."""
    env, m, steps = _case(cfgname, N, general)
    D = env.num_dof
    owners = sorted({b for b, _ in m["points"]})
    skipped = total = touching = 0
    worst = 0.0
    for k, r in enumerate(steps):
        mm, err, ok = _compare_step(m, r, D)
        skipped += int((~ok).sum()); total += N
        ratio = float((err / mm["E"])[ok].max())
        worst = max(worst, ratio)
        print(f"{cfgname} step {k}: worst residual / bound {ratio:.3f}, skipped {int((~ok).sum())}, resets {int(r['reset'].sum())}, lowest point "
              f"{mm['zmin'].min() * 1e3:.1f} mm")
        assert not (err > mm["E"])[ok].any(), (k, ratio, np.argwhere((err > mm["E"]) & ok[:, None])[:5].tolist())
        keep = torch.from_numpy(~r["reset"]).to(r["tau0"].device)
        assert torch.equal(r["tau0"][keep], r["torques"][keep]), (k, float((r["tau0"] - r["torques"])[keep].abs().max()))
        assert np.array_equal(r["root"][~r["reset"]], r["frame_root"][~r["reset"]]) and np.array_equal(r["dof_pos"][~r["reset"]], r["frame_q"][~r["reset"]])
        c = r["frame_contact"].cpu().double().numpy()
        rest = c.copy(); rest[:, owners] = 0.0
        assert not rest.any()
        fsum = np.zeros((N, len(owners), 3))
        for j, (b, _) in enumerate(m["points"]):
            fsum[:, owners.index(b)] += mm["f"][:, j]
        # the last sub-step's forces from a state that is off by at most E: per point stiffness x its height's error + normal_damping x its
        # velocity's error (levers under 1 m), the friction at most (1 + friction) of that plus its direction's; four points per body
        E = mm["E"]
        ez = E[:, 2] + E[:, 3:6].sum(1) + E[:, 12:12 + D].sum(1)
        ev = E[:, 6:9].sum(1) + E[:, 9:12].sum(1) + E[:, 12 + D:].sum(1) + np.abs(np.concatenate([got_v(r), r["frame_v"]], 1)).max(1) * ez
        tolc = 4 * (1 + m["friction"]) * (m["stiffness"] * ez + m["normal_damping"] * ev) + m["friction"] * np.abs(fsum[..., 2]).sum(1) / m["slip_velocity"] * ev
        tolc = tolc[:, None, None] + GAMMA * 4 * (1.0 + np.abs(fsum))
        assert (np.abs(c[:, owners] - fsum)[ok] <= tolc[ok]).all(), float((np.abs(c[:, owners] - fsum)[ok] / tolc[ok]).max())
        touching += int((np.abs(c[:, owners, :2]).sum(-1) > 0).sum())
    print(f"{cfgname}: worst residual / bound over the run {worst:.3f}; {skipped} of {total} pairs skipped; {touching} foot-steps with tangential force")
    assert skipped <= 0.01 * total, (skipped, total)
    assert touching > 0, "no foot ever carried a tangential force: the three components were never exercised"
    assert sum(int(r["reset"].sum()) for r in steps) < len(steps) * N


def test_falling_terminates_and_the_reset_is_picked_up():
    """zero actions at N = 33: within the clip's length some env is reset because the robot fell (terminate_by_gravity or motion-far, not a
    time-out), and on the following step that env's frame starts from the reset root the step wrote into root_states (the model stepped from
    it agrees with the frame).  A fallen robot is an ordinary state: nothing is provoked on the GPU."""
    N = 33
    cfg, env = _build(WALK, N, False, dr=False)
    env.reset_all()
    s, D = env.simulator, env.num_dof
    m = _env_model(env)
    zero = torch.zeros(N, D, device=env.device)
    max_steps = int(float(env.motion_len.max()) / float(env.dt)) + 2
    fell = None
    for k in range(max_steps):
        env.step({"actions": zero})
        fallen = (env.reset_buf.bool() & ~env.time_out_buf.bool()).cpu().numpy()
        if fallen.any():
            fell = np.flatnonzero(fallen)
            break
    assert fell is not None, f"no env fell within {max_steps} steps"
    print(f"step {k}: envs {fell.tolist()} fell; root height {_np(s.replay['root'][0])[fell, 2]}")
    P = _torque_params(env)
    pre = dict(q=_np(s.dof_pos), v=_np(s.dof_vel), root=_np(s.robot_root_states))
    assert not np.array_equal(pre["root"][fell], _np(s.replay["root"][0])[fell]), "the step did not write a reset root"
    a_del = jm.delayed_action(np.zeros((N, D)), float(env._c.action_clip_value), None, None, False)
    env.step({"actions": zero})
    torch.cuda.synchronize()
    mm = _model_step(m, pre["root"], pre["q"], pre["v"], a_del, P)
    got = fm.state(_np(s.replay["root"][0]), _np(s.replay["dof_pos"][0]), _np(s.replay["dof_vel"][0]))
    err = fm.state_error(got, mm["s"], D)
    ok = (mm["margin"].min(axis=1) >= 1e-5) & (mm["touch"] >= 1e-6)
    assert ok[fell].any()
    sel = fell[ok[fell]]
    print(f"after the reset: worst residual / bound {float((err / mm['E'])[sel].max()):.3f}")
    assert (err[sel] <= mm["E"][sel]).all()


def _rollouts(rollout_graph, rollouts=3):
    """MHPPO at 64 envs, 8 steps per rollout, `_training_step` after every rollout; as tests/test_gpu_articulated_sim.py _rollouts"""
    from pbhc_amd.agents.mh_ppo import MHPPO

    flags = {"PBHC_ROLLOUT_GRAPH": "1" if rollout_graph else "0", "PBHC_ROLLOUT_SPLIT": "1", "PBHC_CRITIC_BATCHED": "1", "PBHC_FUSED_SAMPLE": "1"}
    os.environ.update(flags)
    try:
        cfg, env = _build(WALK, 64, False, extra={"algo.config.num_steps_per_env": 8}, seed=11, noise_off=False)
        algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device=DEV)
        algo.setup()
        algo._train_mode()
        obs = env.reset_all()
        used = []
        gperm = torch.Generator().manual_seed(23)
        start = algo._pflat.clone()
        for r in range(rollouts):
            algo.storage.clear()
            obs = algo._rollout_step(obs)
            used.append(bool(getattr(algo, "_rollout_used_graph", False)))
            n = algo.storage.num_envs * algo.storage.num_transitions_per_env
            algo._training_step(indices=torch.randperm(n, generator=gperm).to(DEV))
        torch.cuda.synchronize()
        out = {k: getattr(algo, k).clone() for k in ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step")}
        out.update(dof_state=env.simulator.dof_state.clone(), root=env.simulator.robot_root_states.clone(), globals=env.globals.clone(),
                   frame_q=env.simulator.replay["dof_pos"].clone(), frame_root=env.simulator.replay["root"].clone(),
                   frame_contact=env.simulator.replay["contact"].clone(), actions=algo.storage.actions.clone(), rewards=algo.storage.rewards.clone())
        return out, used, start
    finally:
        for k in flags:
            os.environ.pop(k, None)


def test_captured_rollout_equals_the_eager_loop():
    """the simulator's launch inside the rollout hipGraph: weights, Adam moments, root and dof_state bit-identical to the step-by-step loop"""
    a, used_a, start = _rollouts(True)
    b, used_b, _ = _rollouts(False)
    assert used_a == [False, True, True] and not any(used_b)
    assert not torch.equal(a["_pflat"], start)
    assert bool(torch.isfinite(a["dof_state"]).all()) and bool(torch.isfinite(a["root"]).all())
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_resume_is_bit_identical():
    """six env steps in one run; in a second run three steps, state_dict(), a fresh env, load_state_dict(), three more: the root the
    simulator starts from is root_states, which the env's state_dict already holds"""
    N = 70
    sc = scenario(N, 23, 100.0)

    def steps(env, ks):
        for k in ks:
            obs, _, _, _ = env.step({"actions": torch.from_numpy(sc["actions"][k]).to(env.device)})
        torch.cuda.synchronize()
        return obs

    _, env_a = _build(WALK, N, False, seed=5, noise_off=False)
    _prepare(env_a, sc)
    obs_a = steps(env_a, range(6))
    _, env_b = _build(WALK, N, False, seed=5, noise_off=False)
    _prepare(env_b, sc)
    steps(env_b, range(3))
    sd = env_b.state_dict()
    _, env_c = _build(WALK, N, False, seed=5, noise_off=False)
    env_c.load_state_dict(sd)
    obs_c = steps(env_c, range(3, 6))
    for k in obs_a:
        assert torch.equal(obs_a[k], obs_c[k]), k
    assert torch.equal(env_a.simulator.dof_state, env_c.simulator.dof_state)
    assert torch.equal(env_a.reset_buf, env_c.reset_buf)
    assert torch.equal(env_a.simulator.robot_root_states, env_c.simulator.robot_root_states)
    assert torch.equal(env_a.simulator.replay["root"], env_c.simulator.replay["root"])
    assert int(env_a._episode_length_buf.min()) < 6, "no env reset inside the six steps"
