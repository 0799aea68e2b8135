"""ArticulatedSim on the GPU (pbhc_amd/simulator/articulated_sim.py, csrc/pbhc_articulated_sim.hip): the device function against the float64
model of tests/articulated_model.py (a different formulation: Jacobians and a classical Newton-Euler sweep against the kernel's
articulated-body algorithm) through the test-only export, then through the env one control step at a time, the first sub-step's torque
against the step's own `torques`, the root / contact frame, graph = eager, resume, and the closed loop.

Bounds.  Per element, float64, from magnitudes: a relative error gamma = K 2^-24 of every product that enters q'' moves it by at most
    gamma (|Mt^-1| (|Mt| |q''| + |tau| + |b v| + sum |terms of c|))_i            (articulated_model.qdd_bound_terms)
and that is carried through the sub-steps as v += h q'', q += h v are (articulated_model.substeps: bv, bq), plus the roundings of the state
itself, 4 eps per sub-step of the largest |v| and |q|.  Over the 100 sub-steps of the passive runs the error of earlier sub-steps also comes
back through dq''/d(q, v) (a falling tree is sensitive to its state); there the bound carries |dq''/dq| and |dq''/dv| (central differences of
the model) as well.  K is not chosen by what the kernel gives: the model is re-run in numpy float32 on the same inputs and K set so that this
restatement stays at <= 0.25 of the bound (asserted below, without the GPU's result): the kernel orders its operations differently from
the model, hence the factor 4.
    K_QDD = 16: the float32 restatement's worst error is 2.9 eps x the terms (G1 23 dof, three seeds), 0.18 of the bound, and 0.18 of the
    carried bound after 100 sub-steps; each test prints its own figures.  The kernel's worst residual / bound as measured on an MI355X: q'' of
    one sub-step 0.15 (tree) / 0.27 (G1 23) / 0.25 (G1 29), columns of Mt^-1 0.04, 100 sub-steps 0.33, through the env 0.12 / 0.09 / 0.10
    (walk / student / teacher); also in DESIGN.md §8.

The scenario through the env is tests/test_gpu_joint_sim.py's (`scenario`): control delay, PD-gain DR, RAO and RFI on, two torque limits lowered
to 1 N m, joints started beyond a limit, envs that run off their clip — with armature 0.02, damping 0.05, gravity on."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.simulator import articulated_sim as asim
from pbhc_amd.skeleton import Skeleton
from pbhc_amd.utils.config import load_config
from tests import articulated_model as am
from tests import joint_sim_model as jm
from tests.helpers import GOLDEN, build_hip_env
from tests.test_gpu_joint_sim import scenario

pytestmark = pytest.mark.gpu

SIM = "pbhc_amd.simulator.articulated_sim.ArticulatedSim"
WALK, STUDENT, TEACHER = "v1_g1_23dof_walk.yaml", "v2_g1_23dof_student.yaml", "v2_g1_29dof_teacher.yaml"
G1, G1_29 = "mjcf/g1_23dof_lock_wrist_fitmotionONLY.xml", "mjcf/g1_29dof_rev_1_0.xml"
TREE = "mjcf/articulated_tree.xml"
WALK_CASE = (WALK, 70, False)
CASES = [WALK_CASE, (STUDENT, 33, True), (TEACHER, 9, True)]
MJCF_OF = {WALK: G1, STUDENT: G1, TEACHER: G1_29}
LOWERED = (2, 10)                                          # dofs whose torque limit is lowered
ARM, DAMP = 0.02, 0.05
EPS = 2.0 ** -24
K_QDD = 16
GAMMA = K_QDD * EPS
DEV = "cuda:0"
H = 0.005


def case_overrides(cfgname, dr=True, extra=None, sim=True, spec=None):
    base = load_config(os.path.join(GOLDEN, "configs", cfgname), {}, now="test")
    lim = [float(x) for x in base.robot.dof_effort_limit_list]
    if dr:
        for d in LOWERED:
            lim[d] = 1.0
    ov = {"domain_rand.push_robots": False, "robot.dof_effort_limit_list": lim, "robot.motion.asset.assetFileName": MJCF_OF[cfgname],
          "domain_rand.randomize_ctrl_delay": dr, "domain_rand.ctrl_delay_step_range": [0, 2], "domain_rand.randomize_pd_gain": dr,
          "domain_rand.use_rao": dr, "domain_rand.randomize_torque_rfi": dr, "domain_rand.randomize_rfi_lim": dr}
    if sim:
        ov["simulator._target_"] = SIM
        ov["simulator.config.articulated_sim"] = dict({"armature": ARM, "damping": DAMP}, **(spec or {}))
    ov.update(extra or {})
    return ov


def _seed_all(seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)


def _build(cfgname, N, general, dr=True, extra=None, seed=3, noise_off=True, spec=None):
    _seed_all(seed)
    return build_hip_env(cfgname, N, general=general, overrides=case_overrides(cfgname, dr, extra, spec=spec), noise_off=noise_off)


def _np(t):
    return t.detach().double().cpu().numpy()


# ---- the test-only export ------------------------------------------------------------------------------------------------------------------
def _debug(sk, p, base13, q, v, tau, steps, h=H, limits=None, place=None):
    """pbhc_debug_articulated_substeps on float32 copies of the inputs -> (q, v, qdd0) float64 numpy.  place(name, tensor) -> tensor: where
    every device operand goes (tests/test_gpu_step_memory.py: into arenas)"""
    place = place or (lambda name, x: x)
    t = lambda name, a: place(name, torch.as_tensor(np.asarray(a, np.float32)).to(DEV).contiguous())
    tb, tq, tv, tt = t("base", base13), t("q", q), t("v", v), t("tau", tau)
    n = tq.shape[0]
    oq, ov, oa = (place(name, torch.zeros_like(tq)) for name in ("out_q", "out_v", "out_qdd0"))
    lim = None if limits is None else np.ascontiguousarray(limits, np.float32)
    csk = sk.to_c()
    _lib.check(_lib.lib().pbhc_debug_articulated_substeps(C.byref(csk), C.byref(p), tb.data_ptr(), tq.data_ptr(), tv.data_ptr(), tt.data_ptr(), n, steps, h,
                                                          int(limits is not None), None if lim is None else lim.ctypes.data, oq.data_ptr(), ov.data_ptr(),
                                                          oa.data_ptr(), _lib.current_stream()), "pbhc_debug_articulated_substeps")
    torch.cuda.synchronize()
    return _np(oq), _np(ov), _np(oa)


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def random_inputs(sk, N, seed, moving_base=True):
    """float32-representable (q, v, tau, base13) and the model's base dict from the same numbers"""
    rng = np.random.default_rng(seed)
    D = sk.num_dof
    q, v, tau = _f32(rng.uniform(-0.6, 0.6, (N, D))), _f32(2.0 * rng.standard_normal((N, D))), _f32(10.0 * rng.standard_normal((N, D)))
    b13 = np.zeros((N, 13))
    b13[:, 3] = 1.0
    if moving_base:
        quat = rng.standard_normal((N, 4))
        b13 = np.concatenate([quat / np.linalg.norm(quat, axis=1, keepdims=True), rng.standard_normal((N, 3)), 3.0 * rng.standard_normal((N, 3)),
                              2.0 * rng.standard_normal((N, 3))], 1)
    b13 = _f32(b13)
    return q, v, tau, b13, base_of(b13)


def base_of(b13, gravity=(0.0, 0.0, -9.81)):
    b13 = np.asarray(b13, np.float64)
    return dict(R0=am.quat_xyzw_to_matrix(b13[:, 0:4]), w0=b13[:, 4:7], alpha0=b13[:, 7:10], a0g=b13[:, 10:13] - np.asarray(gravity, np.float64))


def _sk(mjcf):
    return Skeleton.from_mjcf(os.path.join(GOLDEN, mjcf))


def _report(what, err, tol, err32=None):
    r = float((err / tol).max())
    msg = f"{what}: kernel worst residual / bound {r:.3f}"
    if err32 is not None:
        msg += f", float32 restatement {float((err32 / tol).max()):.3f}"
    print(msg)
    return r


@pytest.mark.parametrize("mjcf,N", [(TREE, 33), (G1, 33), (G1_29, 9)])
def test_qdd_of_one_substep_equals_the_model(mjcf, N):
    """random poses (+-0.6 rad), velocities (sigma 2 rad/s), torques (sigma 10 N m), base orientations, angular velocities and accelerations:
    q'' = dv / h of ONE sub-step against the model, per element within gamma x the bound terms; the float32 restatement within a quarter of it"""
    sk = _sk(mjcf)
    m = am.model(sk, ARM, DAMP)
    p = asim.ArticulatedSim.params(sk, ARM, DAMP)
    q, v, tau, b13, base = random_inputs(sk, N, 5)
    want, d = am.forward(m, q, v, tau, base, H)
    tol = GAMMA * am.qdd_bound_terms(m, want, tau, v, d)
    want32, _ = am.forward(m, q, v, tau, base, H, np.float32)
    _, _, got = _debug(sk, p, b13, q, v, tau, 1)
    err, err32 = np.abs(got - want), np.abs(want32 - want)
    _report(f"{mjcf} q'' (largest |q''| {np.abs(want).max():.0f})", err, tol, err32)
    assert (err32 <= 0.25 * tol).all(), ("K_QDD is too small for the float32 restatement", float((err32 / tol).max()))
    assert (err <= tol).all(), (float((err / tol).max()), np.argwhere(err > tol)[:5].tolist())


@pytest.mark.parametrize("mjcf", [TREE, G1, G1_29])
def test_columns_of_the_inverse_inertia_matrix(mjcf):
    """D + 1 torque vectors at one state (0 and the unit vectors): q''(e_i) - q''(0) is column i of (M + diag(armature + h b))^-1 — the whole
    matrix the kernel never forms.  Bound: the two q'' bounds added."""
    sk = _sk(mjcf)
    D = sk.num_dof
    m = am.model(sk, ARM, DAMP)
    p = asim.ArticulatedSim.params(sk, ARM, DAMP)
    q1, v1, _, b1, _ = random_inputs(sk, 1, 9)
    rep = lambda a: np.repeat(a, D + 1, axis=0)
    q, v, b13 = rep(q1), rep(v1), rep(b1)
    tau = np.concatenate([np.zeros((1, D)), np.eye(D)], 0)
    base = base_of(b13)
    want, d = am.forward(m, q, v, tau, base, H)
    terms = am.qdd_bound_terms(m, want, tau, v, d)
    _, _, got = _debug(sk, p, b13, q, v, tau, 1)
    Minv = np.linalg.inv(d["Mt"][0])
    cols, tol = (got[1:] - got[0]).T, GAMMA * (terms[1:] + terms[0]).T
    err = np.abs(cols - Minv)
    _report(f"{mjcf} Mt^-1 (cond {np.linalg.cond(d['Mt'][0]):.0f}, largest entry {np.abs(Minv).max():.1f})", err, tol)
    assert (err <= tol).all(), float((err / tol).max())
    assert np.abs(Minv - np.diag(np.diag(Minv))).max() > 1.0, "no coupling to speak of"


def _carried_bound(m, q0, v0, tau, base, h, steps, dtype=np.float64):
    """the model's trajectory under a constant torque and the first-order error bound of a float32 run of it: per sub-step
        e_v += h (gamma terms + |dq''/dq| e_q + |dq''/dv| e_v) + 4 eps |v|,   e_q += h e_v + 4 eps |q|"""
    N, D = q0.shape
    q, v = q0.copy(), v0.copy()
    e_q, e_v = np.zeros((N, D)), np.zeros((N, D))
    dlt = 1e-6
    tile = lambda a: np.tile(a, (4 * D + 1,) + (1,) * (a.ndim - 1))
    baseT = {k: tile(x) for k, x in base.items()}
    for _ in range(steps):
        Q, V = tile(q), tile(v)
        for d in range(D):
            Q[(1 + 2 * d) * N:(2 + 2 * d) * N, d] += dlt; Q[(2 + 2 * d) * N:(3 + 2 * d) * N, d] -= dlt
            V[(1 + 2 * D + 2 * d) * N:(2 + 2 * D + 2 * d) * N, d] += dlt; V[(2 + 2 * D + 2 * d) * N:(3 + 2 * D + 2 * d) * N, d] -= dlt
        qdd, dd = am.forward(m, Q, V, tile(tau), baseT, h)
        d0 = {k: x[:N] for k, x in dd.items()}
        terms = am.qdd_bound_terms(m, qdd[:N], tau, v, d0)
        Jq = np.stack([(qdd[(1 + 2 * d) * N:(2 + 2 * d) * N] - qdd[(2 + 2 * d) * N:(3 + 2 * d) * N]) / (2 * dlt) for d in range(D)], -1)
        Jv = np.stack([(qdd[(1 + 2 * D + 2 * d) * N:(2 + 2 * D + 2 * d) * N] - qdd[(2 + 2 * D + 2 * d) * N:(3 + 2 * D + 2 * d) * N]) / (2 * dlt) for d in range(D)], -1)
        v = v + h * qdd[:N]
        q = q + h * v
        e_v = e_v + h * (GAMMA * terms + np.einsum("nij,nj->ni", np.abs(Jq), e_q) + np.einsum("nij,nj->ni", np.abs(Jv), e_v)) + 4 * EPS * np.abs(v)
        e_q = e_q + h * e_v + 4 * EPS * np.abs(q)
    return q, v, e_q, e_v


def _energy(m, q, v, base):
    d = am.dynamics(m, q, v, base)
    return d["T"] + 0.5 * (m["armature"] * v * v).sum(1) + d["V"], d


def test_a_hundred_substeps_of_the_passive_tree_and_gravity_compensation():
    """the seven-body tree, base at rest, damping 0, limits off, 100 sub-steps of 5 ms in ONE launch.  Rows 0..3: no torque, started at rest from
    random poses — state and total energy against the model's trajectory.  Rows 4..7: tau = c(q, 0) (float32), the gravity compensation —
    the pose holds: the model's own trajectory under that rounded torque barely moves, and the kernel stays within the bound of it.
    The energy's bound is the state's carried through |dE/dq| (central differences) and dE/dv = (M + armature) v."""
    sk = _sk(TREE)
    D, steps = sk.num_dof, 100
    m = am.model(sk, ARM, 0.0)
    p = asim.ArticulatedSim.params(sk, ARM, 0.0)
    q4 = _f32(np.random.default_rng(3).uniform(-0.6, 0.6, (4, D)))
    q0 = np.concatenate([q4, q4], 0)
    v0 = np.zeros((8, D))
    base = am.rest_base(8)
    b13 = np.zeros((8, 13)); b13[:, 3] = 1.0
    hold = _f32(am.dynamics(m, q4, np.zeros((4, D)), am.rest_base(4))["c"])
    tau = np.concatenate([np.zeros((4, D)), hold], 0)
    qm, vm, e_q, e_v = _carried_bound(m, q0, v0, tau, base, H, steps)
    r32 = am.substeps(m, q0, v0, lambda q_, v_: tau.astype(np.float32), base, H, steps, dtype=np.float32)
    gq, gv, _ = _debug(sk, p, b13, q0, v0, tau, steps)
    rq = _report("100 sub-steps, q", np.abs(gq - qm), e_q, np.abs(r32["q"] - qm))
    rv = _report("100 sub-steps, v", np.abs(gv - vm), e_v, np.abs(r32["v"] - vm))
    assert (np.abs(r32["q"] - qm) <= 0.25 * e_q).all() and (np.abs(r32["v"] - vm) <= 0.25 * e_v).all(), "K_QDD is too small for the float32 restatement"
    assert rq <= 1.0 and rv <= 1.0
    # the passive rows moved, the compensated ones did not
    assert np.abs(qm[:4] - q0[:4]).max() > 0.3 and np.abs(vm[:4]).max() > 1.0
    print(f"gravity compensation: model drift {np.abs(qm[4:] - q0[4:]).max():.2e} rad, kernel drift {np.abs(gq[4:] - q0[4:]).max():.2e} rad, "
          f"bound {e_q[4:].max():.2e}")
    assert np.abs(gq[4:] - q0[4:]).max() < np.abs(qm[4:] - q0[4:]).max() + e_q[4:].max()
    assert np.abs(gq[4:] - q0[4:]).max() < 1e-3
    # total energy of the passive rows
    Em, dm = _energy(m, qm[:4], vm[:4], am.rest_base(4))
    Eg, _ = _energy(m, gq[:4], gv[:4], am.rest_base(4))
    E0, _ = _energy(m, q0[:4], v0[:4], am.rest_base(4))
    dEdv = np.abs(np.einsum("nij,nj->ni", am.mtilde(m, dm["M"]), vm[:4]))
    dEdq = np.zeros((4, D))
    for d in range(D):
        qp, qn = qm[:4].copy(), qm[:4].copy()
        qp[:, d] += 1e-6; qn[:, d] -= 1e-6
        dEdq[:, d] = np.abs(_energy(m, qp, vm[:4], am.rest_base(4))[0] - _energy(m, qn, vm[:4], am.rest_base(4))[0]) / 2e-6
    tolE = (dEdq * e_q[:4]).sum(1) + (dEdv * e_v[:4]).sum(1)
    print(f"energy: start {E0}, model end {Em}, kernel end {Eg}, |kernel - model| / bound {np.abs(Eg - Em) / tolE}")
    assert (np.abs(Eg - Em) <= tolE).all()
    assert (np.abs(Eg - E0) < 0.05 * np.abs(dm["T"]).max() + tolE).all(), "the kernel's energy left the start by more than 5 % of the kinetic energy"


# ---- through the env ---------------------------------------------------------------------------------------------------------------------
def _torque_params(env, u_rfi=None):
    """the torque law's parameters from the env's own float32 values (config struct, DR scales as they stand NOW)"""
    c, D = env._c, env.num_dof
    f = lambda a: np.array([a[d] for d in range(D)], np.float64)
    return dict(control_type=int(c.control_type), Kp=f(c.p_gains), Kd=f(c.d_gains), action_scale=f(c.action_scale), torque_limit=f(c.torque_limits),
                lo=np.array([c.hard_dof_pos_limits[d][0] for d in range(D)], np.float64), hi=np.array([c.hard_dof_pos_limits[d][1] for d in range(D)], np.float64),
                default=_np(env.default_dof_pos) if c.randomize_default_dof_pos else f(c.default_dof_pos),
                kp=_np(env._kp_scale), kd=_np(env._kd_scale), rfi_scale=_np(env._rfi_lim_scale), rao_scale=_np(env._rao_scale),
                u_rfi=None if (u_rfi is None or not c.randomize_torque_rfi) else np.asarray(u_rfi, np.float64), rfi_lim=float(c.rfi_lim), n_ps=None,
                ps_rfi_lim=0.0, use_rao=bool(c.use_rao), clip_torques=bool(c.clip_torques), h=float(c.sim_dt), decimation=int(env.simulator._params.decimation))


def _tau_abs(q, v, a_del, P):
    """what the float32 torque's error scales with: its terms' magnitudes and, inside the kp term, the operands of the cancelling sum
    (as tests/test_gpu_joint_sim.py's bound against the float64 model)"""
    t_p, t_d, noise, _ = jm.torque_terms(q, v, a_del, P)
    inner = np.abs(a_del * P["action_scale"]) + np.abs(P["default"]) + np.abs(q)
    return np.abs(t_p) + np.abs(t_d) + np.abs(noise) + (P["kp"] * P["Kp"] * inner if P["control_type"] == 0 else 0.0)


def _model_step(m, q, v, a_del, P, base, limits=True):
    """the control step's sub-steps on the model; the torque's own float32 error enters the bound through _tau_abs"""
    h, dec = P["h"], P["decimation"]
    q, v = np.array(q, np.float64), np.array(v, np.float64)
    bq, bv = np.zeros_like(q), np.zeros_like(q)
    vmax, qmax = np.abs(v), np.abs(q)
    margin = np.full(q.shape, np.inf)
    tau0 = None
    for s in range(dec):
        tau = jm.torque(q, v, a_del, P)
        if s == 0:
            tau0 = tau
        qdd, d = am.forward(m, q, v, tau, base, h)
        terms = am.qdd_bound_terms(m, qdd, _tau_abs(q, v, a_del, P), v, d)
        v = v + h * qdd
        q = q + h * v
        bv = bv + h * terms
        bq = bq + h * bv
        vmax, qmax = np.maximum(vmax, np.abs(v)), np.maximum(qmax, np.abs(q))
        margin = np.minimum(margin, np.minimum(np.abs(q - P["lo"]), np.abs(q - P["hi"])))
        if limits:
            q, v = am.clamp(q, v, P["lo"], P["hi"])
    tol_v = GAMMA * bv + 4 * EPS * dec * vmax
    tol_q = GAMMA * bq + h * dec * tol_v + 4 * EPS * dec * qmax
    return dict(q=q, v=v, tau0=tau0, margin=margin, tol_q=tol_q, tol_v=tol_v)


def _prepare(env, sc):
    """reset, then the scenario's initial state: joints beyond a limit, envs about to run off their clip"""
    env.reset_all()
    s = env.simulator
    lim = s.hard_dof_pos_limits
    N, D = env.num_envs, env.num_dof
    for e, d, side in sc["beyond_limit"]:
        s.dof_pos[e, d] = lim[d, side] + (0.05 if side else -0.05)
    for e in sc["ending"]:
        e = min(e, N - 1)
        env.motion_start_times[e] = env.motion_len[e] - 3.5 * env.dt - env._episode_length_buf[e].float() * env.dt
    torch.cuda.synchronize()


def _run_case(cfgname, N, general, inject, base_acceleration=True):
    """six steps; per step the kernel's frame, tau0, base accelerations and the step's torques, next to the model's prediction from the kernel's
    OWN pre-step state and the base the kernel itself wrote (root row) and used (accelerations)"""
    cfg, env = _build(cfgname, N, general, spec={"base_acceleration": base_acceleration})
    D = env.num_dof
    sc = scenario(N, D, float(env._c.action_clip_value))
    _prepare(env, sc)
    s = env.simulator
    s.set_debug_torques(True)
    s.set_debug_base(True)
    m = am.model(env.skeleton, ARM, DAMP)
    out = []
    for k in range(sc["steps"]):
        u = torch.from_numpy(sc["u_rfi"][k]).to(env.device) if inject else None
        env.set_injected_draws(u_rfi=u)
        P = _torque_params(env, sc["u_rfi"][k] if inject else None)
        pre = dict(q=_np(s.dof_pos), v=_np(s.dof_vel), queue=_np(env.action_queue), delay=env.action_delay_idx.cpu().numpy(),
                   ep=env._episode_length_buf.clone(), start=env.motion_start_times.clone(), ids=env.motion_ids.clone())
        a_del = jm.delayed_action(sc["actions"][k], float(env._c.action_clip_value), pre["queue"], pre["delay"], bool(env._c.randomize_ctrl_delay))
        env.step({"actions": torch.from_numpy(sc["actions"][k]).to(env.device)})
        torch.cuda.synchronize()
        froot, bacc = _np(s.replay["root"][0]), _np(s.base_acc)
        base = dict(R0=am.quat_xyzw_to_matrix(froot[:, 3:7]), w0=froot[:, 10:13], alpha0=bacc[:, 3:6], a0g=bacc[:, 0:3] - s.gravity)
        r = dict(P=P, pre=pre, a_del=a_del, base_acc=bacc, reset=env.reset_buf.bool().cpu().numpy(), time_outs=int(env.time_out_buf.sum()),
                 frame_q=_np(s.replay["dof_pos"][0]), frame_v=_np(s.replay["dof_vel"][0]), frame_root=s.replay["root"][0].clone(),
                 frame_contact=s.replay["contact"][0].clone(), dof_pos=_np(s.dof_pos), dof_vel=_np(s.dof_vel), root=s.robot_root_states.clone(),
                 tau0=s.tau0.clone(), torques=env.torques.clone())
        if inject:
            r["model"] = _model_step(m, pre["q"], pre["v"], a_del, P, base)
        out.append(r)
    return env, sc, out


_RUNS = {}


def _case(cfgname, N, general, inject=True, base_acceleration=True):
    key = (cfgname, N, general, inject, base_acceleration)
    if key not in _RUNS:
        _RUNS[key] = _run_case(*key)
    return _RUNS[key]


@pytest.mark.parametrize("cfgname,N,general,bacc", [c + (True,) for c in CASES] + [WALK_CASE + (False,)])
def test_frame_equals_the_model_one_step_at_a_time(cfgname, N, general, bacc):
    """From the kernel's own post-step state of step k - 1 (resets included), the queue peeked before step k, the DR scales and the base of
    the kernel's own root row, the model's (q, v) after the sub-steps is the frame step k consumed, per element within the bound of the
    module docstring.  An (env, step) pair in which the model has a pre-clamp position within 1e-5 rad of a limit is skipped (the velocity
    zeroing is discontinuous there and the coupling spreads it); at most 1 % of the pairs (tests/test_articulated_sim_cpu.py)."""
    env, sc, steps = _case(cfgname, N, general, True, bacc)
    skipped = total = time_outs = clipped = limited = 0
    worst = 0.0
    for k, r in enumerate(steps):
        P, mm = r["P"], r["model"]
        ok = np.broadcast_to((mm["margin"].min(axis=1) >= 1e-5)[:, None], mm["q"].shape)
        skipped += int((~ok[:, 0]).sum()); total += N
        ev, eq = np.abs(r["frame_v"] - mm["v"]), np.abs(r["frame_q"] - mm["q"])
        rv, rq = float((ev / mm["tol_v"])[ok].max()), float((eq / mm["tol_q"])[ok].max())
        worst = max(worst, rv, rq)
        print(f"{cfgname} base_acceleration {bacc} step {k}: worst |dv| / bound {rv:.3f}, worst |dq| / bound {rq:.3f}, skipped envs {int((~ok[:, 0]).sum())}, "
              f"resets {int(r['reset'].sum())}, largest base acceleration {np.abs(r['base_acc']).max():.2f}")
        assert not (ev > mm["tol_v"])[ok].any(), (k, rv, np.argwhere((ev > mm["tol_v"]) & ok)[:5].tolist())
        assert not (eq > mm["tol_q"])[ok].any(), (k, rq, np.argwhere((eq > mm["tol_q"]) & ok)[:5].tolist())
        keep = ~r["reset"]
        assert np.array_equal(r["dof_pos"][keep], r["frame_q"][keep]) and np.array_equal(r["dof_vel"][keep], r["frame_v"][keep])
        time_outs += r["time_outs"]
        tl = P["torque_limit"]
        clipped += int((np.abs(jm.torque_terms(r["pre"]["q"], r["pre"]["v"], r["a_del"], P)[3]) > tl)[:, list(LOWERED)].sum())
        limited += int(((mm["q"] == P["lo"]) | (mm["q"] == P["hi"])).sum())
        if not bacc:
            assert not r["base_acc"].any()
    print(f"{cfgname}: worst residual / bound over the run {worst:.3f}; {skipped} of {total} pairs skipped, {limited} elements on a limit, {clipped} clips")
    assert skipped <= 0.01 * total, (skipped, total)
    assert clipped > 0 and limited > 0, "the torque clip / the joint limits never bound"
    assert sum(int(r["reset"].sum()) for r in steps) < len(steps) * N, "every env reset in every step: nothing was compared"
    if bacc:
        assert max(np.abs(r["base_acc"]).max() for r in steps) > 0.1, "the base never accelerated"
    if cfgname != TEACHER:                                   # (the teacher's nine envs: the scenario's early endings fall on envs that reset first)
        assert time_outs > 0, "no env timed out inside the six steps"


@pytest.mark.parametrize("inject", [True, False])
@pytest.mark.parametrize("cfgname,N,general", CASES)
def test_first_substep_torque_is_the_steps_torque(cfgname, N, general, inject):
    """tau0 of the simulator's launch IS the `torques` the step itself computed, bit for bit (both units are built without contraction and
    evaluate the same expression); with the in-kernel draw (inject False) this holds only if both launches key Philox with the same
    (seed, env, step counter, stream, dof) — here dof = lane - 1."""
    env, sc, steps = _case(cfgname, N, general, inject)
    for k, r in enumerate(steps):
        keep = torch.from_numpy(~r["reset"]).to(r["tau0"].device)
        assert torch.equal(r["tau0"][keep], r["torques"][keep]), (k, float((r["tau0"] - r["torques"])[keep].abs().max()))
        assert float(r["tau0"].abs().max()) > 0
    assert bool(env._c.randomize_torque_rfi) and float(env._c.rfi_lim) > 0


def _front_inputs(env):
    """the live tensors the simulators' kernels read in front of the joint law, and the step's queue shift"""
    s = env.simulator
    return dict(dof_state=s.dof_state, queue=env.action_queue, delay=env.action_delay_idx, kp=env._kp_scale, kd=env._kd_scale, rfi=env._rfi_lim_scale,
                rao=env._rao_scale, ep=env._episode_length_buf, start=env.motion_start_times, ids=env.motion_ids, origins=env.env_origins,
                globals=env.globals)


@pytest.mark.parametrize("inject", [True, False])
def test_the_front_of_the_step_is_the_joint_simulators_bit_for_bit(inject):
    """Everything in front of the joint law — the loads, the draws, the delayed action, the first sub-step's torque, the root row, the contact
    rule — is one piece of device code (csrc/pbhc_closed_loop.h) under two lane mappings: from the same state, queue and scales and the same
    action, ONE step of ArticulatedSim and of JointSpaceSim (same skeleton, any inertias) gives the same tau0, root frame, contact frame and
    action queue, bit for bit.  N = 33: four full groups of 8 envs and a tail workgroup of one.
    reset_all() ends with one zero-action step (base_task.py:83-93), which already runs each simulator's OWN joint law: after it the two
    (q, v) differ, as they must.  So the articulated env's pre-step inputs are copied into the joint-space env, and asserted equal, before
    the step that is compared."""
    N = 33
    sc = scenario(N, 23, 100.0)
    envs = []
    for target in (SIM, "pbhc_amd.simulator.joint_sim.JointSpaceSim"):
        spec = {"inertia": [float(x) for x in sc["inertia"](23)], "damping": DAMP}
        cfg, env = _build(WALK, N, False, extra={"simulator._target_": target, "simulator.config.joint_sim": spec})
        assert type(env.simulator).__name__ == target.rsplit(".", 1)[1] and env.num_dof == 23
        assert float(env._c.action_clip_value) == 100.0
        _prepare(env, sc)
        env.simulator.set_debug_torques(True)
        env.set_injected_draws(u_rfi=torch.from_numpy(sc["u_rfi"][0]).to(env.device) if inject else None)
        envs.append(env)
    art, jnt = (_front_inputs(e) for e in envs)
    print("differ after reset_all:", [k for k in art if not torch.equal(art[k], jnt[k])])
    for k in art:
        jnt[k].copy_(art[k])
    torch.cuda.synchronize()
    pre = [{k: v.clone() for k, v in _front_inputs(e).items()} for e in envs]
    for k in pre[0]:
        assert torch.equal(pre[0][k], pre[1][k]), ("the two simulators do not start from the same state", k)
    assert int(pre[0]["delay"].max()) > 0, "no env has a delayed action"
    out = []
    for env in envs:
        env.step({"actions": torch.from_numpy(sc["actions"][0]).to(env.device)})
        torch.cuda.synchronize()
        s = env.simulator
        out.append(dict(tau0=s.tau0.clone(), root=s.replay["root"][0].clone(), contact=s.replay["contact"][0].clone(), queue=env.action_queue.clone()))
    a, j = out
    for k in a:
        assert torch.equal(a[k], j[k]), (k, float((a[k] - j[k]).abs().max()))
    assert float(a["tau0"].abs().max()) > 0 and float(a["contact"].abs().max()) > 0 and float(a["queue"].abs().max()) > 0


@pytest.mark.parametrize("cfgname,N,general", CASES)
def test_root_contact_and_base_acceleration_of_the_frame(cfgname, N, general):
    """the root the step consumed = the library's root body at (episode_length + 2) dt + start (pre-step values) + env origin; the contact frame
    holds contact_force or 0 on the feet's z and 0 everywhere else (both as JointSpaceSim's).  The base accelerations the kernel used are
    (v(t) - v(t - dt)) / dt of the library's root velocities: the two lookups agree with the library's to 3e-5 (1 + |v|) each (the root
    test's own tolerance), so the quotient to 2 x that / dt."""
    from tests.test_gpu_parity import close

    env, sc, steps = _case(cfgname, N, general)
    feet = env.feet_indices.cpu().tolist()
    cf = env.simulator.contact_force
    on = 0
    for k, r in enumerate(steps):
        pre = r["pre"]
        t = (pre["ep"] + 2).float() * env.dt + pre["start"]
        ref = env._motion_lib.get_motion_state(pre["ids"], t, offset=env.env_origins)
        prev = env._motion_lib.get_motion_state(pre["ids"], t - env.dt, offset=env.env_origins)
        want = torch.cat([ref["root_pos"], ref["root_rot"], ref["root_vel"], ref["root_ang_vel"]], dim=1)
        keep = torch.from_numpy(~r["reset"])
        tol = torch.full((N, 13), 3e-5)
        tol[:, 3:7] = 2e-4
        close(r["root"].cpu()[keep], want.cpu()[keep], tol[keep], f"{cfgname} step {k} root", rtol=3e-5)
        close(r["frame_root"].cpu(), want.cpu(), tol, f"{cfgname} step {k} frame root", rtol=3e-5)
        v1 = np.concatenate([_np(ref["root_vel"]), _np(ref["root_ang_vel"])], 1)
        v0 = np.concatenate([_np(prev["root_vel"]), _np(prev["root_ang_vel"])], 1)
        acc = (v1 - v0) / float(env.dt)
        tol_a = 2 * 3e-5 * (1 + np.maximum(np.abs(v1), np.abs(v0))) / float(env.dt)
        assert (np.abs(r["base_acc"] - acc) <= tol_a).all(), (k, float((np.abs(r["base_acc"] - acc) / tol_a).max()))
        c = r["frame_contact"].cpu()
        z = c[:, feet, 2]
        assert bool(((z == cf) | (z == 0)).all())
        on += int((z == cf).sum())
        rest = c.clone()
        rest[:, feet, 2] = 0
        assert float(rest.abs().max()) == 0.0
        if "contact_mask" in ref:
            assert torch.equal(z.bool(), (ref["contact_mask"] > 0.5).cpu())
    assert on > 0, "no foot was ever in contact"


def test_the_loop_is_closed():
    """20 steps at N = 64, DR and noise off: with a* = (q_ref(next) - q_default) / action_scale the final mean |dif_joint_angles| is smaller
    than with zero actions, on the model (stepped alongside from the kernel's base) and on the kernel, and the two agree on both figures
    to 1 % (they run the same law for 80 sub-steps).  Figures: DESIGN.md §8."""
    N, T = 64, 20
    res = {}
    for policy in ("track", "zero"):
        cfg, env = _build(WALK, N, False, dr=False)
        env.reset_all()
        s, D = env.simulator, env.num_dof
        s.set_debug_base(True)
        env.motion_start_times.zero_()
        env._episode_length_buf.zero_()
        torch.cuda.synchronize()
        m = am.model(env.skeleton, ARM, DAMP)
        P = _torque_params(env)
        qm, vm = _np(s.dof_pos), _np(s.dof_vel)
        scale = torch.tensor(P["action_scale"], dtype=torch.float32, device=env.device)
        qdef = torch.tensor(P["default"], dtype=torch.float32, device=env.device)
        resets = 0
        for k in range(T):
            t = (env._episode_length_buf + 2).float() * env.dt + env.motion_start_times
            qref = env._motion_lib.get_motion_state(env.motion_ids, t, offset=env.env_origins)["dof_pos"]
            a = ((qref - qdef) / scale).contiguous() if policy == "track" else torch.zeros(N, D, device=env.device)
            env.step({"actions": a})
            torch.cuda.synchronize()
            froot, bacc = _np(s.replay["root"][0]), _np(s.base_acc)
            base = dict(R0=am.quat_xyzw_to_matrix(froot[:, 3:7]), w0=froot[:, 10:13], alpha0=bacc[:, 3:6], a0g=bacc[:, 0:3] - s.gravity)
            a_del = jm.delayed_action(_np(a), float(env._c.action_clip_value), None, None, False)
            r = am.substeps(m, qm, vm, lambda q_, v_: jm.torque(q_, v_, a_del, P), base, P["h"], P["decimation"], P["lo"], P["hi"])
            qm, vm = r["q"], r["v"]
            resets += int(env.reset_buf.sum())
        assert resets == 0, "an env reset inside the 20 steps: the model does not follow resets"
        res[policy] = (float(np.linalg.norm(_np(qref) - qm, axis=1).mean()), float((qref - s.dof_pos).norm(dim=1).mean()))
    print(f"closed loop, final mean |dif_joint_angles|: track model {res['track'][0]:.5f} kernel {res['track'][1]:.5f}; "
          f"zero actions model {res['zero'][0]:.5f} kernel {res['zero'][1]:.5f}")
    assert res["track"][0] < res["zero"][0], ("the float64 model does not show the ordering", res)
    assert res["track"][1] < res["zero"][1], res
    for policy in res:
        assert abs(res[policy][0] - res[policy][1]) < 0.01 * res[policy][0], res


def _rollouts(rollout_graph, rollouts=3):
    """MHPPO at 64 envs, 8 steps per rollout, `_training_step` after every rollout; as tests/test_gpu_joint_sim.py _rollouts"""
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
                   frame_q=env.simulator.replay["dof_pos"].clone(), actions=algo.storage.actions.clone(), rewards=algo.storage.rewards.clone())
        return out, used, start
    finally:
        for k in flags:
            os.environ.pop(k, None)


def test_captured_rollout_equals_the_eager_loop():
    """the simulator's launch inside the rollout hipGraph: weights, Adam moments and dof_state bit-identical to the step-by-step loop (the
    child -> parent sums run in a fixed order)"""
    a, used_a, start = _rollouts(True)
    b, used_b, _ = _rollouts(False)
    assert used_a == [False, True, True] and not any(used_b)
    assert not torch.equal(a["_pflat"], start)
    assert bool(torch.isfinite(a["dof_state"]).all())
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_resume_is_bit_identical():
    """six env steps in one run; in a second run three steps, state_dict(), a fresh env, load_state_dict(), three more"""
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
    assert int(env_a._episode_length_buf.min()) < 6, "no env reset inside the six steps"
