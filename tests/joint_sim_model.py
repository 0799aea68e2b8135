"""The joint-space simulator's integrator, restated in float64 numpy (csrc/pbhc_joint_sim.hip k_joint_sim; the torque formula is the step's,
legged_robot_base.py:795-838).  Test-side only: the product never imports this file.

Everything is elementwise over [N, D] arrays.  `P` is a dict:
    control_type   0 "P" | 2 "T"
    Kp, Kd, action_scale, torque_limit, lo, hi, inertia, damping      [D]
    default        [D] or [N, D]
    kp, kd, rfi_scale, rao_scale                                      [N, D]   the env's DR scales
    u_rfi          [N, D] uniforms of this control step, or None (RFI off)
    rfi_lim        float
    n_ps           [N, D] normals of parallel_serial_tau (0 on dofs outside the list), or None;  ps_rfi_lim float
    use_rao, clip_torques, enforce_limits                             bool
    h, decimation  sub-step and count
"""
import numpy as np


def delayed_action(actions_in, clip, queue, delay_idx, randomize_ctrl_delay):
    """the action the step applies: clipped, then — with a control delay — the queue entry its delay index names AFTER the step's shift:
    the new action for index 0, else entry idx - 1 of the queue as it stands BEFORE the step.  queue [N, Q, D], delay_idx [N]"""
    a = np.clip(np.asarray(actions_in, np.float64), -clip, clip)
    if not randomize_ctrl_delay:
        return a
    out = a.copy()
    queue = np.asarray(queue, np.float64)
    for n, i in enumerate(np.asarray(delay_idx).astype(int)):
        if i > 0:
            out[n] = queue[n, i - 1]
    return out


def torque_terms(q, v, a_delayed, P):
    """-> (kp term, kd term, noise term (rfi + ps_tau + rao), unclipped sum), float64"""
    f = lambda x: np.asarray(x, np.float64)
    tl = f(P["torque_limit"])
    a_sc = f(a_delayed) * f(P["action_scale"])
    if P["control_type"] == 0:
        t_p = f(P["kp"]) * f(P["Kp"]) * (a_sc + f(P["default"]) - q)
        t_d = -f(P["kd"]) * f(P["Kd"]) * v
    else:
        t_p, t_d = a_sc, np.zeros_like(a_sc)
    noise = np.zeros_like(a_sc)
    if P.get("u_rfi") is not None:
        noise = noise + (f(P["u_rfi"]) * 2.0 - 1.0) * P["rfi_lim"] * f(P["rfi_scale"]) * tl
    if P.get("n_ps") is not None:
        noise = noise + (P["ps_rfi_lim"] * tl) * f(P["n_ps"])
    if P["use_rao"]:
        noise = noise + f(P["rao_scale"]) * tl
    return t_p, t_d, noise, t_p + t_d + noise


def torque(q, v, a_delayed, P):
    tq = torque_terms(q, v, a_delayed, P)[3]
    if P["clip_torques"]:
        tl = np.asarray(P["torque_limit"], np.float64)
        tq = np.clip(tq, -tl, tl)
    return tq


def substeps(q, v, a_delayed, P):
    """`decimation` sub-steps from (q, v) -> dict(q, v, tau0, vmax = max over the sub-steps of |v_s| (the start included),
    margin = the smallest distance of a PRE-clamp position to a hard limit over the sub-steps)"""
    q, v = np.array(q, np.float64), np.array(v, np.float64)
    h, I, b = float(P["h"]), np.asarray(P["inertia"], np.float64), np.asarray(P["damping"], np.float64)
    lo, hi = np.asarray(P["lo"], np.float64), np.asarray(P["hi"], np.float64)
    vmax = np.abs(v)
    margin = np.full(q.shape, np.inf)
    tau0 = None
    for s in range(int(P["decimation"])):
        tq = torque(q, v, a_delayed, P)
        if s == 0:
            tau0 = tq
        v = (v + h * tq / I) / (1.0 + h * b / I)
        q = q + h * v
        vmax = np.maximum(vmax, np.abs(v))
        margin = np.minimum(margin, np.minimum(np.abs(q - lo), np.abs(q - hi)))
        if P["enforce_limits"]:
            below, above = q < lo, q > hi
            q = np.where(below, lo, np.where(above, hi, q))
            v = np.where((below & (v < 0)) | (above & (v > 0)), 0.0, v)
    return dict(q=q, v=v, tau0=tau0, vmax=vmax, margin=margin)
