"""The articulated simulator's joint law (include/pbhc_hip.h, PbhcArticulatedParams), restated in numpy.  Test-side only: the product never
imports this file.

The kernel runs the articulated-body algorithm with spatial vectors about the base's origin.  This file is written the other way round, so
that agreement means something:
    M(q)   from body Jacobians:  sum_b  m_b Jv_b^T Jv_b + Jw_b^T (R_b I_b R_b^T) Jw_b     (Jv_b: of the link's centre of mass)
    c      from a Newton-Euler sweep in world coordinates with CLASSICAL accelerations (of each link's origin and centre of mass) that gives
           every link's net force F_b and net moment N_b about its centre of mass at q'' = 0, projected with the same Jacobians:
           c = sum_b Jv_b^T F_b + Jw_b^T N_b
    q''    a dense solve of (M + diag(armature + h b)) q'' = tau - b v - c
Everything is batched over the leading axis N; `dtype` float64 is the model, float32 the restatement that calibrates the GPU tests' bound.

`model(skeleton)` -> dict of the tree's constants; `base` is a dict R0 [N,3,3], w0, alpha0, a0g [N,3] (a0g = a_0 - g).
"""
import numpy as np


def quat_xyzw_to_matrix(q):
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def model(sk, armature=0.0, damping=0.0, gravity=(0.0, 0.0, -9.81)):
    """the tree's constants from a pbhc_amd.skeleton.Skeleton, from its float32 tables (what the kernel is given) held in float64"""
    B, D = sk.num_bodies, sk.num_dof
    ax = np.asarray(sk.dof_axis, np.float32).astype(np.float64)
    ax = ax / np.linalg.norm(ax, axis=1, keepdims=True)
    lq = np.asarray(sk.local_rot_wxyz, np.float32).astype(np.float64)[:B]
    parents = [int(p) for p in sk.parents[:B]]
    anc = []                                                   # anc[b]: the bodies on the path root -> b, b included, root excluded
    for b in range(B):
        path, n = [], b
        while n > 0:
            path.append(n)
            n = parents[n]
        anc.append(path[::-1])
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    per = lambda a: np.full(D, float(a)) if np.ndim(a) == 0 else np.asarray(a, np.float64)
    return dict(B=B, D=D, parents=parents, anc=anc, offset=np.asarray(sk.offsets, np.float32).astype(np.float64)[:B],
                local_rot=quat_xyzw_to_matrix(lq[:, [1, 2, 3, 0]]), axis=ax, mass=f32(sk.body_mass), com=f32(sk.body_com), inertia=f32(sk.body_inertia),
                armature=f32(per(armature)), damping=f32(per(damping)), gravity=np.asarray(gravity, np.float64))


def _rot(axis, angle, dt):
    """Rodrigues: rotation about the unit `axis` [3] by `angle` [N] -> [N,3,3]"""
    a = axis.astype(dt)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dt)
    s, c = np.sin(angle.astype(dt))[:, None, None], np.cos(angle.astype(dt))[:, None, None]
    return (np.eye(3, dtype=dt) + s * K + (1 - c) * (K @ K)).astype(dt)


def kinematics(m, q, R0, dtype=np.float64):
    """-> R [N,B,3,3], p [N,B,3] (relative to the root's origin), a [N,D,3] the joint axes in the world"""
    dt = dtype
    q = np.asarray(q, dt)
    N, B = q.shape[0], m["B"]
    R = np.zeros((N, B, 3, 3), dt)
    p = np.zeros((N, B, 3), dt)
    a = np.zeros((N, m["D"], 3), dt)
    R[:, 0] = np.asarray(R0, dt)
    for b in range(1, B):
        pa = m["parents"][b]
        R[:, b] = R[:, pa] @ m["local_rot"][b].astype(dt) @ _rot(m["axis"][b - 1], q[:, b - 1], dt)
        p[:, b] = p[:, pa] + R[:, pa] @ m["offset"][b].astype(dt)
        a[:, b - 1] = R[:, b] @ m["axis"][b - 1].astype(dt)
    return R, p, a


def _jacobians(m, R, p, a, dt):
    """per body b >= 1: the centre of mass r_b [N,3], Jv_b, Jw_b [N,3,D], the world inertia Iw_b [N,3,3]"""
    N, B, D = R.shape[0], m["B"], m["D"]
    out = []
    for b in range(1, B):
        r = p[:, b] + R[:, b] @ m["com"][b].astype(dt)
        Jv, Jw = np.zeros((N, 3, D), dt), np.zeros((N, 3, D), dt)
        for j in m["anc"][b]:
            Jw[:, :, j - 1] = a[:, j - 1]
            Jv[:, :, j - 1] = np.cross(a[:, j - 1], r - p[:, j])
        Iw = R[:, b] @ m["inertia"][b].astype(dt) @ np.swapaxes(R[:, b], 1, 2)
        out.append((r, Jv, Jw, Iw))
    return out


def dynamics(m, q, v, base, dtype=np.float64, qdd=None):
    """-> dict: M [N,D,D] (no armature), c [N,D] (the inverse dynamics at `qdd`, default 0: Coriolis, centrifugal, gravity, base motion),
    c_abs [N,D] (the same sum with every product's magnitude: what the rounding error of c scales with), T, V [N] (kinetic energy of the joint
    motion alone — meaningful with the base at rest — and gravitational potential energy)"""
    dt = dtype
    q, v = np.asarray(q, dt), np.asarray(v, dt)
    N, B, D = q.shape[0], m["B"], m["D"]
    R, p, a = kinematics(m, q, base["R0"], dt)
    jac = _jacobians(m, R, p, a, dt)
    w = np.zeros((N, B, 3), dt); wd = np.zeros((N, B, 3), dt); pdd = np.zeros((N, B, 3), dt)
    w[:, 0], wd[:, 0], pdd[:, 0] = np.asarray(base["w0"], dt), np.asarray(base["alpha0"], dt), np.asarray(base["a0g"], dt)
    M = np.zeros((N, D, D), dt)
    c = np.zeros((N, D), dt); c_abs = np.zeros((N, D), dt)
    V = np.zeros(N, dt)
    g = m["gravity"].astype(dt)
    for b in range(1, B):
        pa = m["parents"][b]
        aq = a[:, b - 1] * v[:, b - 1:b]
        w[:, b] = w[:, pa] + aq
        wd[:, b] = wd[:, pa] + np.cross(w[:, pa], aq)
        if qdd is not None:
            wd[:, b] = wd[:, b] + a[:, b - 1] * np.asarray(qdd, dt)[:, b - 1:b]
        d = p[:, b] - p[:, pa]
        pdd[:, b] = pdd[:, pa] + np.cross(wd[:, pa], d) + np.cross(w[:, pa], np.cross(w[:, pa], d))
        r, Jv, Jw, Iw = jac[b - 1]
        rc = r - p[:, b]
        mass = dt(m["mass"][b])
        F = mass * (pdd[:, b] + np.cross(wd[:, b], rc) + np.cross(w[:, b], np.cross(w[:, b], rc)))
        Iw_w = np.einsum("nij,nj->ni", Iw, w[:, b])
        Nn = np.einsum("nij,nj->ni", Iw, wd[:, b]) + np.cross(w[:, b], Iw_w)
        c += np.einsum("nid,ni->nd", Jv, F) + np.einsum("nid,ni->nd", Jw, Nn)
        c_abs += np.einsum("nid,ni->nd", np.abs(Jv), np.abs(F)) + np.einsum("nid,ni->nd", np.abs(Jw), np.abs(Nn))
        M += mass * np.einsum("nid,nie->nde", Jv, Jv) + np.einsum("nid,nij,nje->nde", Jw, Iw, Jw)
        V -= mass * (r @ g)
    T = 0.5 * np.einsum("nd,nde,ne->n", v, M, v)
    return dict(M=M, c=c, c_abs=c_abs, T=T, V=V)


def mtilde(m, M, h=0.0):
    """M + diag(armature + h b)"""
    return M + np.diag(m["armature"] + h * m["damping"]).astype(M.dtype)


def forward(m, q, v, tau, base, h=0.0, dtype=np.float64):
    """-> (q'' = dv / h of the definition, the dynamics dict with Mt = M + diag(armature + h b) and rhs added)"""
    dt = dtype
    d = dynamics(m, q, v, base, dt)
    Mt = mtilde(m, d["M"], dt(h)).astype(dt)
    rhs = (np.asarray(tau, dt) - m["damping"].astype(dt) * np.asarray(v, dt) - d["c"]).astype(dt)
    d.update(Mt=Mt, rhs=rhs)
    return np.linalg.solve(Mt, rhs[..., None])[..., 0].astype(dt), d


def qdd_bound_terms(m, qdd, tau, v, d):
    """|Mt^-1| (|Mt| |q''| + |tau| + |b v| + sum |terms of c|)  per element, float64: what the float32 error of q'' scales with"""
    Minv = np.linalg.inv(d["Mt"].astype(np.float64))
    inner = np.einsum("nde,ne->nd", np.abs(d["Mt"]), np.abs(qdd)) + np.abs(tau) + np.abs(m["damping"] * v) + d["c_abs"]
    return np.einsum("nde,ne->nd", np.abs(Minv), inner)


def clamp(q, v, lo, hi):
    below, above = q < lo, q > hi
    qn = np.where(below, lo, np.where(above, hi, q))
    vn = np.where((below & (v < 0)) | (above & (v > 0)), 0.0, v).astype(v.dtype)
    return qn.astype(q.dtype), vn


def substeps(m, q, v, torque_fn, base, h, steps, lo=None, hi=None, dtype=np.float64):
    """`steps` sub-steps of the definition; torque_fn(q, v) -> tau [N,D].  -> dict(q, v, tau0, qdd0, margin = the smallest distance of a
    PRE-clamp position to a hard limit over the sub-steps (inf without limits), err = the accumulated per-element bound terms: for every
    sub-step s the pair (bq_s, bv_s) such that a relative error gamma of each q'' moves v by at most gamma * bv and q by gamma * bq, the
    errors of earlier sub-steps carried through |dq''/d(q, v)| being of second order in h and left out, as tests/test_gpu_joint_sim.py does)"""
    dt = dtype
    q, v = np.array(q, dt), np.array(v, dt)
    margin = np.full(q.shape, np.inf)
    tau0 = qdd0 = None
    bv = np.zeros(q.shape, np.float64)
    bq = np.zeros(q.shape, np.float64)
    vmax = np.abs(v).astype(np.float64)
    for s in range(steps):
        tau = np.asarray(torque_fn(q, v), dt)
        qdd, d = forward(m, q, v, tau, base, h, dt)
        if s == 0:
            tau0, qdd0 = tau, qdd
        terms = qdd_bound_terms(m, qdd.astype(np.float64), tau.astype(np.float64), v.astype(np.float64), d)
        v = (v + dt(h) * qdd).astype(dt)
        q = (q + dt(h) * v).astype(dt)
        bv = bv + h * terms
        bq = bq + h * bv
        vmax = np.maximum(vmax, np.abs(v))
        if lo is not None:
            margin = np.minimum(margin, np.minimum(np.abs(q - lo), np.abs(q - hi)))
            q, v = clamp(q, v, np.asarray(lo, dt), np.asarray(hi, dt))
    return dict(q=q, v=v, tau0=tau0, qdd0=qdd0, margin=margin, bq=bq, bv=bv, vmax=vmax)


def rest_base(N, gravity=(0.0, 0.0, -9.81)):
    z = np.zeros((N, 3))
    return dict(R0=np.broadcast_to(np.eye(3), (N, 3, 3)).copy(), w0=z.copy(), alpha0=z.copy(), a0g=z - np.asarray(gravity, np.float64))
