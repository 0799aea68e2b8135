"""The floating-base simulator's law (include/pbhc_hip.h, PbhcFloatingParams), restated in numpy.  Test-side only: the product never imports
this file.

The kernel runs the articulated-body algorithm (spatial vectors about every link's own origin, the root's 6 x 6 solved last).  This file is
written the other way round, so that agreement means something:
    H(q)   (6+D) x (6+D) from body Jacobians that include the six root columns:  sum_b m_b Jv_b^T Jv_b + Jw_b^T (R_b I_b R_b^T) Jw_b
           (Jv_b: of the link's centre of mass; generalised velocities [v_0 world, of the root's origin; w_0 world; qd])
    C      from a Newton-Euler sweep in world coordinates with CLASSICAL accelerations over ALL links, the root included, that gives every
           link's net force F_b and net moment N_b about its centre of mass at zero generalised acceleration, the root's origin
           accelerating at -g, projected with the same Jacobians
    f_k    the points' forces by the contact law, entering as J_k^T f_k
    x''    a dense solve of (H + diag(0_6, armature + h b)) [a_0; alpha_0; q''] = [0; 0; tau - b v] - C + sum_k J_k^T f_k
    step   v_0 += h a_0; w_0 += h alpha_0; v += h q''; p_0 += h v_0; R_0 <- exp(h w_0) R_0 (a quaternion, renormalised); q += h v; clamp
Everything is batched over the leading axis N; `dtype` float64 is the model, float32 the restatement that calibrates the GPU tests' bound.
A state is a dict p0 [N,3], quat [N,4] xyzw, v0, w0 [N,3], q, v [N,D].
"""
import numpy as np

from tests import articulated_model as am


def model(sk, armature=0.0, damping=0.0, gravity=(0.0, 0.0, -9.81), points=(), stiffness=0.0, normal_damping=0.0, friction=0.0,
          slip_velocity=0.1, ground_height=0.0):
    """articulated_model.model plus the contact points (list of (body, r [3])), from their float32 values, and the contact law"""
    m = am.model(sk, armature, damping, gravity)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    m.update(points=[(int(b), f32(r)) for b, r in points], stiffness=float(np.float32(stiffness)), normal_damping=float(np.float32(normal_damping)),
             friction=float(np.float32(friction)), slip_velocity=float(np.float32(slip_velocity)), ground_height=float(np.float32(ground_height)),
             gravity=f32(gravity))
    return m


def quat_to_matrix(q, dt=np.float64):
    q = np.asarray(q, dt)
    q = (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(dt)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one = dt(1)
    return np.stack([np.stack([one - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), one - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), one - 2 * (x * x + y * y)], -1)], -2).astype(dt)


def quat_mul(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def quat_exp(rotvec, dt=np.float64):
    """the unit quaternion of the rotation vector [N,3]"""
    half = (np.asarray(rotvec, dt) * dt(0.5)).astype(dt)
    th = np.linalg.norm(half, axis=-1, keepdims=True).astype(dt)
    sc = np.where(th > 1e-6, np.sin(th) / np.where(th > 1e-6, th, 1), 1).astype(dt)
    return np.concatenate([half * sc, np.cos(th)], -1).astype(dt)


def _skew(r):
    z = np.zeros_like(r[..., 0])
    return np.stack([np.stack([z, -r[..., 2], r[..., 1]], -1), np.stack([r[..., 2], z, -r[..., 0]], -1), np.stack([-r[..., 1], r[..., 0], z], -1)], -2)


def _point_jacobian(m, x, p, a, b, dt):
    """J [N,3,6+D] of the world velocity of the point x [N,3] (relative to the root's origin) fixed to body b"""
    N, D = x.shape[0], m["D"]
    J = np.zeros((N, 3, 6 + D), dt)
    J[:, :, 0:3] = np.eye(3, dtype=dt)
    J[:, :, 3:6] = -_skew(x)
    for j in m["anc"][b]:
        J[:, :, 5 + j] = np.cross(a[:, j - 1], x - p[:, j])
    return J


def dynamics(m, q, v, R0, w0, acc=None, dtype=np.float64):
    """-> dict: H [N,n,n] (no armature), C [N,n] (the inverse dynamics at the generalised acceleration `acc`, default 0, MINUS H acc: Coriolis,
    centrifugal and gravity terms), C_abs (the same sum with every product's magnitude), and of the sweep at `acc` the links' net forces
    F [N,B,3], net moments about their centres of mass Nn [N,B,3] and centres of mass r [N,B,3] relative to the root's origin"""
    dt = dtype
    q, v = np.asarray(q, dt), np.asarray(v, dt)
    N, B, D = q.shape[0], m["B"], m["D"]
    n = 6 + D
    R, p, a = am.kinematics(m, q, R0, dt)
    g = m["gravity"].astype(dt)
    acc = np.zeros((N, n), dt) if acc is None else np.asarray(acc, dt)
    w = np.zeros((N, B, 3), dt); wd = np.zeros((N, B, 3), dt); pdd = np.zeros((N, B, 3), dt)
    w[:, 0], wd[:, 0], pdd[:, 0] = np.asarray(w0, dt), acc[:, 3:6], acc[:, 0:3] - g
    H = np.zeros((N, n, n), dt)
    proj = np.zeros((N, n), dt); proj_abs = np.zeros((N, n), dt)
    Fs, Ns, rs = np.zeros((N, B, 3), dt), np.zeros((N, B, 3), dt), np.zeros((N, B, 3), dt)
    for b in range(B):
        if b >= 1:
            pa = m["parents"][b]
            aq = a[:, b - 1] * v[:, b - 1:b]
            w[:, b] = w[:, pa] + aq
            wd[:, b] = wd[:, pa] + np.cross(w[:, pa], aq) + a[:, b - 1] * acc[:, 5 + b:6 + b]
            d = p[:, b] - p[:, pa]
            pdd[:, b] = pdd[:, pa] + np.cross(wd[:, pa], d) + np.cross(w[:, pa], np.cross(w[:, pa], d))
        rc = np.einsum("nij,j->ni", R[:, b], m["com"][b].astype(dt))
        r = p[:, b] + rc
        Jv = _point_jacobian(m, r, p, a, b, dt)
        Jw = np.zeros((N, 3, n), dt)
        Jw[:, :, 3:6] = np.eye(3, dtype=dt)
        for j in m["anc"][b]:
            Jw[:, :, 5 + j] = a[:, j - 1]
        Iw = R[:, b] @ m["inertia"][b].astype(dt) @ np.swapaxes(R[:, b], 1, 2)
        mass = dt(m["mass"][b])
        F = mass * (pdd[:, b] + np.cross(wd[:, b], rc) + np.cross(w[:, b], np.cross(w[:, b], rc)))
        Nn = np.einsum("nij,nj->ni", Iw, wd[:, b]) + np.cross(w[:, b], np.einsum("nij,nj->ni", Iw, w[:, b]))
        proj += np.einsum("nid,ni->nd", Jv, F) + np.einsum("nid,ni->nd", Jw, Nn)
        proj_abs += np.einsum("nid,ni->nd", np.abs(Jv), np.abs(F)) + np.einsum("nid,ni->nd", np.abs(Jw), np.abs(Nn))
        H += mass * np.einsum("nid,nie->nde", Jv, Jv) + np.einsum("nid,nij,nje->nde", Jw, Iw, Jw)
        Fs[:, b], Ns[:, b], rs[:, b] = F, Nn, r
    C = proj - np.einsum("nde,ne->nd", H, acc)
    return dict(H=H, C=C.astype(dt), C_abs=proj_abs, F=Fs, Nn=Ns, r=rs, R=R, p=p, a=a, w=w)


def contact(m, s, kin, dtype=np.float64):
    """the points' forces from the state `s` -> f [N,K,3], J [N,K,3,n], f_abs [N,K,3] (what the float32 error of f scales with: the operands of
    the cancelling sum in delta times the stiffness, the velocity's terms times the damping, and the friction's direction), z [N,K] heights"""
    dt = dtype
    R, p, a = kin["R"], kin["p"], kin["a"]
    N, K, n = R.shape[0], len(m["points"]), 6 + m["D"]
    gv = np.concatenate([np.asarray(s["v0"], dt), np.asarray(s["w0"], dt), np.asarray(s["v"], dt)], 1)
    f, J, f_abs, zs = np.zeros((N, K, 3), dt), np.zeros((N, K, 3, n), dt), np.zeros((N, K, 3)), np.zeros((N, K), dt)
    k_, d_, mu, vs, gh = (dt(m[x]) for x in ("stiffness", "normal_damping", "friction", "slip_velocity", "ground_height"))
    for k, (b, r) in enumerate(m["points"]):
        rw = np.einsum("nij,j->ni", R[:, b], r.astype(dt))
        x = p[:, b] + rw
        J[:, k] = _point_jacobian(m, x, p, a, b, dt)
        xd = np.einsum("nid,nd->ni", J[:, k], gv)
        z = np.asarray(s["p0"], dt)[:, 2] + x[:, 2]
        delta = gh - z
        fn = np.maximum(dt(0), k_ * delta - d_ * xd[:, 2])
        on = delta > 0
        fn = np.where(on, fn, dt(0)).astype(dt)
        vt = np.sqrt(xd[:, 0] ** 2 + xd[:, 1] ** 2)
        sc = (mu * fn / np.maximum(vt, vs)).astype(dt)
        f[:, k] = np.stack([-sc * xd[:, 0], -sc * xd[:, 1], fn], -1)
        zs[:, k] = z
        # magnitudes, float64
        xd_abs = np.einsum("nid,nd->ni", np.abs(J[:, k]), np.abs(gv)).astype(np.float64)
        z_abs = abs(float(gh)) + np.abs(np.asarray(s["p0"], np.float64)[:, 2]) + np.linalg.norm(p[:, b], axis=1) + np.linalg.norm(r)
        for j in m["anc"][b]:
            z_abs = z_abs + np.linalg.norm(m["offset"][j])
        fn_abs = np.where(on, float(k_) * z_abs + float(d_) * xd_abs[:, 2], 0.0)
        ratio = np.minimum(1.0, vt / float(vs)).astype(np.float64)
        dir_abs = np.linalg.norm(xd_abs[:, :2], axis=1) / np.maximum(vt.astype(np.float64), float(vs))
        ft_abs = float(mu) * (fn_abs * ratio + fn.astype(np.float64) * dir_abs)
        f_abs[:, k] = np.stack([ft_abs, ft_abs, fn_abs], -1)
    return f, J, f_abs, zs


def forward(m, s, tau, h=0.0, dtype=np.float64, contact_on=True, tau_abs=None):
    """-> (acc [N,6+D] = [a_0, alpha_0, q''], f [N,K,3], dict with Ht, rhs, terms = |Ht^-1| (|Ht| |acc| + |tau| + |b v| + C_abs + sum |J_k|^T f_abs_k)
    per element in float64: what the float32 error of acc scales with)"""
    dt = dtype
    N, D = np.asarray(s["q"]).shape
    R0 = quat_to_matrix(s["quat"], dt)
    d = dynamics(m, s["q"], s["v"], R0, s["w0"], None, dt)
    Ht = d["H"].copy()
    idx = np.arange(D) + 6
    Ht[:, idx, idx] += (m["armature"] + h * m["damping"]).astype(dt)
    rhs = -d["C"]
    tau, v = np.asarray(tau, dt), np.asarray(s["v"], dt)
    rhs[:, 6:] += tau - m["damping"].astype(dt) * v
    rhs_abs = d["C_abs"].astype(np.float64).copy()
    rhs_abs[:, 6:] += (np.abs(tau) if tau_abs is None else np.asarray(tau_abs, np.float64)) + np.abs(m["damping"] * v)
    f, J, f_abs, z = contact(m, s, d, dt)
    if not contact_on:
        f, f_abs = np.zeros_like(f), np.zeros_like(f_abs)
    rhs = (rhs + np.einsum("nkid,nki->nd", J, f)).astype(dt)
    rhs_abs += np.einsum("nkid,nki->nd", np.abs(J).astype(np.float64), f_abs)
    acc = np.linalg.solve(Ht, rhs[..., None])[..., 0].astype(dt)
    Hi = np.linalg.inv(Ht.astype(np.float64))
    terms = np.einsum("nde,ne->nd", np.abs(Hi), np.einsum("nde,ne->nd", np.abs(Ht).astype(np.float64), np.abs(acc).astype(np.float64)) + rhs_abs)
    d.update(Ht=Ht, rhs=rhs, terms=terms, J=J, f_abs=f_abs, z=z, R0=R0)
    return acc, f, d


def integrate(m, s, acc, h, lo=None, hi=None, dtype=np.float64):
    dt = dtype
    h = dt(h)
    v0 = (np.asarray(s["v0"], dt) + h * acc[:, 0:3]).astype(dt)
    w0 = (np.asarray(s["w0"], dt) + h * acc[:, 3:6]).astype(dt)
    v = (np.asarray(s["v"], dt) + h * acc[:, 6:]).astype(dt)
    p0 = (np.asarray(s["p0"], dt) + h * v0).astype(dt)
    quat = quat_mul(quat_exp(h * w0, dt), np.asarray(s["quat"], dt)).astype(dt)
    quat = (quat / np.linalg.norm(quat, axis=-1, keepdims=True)).astype(dt)
    q = (np.asarray(s["q"], dt) + h * v).astype(dt)
    margin = np.full(q.shape, np.inf)
    if lo is not None:
        margin = np.minimum(np.abs(q - lo), np.abs(q - hi))
        q, v = am.clamp(q, v, np.asarray(lo, dt), np.asarray(hi, dt))
    return dict(p0=p0, quat=quat, v0=v0, w0=w0, q=q, v=v), margin


def state(root13, q, v, dtype=np.float64):
    r = np.asarray(root13, dtype)
    return dict(p0=r[:, 0:3], quat=r[:, 3:7], v0=r[:, 7:10], w0=r[:, 10:13], q=np.asarray(q, dtype), v=np.asarray(v, dtype))


def root13(s):
    return np.concatenate([s["p0"], s["quat"], s["v0"], s["w0"]], 1)


def substeps(m, s, torque_fn, h, steps, lo=None, hi=None, dtype=np.float64, contact_on=True):
    """`steps` sub-steps; torque_fn(q, v) -> tau.  -> dict(s = the final state, tau0, acc0, f0 of the first sub-step, f = the last sub-step's
    forces, margin, zmin [N] = the lowest point height met at the start of any sub-step)"""
    dt = dtype
    s = {k: np.array(x, dt) for k, x in s.items()}
    margin = np.full(s["q"].shape, np.inf)
    out = {}
    zmin = np.full(s["q"].shape[0], np.inf)
    for i in range(steps):
        tau = np.asarray(torque_fn(s["q"], s["v"]), dt)
        acc, f, d = forward(m, s, tau, h, dt, contact_on)
        if i == 0:
            out.update(tau0=tau, acc0=acc, f0=f)
        if d["z"].shape[1]:
            zmin = np.minimum(zmin, d["z"].min(axis=1))
        s, mg = integrate(m, s, acc, h, lo, hi, dt)
        margin = np.minimum(margin, mg)
    out.update(s=s, f=f, margin=margin, zmin=zmin)
    return out


# ---- the carried bound ---------------------------------------------------------------------------------------------------------------------
def _perturbed(s, i, dlt, D):
    """the state moved by dlt along error coordinate i of [p0 3, theta 3 (world rotation vector), v0 3, w0 3, q D, v D]"""
    t = {k: x.copy() for k, x in s.items()}
    if i < 3:
        t["p0"][:, i] += dlt
    elif i < 6:
        rv = np.zeros((s["q"].shape[0], 3)); rv[:, i - 3] = dlt
        t["quat"] = quat_mul(quat_exp(rv), s["quat"])
    elif i < 9:
        t["v0"][:, i - 6] += dlt
    elif i < 12:
        t["w0"][:, i - 9] += dlt
    elif i < 12 + D:
        t["q"][:, i - 12] += dlt
    else:
        t["v"][:, i - 12 - D] += dlt
    return t


def carried_bound(m, s0, torque_fn, h, steps, gamma, eps, contact_on=True, lo=None, hi=None, tau_abs_fn=None, tile_fn=None, dlt=1e-6):
    """the model's trajectory under torque_fn(q, v) and the first-order bound of a float32 run of it, per error coordinate
    e = [p0, theta, v0, w0, q, v]: per sub-step, with A = |d acc / d state| by central differences of the model (the torque law included),
        e_vel += h (gamma terms + A e) + 4 eps |vel|,    e_pos += h e_vel + 4 eps |pos|     (theta: |pos| = 1, a unit quaternion)
    All perturbed states of a sub-step go through the model in ONE batch; torque_fn is then called with (2 n_e + 1) N rows, `tile_fn(k)`
    telling it so beforehand (None: torque_fn broadcasts).  tau_abs_fn(q, v): the magnitudes the torque's own float32 error scales with.
    -> dict(s = final state, E [N, 12 + 2 D], tau0, acc0, f = the last sub-step's forces, margin = the smallest distance of a pre-clamp
    position to a limit, touch = the smallest |delta| of any point at the start of a sub-step, zmin)"""
    s = {k: np.array(x, np.float64) for k, x in s0.items()}
    N, D = s["q"].shape
    n, ne = 6 + D, 12 + 2 * D
    E = np.zeros((N, ne))
    pos_idx = list(range(0, 6)) + list(range(12, 12 + D))
    vel_idx = list(range(6, 12)) + list(range(12 + D, ne))
    skip = (0, 1, 6, 7, 8) if (not contact_on or not m["points"]) else (0, 1)     # x, y (and without contact all of p0, v0) move no acceleration
    live = [i for i in range(ne) if i not in skip and not (i == 2 and (not contact_on or not m["points"]))]
    margin, touch, zmin = np.full((N, D), np.inf), np.full(N, np.inf), np.full(N, np.inf)
    out = {}
    if tile_fn is not None:
        tile_fn(2 * len(live) + 1)
    for step in range(steps):
        parts = [s] + [_perturbed(s, i, sg * dlt, D) for i in live for sg in (1.0, -1.0)]
        big = {k: np.concatenate([t[k] for t in parts], 0) for k in s}
        tau_big = np.asarray(torque_fn(big["q"], big["v"]), np.float64)
        tau_big = np.broadcast_to(tau_big, big["q"].shape) if tau_big.shape != big["q"].shape else tau_big
        ta = None if tau_abs_fn is None else np.asarray(tau_abs_fn(big["q"], big["v"]), np.float64)
        acc_big, f_big, d = forward(m, big, tau_big, h, np.float64, contact_on, tau_abs=ta)
        acc, f, terms = acc_big[:N], f_big[:N], d["terms"][:N]
        A = np.zeros((N, n, ne))
        for j, i in enumerate(live):
            A[:, :, i] = np.abs(acc_big[(1 + 2 * j) * N:(2 + 2 * j) * N] - acc_big[(2 + 2 * j) * N:(3 + 2 * j) * N]) / (2 * dlt)
        if step == 0:
            out.update(tau0=tau_big[:N], acc0=acc, f0=f, terms0=terms, f_abs0=d["f_abs"][:N])
        if d["z"].shape[1]:
            zmin = np.minimum(zmin, d["z"][:N].min(axis=1))
            touch = np.minimum(touch, np.abs(m["ground_height"] - d["z"][:N]).min(axis=1))
        s, mg = integrate(m, s, acc, h, lo, hi)
        margin = np.minimum(margin, mg)
        velmag = np.concatenate([np.abs(s["v0"]), np.abs(s["w0"]), np.abs(s["v"])], 1)
        posmag = np.concatenate([np.abs(s["p0"]), np.ones((N, 3)), np.abs(s["q"])], 1)
        E[:, vel_idx] += h * (gamma * terms + np.einsum("nai,ni->na", A, E)) + 4 * eps * velmag
        E[:, pos_idx] += h * E[:, vel_idx] + 4 * eps * posmag
    out.update(s=s, E=E, f=f, margin=margin, touch=touch, zmin=zmin)
    return out


def state_diff(got, want):
    """got - want per error coordinate [p0, theta, v0, w0, q, v], signed; theta: twice the vector part of got (x) want^-1"""
    conj = want["quat"] * np.array([-1.0, -1.0, -1.0, 1.0])
    dq = quat_mul(got["quat"] / np.linalg.norm(got["quat"], axis=-1, keepdims=True), conj / np.linalg.norm(conj, axis=-1, keepdims=True))
    dq = dq * np.where(dq[:, 3:4] < 0, -1.0, 1.0)
    return np.concatenate([got["p0"] - want["p0"], 2 * dq[:, :3], got["v0"] - want["v0"], got["w0"] - want["w0"], got["q"] - want["q"],
                           got["v"] - want["v"]], 1)


def transported_bound(m, s0, tau, h, steps, gamma, eps, dlt=1e-6):
    """For runs long enough that carrying magnitudes alone turns a stable contact spring's oscillation into exponential growth: the same
    local errors per sub-step (velocities h gamma terms + 4 eps |vel|, positions h times that + 4 eps |pos|), each carried to the end
    through the model's own SIGNED state-transition matrices Phi_s = d state_{s+1} / d state_s (central differences of the whole sub-step
    under the constant torque `tau`, in the error coordinates) and only then taken in magnitude:  E = sum_s |Phi_{T-1} ... Phi_{s+1}| delta_s.
    -> dict(s, E, zmin, touch) as carried_bound's"""
    s = {k: np.array(x, np.float64) for k, x in s0.items()}
    N, D = s["q"].shape
    ne = 12 + 2 * D
    pos_idx = list(range(0, 6)) + list(range(12, 12 + D))
    vel_idx = list(range(6, 12)) + list(range(12 + D, ne))
    tau = np.asarray(tau, np.float64)
    Phis, deltas = [], []
    zmin, touch = np.full(N, np.inf), np.full(N, np.inf)
    for step in range(steps):
        parts = [s] + [_perturbed(s, i, sg * dlt, D) for i in range(ne) for sg in (1.0, -1.0)]
        big = {k: np.concatenate([t[k] for t in parts], 0) for k in s}
        acc_big, f_big, d = forward(m, big, np.tile(tau, (2 * ne + 1, 1)), h)
        nxt, _ = integrate(m, big, acc_big, h)
        cut = lambda j: {k: x[j * N:(j + 1) * N] for k, x in nxt.items()}
        Phi = np.stack([(state_diff(cut(1 + 2 * i), cut(2 + 2 * i))) / (2 * dlt) for i in range(ne)], -1)      # [N, ne(out), ne(in)]
        zmin = np.minimum(zmin, d["z"][:N].min(axis=1))
        touch = np.minimum(touch, np.abs(m["ground_height"] - d["z"][:N]).min(axis=1))
        s = cut(0)
        delta = np.zeros((N, ne))
        velmag = np.concatenate([np.abs(s["v0"]), np.abs(s["w0"]), np.abs(s["v"])], 1)
        posmag = np.concatenate([np.abs(s["p0"]), np.ones((N, 3)), np.abs(s["q"])], 1)
        delta[:, vel_idx] = h * gamma * d["terms"][:N] + 4 * eps * velmag
        delta[:, pos_idx] = h * delta[:, vel_idx] + 4 * eps * posmag
        Phis.append(Phi); deltas.append(delta)
    E = np.zeros((N, ne))
    Psi = np.broadcast_to(np.eye(ne), (N, ne, ne)).copy()
    for step in range(steps - 1, -1, -1):
        E += np.einsum("nij,nj->ni", np.abs(Psi), deltas[step])
        Psi = Psi @ Phis[step]
    return dict(s=s, E=E, zmin=zmin, touch=touch)


def state_error(got, want, D=None):
    return np.abs(state_diff(got, want))


def momentum(m, s):
    """total linear momentum P [N,3] and angular momentum about the world origin L [N,3], and the centre of mass [N,3], float64"""
    R0 = quat_to_matrix(s["quat"])
    R, p, a = am.kinematics(m, s["q"], R0)
    N, B = R.shape[0], m["B"]
    P, L, com, mt = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3)), 0.0
    w, vo = np.zeros((N, B, 3)), np.zeros((N, B, 3))
    w[:, 0], vo[:, 0] = s["w0"], s["v0"]
    for b in range(B):
        if b >= 1:
            pa = m["parents"][b]
            w[:, b] = w[:, pa] + a[:, b - 1] * s["v"][:, b - 1:b]
            vo[:, b] = vo[:, pa] + np.cross(w[:, pa], p[:, b] - p[:, pa])
        rc = np.einsum("nij,j->ni", R[:, b], m["com"][b])
        x = s["p0"] + p[:, b] + rc
        vc = vo[:, b] + np.cross(w[:, b], rc)
        Iw = R[:, b] @ m["inertia"][b] @ np.swapaxes(R[:, b], 1, 2)
        P += m["mass"][b] * vc
        L += m["mass"][b] * np.cross(x, vc) + np.einsum("nij,nj->ni", Iw, w[:, b])
        com += m["mass"][b] * x
        mt += m["mass"][b]
    return P, L, com / mt


# ---- the inputs the CPU calibration and the GPU tests share -----------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def sample_points(sk):
    """contact points for a test skeleton: four under every leaf link whose name says foot or ankle_roll (or, on the hand-written tree, under
    c and f), and single points on the root, an inner link and the other leaves"""
    names = list(sk.body_names)
    parents = [int(p) for p in sk.parents[:len(names)]]
    leaves = [b for b in range(1, len(names)) if b not in parents]
    feet = [b for b in leaves if "ankle_roll" in names[b] or names[b] in ("c", "f")]
    pts = []
    for b in feet:
        pts += [(b, [0.13, 0.03, -0.035]), (b, [0.13, -0.03, -0.035]), (b, [-0.05, 0.03, -0.035]), (b, [-0.05, -0.03, -0.035])]
    pts += [(0, [0.0, 0.0, -0.08]), (0, [0.05, 0.1, 0.02]), (2, [0.02, 0.0, -0.1])]
    pts += [(b, [0.0, 0.01, -0.05]) for b in leaves if b not in feet]
    return sorted(pts, key=lambda t: t[0])


def random_states(m, N, seed, clear=1e-3):
    """float32-representable states for the one-sub-step tests: tilted, spinning roots; every third robot nearly at rest (its points slide
    below the slip velocity); the root's height set so that about a third of the robot's points are under the ground and none is within
    `clear` of it (the law is discontinuous at touch-down when the point moves down).  -> (root13, q, v, tau) float64 arrays"""
    rng = np.random.default_rng(seed)
    D = m["D"]
    q, v, tau = f32(rng.uniform(-0.6, 0.6, (N, D))), f32(2.0 * rng.standard_normal((N, D))), f32(10.0 * rng.standard_normal((N, D)))
    quat = rng.standard_normal((N, 4))
    quat = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    v0, w0 = rng.standard_normal((N, 3)), 1.5 * rng.standard_normal((N, 3))
    slow = np.arange(N) % 3 == 2
    v[slow] = f32(0.01 * v[slow]); v0[slow] *= 0.01; w0[slow] *= 0.01
    quat = f32(quat)
    R, p, a = am.kinematics(m, q, quat_to_matrix(quat))
    p0 = np.concatenate([rng.uniform(-2.0, 2.0, (N, 2)), np.zeros((N, 1))], 1)
    for n in range(N):
        xz = np.sort([p[n, b, 2] + (R[n, b] @ r)[2] for b, r in m["points"]])
        k = max(1, len(xz) // 3)
        for kk in list(range(k, len(xz))) + list(range(k - 1, 0, -1)):     # the first gap wide enough
            if xz[kk] - xz[kk - 1] > 4 * clear:
                break
        else:
            raise AssertionError("no clear gap between the points' heights")
        p0[n, 2] = m["ground_height"] - 0.5 * (xz[kk] + xz[kk - 1])
    root = f32(np.concatenate([p0, quat, v0, w0], 1))
    return root, q, v, tau


# the drop test's law passes the product's own screen on the tree (a_n 0.02, b_n 0.09, b_t 1.1 at 200 Hz); the joints are held by a passive
# damping of 20 N m s / rad, which the kernel takes implicitly
DROP_LAW = dict(stiffness=1500.0, normal_damping=40.0, friction=0.8, slip_velocity=0.4, ground_height=0.0)
DROP_DAMP = 20.0


def drop_points(sk):
    """the drop test's points: the hand-written tree has ONE leg (a - b - c; f is an arm above the base), so it stands on the four corners of
    a level sole under c wide enough to hold the tree's centre of mass, which lies 4 cm behind and 11 cm beside c's origin.  The corners
    are given in world axes at the default pose and turned into c's own frame."""
    m = am.model(sk)
    R, _, _ = am.kinematics(m, np.zeros((1, m["D"])), np.eye(3)[None])
    return [(3, R[0, 3].T @ np.array(w)) for w in ([0.15, 0.1, -0.03], [0.15, -0.3, -0.03], [-0.2, 0.1, -0.03], [-0.2, -0.3, -0.03])]


def drop_inputs(m, N):
    """the tree upright at its default pose q = 0, released with its lowest point 2 mm above the ground, small random tilts and spins.  The
    constant torque (float32) is the one that holds the default pose while the tree STANDS: the statics of the upright tree on its points,
    tau = C_joints - (sum_k J_k^T f_k)_joints with the vertical forces f_k of least norm that carry the weight and its moments."""
    rng = np.random.default_rng(11)
    D = m["D"]
    q = np.zeros((N, D))
    rv = 0.03 * rng.standard_normal((N, 3))
    quat = f32(quat_exp(rv))
    R, p, _ = am.kinematics(m, q, quat_to_matrix(quat))
    low = np.array([min(p[n, b, 2] + (R[n, b] @ r)[2] for b, r in m["points"]) for n in range(N)])
    root = np.concatenate([rng.uniform(-1, 1, (N, 2)), (m["ground_height"] + 0.002 - low)[:, None], quat, 0.05 * rng.standard_normal((N, 3)),
                           0.1 * rng.standard_normal((N, 3))], 1)
    up = state(np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]), q[:1], q[:1])
    d = dynamics(m, up["q"], up["v"], np.eye(3)[None], up["w0"])
    _, J, _, _ = contact(m, up, d)
    Jz = J[0, :, 2, :]                                       # [K, 6 + D]: a unit vertical force on point k
    fz = np.linalg.lstsq(Jz[:, [2, 3, 4]].T, d["C"][0, [2, 3, 4]], rcond=None)[0]
    assert (fz > 0).all(), "the centre of mass is not over the sole"
    tau = f32(np.tile((d["C"][0] - Jz.T @ fz)[6:], (N, 1)))
    return f32(root), q, np.zeros((N, D)), tau
