"""FloatingBaseSim — a free root and ground contact behind the simulator surface.

Select it with `simulator._target_: pbhc_amd.simulator.floating_sim.FloatingBaseSim`.  It has ArticulatedSim's surface and place in the step
(one launch per control step in front of the fused step, writing the one-frame window; csrc/pbhc_floating_sim.hip, `k_floating_sim`), its
kinematics, link inertias, torque law, delayed-action peek, draws, `tau0` and limits clamp.  What differs: the root is six more degrees of
freedom of the same tree (the root link's own mass and inertia count) and the ground pushes back at contact points fixed to the links.  The
state is `robot_root_states` and `dof_state`, both what the previous step left, resets included.  Every physics sub-step of h = 1 / sim.fps:

    tau from the current (q, v);
    per contact point k (r_k in the frame of body b_k, world height z_k, world velocity xd_k), from the state at the start of the sub-step:
        delta = ground_height - z_k;   delta > 0:  f_n = max(0, stiffness delta - normal_damping xd_z),
        f_t = -friction f_n xd_t / max(|xd_t|, slip_velocity)   (Coulomb, linear below the slip velocity);   else no force
    H(q) [a_0; alpha_0; q''] = [0; 0; tau - b v] - C(q, v, w_0) + sum_k J_k^T f_k + H [g; 0; 0]      (diag(armature + h b) on the joint block)
    v_0 += h a_0;  w_0 += h alpha_0;  v += h q'';  p_0 += h v_0;  R_0 <- exp(h w_0) R_0;  q += h v;  the joint clamp

The frame holds the integrated root and joints and, for every body that owns contact points, all three components of the sum of its
points' forces at the last sub-step.  The clip's root, its contact mask and a `contact_force` are NOT read: the env's terminations
(terminate_by_gravity, terminate_when_motion_far, low height) fire because the robot fell.

What it still is NOT: a physics engine.  Contact is a penalty spring on a plane at a handful of points (no constraint solver, no terrain, no
self-collision), friction is regularised below the slip velocity (a standing robot creeps) and the integrator is explicit.

Domain randomisation is opt-in (`domain_rand` below; every flag false: the code and arithmetic of a simulator without it).  A flag that is on
makes the simulator honour the matching switch of the env's `domain_rand` section, from the tensors the stub surface already draws, saves
and shows to the critic — what the critic observes is what the kernel integrates, and no new host draw is made for them:
    link_mass  (randomize_link_mass)   the mass of body randomize_link_body_names[i] in env n is its nominal mass x _link_mass_scale[n, i];
                                       the inertia tensor about the centre of mass is left as it is, as the reference leaves it
    base_com   (randomize_base_com)    the centre of mass of torso_link (pelvis on a skeleton without it; the root link on one with
                                       neither name, where the reference would fail) += _base_com_bias[n], body frame
    friction   (randomize_friction)    env n uses friction_coeffs[n] in place of `friction`
    push       (push_robots)           every push_interval_s (whole seconds, redrawn per push from {lo .. hi - 1}) the root's world linear
                                       velocity x, y gets += U(-max_push_vel_xy, max_push_vel_xy) (with _push_fixed; = without), in the
                                       kernel, in front of the first sub-step of the control step after the one whose end the reference
                                       writes it at; an env the previous step reset renews its interval but is not pushed.  State:
                                       push_counter, push_interval, push_vel (in the state dict), draws from Philox stream 22 or
                                       `set_injected_push`; the initial intervals are drawn in create_envs after the stub's own draws
A flag whose switch is off gives identity tables.  The tables are built at `bind` and by `refresh_tables()` (after the tensors were written
in place; `load_state_dict` calls it).  Still NOT randomised: the inertia tensors (randomize_link_inertia), an added base mass
(randomize_base_mass), per-link centres of mass (randomize_link_com) and heavy_upper stay ignored; a push is a step in velocity, not a force.

Config, under `simulator.config.floating_sim` (any other key is refused by name):
    armature: 0.0                               scalar | list of D, kg m^2 added to the diagonal of the joint block
    damping: 0.0                                scalar | list of D, passive joint damping N m s / rad (taken implicitly)
    gravity: [0, 0, -9.81]                      m / s^2, world
    enforce_limits: true                        clamp q to the hard joint limits, zero an outward velocity
    contact_points: {body name: [[x, y, z], ...]}     REQUIRED; body frame, m; at most 4 per body; any real body may carry points
    stiffness: 10000.0                          N / m per point
    normal_damping: 100.0                       N s / m per point
    friction: 0.8
    slip_velocity: 0.4                          m / s (the G1 at 200 Hz needs about 0.3: see the screen)
    ground_height: 0.0                          m, world z of the plane
    domain_rand: {link_mass: false, base_com: false, friction: false, push: false}      see above; any other sub-key is refused by name
It needs the link masses and inertia tensors, which only the robot's MJCF holds: robot.motion.asset.assetFileName = the .xml.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .. import dist as pdist
from ..skeleton import Skeleton
from .articulated_sim import _matrix_wxyz, _skew, pd_stability_margins
from .closed_loop import ClosedLoopSim, _per_dof

KEY = "simulator.config.floating_sim"
KEYS = ("armature", "damping", "gravity", "enforce_limits", "contact_points", "stiffness", "normal_damping", "friction", "slip_velocity",
        "ground_height", "domain_rand")
DR_KEYS = ("link_mass", "base_com", "friction", "push")
MAX_BODIES = _lib.K["PBHC_ART_MAX_BODIES"]
MAX_POINTS = _lib.K["PBHC_FLOAT_MAX_POINTS"]


def _tree_kinematics(skeleton, q, R0):
    """-> R [B] rotation matrices, p [B] link origins relative to the root's origin (world axes), a [B] world joint axes (a[0] unused)"""
    B = skeleton.num_bodies
    parents = [int(x) for x in skeleton.parents[:B]]
    R, p, a = [np.asarray(R0, np.float64)] + [None] * (B - 1), [np.zeros(3)] + [None] * (B - 1), [None] * B
    for b in range(1, B):
        ax = np.asarray(skeleton.dof_axis[b - 1], np.float64)
        ax = ax / np.linalg.norm(ax)
        K = _skew(ax)
        rot = np.eye(3) + np.sin(q[b - 1]) * K + (1.0 - np.cos(q[b - 1])) * (K @ K)
        R[b] = R[parents[b]] @ _matrix_wxyz(skeleton.local_rot_wxyz[b]) @ rot
        p[b] = p[parents[b]] + R[parents[b]] @ np.asarray(skeleton.offsets[b], np.float64)
        a[b] = R[b] @ ax
    return parents, R, p, a


def _support(parents, b):
    """the joints (bodies >= 1) on the path root -> b"""
    out = []
    while b > 0:
        out.append(b)
        b = parents[b]
    return out


def floating_inertia(skeleton, q, R0=None, mass=None):
    """H(q) [(6+D),(6+D)] of the free-floating tree, host-side float64, generalised velocities [v_0 (world, of the root's origin); w_0 (world);
    qd]: every link's 6 x 6 spatial inertia about the root's origin in world axes, and  H = sum_b S_b^T I_b S_b  with S_b the motion subspace
    of the coordinates that move link b — the root's six, [0; e_i] and [e_i; 0], and S_d = [a_d; p_d x a_d] of the joints on its path.
    `mass` [B]: in place of the skeleton's link masses (the stability screen's corner)."""
    B, D = skeleton.num_bodies, skeleton.num_dof
    q = np.asarray(q, np.float64).reshape(D)
    parents, R, p, a = _tree_kinematics(skeleton, q, np.eye(3) if R0 is None else R0)
    S = np.zeros((6, 6 + D))                                 # rows [angular; linear of the point at the root's origin]
    S[3:, 0:3] = np.eye(3)
    S[:3, 3:6] = np.eye(3)
    for b in range(1, B):
        S[:, 5 + b] = np.concatenate([a[b], np.cross(p[b], a[b])])
    H = np.zeros((6 + D, 6 + D))
    for b in range(B):
        m = float(skeleton.body_mass[b] if mass is None else mass[b])
        cx = _skew(p[b] + R[b] @ np.asarray(skeleton.body_com[b], np.float64))
        I = np.zeros((6, 6))
        I[:3, :3] = R[b] @ np.asarray(skeleton.body_inertia[b], np.float64) @ R[b].T + m * (cx @ cx.T)
        I[:3, 3:] = m * cx
        I[3:, :3] = m * cx.T
        I[3:, 3:] = m * np.eye(3)
        cols = list(range(6)) + [5 + j for j in _support(parents, b)]
        Sb = S[:, cols]
        H[np.ix_(cols, cols)] += Sb.T @ I @ Sb
    return H


def point_jacobians(skeleton, q, R0, points):
    """`points`: list of (body index, r [3] in the body's frame).  -> x [K,3] the points relative to the root's origin (world axes) and
    J [K,3,6+D] with xd_k = J_k [v_0; w_0; qd]"""
    D = skeleton.num_dof
    q = np.asarray(q, np.float64).reshape(D)
    parents, R, p, a = _tree_kinematics(skeleton, q, R0)
    x = np.zeros((len(points), 3))
    J = np.zeros((len(points), 3, 6 + D))
    for k, (b, r) in enumerate(points):
        x[k] = p[b] + R[b] @ np.asarray(r, np.float64)
        J[k, :, 0:3] = np.eye(3)
        J[k, :, 3:6] = -_skew(x[k])
        for j in _support(parents, b):
            J[k, :, 5 + j] = np.cross(a[j], x[k] - p[j])
    return x, J


def contact_stability_margins(h, Ht, Jn, Jt, stiffness, normal_damping, tangential_slope):
    """The explicit penalty contact of one sub-step with every point touching: along an eigenvector the update is the explicit PD's
    (pd_stability_margins), with the normal spring k and damper d of every point acting through the normal rows Jn [K,6+D] of the points'
    Jacobians and the friction's viscous slope per point (below the slip velocity: friction x the point's load / slip_velocity) through the
    tangential rows Jt [2K,6+D].
    -> dict a_n = h^2 lambda_max(Ht^-1 Jn^T k Jn), b_n = h lambda_max(Ht^-1 Jn^T d Jn), b_t = h lambda_max(Ht^-1 Jt^T slope Jt), float64;
    stable needs b < 2 and a + 2 b < 4 for (a_n, b_n) and for (0, b_t).  One pose, every point loaded at once, the three taken apart: a
    SCREEN, not a proof."""
    Li = np.linalg.inv(np.linalg.cholesky(np.asarray(Ht, np.float64)))
    lam = lambda J, c: float(np.linalg.eigvalsh(Li @ (c * (J.T @ J)) @ Li.T).max()) if len(J) else 0.0
    Jn, Jt = np.asarray(Jn, np.float64), np.asarray(Jt, np.float64)
    return dict(a_n=h * h * lam(Jn, stiffness), b_n=h * lam(Jn, normal_damping), b_t=h * lam(Jt, tangential_slope))


def _number(cfg, name, default):
    v = cfg.get(name, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise _lib.PbhcError(f"{KEY}.{name}: expected a number, got {v!r}")
    return float(v)


class FloatingBaseSim(ClosedLoopSim):
    KEY = KEY
    STEP = "pbhc_floating_sim_step"

    def __init__(self, config, device):
        cfg = config.simulator.config.get("floating_sim", None) or {}
        for k in cfg.keys():
            if k not in KEYS:
                raise _lib.PbhcError(f"{KEY}.{k}: unknown key (known: {', '.join(KEYS)})")
        self._refuse_velocity_control(config)
        self._parse_passive(cfg, len(config.robot.dof_names))
        try:
            self.gravity = np.asarray([float(x) for x in cfg.get("gravity", [0.0, 0.0, -9.81])], np.float64)
        except (TypeError, ValueError):
            self.gravity = np.zeros(0)
        if self.gravity.shape != (3,):
            raise _lib.PbhcError(f"{KEY}.gravity: expected a list of 3 numbers, got {cfg.get('gravity')!r}")
        self.enforce_limits = bool(cfg.get("enforce_limits", True))
        self.stiffness = _number(cfg, "stiffness", 10000.0)
        self.normal_damping = _number(cfg, "normal_damping", 100.0)
        self.friction = _number(cfg, "friction", 0.8)
        self.slip_velocity = _number(cfg, "slip_velocity", 0.4)
        self.ground_height = _number(cfg, "ground_height", 0.0)
        if self.stiffness < 0 or self.normal_damping < 0 or self.friction < 0:
            raise _lib.PbhcError(f"{KEY}: stiffness, normal_damping and friction must not be negative")
        if not self.slip_velocity > 0:
            raise _lib.PbhcError(f"{KEY}.slip_velocity: must be positive, got {self.slip_velocity!r}")
        skeleton = Skeleton.from_motion_config(config.robot.motion)
        self.points = self.parse_points(cfg.get("contact_points", None), skeleton)
        self.dr = self.parse_domain_rand(cfg.get("domain_rand", None))
        self.margins = self.check_model(config, skeleton, self._armature, self.points, self.stiffness, self.normal_damping, self.friction,
                                        self.slip_velocity, self.gravity, domain_rand=self.dr)
        super().__init__(config, device)
        self.root_acc = None
        self._points_dev = None
        self._inertial_dev = self._friction_dev = self._u_push = None
        self.push_counter = self.push_interval = self.push_vel = None

    # ---- construction-time checks (no GPU) -----------------------------------------------------------------------------------------
    @staticmethod
    def parse_points(spec, skeleton):
        """`contact_points` -> list of (body index, r float64 [3]) in body order, then in the order given; refusals by name"""
        if spec is None or not hasattr(spec, "keys") or len(spec.keys()) == 0:
            raise _lib.PbhcError(f"{KEY}.contact_points: missing or empty; give {{body name: [[x, y, z], ...]}} with at most {MAX_POINTS} points "
                                 "per body (without contact points the robot falls through the ground)")
        names = list(skeleton.body_names)
        per_body = {}
        for name in spec.keys():
            if name not in names:
                raise _lib.PbhcError(f"{KEY}.contact_points.{name}: unknown body (the skeleton's bodies: {', '.join(names)})")
            try:
                pts = np.asarray([[float(x) for x in pt] for pt in spec[name]], np.float64)
            except (TypeError, ValueError):
                pts = np.zeros((0, 0))
            if pts.ndim != 2 or pts.shape[1:] != (3,) or len(pts) == 0:
                raise _lib.PbhcError(f"{KEY}.contact_points.{name}: expected a non-empty list of [x, y, z] points, got {spec[name]!r}")
            if len(pts) > MAX_POINTS:
                raise _lib.PbhcError(f"{KEY}.contact_points.{name}: {len(pts)} points; a body carries at most {MAX_POINTS}")
            per_body[names.index(name)] = pts
        return [(b, r) for b in sorted(per_body) for r in per_body[b]]

    @staticmethod
    def parse_domain_rand(spec):
        """`domain_rand` -> {link_mass, base_com, friction, push: bool}, all False by default; an unknown sub-key or a value that is no
        boolean is refused by name"""
        out = dict.fromkeys(DR_KEYS, False)
        if spec is None:
            return out
        if not hasattr(spec, "keys"):
            raise _lib.PbhcError(f"{KEY}.domain_rand: expected a mapping of {', '.join(DR_KEYS)} to booleans, got {spec!r}")
        for k in spec.keys():
            if k not in DR_KEYS:
                raise _lib.PbhcError(f"{KEY}.domain_rand.{k}: unknown key (known: {', '.join(DR_KEYS)})")
            if not isinstance(spec[k], bool):
                raise _lib.PbhcError(f"{KEY}.domain_rand.{k}: expected true or false, got {spec[k]!r}")
            out[k] = spec[k]
        return out

    @staticmethod
    def _named_bodies(skeleton, link_names):
        names = list(skeleton.body_names)
        for name in link_names:
            if name not in names:
                raise _lib.PbhcError(f"domain_rand.randomize_link_body_names: '{name}' is no body of the skeleton ({', '.join(names)})")
        return [names.index(name) for name in link_names]

    @staticmethod
    def inertial_table(skeleton, link_names, mass_scale=None, base_com_bias=None):
        """The per-env rows the kernel reads in place of the params' mass and centre of mass (PbhcFloatingParams.env_inertial), GPU-free.
        link_names: domain_rand.randomize_link_body_names; mass_scale [N, len(link_names)] (None: 1) and base_com_bias [N, 3] (None: 0),
        numpy or CPU torch.  -> float32 numpy [N, PBHC_ART_MAX_BODIES, 4]: row (n, b) = (mass, com_x, com_y, com_z), in float32 arithmetic
        nominal mass x scale for the named bodies, nominal centre of mass + bias on torso_link (the body NAMED pelvis on a skeleton without it; on a skeleton with neither name the
        root link, body 0 — a documented fallback for robots whose root has another name; the reference raises there); every other
        body as the skeleton has it; rows b >= B are 0.  A negative mass and a root mass that is not positive are refused by name."""
        as_np = lambda a: np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, np.float32)
        B = skeleton.num_bodies
        if B > MAX_BODIES:
            raise _lib.PbhcError(f"{KEY}: the robot has {B} bodies; at most {MAX_BODIES}")
        if mass_scale is None and base_com_bias is None:
            raise _lib.PbhcError(f"{KEY}: inertial_table needs mass_scale or base_com_bias (they give the number of envs)")
        idx = FloatingBaseSim._named_bodies(skeleton, link_names)
        N = len(mass_scale) if mass_scale is not None else len(base_com_bias)
        table = np.zeros((N, MAX_BODIES, 4), np.float32)
        table[:, :B, 0] = np.asarray(skeleton.body_mass, np.float32)[:B]
        table[:, :B, 1:] = np.asarray(skeleton.body_com, np.float32)[:B]
        if mass_scale is not None:
            sc = as_np(mass_scale)
            if sc.shape != (N, len(idx)):
                raise _lib.PbhcError(f"{KEY}: mass_scale: expected [{N}, {len(idx)}] (one column per name of randomize_link_body_names), got {list(sc.shape)}")
            for i, b in enumerate(idx):
                table[:, b, 0] *= sc[:, i]
        if base_com_bias is not None:
            bias = as_np(base_com_bias)
            if bias.shape != (N, 3):
                raise _lib.PbhcError(f"{KEY}: base_com_bias: expected [{N}, 3], got {list(bias.shape)}")
            names = list(skeleton.body_names)
            # (a skeleton with neither name: its root link, which is what pelvis is on the robots that have one)
            table[:, names.index("torso_link") if "torso_link" in names else (names.index("pelvis") if "pelvis" in names else 0), 1:] += bias
        if not (table[:, :, 0] >= 0).all():
            n, b = np.argwhere(~(table[:, :, 0] >= 0))[0]
            raise _lib.PbhcError(f"{KEY}.domain_rand.link_mass: the mass of '{skeleton.body_names[b]}' in env {n} is negative ({table[n, b, 0]:g})")
        if not (table[:, 0, 0] > 0).all():
            n = int(np.argwhere(~(table[:, 0, 0] > 0))[0, 0])
            raise _lib.PbhcError(f"{KEY}.domain_rand.link_mass: the root link '{skeleton.body_names[0]}' has no mass in env {n} "
                                 f"({table[n, 0, 0]:g}); a free root needs one")
        return table

    @classmethod
    def check_model(cls, config, skeleton, armature, points, stiffness, normal_damping, friction, slip_velocity, gravity, *, domain_rand=None):
        """`domain_rand` (the section's flags; None: none): with link_mass or friction on and the env's switch on, the screen is taken at the
        worst corner of the ranges it can name cheaply — Ht from the masses at link_mass_range[0] (the lightest robot: the PD's and the normal
        contact's margins, and the friction's), the friction's slope from friction_range[1] x the weight at link_mass_range[1] — and a refusal
        names the corner.  The centre-of-mass bias is left out: one pose, one corner, a SCREEN and not a proof.
        Refuse, by name: a skeleton without masses and inertias, more bodies than the kernel's lanes, a negative link mass or a massless
        root, an Ht = H(q_default) + diag(armature) that is not positive definite, an explicit PD (against the joint block, as ArticulatedSim)
        or an explicit contact (contact_stability_margins, at the default pose, upright, every point on the ground) that its stability screen
        does not pass.  -> the margins (dict)"""
        if skeleton.body_mass is None or skeleton.body_inertia is None:
            raise _lib.PbhcError(f"{KEY}: the skeleton has no link masses and inertia tensors; load it from the robot's MJCF "
                                 "(Skeleton.from_mjcf, robot.motion.asset.assetFileName = the .xml)")
        if skeleton.num_bodies > MAX_BODIES:
            raise _lib.PbhcError(f"{KEY}: the robot has {skeleton.num_bodies} bodies; the kernel holds one body per lane of a 32-lane group "
                                 f"(at most {MAX_BODIES})")
        mass = np.asarray(skeleton.body_mass, np.float64)
        if (mass < 0).any():
            raise _lib.PbhcError(f"{KEY}: a link mass is negative")
        if not mass[0] > 0:
            raise _lib.PbhcError(f"{KEY}: the root link '{skeleton.body_names[0]}' has no mass; a free root needs one")
        rc = config.robot
        D = skeleton.num_dof
        flags, dr = domain_rand or {}, config.domain_rand
        mass_lo, mass_hi, at_lo, at_hi = mass, mass, "", ""
        if flags.get("link_mass", False) and dr.get("randomize_link_mass", False):
            idx = sorted(set(cls._named_bodies(skeleton, list(dr.get("randomize_link_body_names", [])))))
            lo, hi = float(dr.link_mass_range[0]), float(dr.link_mass_range[1])
            mass_lo, mass_hi = mass.copy(), mass.copy()
            mass_lo[idx] *= lo
            mass_hi[idx] *= hi
            if (mass_lo < 0).any() or not mass_lo[0] > 0:
                raise _lib.PbhcError(f"{KEY}.domain_rand.link_mass: at domain_rand.link_mass_range[0] = {lo:g} a link mass is negative or the "
                                     f"root link '{skeleton.body_names[0]}' has no mass")
            at_lo, at_hi = f", at domain_rand.link_mass_range[0] = {lo:g}", f" and domain_rand.link_mass_range[1] = {hi:g}"
        if flags.get("friction", False) and dr.get("randomize_friction", False):
            friction = float(dr.friction_range[1])
            if friction < 0 or float(dr.friction_range[0]) < 0:
                raise _lib.PbhcError(f"{KEY}.domain_rand.friction: domain_rand.friction_range {list(dr.friction_range)} has a negative end")
            at_hi = f", at domain_rand.friction_range[1] = {friction:g}" + at_hi + (at_lo.replace(", at", " and") if at_lo else "")
        elif at_lo:
            at_hi = at_lo + at_hi
        q0 = np.asarray([float(rc.init_state.default_joint_angles[n]) for n in rc.dof_names], np.float64)
        Ht = floating_inertia(skeleton, q0, mass=mass_lo) + np.diag(np.concatenate([np.zeros(6), armature]))
        try:
            np.linalg.cholesky(Ht)
        except np.linalg.LinAlgError:
            raise _lib.PbhcError(f"{KEY}: H(q_default) + diag(armature) is not positive definite (smallest eigenvalue "
                                 f"{float(np.linalg.eigvalsh(Ht).min()):.3g}); a massless link needs an armature") from None
        h = 1.0 / config.simulator.config.sim.fps
        out = dict(h=h)
        if rc.control.control_type == "P":
            K, Kd = cls._top_gains(config)
            a, b = pd_stability_margins(h, K, Kd, Ht[6:, 6:])
            out.update(a_pd=a, b_pd=b)
            if b >= 2.0 or a + 2.0 * b >= 4.0:
                raise _lib.PbhcError(f"{KEY}: the explicit PD is unstable at the physics sub-step h = {h:g} s: a = h^2 lambda_max(Mt^-1 K) = {a:.4g}, "
                                     f"b = h lambda_max(Mt^-1 Kd) = {b:.4g}; stable needs b < 2 and a + 2 b < 4{at_lo} (raise the armature, lower the "
                                     "gains or raise simulator.config.sim.fps)")
        _, J = point_jacobians(skeleton, q0, np.eye(3), points)
        weight = float(mass_hi.sum() * np.linalg.norm(gravity))
        # the friction's viscous slope below the slip velocity: friction x (total weight) / slip_velocity in all, every point carrying its
        # share of the weight as the robot stands
        slope = friction * weight / slip_velocity / len(points)
        m = contact_stability_margins(h, Ht, J[:, 2, :], J[:, :2, :].reshape(-1, 6 + D), stiffness, normal_damping, slope)
        out.update(m, weight=weight, tangential_slope=slope, friction=friction)
        if m["b_n"] >= 2.0 or m["a_n"] + 2.0 * m["b_n"] >= 4.0:
            raise _lib.PbhcError(f"{KEY}: the explicit contact is unstable at the physics sub-step h = {h:g} s: a = h^2 lambda_max(H^-1 Jn^T k Jn) = "
                                 f"{m['a_n']:.4g}, b = h lambda_max(H^-1 Jn^T d Jn) = {m['b_n']:.4g}; stable needs b < 2 and a + 2 b < 4{at_lo} (raise "
                                 "simulator.config.sim.fps, lower the stiffness or the normal_damping)")
        if m["b_t"] >= 2.0:
            raise _lib.PbhcError(f"{KEY}: the regularised friction is unstable at the physics sub-step h = {h:g} s: b = h lambda_max(H^-1 Jt^T c Jt) = "
                                 f"{m['b_t']:.4g} with the viscous slope c = friction x weight / slip_velocity / points = {slope:.4g} N s / m per point; stable needs "
                                 f"b < 2{at_hi} (raise simulator.config.sim.fps or the slip_velocity, lower the friction)")
        return out

    # ---- per-env randomisation ----------------------------------------------------------------------------------------------------------
    def _push_on(self):
        return self.dr["push"] and bool(self.env_config.domain_rand.get("push_robots", False))

    def create_envs(self, num_envs, env_origins, base_init_state):
        """the stub's per-env draws, then — only with domain_rand.push on — the first push intervals, from the same host generator"""
        super().create_envs(num_envs, env_origins, base_init_state)
        if not self._push_on():
            return
        dr, dev = self.env_config.domain_rand, self.device
        lo, hi = int(dr.push_interval_s[0]), int(dr.push_interval_s[1])
        if not 0 <= lo < hi:
            raise _lib.PbhcError(f"{KEY}.domain_rand.push: domain_rand.push_interval_s {[lo, hi]}: expected 0 <= lo < hi (whole seconds, hi exclusive)")
        if float(dr.max_push_vel_xy) < 0:
            raise _lib.PbhcError(f"{KEY}.domain_rand.push: domain_rand.max_push_vel_xy must not be negative, got {dr.max_push_vel_xy!r}")
        self.push_interval = torch.randint(lo, hi, (num_envs,), device=dev, generator=pdist.host_generator(dev)).to(torch.int32)
        self.push_counter = torch.zeros(num_envs, dtype=torch.int32, device=dev)
        self.push_vel = torch.zeros(num_envs, 2, device=dev)

    def _state_tensors(self):
        out = super()._state_tensors()
        if self.push_counter is not None:
            out.update(push_counter=self.push_counter, push_interval=self.push_interval, push_vel=self.push_vel)
        return out

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        if self._params is not None:
            self.refresh_tables()

    def refresh_tables(self):
        """rebuild the device tables of link_mass / base_com / friction from `_link_mass_scale`, `_base_com_bias` and `friction_coeffs` as
        they stand now, in place (the kernel's parameters, and a captured graph, keep their addresses).  Refuses by name a mass that is
        negative, a root without mass and a negative friction."""
        dr = self.env_config.domain_rand
        if self._inertial_dev is not None:
            scale = self._link_mass_scale if self.dr["link_mass"] and dr.get("randomize_link_mass", False) else None
            bias = self._base_com_bias if self.dr["base_com"] and dr.get("randomize_base_com", False) else None
            if scale is None and bias is None:
                bias = torch.zeros(self.num_envs, 3)
            names = list(dr.get("randomize_link_body_names", [])) if scale is not None else []
            self._inertial_dev.copy_(torch.from_numpy(self.inertial_table(self.skeleton, names, scale, bias)))
        if self._friction_dev is not None:
            if dr.get("randomize_friction", False):
                fr = self.friction_coeffs.reshape(self.num_envs).to(torch.float32)
                if bool((fr < 0).any()):
                    raise _lib.PbhcError(f"{KEY}.domain_rand.friction: friction_coeffs has a negative entry ({float(fr.min()):g})")
                self._friction_dev.copy_(fr)
            else:
                self._friction_dev.fill_(self.friction)

    def set_injected_push(self, u=None):
        """u [N,3] float32 device tensor: the (interval, x, y) uniforms in [0, 1) of the pushes that fire from now on, read by every step
        until replaced (None: back to the kernel's own draws).  Only with domain_rand.push on."""
        if self.push_counter is None:
            raise _lib.PbhcError(f"{KEY}.domain_rand.push is off (or domain_rand.push_robots is): there is no push to inject draws into")
        self._u_push = None if u is None else _lib.require_gpu_tensor(u, "u_push", torch.float32, (self.num_envs, 3))
        self._params.u_push = _lib.ptr(self._u_push)

    def bind(self, env):
        """called by the env at the end of its construction: the one-frame window, the inertial and point tables, the per-env tables of the
        randomisation that is on, the kernel's parameters"""
        self._bind_window()
        N, dev = self.num_envs, self.device
        if self.dr["link_mass"] or self.dr["base_com"]:
            self._inertial_dev = torch.zeros(N, MAX_BODIES, 4, device=dev)
        if self.dr["friction"]:
            self._friction_dev = torch.zeros(N, device=dev)
        self.refresh_tables()
        self._params, self._points_dev = self.params(self.skeleton, self._armature, self._damping, self.points, self.device, gravity=self.gravity,
                                                     stiffness=self.stiffness, normal_damping=self.normal_damping, friction=self.friction,
                                                     slip_velocity=self.slip_velocity, ground_height=self.ground_height,
                                                     env_inertial=self._inertial_dev, env_friction=self._friction_dev)
        p = self._params
        p.enforce_limits, p.decimation = int(self.enforce_limits), int(self.decimation)
        if self.push_counter is not None:
            dr = self.env_config.domain_rand
            p.push_counter, p.push_interval, p.push_vel = self.push_counter.data_ptr(), self.push_interval.data_ptr(), self.push_vel.data_ptr()
            p.push_lo, p.push_hi = int(dr.push_interval_s[0]), int(dr.push_interval_s[1])
            p.max_push_vel_xy, p.push_fixed = float(dr.max_push_vel_xy), int(bool(dr.get("_push_fixed", False)))

    @staticmethod
    def params(skeleton, armature, damping, points, device, gravity=(0.0, 0.0, -9.81), stiffness=0.0, normal_damping=0.0, friction=0.0,
               slip_velocity=0.1, ground_height=0.0, *, env_inertial=None, env_friction=None):
        """-> (PbhcFloatingParams with the inertial table of `skeleton` and the contact law, the device point table it points to — keep it
        alive as long as the params are used).  `points`: list of (body index, r [3]).  env_inertial: float32 [N, 32, 4] tensor on `device`
        (`inertial_table`, uploaded), env_friction: float32 [N]; the params point to them and the CALLER keeps them alive; None: off."""
        B, D = skeleton.num_bodies, skeleton.num_dof
        if B > MAX_BODIES:
            raise _lib.PbhcError(f"{KEY}: the robot has {B} bodies; at most {MAX_BODIES}")
        p = _lib.PbhcFloatingParams()
        I = np.asarray(skeleton.body_inertia, np.float64)
        for b in range(B):
            p.mass[b] = float(skeleton.body_mass[b])
            for k in range(3):
                p.com[b][k] = float(skeleton.body_com[b][k])
            for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
                p.inertia[b][k] = float(I[b, i, j])
        arm, dmp = _per_dof(armature, D, "armature", KEY), _per_dof(damping, D, "damping", KEY)
        for d in range(D):
            p.armature[d], p.damping[d] = float(arm[d]), float(dmp[d])
        for k in range(3):
            p.gravity[k] = float(gravity[k])
        p.stiffness, p.normal_damping, p.friction = float(stiffness), float(normal_damping), float(friction)
        p.slip_velocity, p.ground_height = float(slip_velocity), float(ground_height)
        table = np.zeros((MAX_BODIES, MAX_POINTS, 3), np.float32)
        count = [0] * MAX_BODIES
        for b, r in points:
            if not 0 <= b < B:
                raise _lib.PbhcError(f"{KEY}: a contact point names body {b}; the robot has {B}")
            if count[b] >= MAX_POINTS:
                raise _lib.PbhcError(f"{KEY}: body {b} carries more than {MAX_POINTS} contact points")
            table[b, count[b]] = np.asarray(r, np.float32)
            count[b] += 1
        for b in range(MAX_BODIES):
            p.num_points[b] = count[b]
        dev_table = torch.from_numpy(table).to(device).contiguous()
        p.points = dev_table.data_ptr()
        p.tau0 = None
        p.root_acc = None
        for name, t, tail in (("env_inertial", env_inertial, (MAX_BODIES, 4)), ("env_friction", env_friction, ())):
            if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape[1:]) == tail
                                      and t.device == dev_table.device):
                raise _lib.PbhcError(f"{KEY}: {name}: expected a contiguous float32 [N{''.join(', ' + str(x) for x in tail)}] tensor on {dev_table.device}")
            setattr(p, name, None if t is None else t.data_ptr())
        return p, dev_table

    def set_debug_root(self, on=True):
        """keep the root's linear and angular acceleration of every control step's last sub-step in `self.root_acc [N, 6]`"""
        self.root_acc = torch.zeros(self.num_envs, 6, device=self.device) if on else None
        self._params.root_acc = self.root_acc.data_ptr() if on else None
