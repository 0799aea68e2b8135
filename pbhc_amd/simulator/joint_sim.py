"""JointSpaceSim — a closed-loop simulator behind the ReplaySimStub surface.

Select it with `simulator._target_: pbhc_amd.simulator.joint_sim.JointSpaceSim`.  Where the replay stub plays back a recorded window of
`(root, q, q-dot, contact)` frames that no action can move, this class WRITES the frame every control step from the state the previous step
left and the action the policy just chose (csrc/pbhc_joint_sim.hip, `k_joint_sim`, one launch in front of the fused step):

  * the robot hangs on a gantry: the root is carried along the clip's own root trajectory at the env's current reference time;
  * every joint obeys  I_d q'' = tau_d - b_d q'  under the env's own PD law, integrated over the `control_decimation` physics sub-steps
    with the torque recomputed in every sub-step (the reference's _physics_step, legged_robot_base.py:287-295,795-838);
  * a foot is in contact when the clip says so (its contact mask, or its reference height below `foot_height_threshold`).

It is NOT a physics engine: no gravity, no coupling between joints, no contact dynamics.  What it gives is the loop — PPO, the curricula,
failure-weighted sampling, evaluate_library() and exact resume act on a state that depends on the policy.

Config, under `simulator.config.joint_sim` (all optional):
    inertia: "subtree" | scalar | list of D     kg m^2 per joint; "subtree" (the default) derives it from the MJCF's link masses
    armature: 0.0                               scalar | list of D, added to the inertia
    damping: 0.0                                scalar | list of D, passive joint damping N m s / rad (taken implicitly)
    contact_force: 300.0                        N on z of a foot in contact
    foot_height_threshold: 0.06                 m, for libraries without contact masks
    enforce_limits: true                        clamp q to the hard joint limits, zero an outward velocity
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .closed_loop import ClosedLoopSim, _per_dof  # noqa: F401  (_per_dof: re-exported)

KEY = "simulator.config.joint_sim"


def _quat_rotate_xyzw(q, v):
    """rotate v [..., 3] by the unit quaternion q [..., 4] (xyzw), float64"""
    u, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def subtree_inertia(skeleton, body_pos, body_rot_xyzw, armature=0.0):
    """`inertia: "subtree"`: what joint d would have to turn if every joint below it were locked, with every link's mass taken as a POINT
    at the link's origin (not at its centre of mass, and without the link's own inertia tensor):

        I_d = armature_d + sum over the bodies c of the subtree of body d + 1 of  m_c |a_d x (p_c - p_joint)|^2

    a_d: joint d's axis in the world, p_joint: the origin of the body it drives, p_c: the origin of link c — all at the pose
    `body_pos [B,3]`, `body_rot_xyzw [B,4]` (the rigid-body state of the default joint angles).  Host-side, float64.  Needs the link masses
    (`Skeleton.body_mass`, only an MJCF holds them): refused by name without them."""
    if getattr(skeleton, "body_mass", None) is None:
        raise _lib.PbhcError(f'{KEY}.inertia: "subtree" needs the link masses, and the skeleton has none; load it from the robot\'s MJCF '
                             "(Skeleton.from_mjcf, robot.motion.asset.assetFileName = the .xml) or give the inertias as numbers")
    B, D = skeleton.num_bodies, skeleton.num_dof
    pos = np.asarray(body_pos, np.float64).reshape(B, 3)
    rot = np.asarray(body_rot_xyzw, np.float64).reshape(B, 4)
    rot = rot / np.linalg.norm(rot, axis=-1, keepdims=True)
    mass = np.asarray(skeleton.body_mass, np.float64)
    parents = np.asarray(skeleton.parents[:B])
    arm = _per_dof(armature, D, "armature", KEY)
    out = np.zeros(D, np.float64)
    for d in range(D):
        b = d + 1                                            # dof d drives body d + 1
        axis = _quat_rotate_xyzw(rot[b], np.asarray(skeleton.dof_axis[d], np.float64))
        axis = axis / np.linalg.norm(axis)
        total = 0.0
        for c in range(b, B):                                # DFS order: descendants come after their ancestor
            n = c
            while n > b:
                n = int(parents[n])
            if n == b:
                total += mass[c] * float(np.sum(np.cross(axis, pos[c] - pos[b]) ** 2))
        out[d] = arm[d] + total
    return out


def pd_stability_margins(h, kp_gain, kd_gain, inertia):
    """The explicit PD of one sub-step, v' = v + h (-K (q - q*) - Kd v) / I, q' = q + h v': with a = h^2 K / I and b = h Kd / I its update
    matrix has trace 2 - a - b and determinant 1 - b, and the Jury conditions of a stable pair of roots are  b < 2  and  a + 2 b < 4.
    -> (a, b), arrays over the dofs.  (Passive damping, taken implicitly, only widens the stable region: ignored.)"""
    K, Kd, I = (np.asarray(x, np.float64) for x in (kp_gain, kd_gain, inertia))
    return h * h * K / I, h * Kd / I


def check_pd_stability(h, kp_gain, kd_gain, inertia, names=None):
    """refuse, by name, the first dof whose explicit PD is unstable at sub-step h (gains at the top of their DR ranges)"""
    a, b = pd_stability_margins(h, kp_gain, kd_gain, inertia)
    for d in range(len(a)):
        if b[d] >= 2.0 or a[d] + 2.0 * b[d] >= 4.0:
            who = names[d] if names is not None else f"dof {d}"
            raise _lib.PbhcError(f"{KEY}: the explicit PD of {who} is unstable at the physics sub-step h = {h:g} s: a = h^2 kp Kp / I = {a[d]:.4g}, "
                                 f"b = h kd Kd / I = {b[d]:.4g}; stable needs b < 2 and a + 2 b < 4 (raise the inertia / armature, lower the gains "
                                 "or raise simulator.config.sim.fps)")


class JointSpaceSim(ClosedLoopSim):
    KEY = KEY
    STEP = "pbhc_joint_sim_step"

    def __init__(self, config, device):
        js = config.simulator.config.get("joint_sim", None) or {}
        D = len(config.robot.dof_names)
        self._refuse_velocity_control(config)
        self._inertia_spec = js.get("inertia", "subtree")
        if isinstance(self._inertia_spec, str):
            if self._inertia_spec != "subtree":
                raise _lib.PbhcError(f'{KEY}.inertia: expected a number, a list of {D} numbers or "subtree", got {self._inertia_spec!r}')
        else:
            self._inertia_spec = _per_dof(self._inertia_spec, D, "inertia", KEY)
        self._parse_passive(js, D)
        self._parse_options(js)
        if not isinstance(self._inertia_spec, str):
            self.inertia = self._checked_inertia(self._inertia_spec + self._armature, list(config.robot.dof_names))
            self._check_stability(config, self.inertia)
        else:
            self.inertia = None                              # needs the rigid-body state of the default pose: bind()
        super().__init__(config, device)

    # ---- construction-time checks (no GPU) -----------------------------------------------------------------------------------------
    @staticmethod
    def _checked_inertia(inertia, names):
        for d, v in enumerate(inertia):
            if not (np.isfinite(v) and v > 0.0):
                raise _lib.PbhcError(f"{KEY}.inertia: the inertia of {names[d]} (armature included) is {v:g}; it must be > 0")
        return np.asarray(inertia, np.float64)

    @classmethod
    def _check_stability(cls, config, inertia):
        if config.robot.control.control_type != "P":
            return                                           # "T": the scaled action is the torque, no feedback gain
        K, Kd = cls._top_gains(config)
        check_pd_stability(1.0 / config.simulator.config.sim.fps, K, Kd, inertia, list(config.robot.dof_names))

    def load_assets(self):
        out = super().load_assets()
        if self.inertia is None and self.skeleton.body_mass is None:
            subtree_inertia(self.skeleton, None, None)       # refuses by name: no link masses
        return out

    def bind(self, env):
        """called by the env at the end of its construction: the one-frame window, the inertias, the kernel's parameters"""
        N, D, B, dev = self.num_envs, self.num_dof, self.num_bodies, self.device
        if self.inertia is None:                             # "subtree": rigid-body state of ONE env at the default joint angles
            root = torch.zeros(1, 13, device=dev)
            root[0, 6] = 1.0
            q0 = torch.tensor([[float(env._c.default_dof_pos[d]) for d in range(D)]], dtype=torch.float32, device=dev)
            rb = torch.zeros(1, B, 13, device=dev)
            _lib.check(_lib.lib().pbhc_sim_fk(C.byref(self._csk), root.data_ptr(), q0.data_ptr(), torch.zeros_like(q0).data_ptr(), 1, 1,
                                              rb.data_ptr(), _lib.current_stream()), "pbhc_sim_fk")
            rb = rb[0].double().cpu().numpy()
            self.inertia = self._checked_inertia(subtree_inertia(self.skeleton, rb[:, 0:3], rb[:, 3:7], self._armature), self.dof_names)
            self._check_stability(self.config, self.inertia)
        self._bind_window()
        p = _lib.PbhcJointSimParams()
        for d in range(D):
            p.inertia[d], p.damping[d] = float(self.inertia[d]), float(self._damping[d])
        self._fill_common(p)
        self._params = p
