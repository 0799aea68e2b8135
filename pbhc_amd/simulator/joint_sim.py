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
from .replay_stub import ReplaySimStub

KEY = "simulator.config.joint_sim"


def _per_dof(value, D, name, key=KEY):
    """scalar or list of D -> float64 [D]; a list of another length is refused by name"""
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        return np.full(D, float(value), np.float64)
    try:
        v = [float(x) for x in value]
    except (TypeError, ValueError):
        raise _lib.PbhcError(f"{key}.{name}: expected a number or a list of {D} numbers, got {value!r}") from None
    if len(v) != D:
        raise _lib.PbhcError(f"{key}.{name}: a list must have one entry per dof ({D}), got {len(v)}")
    return np.asarray(v, np.float64)


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
    arm = _per_dof(armature, D, "armature")
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


class JointSpaceSim(ReplaySimStub):
    def __init__(self, config, device):
        js = config.simulator.config.get("joint_sim", None) or {}
        D = len(config.robot.dof_names)
        if config.robot.control.control_type == "V":
            raise _lib.PbhcError(f'{KEY}: robot.control.control_type "V" is not supported (its damping term differences the velocity over '
                                 'control steps, which has no meaning inside a sub-step); use "P" or "T"')
        self._inertia_spec = js.get("inertia", "subtree")
        if isinstance(self._inertia_spec, str):
            if self._inertia_spec != "subtree":
                raise _lib.PbhcError(f'{KEY}.inertia: expected a number, a list of {D} numbers or "subtree", got {self._inertia_spec!r}')
        else:
            self._inertia_spec = _per_dof(self._inertia_spec, D, "inertia")
        self._armature = _per_dof(js.get("armature", 0.0), D, "armature")
        self._damping = _per_dof(js.get("damping", 0.0), D, "damping")
        if (self._armature < 0).any() or (self._damping < 0).any():
            raise _lib.PbhcError(f"{KEY}: armature and damping must not be negative")
        self.contact_force = float(js.get("contact_force", 300.0))
        self.foot_height_threshold = float(js.get("foot_height_threshold", 0.06))
        self.enforce_limits = bool(js.get("enforce_limits", True))
        if not isinstance(self._inertia_spec, str):
            self.inertia = self._checked_inertia(self._inertia_spec + self._armature, list(config.robot.dof_names))
            self._check_stability(config, self.inertia)
        else:
            self.inertia = None                              # needs the rigid-body state of the default pose: bind()
        super().__init__(config, device)
        self._params = None
        self.tau0 = None

    # ---- construction-time checks (no GPU) -----------------------------------------------------------------------------------------
    @staticmethod
    def _checked_inertia(inertia, names):
        for d, v in enumerate(inertia):
            if not (np.isfinite(v) and v > 0.0):
                raise _lib.PbhcError(f"{KEY}.inertia: the inertia of {names[d]} (armature included) is {v:g}; it must be > 0")
        return np.asarray(inertia, np.float64)

    @staticmethod
    def _top_gains(config):
        """per dof: kp Kp and kd Kd at the top of the DR gain ranges (robot.control gains by name, as env_config matches them)"""
        rc, dr = config.robot, config.domain_rand
        ctrl = rc.control
        K, Kd = [], []
        for name in rc.dof_names:
            k = kd = 0.0
            for joint in ctrl.stiffness.keys():
                if joint in name:
                    k, kd = float(ctrl.stiffness[joint]), float(ctrl.damping[joint])
            K.append(k); Kd.append(kd)
        K, Kd = np.asarray(K, np.float64), np.asarray(Kd, np.float64)
        if dr.get("randomize_pd_gain", False):
            K, Kd = K * float(dr.kp_range[1]), Kd * float(dr.kd_range[1])
        pspd = dr.get("parallel_serial_pd", None)
        if pspd is not None and pspd.get("enable", False):
            K, Kd = K * max(1.0, float(pspd.ratio[1])), Kd * max(1.0, float(pspd.ratio[1]))
        return K, Kd

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

    # ---- the window is the simulator's own -------------------------------------------------------------------------------------------
    def set_replay(self, *a, **k):
        raise _lib.PbhcError("JointSpaceSim.set_replay: the simulator writes its own one-frame window every control step; a replay window "
                             "belongs to ReplaySimStub")

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
        p.contact_force, p.foot_height_threshold = self.contact_force, self.foot_height_threshold
        p.enforce_limits, p.decimation = int(self.enforce_limits), int(self.decimation)
        p.tau0 = None
        self._params = p

    def _bind_window(self):
        """the one-frame window the simulator's kernel writes and the step reads"""
        N, B, dev = self.num_envs, self.num_bodies, self.device
        # contact is zeroed ONCE, here: the kernel writes z of the foot bodies and nothing else
        self.replay = dict(root=self.robot_root_states.clone()[None].contiguous(), dof_pos=self.dof_pos.clone()[None].contiguous(),
                           dof_vel=self.dof_vel.clone()[None].contiguous(), contact=torch.zeros(1, N, B, 3, device=dev))
        self.replay_len = 1
        self.frame_cursor.zero_()
        self._host_frame = 0
        self.replay_version += 1

    def set_debug_torques(self, on=True):
        """keep the first sub-step's torque of every control step in `self.tau0 [N, D]` (what the step reports as `torques`)"""
        self.tau0 = torch.zeros(self.num_envs, self.num_dof, device=self.device) if on else None
        self._params.tau0 = self.tau0.data_ptr() if on else None

    def advance(self, env):
        """the frame of the control step about to be launched, on the current (stepping) stream"""
        _lib.check(_lib.lib().pbhc_joint_sim_step(env._env, C.byref(env._io), C.byref(self._params), _lib.current_stream()), "pbhc_joint_sim_step")
