"""ClosedLoopSim — what the closed-loop simulators behind the ReplaySimStub surface share (JointSpaceSim, ArticulatedSim).

Where the replay stub plays back a recorded window that no action can move, a closed-loop simulator WRITES a one-frame window every control
step from the state the previous step left and the action the policy just chose: one launch of its kernel in front of the fused step
(`advance`, the export named by `STEP`; the kernels' shared device code is csrc/pbhc_closed_loop.h).  A subclass sets `KEY` (its config
section, which error texts name) and `STEP`, parses its section in `__init__` with the helpers below — in the order in which its refusals are
to fire — and builds its kernel's parameters in `bind`, which the env calls at the end of its construction.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .replay_stub import ReplaySimStub


def _per_dof(value, D, name, key):
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


class ClosedLoopSim(ReplaySimStub):
    KEY = None                                               # "simulator.config.<section>"
    STEP = None                                              # the export that launches the kernel: (env, io, params, stream)

    def __init__(self, config, device):
        super().__init__(config, device)
        self._params = None
        self.tau0 = None

    # ---- construction-time parsing and checks (no GPU) -------------------------------------------------------------------------------
    @classmethod
    def _refuse_velocity_control(cls, config):
        if config.robot.control.control_type == "V":
            raise _lib.PbhcError(f'{cls.KEY}: robot.control.control_type "V" is not supported (its damping term differences the velocity over '
                                 'control steps, which has no meaning inside a sub-step); use "P" or "T"')

    def _parse_passive(self, cfg, D):
        self._armature = _per_dof(cfg.get("armature", 0.0), D, "armature", self.KEY)
        self._damping = _per_dof(cfg.get("damping", 0.0), D, "damping", self.KEY)
        if (self._armature < 0).any() or (self._damping < 0).any():
            raise _lib.PbhcError(f"{self.KEY}: armature and damping must not be negative")

    def _parse_options(self, cfg):
        self.contact_force = float(cfg.get("contact_force", 300.0))
        self.foot_height_threshold = float(cfg.get("foot_height_threshold", 0.06))
        self.enforce_limits = bool(cfg.get("enforce_limits", True))

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

    # ---- the window is the simulator's own -------------------------------------------------------------------------------------------
    def set_replay(self, *a, **k):
        raise _lib.PbhcError(f"{type(self).__name__}.set_replay: the simulator writes its own one-frame window every control step; a replay window "
                             "belongs to ReplaySimStub")

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

    def _fill_common(self, p):
        """the fields every closed-loop kernel's parameters have"""
        p.contact_force, p.foot_height_threshold = self.contact_force, self.foot_height_threshold
        p.enforce_limits, p.decimation = int(self.enforce_limits), int(self.decimation)
        p.tau0 = None

    def set_debug_torques(self, on=True):
        """keep the first sub-step's torque of every control step in `self.tau0 [N, D]` (what the step reports as `torques`)"""
        self.tau0 = torch.zeros(self.num_envs, self.num_dof, device=self.device) if on else None
        self._params.tau0 = self.tau0.data_ptr() if on else None

    def advance(self, env):
        """the frame of the control step about to be launched, on the current (stepping) stream"""
        _lib.check(getattr(_lib.lib(), self.STEP)(env._env, C.byref(env._io), C.byref(self._params), _lib.current_stream()), self.STEP)
