"""`robot.motion.interpolation`: lead-in / lead-out frames between a default pose and every clip, added at ingestion on the device.

The reference does this offline, one clip and 23 joints at a time (robot_motion_process/motion_interpolation_pkl.py: "so that the processed
motion data all begin and end with the default pose ... useful for deployment").  Here it is a key of the motion config, any joint count,
one launch for the whole library (`pbhc_motion_extend_batch`, csrc/pbhc_motion_extend.hip; semantics and deviations: DESIGN §8).

This module is the host side only: the parsed and validated settings (`Interpolation`) and the `[start:end]` trim.  There is no CPU
implementation of the frames themselves.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib

KEYS = ("start_frames", "end_frames", "clip_start", "clip_end", "knee_modify", "default_pose", "contact")
DEFAULT_HEIGHT = 0.8                       # the script's default pose: 0.8 m, identity rotation
DEFAULT_QUAT_XYZW = (0.0, 0.0, 0.0, 1.0)


def knee_frames_ok(n):
    """The frame counts the reference's lower_dof_interpolation accepts: with h = n // 2 moving frames per leg and k = h // 2, its knee
    ramps of k and k + 1 samples must fill the h frames (30, 6, 7 do; 60, 4 do not).  0 = nothing at that end."""
    return n == 0 or 2 * ((n // 2) // 2) + 1 == n // 2


@dataclass
class Interpolation:
    """Validated settings.  default_pose: 7 + D floats (translation, xyzw quaternion, joints in dof order); dof_names: the skeleton's dof
    names in order (needed for knee_modify only, which moves dofs 3 and 9 as knees)."""
    num_dof: int
    default_pose: np.ndarray
    start_frames: int = 30
    end_frames: int = 30
    clip_start: int = 0
    clip_end: int = -1                     # -1: to the clip's end
    knee_modify: bool = False
    contact: float = 0.5
    dof_names: list = field(default=None)

    def __post_init__(self):
        self.start_frames, self.end_frames = int(self.start_frames), int(self.end_frames)
        self.clip_start, self.clip_end = int(self.clip_start), int(self.clip_end)
        self.knee_modify, self.contact = bool(self.knee_modify), float(self.contact)
        if self.start_frames < 0 or self.end_frames < 0:
            raise _lib.PbhcError(f"interpolation: start_frames {self.start_frames} / end_frames {self.end_frames} must be >= 0")
        if self.clip_start < 0 or self.clip_end < -1:
            raise _lib.PbhcError(f"interpolation: clip_start {self.clip_start} / clip_end {self.clip_end} must be >= 0 (clip_end -1: the clip's end)")
        if self.clip_end != -1 and self.clip_end <= self.clip_start:
            raise _lib.PbhcError(f"interpolation: clip_end {self.clip_end} <= clip_start {self.clip_start} leaves no frame")
        pose = np.asarray(self.default_pose, dtype=np.float64).reshape(-1)
        if pose.shape[0] != 7 + self.num_dof:
            raise _lib.PbhcError(f"interpolation: default_pose has {pose.shape[0]} values, expected 7 + {self.num_dof} (translation, xyzw quaternion, joints)")
        if not np.all(np.isfinite(pose)) or not np.linalg.norm(pose[3:7]) > 1e-6:
            raise _lib.PbhcError("interpolation: default_pose must be finite with a non-zero quaternion")
        self.default_pose = pose
        if self.knee_modify:
            for n in (self.start_frames, self.end_frames):
                if not knee_frames_ok(n):
                    raise _lib.PbhcError(f"interpolation: knee_modify cannot fill {n} frames: with h = {n} // 2 = {n // 2} moving frames per leg and "
                                         f"k = h // 2 = {n // 4}, the knee ramps hold 2 k + 1 = {2 * (n // 4) + 1} samples, not h (the reference "
                                         "raises ValueError there; 30, 6 and 7 work)")
            names = list(self.dof_names) if self.dof_names is not None else []
            if self.num_dof < 12 or len(names) != self.num_dof or "knee" not in str(names[3]) or "knee" not in str(names[9]):
                raise _lib.PbhcError("interpolation: knee_modify moves dofs 0..5 and 6..11 as the legs and dofs 3 and 9 as the knees; this "
                                     f"skeleton's dofs 3 and 9 are {names[3] if len(names) > 3 else None!r} and {names[9] if len(names) > 9 else None!r}")

    @property
    def active(self):
        return self.start_frames + self.end_frames > 0

    @property
    def added(self):
        return self.start_frames + self.end_frames

    def trim(self, clip):
        """The script's [start:end] cut, on the host arrays of one clip dict."""
        if self.clip_start == 0 and self.clip_end == -1:
            return clip
        F = np.asarray(clip["pose_aa"]).shape[0]
        end = F if self.clip_end == -1 else self.clip_end
        if self.clip_start >= min(end, F):
            raise _lib.PbhcError(f"interpolation: clip_start {self.clip_start} is past the end of a clip of {F} frames")
        out = dict(clip)
        for k in ("pose_aa", "root_trans_offset", "contact_mask"):
            if k in clip:
                out[k] = np.asarray(clip[k])[self.clip_start:end]
        for k in ("dof", "root_rot", "smpl_joints"):                       # per-frame arrays of the reference's pickles this project does not read
            if k in clip and np.asarray(clip[k]).shape[:1] == (F,):
                out[k] = np.asarray(clip[k])[self.clip_start:end]
        return out

    def to_c(self, device):
        """-> (PbhcMotionExtend, the device tensor its default_dof points to: keep it alive across the launch)"""
        import torch

        d_dof = torch.from_numpy(self.default_pose[7:].astype(np.float32)).to(device)
        p = _lib.PbhcMotionExtend()
        p.start_frames, p.end_frames, p.knee_modify = self.start_frames, self.end_frames, int(self.knee_modify)
        p.default_height = float(self.default_pose[2])
        for k in range(4):
            p.default_quat_xyzw[k] = float(self.default_pose[3 + k])
        p.default_dof = C.c_void_p(d_dof.data_ptr())
        p.contact_fill = self.contact
        return p, d_dof

    @classmethod
    def from_config(cls, icfg, num_dof, robot=None, dof_names=None):
        """icfg = config.robot.motion.interpolation (None / absent: returns None).  robot = config.robot supplies the default joints
        (init_state.default_joint_angles in dof order) when `default_pose` is omitted, and the dof names knee_modify is checked against."""
        if icfg is None:
            return None
        icfg = dict(icfg)
        unknown = sorted(set(icfg) - set(KEYS))
        if unknown:
            raise _lib.PbhcError(f"robot.motion.interpolation: unknown key(s) {unknown}; known: {list(KEYS)}")
        if dof_names is None and robot is not None:
            dof_names = list(robot.dof_names)
        pose = icfg.get("default_pose", None)
        if pose is None:
            if robot is None:
                raise _lib.PbhcError("robot.motion.interpolation without default_pose needs robot.init_state.default_joint_angles (pass robot=config.robot)")
            angles = robot.init_state.default_joint_angles
            pose = [0.0, 0.0, DEFAULT_HEIGHT, *DEFAULT_QUAT_XYZW] + [float(angles[n]) for n in robot.dof_names]
        return cls(num_dof=num_dof, default_pose=np.asarray(list(pose), dtype=np.float64), start_frames=icfg.get("start_frames", 30),
                   end_frames=icfg.get("end_frames", 30), clip_start=icfg.get("clip_start", 0), clip_end=icfg.get("clip_end", -1),
                   knee_modify=icfg.get("knee_modify", False), contact=icfg.get("contact", 0.5), dof_names=dof_names)
