"""`robot.motion.contact_detection` and `robot.motion.screening`: contact masks derived from a clip's own kinematics, and a stability screen,
for the SOURCE clips of a library at ingestion on the device.

The reference does both offline: `foot_detect` (motion_source/count_pkl_contact_mask.py, smpl_retarget/mink_retarget/convert_fit_motion.py)
writes a clip's `contact_mask`, and the stability filter (smpl_retarget/motion_filter/utils/motion_filter.py: compute_com_cop, compute_diff,
check_conditions) decides which clips are kept.  Here they are two keys of the motion config and one pre-pass of `MotionLib.__init__`
(`pbhc_motion_screen_frames`, `pbhc_motion_screen_clips`, csrc/pbhc_motion_screen.hip; semantics: DESIGN §8), on the raw clips before the
augmentation, the extension and the build — the reference's offline order.

This module is the host side only: the parsed settings.  There is no CPU implementation of the masks or the distances.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

from . import _lib

CONTACT_KEY = "robot.motion.contact_detection"
CONTACT_KEYS = ("enable", "foot_bodies", "vel_threshold", "height_threshold", "overwrite")
SCREEN_KEY = "robot.motion.screening"
SCREEN_KEYS = ("enable", "epsilon_stab", "epsilon_stab_frames", "cop_w", "cop_k", "action")
ACTIONS = ("report", "exclude")
# the reference hard-codes the extended-body indices 6 and 12: in both G1 models these two links
DEFAULT_FEET = ("left_ankle_roll_link", "right_ankle_roll_link")
REPORT_FIELDS = ("stable", "first_dist", "last_dist", "max_dist", "unstable_share", "max_gap")


def _unknown(cfg, keys, key):
    unknown = sorted(set(cfg) - set(keys))
    if unknown:
        raise _lib.PbhcError(f"{key}: unknown key(s) {unknown}; known: {list(keys)}")


@dataclass
class ContactDetection:
    """Validated settings.  foot_bodies: two body names, mask column 0 is the first.  vel_threshold is a squared displacement per FRAME (the
    script's constant): it depends on the clip's fps, as there."""
    enable: bool = False
    foot_bodies: list = field(default_factory=lambda: list(DEFAULT_FEET))
    vel_threshold: float = 0.002
    height_threshold: float = 0.12
    overwrite: bool = False

    def __post_init__(self):
        self.enable, self.overwrite = bool(self.enable), bool(self.overwrite)
        self.foot_bodies = [str(n) for n in self.foot_bodies]
        self.vel_threshold, self.height_threshold = float(self.vel_threshold), float(self.height_threshold)
        if len(self.foot_bodies) != 2 or self.foot_bodies[0] == self.foot_bodies[1]:
            raise _lib.PbhcError(f"{CONTACT_KEY}: foot_bodies {self.foot_bodies} must name two different bodies (mask column 0, column 1)")
        if not (self.vel_threshold > 0.0 and math.isfinite(self.vel_threshold)) or not math.isfinite(self.height_threshold):
            raise _lib.PbhcError(f"{CONTACT_KEY}: vel_threshold {self.vel_threshold} must be > 0 and height_threshold {self.height_threshold} finite")

    @property
    def active(self):
        return self.enable

    def foot_indices(self, skeleton):
        """the two names as indices into the skeleton's extended body list; an unknown name is refused"""
        names = [str(n) for n in skeleton.body_names_ext]
        for n in self.foot_bodies:
            if n not in names:
                raise _lib.PbhcError(f"{CONTACT_KEY}: foot body {n!r} is not a body of the skeleton ({names})")
        return [names.index(n) for n in self.foot_bodies]

    def to_c(self, params, skeleton):
        params.foot[0], params.foot[1] = self.foot_indices(skeleton)
        params.vel_threshold, params.height_threshold = self.vel_threshold, self.height_threshold
        return params

    @classmethod
    def from_config(cls, ccfg):
        """ccfg = config.robot.motion.contact_detection (None / absent: returns None)"""
        if ccfg is None:
            return None
        ccfg = dict(ccfg)
        _unknown(ccfg, CONTACT_KEYS, CONTACT_KEY)
        feet = ccfg.get("foot_bodies", None)
        return cls(enable=ccfg.get("enable", False), foot_bodies=list(feet) if feet is not None else list(DEFAULT_FEET),
                   vel_threshold=ccfg.get("vel_threshold", 0.002), height_threshold=ccfg.get("height_threshold", 0.12),
                   overwrite=ccfg.get("overwrite", False))


@dataclass
class Screening:
    """Validated settings; the defaults are the reference's constants (check_conditions, MotionFilter(cop_w=10, cop_k=100))."""
    enable: bool = False
    epsilon_stab: float = 0.1
    epsilon_stab_frames: int = 100
    cop_w: float = 10.0
    cop_k: float = 100.0
    action: str = "report"

    def __post_init__(self):
        self.enable, self.action = bool(self.enable), str(self.action)
        self.epsilon_stab, self.cop_w, self.cop_k = float(self.epsilon_stab), float(self.cop_w), float(self.cop_k)
        if int(self.epsilon_stab_frames) != self.epsilon_stab_frames or int(self.epsilon_stab_frames) < 1:
            raise _lib.PbhcError(f"{SCREEN_KEY}: epsilon_stab_frames {self.epsilon_stab_frames} must be an integer >= 1")
        self.epsilon_stab_frames = int(self.epsilon_stab_frames)
        if self.action not in ACTIONS:
            raise _lib.PbhcError(f"{SCREEN_KEY}: action {self.action!r}; known: {list(ACTIONS)}")
        if not (self.epsilon_stab > 0.0 and math.isfinite(self.epsilon_stab)):
            raise _lib.PbhcError(f"{SCREEN_KEY}: epsilon_stab {self.epsilon_stab} must be > 0")
        if not (self.cop_w >= 0.0 and math.isfinite(self.cop_w) and self.cop_k >= 0.0 and math.isfinite(self.cop_k)):
            raise _lib.PbhcError(f"{SCREEN_KEY}: cop_w {self.cop_w} and cop_k {self.cop_k} must be >= 0")

    @property
    def active(self):
        return self.enable

    def check_skeleton(self, skeleton):
        """the stability distance needs link masses, which only the MJCF holds"""
        if getattr(skeleton, "body_mass", None) is None:
            raise _lib.PbhcError(f"{SCREEN_KEY}: the skeleton has no link masses; load it from the robot's MJCF (Skeleton.from_mjcf, "
                                 "robot.motion.asset.assetFileName = the .xml) — a skeleton JSON holds them only if it was written from one")
        if not float(skeleton.body_mass.sum()) > 0.0:
            raise _lib.PbhcError(f"{SCREEN_KEY}: the skeleton's link masses add up to {float(skeleton.body_mass.sum())}")

    def to_c(self, params):
        params.epsilon_stab, params.epsilon_stab_frames = self.epsilon_stab, self.epsilon_stab_frames
        params.cop_w, params.cop_k = self.cop_w, self.cop_k
        return params

    @classmethod
    def from_config(cls, scfg):
        """scfg = config.robot.motion.screening (None / absent: returns None)"""
        if scfg is None:
            return None
        scfg = dict(scfg)
        _unknown(scfg, SCREEN_KEYS, SCREEN_KEY)
        return cls(enable=scfg.get("enable", False), epsilon_stab=scfg.get("epsilon_stab", 0.1), epsilon_stab_frames=scfg.get("epsilon_stab_frames", 100),
                   cop_w=scfg.get("cop_w", 10.0), cop_k=scfg.get("cop_k", 100.0), action=scfg.get("action", "report"))


def to_c(contact_detection, screening, skeleton):
    """-> PbhcMotionScreen of the active halves (the other half's members stay zero and are not read)"""
    p = _lib.PbhcMotionScreen()
    if contact_detection is not None and contact_detection.active:
        contact_detection.to_c(p, skeleton)
    if screening is not None and screening.active:
        screening.to_c(p)
    else:
        p.epsilon_stab_frames = 1
    return p


def kept_clips(stable, action):
    """-> indices of the source clips the library keeps; `exclude` with nothing left is refused"""
    stable = [bool(s) for s in stable]
    kept = list(range(len(stable))) if action != "exclude" else [i for i, s in enumerate(stable) if s]
    if not kept:
        raise _lib.PbhcError(f"{SCREEN_KEY}: action exclude: none of the {len(stable)} clip(s) passes the stability screen, the library would be empty")
    return kept
