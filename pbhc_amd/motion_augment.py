"""`robot.motion.augmentation`: mirrored and time-scaled copies of every clip, added at ingestion on the device.

The reference ships seven clips and no tool for this; mirrored and speed-changed copies are the usual way to stretch a small motion set for
a general tracker.  Here it is a key of the motion config: a library of M clips becomes M * V ordinary clips in one launch
(`pbhc_motion_augment_batch`, csrc/pbhc_motion_augment.hip; semantics: DESIGN §8) before the lead-in / lead-out frames and the build.

This module is the host side only: the parsed settings (`Augmentation`), the frame count of a time-scaled clip, and the mirror tables of a
skeleton (`mirror_tables`) with the check that the skeleton IS its own mirror image — a sign flip plus a permutation of the raw arrays is a
correct mirror only then.  There is no CPU implementation of the frames themselves.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib

KEYS = ("mirror", "speeds", "symmetry_tol")
SPEED_MIN, SPEED_MAX = 0.25, 4.0
MIN_FRAMES = 8                             # a variant shorter than this is refused
KEY = "robot.motion.augmentation"


def out_frames(num_frames, speed):
    """Frames of a clip of `num_frames` played at `speed` (the clip keeps its fps): floor((F - 1) / s) + 1 in double, one less if the last
    sample (F' - 1) s would pass the last source frame.  The export and the kernel form the same number the same way."""
    F, s = int(num_frames), float(speed)
    Fo = int(math.floor((F - 1) / s)) + 1
    if (Fo - 1) * s > F - 1:
        Fo -= 1
    return Fo


@dataclass
class MirrorTables:
    """body_perm [Bx] (row b of a mirrored pose is row body_perm[b] of the source), dof_perm / dof_sign [D] (mirrored dof d is dof_sign[d] x
    dof dof_perm[d] of the source), asymmetry: the largest |offset[perm[i]] - (x, -y, z) of offset[i]| found, in metres."""
    body_perm: np.ndarray
    dof_perm: np.ndarray
    dof_sign: np.ndarray
    asymmetry: float


def _partner_name(name):
    swap = {"left": "right", "right": "left"}
    return "_".join(swap.get(tok, tok) for tok in str(name).split("_"))


def mirror_tables(skeleton, symmetry_tol=1e-4):
    """The left <-> right tables of `skeleton` (pbhc_amd.skeleton.Skeleton) for the reflection across the x-z plane, after checking that the
    skeleton is its own mirror image under them; raises PbhcError naming the body or joint that is not."""
    names = [str(n) for n in skeleton.body_names_ext]
    Bx, B, D = len(names), skeleton.num_bodies, skeleton.num_dof
    index = {n: i for i, n in enumerate(names)}
    perm = np.zeros(Bx, dtype=np.int64)
    for i, n in enumerate(names):
        partner = _partner_name(n)
        if partner not in index:
            raise _lib.PbhcError(f"{KEY}: mirror: body {n!r} has no partner {partner!r} in the skeleton")
        perm[i] = index[partner]
    if perm[0] != 0:
        raise _lib.PbhcError(f"{KEY}: mirror: the root body {names[0]!r} must be its own mirror image")
    parents = np.asarray(skeleton.parents, dtype=np.int64)
    offsets = np.asarray(skeleton.offsets, dtype=np.float64)
    local = np.asarray(skeleton.local_rot_wxyz, dtype=np.float64)
    axes = np.asarray(skeleton.dof_axis, dtype=np.float64)
    asym = 0.0
    for i in range(1, Bx):
        j = int(perm[i])
        if (i < B) != (j < B) or parents[j] != perm[parents[i]]:
            raise _lib.PbhcError(f"{KEY}: mirror: body {names[i]!r} hangs on {names[parents[i]]!r}, its partner {names[j]!r} on "
                                 f"{names[parents[j]]!r}: the tree is not left-right symmetric")
        err = float(np.abs(offsets[j] - offsets[i] * [1.0, -1.0, 1.0]).max())
        if not err <= symmetry_tol:
            raise _lib.PbhcError(f"{KEY}: mirror: the offset of body {names[j]!r} differs from the mirrored offset of {names[i]!r} by "
                                 f"{err:.3e} m (symmetry_tol {symmetry_tol:.3e})")
        asym = max(asym, err)
        want = local[i] * [1.0, -1.0, 1.0, -1.0]                 # (w, -x, y, -z)
        if min(np.abs(local[j] - want).max(), np.abs(local[j] + want).max()) > 1e-6:
            raise _lib.PbhcError(f"{KEY}: mirror: the local rotation of body {names[j]!r} is not the mirrored one of {names[i]!r}")
    dof_perm = perm[1:1 + D] - 1                                  # dof d drives body d + 1
    dof_sign = np.zeros(D, dtype=np.float32)
    for d in range(D):
        want = axes[d] * [-1.0, 1.0, -1.0]                       # a rotation vector under the reflection: (-a_x, a_y, -a_z)
        got = axes[dof_perm[d]]
        if np.abs(got - want).max() <= 1e-6:
            dof_sign[d] = 1.0
        elif np.abs(got + want).max() <= 1e-6:
            dof_sign[d] = -1.0
        else:
            raise _lib.PbhcError(f"{KEY}: mirror: the axis {got.tolist()} of the joint of body {names[dof_perm[d] + 1]!r} is not +-(-x, y, -z) "
                                 f"of the axis {axes[d].tolist()} of the joint of body {names[d + 1]!r}")
    return MirrorTables(perm, dof_perm, dof_sign, asym)


@dataclass
class Augmentation:
    """Validated settings.  speeds: the playback speeds BESIDES 1.0, in the order of the key (1.0 itself, if listed, is dropped)."""
    mirror: bool = False
    speeds: list = field(default_factory=list)
    symmetry_tol: float = 1e-4

    def __post_init__(self):
        self.mirror, self.symmetry_tol = bool(self.mirror), float(self.symmetry_tol)
        speeds = [float(s) for s in (self.speeds if self.speeds is not None else [])]
        for s in speeds:
            if not (SPEED_MIN <= s <= SPEED_MAX):
                raise _lib.PbhcError(f"{KEY}: speed {s} is outside [{SPEED_MIN}, {SPEED_MAX}]")
        speeds = [s for s in speeds if s != 1.0]
        if len(set(speeds)) != len(speeds):
            raise _lib.PbhcError(f"{KEY}: speeds {speeds} lists a speed twice")
        if len(speeds) > _lib.K["PBHC_MAX_SPEEDS"]:
            raise _lib.PbhcError(f"{KEY}: {len(speeds)} speeds besides 1.0, at most {_lib.K['PBHC_MAX_SPEEDS']}")
        if not (self.symmetry_tol >= 0.0):
            raise _lib.PbhcError(f"{KEY}: symmetry_tol {self.symmetry_tol} must be >= 0")
        self.speeds = speeds

    @property
    def active(self):
        return self.num_variants > 1

    @property
    def num_variants(self):
        return (1 + len(self.speeds)) * (2 if self.mirror else 1)

    def variant(self, v):
        """-> (mirrored, speed) of variant v: speed-major, the mirror the inner index; variant 0 is the source"""
        si, mi = (v >> 1, v & 1) if self.mirror else (v, 0)
        return bool(mi), 1.0 if si == 0 else self.speeds[si - 1]

    def variant_frames(self, num_frames, what="clip"):
        """frames of every variant of a clip of `num_frames`; refuses a variant of fewer than MIN_FRAMES"""
        out = []
        for v in range(self.num_variants):
            _, s = self.variant(v)
            Fo = out_frames(num_frames, s)
            if Fo < MIN_FRAMES:
                raise _lib.PbhcError(f"{KEY}: {what} has {num_frames} frames, at speed {s} that leaves {Fo}, fewer than {MIN_FRAMES}")
            out.append(Fo)
        return out

    def to_c(self):
        p = _lib.PbhcMotionAugment()
        p.num_variants, p.num_speeds, p.mirror = self.num_variants, len(self.speeds), int(self.mirror)
        for k, s in enumerate(self.speeds):
            p.speeds[k] = s
        return p

    @classmethod
    def from_config(cls, acfg):
        """acfg = config.robot.motion.augmentation (None / absent: returns None)"""
        if acfg is None:
            return None
        acfg = dict(acfg)
        unknown = sorted(set(acfg) - set(KEYS))
        if unknown:
            raise _lib.PbhcError(f"{KEY}: unknown key(s) {unknown}; known: {list(KEYS)}")
        speeds = acfg.get("speeds", None)
        return cls(mirror=acfg.get("mirror", False), speeds=list(speeds) if speeds is not None else [], symmetry_tol=acfg.get("symmetry_tol", 1e-4))
