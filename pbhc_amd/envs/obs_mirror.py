"""The left <-> right mirror of every observation group and of the action vector, as host data: a signed permutation
(index int32[C], sign float32[C]) per group with `mirrored[j] = sign[j] * x[index[j]]`.  Python / numpy only — no device, no pointer: the
env turns the results into tensors (`env.mirror_maps()`), `pbhc_mirror_rows` (csrc/pbhc_mirror.hip) applies them.

The maps are built at the KEY level — a group is its keys in `sorted()` order with the widths `obs_maps.group_maps` uses — not from the
`src` feature indices of the step kernel's maps: several elements may share the ZERO source there, and a feature index says nothing about
how its value transforms.  Every key has a mirror kind (`RULES`) built from `motion_augment.mirror_tables(skeleton)`; the reflection is the one
across the x-z plane that the motion library's mirrored variants use.  A key without a rule, a body list that is not closed under the mirror,
an anchor that is not its own partner or per-joint constants that are not mirror-invariant are refused by name: a map that is only nearly
right would train the policy towards a wrong symmetry without any error showing.

Nothing here enters PbhcEnvConfig, the layout or the specialised kernels' cache key.
"""
import numpy as np

from .. import _lib
from ..motion_augment import _partner_name, mirror_tables
from . import env_config, obs_maps

# kind of every observation key with a rule (DESIGN §8 "Mirror-symmetry loss" lists what each kind does)
RULES = {
    "scalar": ["ref_motion_phase", "root_height", "dr_base_mass", "dr_friction", "dr_ctrl_delay", "dif_root_height", "future_motion_root_height"],
    "polar": ["base_lin_vel", "projected_gravity", "dr_base_com", "anchor_ref_pos", "dif_root_velocity", "future_motion_base_lin_vel"],
    "axial": ["base_ang_vel", "future_motion_base_ang_vel"],
    "yaw_rate": ["future_motion_base_yaw_vel"],
    "roll_pitch": ["roll_pitch", "future_motion_roll_pitch"],
    "joint_signed": ["dof_pos", "dof_vel", "actions", "dif_joint_angles", "dif_joint_velocities", "future_motion_dof_pos"],
    "joint_unsigned": ["dr_kp", "dr_kd"],
    "feet": ["contact_mask", "ref_contact_mask"],
    "quat": ["dif_root_rot"],
    "rot6d": ["anchor_ref_rot"],
    "key_rot6d": ["local_key_body_rot"],
    "key_polar": ["local_key_body_pos", "dif_local_key_body_pos", "local_ref_key_body_pos", "future_motion_local_ref_key_body_pos"],
    "body_polar": ["dif_local_rigid_body_pos", "local_ref_rigid_body_pos"],
    "track_polar": ["vr_3point_pos"],
    "link_mass": ["dr_link_mass"],
    "next_step": ["next_step_ref_motion"],
}
KIND = {key: kind for kind, keys in RULES.items() for key in keys}
NEXT_STEP_PARTS = ["future_motion_root_height", "future_motion_roll_pitch", "future_motion_base_lin_vel", "future_motion_base_yaw_vel",
                   "future_motion_dof_pos", "future_motion_local_ref_key_body_pos"]                # general_tracking.py:554-564, one step each
MASKED_DOF_VEL = (4, 5, 10, 11)                                                                   # general_tracking.py:821-829
INVARIANCE_TOL = 1e-6

POLAR = np.array([1.0, -1.0, 1.0], dtype=np.float32)
AXIAL = np.array([-1.0, 1.0, -1.0], dtype=np.float32)
QUAT_XYZW = np.array([-1.0, 1.0, -1.0, 1.0], dtype=np.float32)
# the first two columns of S R S, S = diag(1, -1, 1): element (i, j) of R takes s_i s_j, in the order [..., 3, 2] flattens to
ROT6D = np.array([POLAR[i] * POLAR[j] for i in range(3) for j in range(2)], dtype=np.float32)


def rule_key(key):
    """the key whose rule `key` takes: a `*_raw` and a `*_noise` key take their plain key's"""
    k = obs_maps.plain_key(key)
    return k[:-6] if k.endswith("_noise") and k[:-6] in KIND else k


def _list_perm(names, what):
    """position of every name's partner within the list `names`; refuses a list that is not closed under the mirror"""
    names = [str(n) for n in names]
    pos = {n: i for i, n in enumerate(names)}
    out = np.zeros(len(names), dtype=np.int64)
    for i, n in enumerate(names):
        partner = _partner_name(n)
        if partner not in pos:
            raise _lib.PbhcError(f"observation mirror: {what} lists {n!r} without its partner {partner!r}: the list is not closed under the mirror")
        out[i] = pos[partner]
    return out


def _blocks(perm, width, sign):
    """`len(perm)` blocks of `width` elements permuted by `perm`, every block signed by `sign`"""
    perm = np.asarray(perm, dtype=np.int64)
    index = (perm[:, None] * width + np.arange(width)[None, :]).reshape(-1)
    return index, np.tile(np.asarray(sign, dtype=np.float32), len(perm))


def _concat(parts):
    """(index, sign) of consecutive segments, each local to its own segment"""
    index, sign, o = [], [], 0
    for idx, sg in parts:
        index.append(np.asarray(idx, dtype=np.int64) + o)
        sign.append(np.asarray(sg, dtype=np.float32))
        o += len(idx)
    return np.concatenate(index), np.concatenate(sign)


def check_involution(index, sign, what=""):
    index, sign = np.asarray(index, dtype=np.int64), np.asarray(sign, dtype=np.float32)
    n = len(index)
    if index.shape != (n,) or sign.shape != (n,) or (n and (index.min() < 0 or index.max() >= n)) \
            or not np.array_equal(index[index], np.arange(n)) or not np.all(sign * sign[index] == 1.0):
        raise _lib.PbhcError(f"observation mirror: the map of {what} is not an involution")


class _Builder:
    def __init__(self, cfg, skel, symmetry_tol):
        rc, ob = cfg.robot, cfg.obs
        self.ob, self.rc, self.dr = ob, rc, cfg.domain_rand
        self.mt = mt = mirror_tables(skel, symmetry_tol)
        self.D = D = skel.num_dof
        self.dims = env_config.flatten_obs_dims(ob)
        self.S = int(ob.get("future_num_steps", 0) or 0)
        names, ext = [str(n) for n in skel.body_names], [str(n) for n in skel.body_names_ext]
        self.key_perm = _list_perm(rc.key_bodies, "robot.key_bodies")
        self.track_perm = _list_perm(rc.motion.get("motion_tracking_link", []), "robot.motion.motion_tracking_link")
        self.link_perm = _list_perm(self.dr.get("randomize_link_body_names", []), "domain_rand.randomize_link_body_names")
        feet = [n for n in names if rc.foot_name in n]
        if len(feet) != 2 or _partner_name(feet[0]) != feet[1]:
            raise _lib.PbhcError(f"observation mirror: the feet {feet} are not one left-right pair")
        # the anchor as env_config._body_sets resolves it: find_rigid_body_indice(...) + 1, sic
        anchor_link = rc.motion.get("anchor_link", "pelvis_link")
        anchor = (names.index(anchor_link) if anchor_link in names else -1) + 1
        if int(mt.body_perm[anchor]) != anchor:
            raise _lib.PbhcError(f"observation mirror: robot.motion.anchor_link {anchor_link!r} resolves to body {ext[anchor]!r}, whose mirror partner is "
                                 f"{ext[int(mt.body_perm[anchor])]!r}: the anchor frame must be its own mirror image")
        self._check_invariants()

    def _check_invariants(self):
        """per-joint constants the observations and the action path use must not tell left from right: `dof_pos` is measured from
        default_dof_pos and an action is scaled by action_scale before it moves a joint.  (No key with a rule reads a joint limit.)"""
        rc, mt, D = self.rc, self.mt, self.D
        dof_names = [str(n) for n in rc.dof_names]
        default = np.array([float(rc.init_state.default_joint_angles[n]) for n in dof_names], dtype=np.float64)
        ctrl = rc.control
        scale = np.zeros(D, dtype=np.float64)
        for i, n in enumerate(dof_names):
            for joint in ctrl.stiffness.keys():
                if joint in n:
                    scale[i] = float(ctrl.action_scale if isinstance(ctrl.action_scale, (int, float)) else ctrl.action_scale[joint])
        for what, have, want in (("robot.init_state.default_joint_angles", default, default[mt.dof_perm] * mt.dof_sign),
                                 ("robot.control.action_scale", scale, scale[mt.dof_perm])):
            bad = np.nonzero(np.abs(have - want) > INVARIANCE_TOL)[0]
            if len(bad):
                d = int(bad[0])
                raise _lib.PbhcError(f"observation mirror: {what} of {dof_names[d]!r} ({have[d]:g}) is not the mirror of its partner "
                                     f"{dof_names[int(mt.dof_perm[d])]!r}'s ({want[d]:g} expected): default_dof_pos and the action scale must be "
                                     f"invariant under the joint mirror within {INVARIANCE_TOL:g}")
        if self.ob.get("masked_dof_vel", False):
            masked = set(MASKED_DOF_VEL)
            for j in MASKED_DOF_VEL:
                if int(mt.dof_perm[j]) not in masked:
                    raise _lib.PbhcError(f"observation mirror: obs.masked_dof_vel masks joint {dof_names[j]!r} but not its partner "
                                         f"{dof_names[int(mt.dof_perm[j])]!r}")

    def step_map(self, key):
        """(index, sign) of ONE step / frame of observation key `key`"""
        k = rule_key(key)
        if k not in KIND:
            raise NotImplementedError(f"observation mirror: observation key {key!r} has no mirror rule")
        kind, mt, D = KIND[k], self.mt, self.D
        one = lambda sign: (np.arange(len(sign)), np.asarray(sign, dtype=np.float32))
        if kind == "scalar":
            m = one(np.ones(self.dims[k], dtype=np.float32))
        elif kind == "polar":
            m = one(POLAR)
        elif kind == "axial":
            m = one(AXIAL)
        elif kind == "yaw_rate":
            m = one([-1.0])
        elif kind == "roll_pitch":
            m = one([-1.0, 1.0])
        elif kind == "joint_signed":
            m = (mt.dof_perm, mt.dof_sign)
        elif kind == "joint_unsigned":
            m = (mt.dof_perm, np.ones(D, dtype=np.float32))
        elif kind == "feet":
            m = (np.array([1, 0]), np.ones(2, dtype=np.float32))
        elif kind == "quat":
            m = one(QUAT_XYZW)
        elif kind == "rot6d":
            m = one(ROT6D)
        elif kind == "key_rot6d":
            m = _blocks(self.key_perm, 6, ROT6D)
        elif kind == "key_polar":
            m = _blocks(self.key_perm, 3, POLAR)
        elif kind == "body_polar":
            m = _blocks(mt.body_perm, 3, POLAR)
        elif kind == "track_polar":
            m = _blocks(self.track_perm, 3, POLAR)
        elif kind == "link_mass":
            m = (self.link_perm, np.ones(len(self.link_perm), dtype=np.float32))
        else:                                                    # next_step: its parts, one step each, in order
            m = _concat([self.step_map(p) for p in NEXT_STEP_PARTS])
        if len(m[0]) != self.dims[k]:
            raise _lib.PbhcError(f"observation mirror: obs_dims[{k}]={self.dims[k]} does not match the {len(m[0])} values the mirror rule of {key!r} covers")
        return m

    def key_map(self, key):
        """(index, sign) of observation key `key` as it stands in a group: history keys frame-major, future keys step-major"""
        k = obs_maps.plain_key(key)
        if k in self.ob.obs_auxiliary:
            parts = []
            for hk, frames in sorted(self.ob.obs_auxiliary[k].items()):
                parts.extend([self.step_map(hk)] * int(frames))
            return _concat(parts)
        m = self.step_map(k)
        if k.startswith("future_motion_") and self.S:
            return _concat([m] * self.S)
        return m

    def group_map(self, keys):
        return _concat([self.key_map(key) for key in sorted(keys)])


def build(cfg, skel, symmetry_tol=1e-4):
    """cfg: the top-level config (robot / obs / domain_rand), skel: pbhc_amd.skeleton.Skeleton -> {group: (index int32[C], sign float32[C])}
    for every group of `obs.obs_dict`, plus "actions".  Raises PbhcError / NotImplementedError naming what has no mirror."""
    b = _Builder(cfg, skel, symmetry_tol)
    maps = {}
    for group, keys in cfg.obs.obs_dict.items():
        try:
            maps[group] = b.group_map(keys)
        except NotImplementedError as e:
            raise NotImplementedError(f"{e} (observation group {group!r})") from None
    if "actions" in maps:
        raise _lib.PbhcError("observation mirror: an observation group named 'actions' collides with the action map")
    maps["actions"] = (b.mt.dof_perm, b.mt.dof_sign)
    out = {}
    for name, (index, sign) in maps.items():
        check_involution(index, sign, name)
        out[name] = (np.ascontiguousarray(index, dtype=np.int32), np.ascontiguousarray(sign, dtype=np.float32))
    return out


def apply(m, x):
    """the numpy statement of a map: x [..., C] -> mirrored [..., C]"""
    index, sign = m
    return np.asarray(x)[..., index] * sign
