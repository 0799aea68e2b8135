"""Config tree (the reference's YAML schema) -> PbhcEnvConfig + device-side output maps.

Host-side, load-time.  Mirrors what the reference derives at construction:
  * obs dims / sorted-key layout      helpers.determine_obs_dim (utils/helpers.py:47-80),
                                      _post_config_observation_callback (legged_robot_base.py:787-793)
  * history buffers                   HistoryHandler.__init__ (envs/env_utils/history_handler.py:12-31)
  * reward list, scales * dt          _prepare_reward_function (legged_robot_base.py:167-233)
  * body index sets                   _setup_robot_body_indices (base_task.py:169-205),
                                      _init_tracking_config / _init_motion_extend (motion_tracking.py:203-242)
  * gains / limits                    _init_buffers (legged_robot_base.py:74-108), isaacgym._process_dof_props
A reward or observation name the kernels do not implement raises NotImplementedError — the
reference would call `_reward_<name>` / `_get_obs_<name>`; we refuse instead of silently skipping.

`build` runs these sections in order; each takes what it reads and fills one region of the struct `c` / the layout `L`:
  1. _control            gains, limits, action scaling, the domain-randomisation ranges of the control path
  2. _body_sets          feet / penalised / upper / lower / track / key index lists, per-body flags and slots
  3. _terminations       termination switches and their curricula, reset-state noise, the refused env options
  4. _rewards            reward terms, their scales and sums, penalty / noise / soft-limit curricula   (+ _noise_process: the OU IMU noise)
  5. obs_maps.feature_layout   which features the observations read and where they sit in the feature row   | host data only (python /
  6. obs_maps.group_maps       every output element as (dst, src, scale, noise); run_length, compact_image  | numpy, no device, no
  8. obs_maps.assign_roles     which waves write which row, and the runs handed to the dynamics waves       | pointer): envs/obs_maps.py
  7. _materialise        the one step that creates device tensors and writes 5, 6 and 8 into the struct
  9. _initial_globals    sigmas, curriculum values and thresholds the env starts from
and record_layout (the evaluation recorder's part).  tests/test_env_config_snapshot.py pins the whole output.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np
import torch

from .. import _lib
from . import obs_maps

K = _lib.K

# Environment switches, all measurement aids:
#   PBHC_PACKED_MAPS     read at import.  0: no compact 16-bit observation maps staged in LDS (PbhcEnvConfig.map_image); diagnosis only
#   PBHC_ROLE0_HANDICAP  read by build.  Weight of the dynamics waves' reward / reset work in the row assignment (obs_maps.assign_roles)
#   PBHC_ROW_HELP_SHARE  read by build.  Share of the observation runs handed to the dynamics waves (obs_maps.assign_roles; default 0)
PACKED_MAPS = os.environ.get("PBHC_PACKED_MAPS", "1") != "0"

SIGMA_KEYS = ["teleop_max_joint_pos", "teleop_upper_body_pos", "teleop_lower_body_pos", "teleop_vr_3point_pos", "teleop_feet_pos",
              "teleop_body_rot", "teleop_body_vel", "teleop_body_ang_vel", "teleop_joint_pos", "teleop_joint_vel",
              # general tracking (rewards/motion_tracking/general_main.yaml)
              "teleop_key_body_pos", "teleop_anchor_body_pos", "teleop_anchor_body_rot", "local_key_body_pos", "local_key_body_rot",
              "key_body_vel", "key_body_ang_vel", "teleop_root_vel", "teleop_root_pose"]
TERM_SIGMAS = {
    "teleop_max_joint_position": [0], "teleop_body_position_extend": [1, 2], "teleop_vr_3point": [3], "teleop_body_position_feet": [4],
    "teleop_body_rotation_extend": [5], "teleop_body_velocity_extend": [6], "teleop_body_ang_velocity_extend": [7],
    "teleop_joint_position": [8], "teleop_joint_velocity": [9],
    "teleop_key_body_position": [10], "teleop_anchor_body_position": [11], "teleop_anchor_body_rotation": [12], "local_key_body_position": [13],
    "local_key_body_rotation": [14], "key_body_velocity": [15], "key_body_ang_velocity": [16], "teleop_root_vel": [17], "teleop_root_pose": [18],
}
V2_ONLY_TERMS = {"teleop_key_body_position", "teleop_anchor_body_position", "teleop_anchor_body_rotation", "local_key_body_position",
                 "local_key_body_rotation", "key_body_velocity", "key_body_ang_velocity", "teleop_root_vel", "teleop_root_pose", "teleop_contact_mask_v2"}
# motion_tracking.py defines these two (:1238-1244, 1286-1292); general_tracking.py does not
V1_ONLY_TERMS = {"teleop_radial_body_velocity_extend", "teleop_radial_joint_velocity"}


def flatten_obs_dims(obs_cfg):
    d = obs_cfg.obs_dims
    if isinstance(d, list):
        return {k: int(v) for item in d for k, v in item.items()}
    return {k: int(v) for k, v in d.items()}


def _group_widths(ob, dims, aux, future_steps=0):
    """width of every observation group; with `future_steps` the future_motion_* keys, which list their PER-STEP dim (obs_ppo_teacher.yaml),
    count that many times"""
    width = lambda k: dims[k] * (future_steps if (k.startswith("future_motion_") and future_steps) else 1) if k in dims else aux[k]
    return {g: sum(width(obs_maps.plain_key(key)) for key in keys) for g, keys in ob.obs_dict.items()}


def determine_obs_dim(cfg):
    """helpers.determine_obs_dim: fills cfg.robot.algo_obs_dim_dict and returns (group dims, key dims, aux dims)."""
    ob = cfg.obs
    assert set(ob.noise_scales.keys()) == set(ob.obs_scales.keys())
    dims = flatten_obs_dims(ob)
    ob.obs_dims = dims
    aux = {}
    for aux_key, aux_cfg in ob.obs_auxiliary.items():
        aux[aux_key] = sum(dims[k] * n for k, n in aux_cfg.items())
    groups = _group_widths(ob, dims, aux)
    cfg.robot.algo_obs_dim_dict = groups
    return groups, dims, aux


def _joint_idx(idx, D, what):
    """domain_rand.<what>.joint_idx as a list of dof indices in [0, D) (D <= PBHC_MAX_DOF); torch's negative indices are taken modulo D, as the
    reference's advanced indexing does.  Out-of-range and repeated entries are refused (the reference raises on the first, and on the
    second its in-place `*=` / `+=` through the index would apply only one of the draws)"""
    out = []
    for j in list(idx):
        j = int(j)
        if not -D <= j < D or D > K["PBHC_MAX_DOF"]:
            raise IndexError(f"domain_rand.{what}.joint_idx: {j} is out of range for {D} dofs (PBHC_MAX_DOF = {K['PBHC_MAX_DOF']})")
        j %= D
        if j in out:
            raise ValueError(f"domain_rand.{what}.joint_idx lists dof {j} twice")
        out.append(j)
    return out


def _scaled_limits(lower, upper, fraction):
    """(m - 0.5 r s, m + 0.5 r s) of a joint range in fp32, operation for operation as the reference's tensors compute it"""
    lo, hi = np.float32(lower), np.float32(upper)
    mid, width = np.float32((lo + hi) / np.float32(2)), np.float32(hi - lo)
    half = np.float32(np.float32(0.5) * width) * np.float32(fraction)
    return float(np.float32(mid - half)), float(np.float32(mid + half))


def _set_indices(c, count, array, indices):
    """an index list into the struct's (count, array) pair"""
    setattr(c, count, len(indices))
    for i, b in enumerate(indices):
        getattr(c, array)[i] = b


@dataclass
class EnvLayout:
    """Everything the host needs to know about the layouts the kernels use.  `build` fills every field; a caller may rely on all of them."""
    dt: float = 0.0                                         # control step [s]
    max_episode_length: float = 0.0                         # in control steps
    ps_pd_idx: list = field(default_factory=list)           # dofs of domain_rand.parallel_serial_pd, in the order of the [N, J] draws ([]: off)
    ps_tau_idx: list = field(default_factory=list)          # dofs of domain_rand.parallel_serial_tau
    feet: list = field(default_factory=list)                # body indices: the two feet
    penalised: list = field(default_factory=list)           # robot.penalize_contacts_on
    upper: list = field(default_factory=list)               # extended-body indices of motion.upper_body_link
    lower: list = field(default_factory=list)               # motion.lower_body_link
    track: list = field(default_factory=list)               # motion.motion_tracking_link
    key: list = field(default_factory=list)                 # robot.key_bodies (general tracking; [] otherwise)
    termination_contact: list = field(default_factory=list)  # robot.terminate_after_contacts_on (listed whether or not terminate_by_contact is on)
    reward_scales: dict = field(default_factory=dict)       # non-zero reward scales x dt, in the config's order (`termination` included)
    reward_names: list = field(default_factory=list)        # the terms of the reward loop: reward_scales without `termination`
    sum_names: list = field(default_factory=list)           # columns of the episode sums: every key of reward_scales
    num_rew_fn: int = 1                                     # columns of the reward buffer
    future_steps: list = field(default_factory=list)        # look-ahead steps of the future_motion_* observations (general tracking; [] otherwise)
    obs_dims: dict = field(default_factory=dict)            # width of every observation key (future keys: per step)
    group_dims: dict = field(default_factory=dict)          # width of the tensor the env hands out per observation group
    hist_keys: list = field(default_factory=list)           # keys with a history buffer, sorted
    hist_len: dict = field(default_factory=dict)            # key -> frames kept
    hist_off: dict = field(default_factory=dict)            # key -> offset of its frames in the history block
    hist_dim: int = 1                                       # width of the history block (>= 1)
    feat_off: dict = field(default_factory=dict)            # feature -> offset in the feature row, of the features in use
    feat_dim_each: dict = field(default_factory=dict)       # feature -> width, of every feature (feature_dims)
    group_names: list = field(default_factory=list)         # observation groups in map order, then "__history__" (the history write-back)
    map_tensors: list = field(default_factory=list)         # per group the device tensors (dst, src, scale, noise) the struct points to
    group_roles: list = field(default_factory=list)         # per group 0: written by the dynamics waves, 1: by the reference / observation waves
    helper_elements: int = 0                                # elements of role-1 rows handed to the dynamics waves (PBHC_ROW_HELP_SHARE)
    map_image: object = None                                # device tensor of the compact maps, or None when they do not apply
    globals0: object = None                                 # float64 array: the initial PBHC_G_* globals
    record: object = None                                   # record_layout(): the evaluation recorder's layout, or None


def build(cfg, skel, motion_lib, num_envs, device, sim_link_mass_dim, seed=0, mode=0):
    """mode 0: LeggedRobotMotionTracking, mode 1: LeggedRobotGeneralTracking."""
    ec, rc, rw, ob = cfg.env.config, cfg.robot, cfg.rewards, cfg.obs
    role0_handicap = float(os.environ.get("PBHC_ROLE0_HANDICAP", "0.1" if mode == 1 else "1e9"))
    row_help_share = float(os.environ.get("PBHC_ROW_HELP_SHARE", "0"))
    D, Bx = skel.num_dof, skel.num_bodies_ext
    if list(rc.dof_names) and len(rc.dof_names) != D:
        raise _lib.PbhcError("config dof_names do not match the skeleton")
    c = _lib.PbhcEnvConfig()
    L = EnvLayout()
    c.abi_version = K["PBHC_ENV_CONFIG_VERSION"]       # the layout of this struct: not every ABI bump moves it
    c.tracking_mode = mode
    c.num_envs = num_envs
    c.skel = skel.to_c()
    sim = cfg.simulator.config.sim
    c.sim_dt = 1.0 / sim.fps
    c.dt = L.dt = dt = sim.control_decimation * (1.0 / sim.fps)
    c.max_episode_length = L.max_episode_length = float(np.ceil(ec.max_episode_length_s / dt))
    c.max_episode_length_s = float(ec.max_episode_length_s)
    _control(c, L, rc, cfg.domain_rand, rw.reward_limit.soft_dof_pos_limit, D)
    body_z = _body_sets(c, L, rc, skel, mode)
    dof_far_thr = _terminations(c, L, ec, rc, skel.body_names, body_z, D, Bx, mode)
    _rewards(c, L, rw, ec, ob, dt, mode)
    # ---- features
    _, dims, aux = determine_obs_dim(cfg)
    S = int(ob.get("future_num_steps", 0)) if mode == 1 else 0
    if S:
        L.future_steps = torch.linspace(start=1, end=ob.future_max_steps, steps=S, dtype=torch.long).tolist()      # general_tracking.py:501-507
        if S > K["PBHC_MAX_FUTURE"]:
            raise _lib.PbhcError("too many future steps")
        c.future_num_steps = S
        for i, v in enumerate(L.future_steps):
            c.future_steps[i] = int(v)
    Sr = int(ob.get("future_ref_steps", 0) or 0) if mode == 0 else 0         # motion_tracking.py:586: look-ahead steps of future_ref_dof_*
    if Sr > K["PBHC_MAX_FUTURE"]:
        raise _lib.PbhcError("too many future_ref_steps")
    feats = dict(obs_maps.OBS_FEATURES, **(obs_maps.OBS_FEATURES_V2 if mode == 1 else obs_maps.OBS_FEATURES_V1))
    if _noise_process(c, ob.get("noise_process", None), dt):
        feats.update(obs_maps.NOISE_PROCESS_FEATURES)
    # widths of the tensors the env hands out: the future group is [N, S * per-step dim] (ppo_mimic.py:206-216)
    L.obs_dims, L.group_dims = dims, _group_widths(ob, dims, aux, S)
    L.hist_keys, L.hist_len, L.hist_off, L.hist_dim = obs_maps.history_layout(ob, dims)
    fdim = obs_maps.feature_dims(D, Bx, len(L.track), len(L.feet), S, len(L.key), Sr, sim_link_mass_dim, L.hist_dim)
    used, row_off, feat_class = obs_maps.feature_layout(ob, feats, fdim, L.hist_keys, mode)
    L.feat_off, L.feat_dim_each = {name: row_off[name] for name in row_off if name in used}, fdim
    maps = obs_maps.group_maps(ob, dims, L, feats, D, S, Sr, mode)
    runs = [obs_maps.run_length(m, feat_class, L.feat_off["HISTORY"]) for m in maps]
    image = obs_maps.compact_image(maps, feat_class) if PACKED_MAPS else None
    roles, helper_runs = obs_maps.assign_roles(maps, runs, L.feat_off, fdim, role0_handicap, row_help_share, mode)
    # ---- the struct and the device tensors
    c.hist_dim, c.dr_link_mass_dim = L.hist_dim, sim_link_mass_dim
    for name, o in row_off.items():
        c.feat_off[K["PBHC_F_" + name]] = o
    c.feat_dim = len(feat_class)
    c.obs_extra = (1 if "ONE" in used else 0) | (2 if "FEET_CONTACT_FORCE" in used else 0) | (4 if "REF_VEL_RELYAW" in used else 0)
    c.future_ref_steps = Sr if ("FUT_REF_DOF_POS" in used or "FUT_REF_DOF_VEL" in used) else 0
    _materialise(c, L, maps, runs, image, roles, helper_runs, device)
    c.clip_observations = float(ec.normalization.clip_observations)
    c.has_contact_mask = int(bool(motion_lib.has_contact_mask))
    if "teleop_contact_mask" in L.reward_names and not motion_lib.has_contact_mask:
        raise AttributeError("teleop_contact_mask reward needs a motion file with contact_mask")   # reference raises too (motion_tracking.py:1156)
    c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    L.globals0 = _initial_globals(rw, ec, ob, dof_far_thr)
    L.record = record_layout(ec, L, D, Bx, mode)
    return c, L


def _control(c, L, rc, dr, soft_dof_pos_limit, D):
    """gains, limits and action scaling per joint; the domain-randomisation ranges of the control path"""
    ctrl = rc.control
    if ctrl.control_type not in ("P", "V", "T"):
        raise NameError(f"Unknown controller type: {ctrl.control_type}")            # legged_robot_base.py:817
    c.control_type = {"P": 0, "V": 1, "T": 2}[ctrl.control_type]
    for i, name in enumerate(rc.dof_names):
        c.default_dof_pos[i] = float(rc.init_state.default_joint_angles[name])
        found = False
        for joint in ctrl.stiffness.keys():
            if joint in name:
                c.p_gains[i] = float(ctrl.stiffness[joint])
                c.d_gains[i] = float(ctrl.damping[joint])
                found = True
                c.action_scale[i] = float(ctrl.action_scale if isinstance(ctrl.action_scale, (int, float)) else ctrl.action_scale[joint])
        if not found:
            raise ValueError(f"PD gain of joint {name} were not defined. Should be defined in the yaml file.")
        c.torque_limits[i] = float(rc.dof_effort_limit_list[i])
        c.dof_vel_limits[i] = float(rc.dof_vel_limit_list[i])
        c.hard_dof_pos_limits[i][0] = float(np.float32(rc.dof_pos_lower_limit_list[i]))
        c.hard_dof_pos_limits[i][1] = float(np.float32(rc.dof_pos_upper_limit_list[i]))
        c.soft_dof_pos_limits[i][0], c.soft_dof_pos_limits[i][1] = _scaled_limits(rc.dof_pos_lower_limit_list[i], rc.dof_pos_upper_limit_list[i], soft_dof_pos_limit)
    c.action_clip_value = float(ctrl.action_clip_value)
    c.clip_torques = int(bool(ctrl.clip_torques))
    c.randomize_torque_rfi = int(bool(dr.randomize_torque_rfi))
    c.rfi_lim = float(dr.get("rfi_lim", 0.0))
    c.use_rao = int(bool(dr.use_rao))
    c.rao_lim = float(dr.get("rao_lim", 0.0))
    c.randomize_ctrl_delay = int(bool(dr.randomize_ctrl_delay))
    c.queue_len = int(dr.ctrl_delay_step_range[1]) + 1 if dr.randomize_ctrl_delay else 1
    c.ctrl_delay_range[0], c.ctrl_delay_range[1] = int(dr.ctrl_delay_step_range[0]), int(dr.ctrl_delay_step_range[1])
    c.randomize_pd_gain = int(bool(dr.randomize_pd_gain))
    c.kp_range[0], c.kp_range[1] = float(dr.kp_range[0]), float(dr.kp_range[1])
    c.kd_range[0], c.kd_range[1] = float(dr.kd_range[0]), float(dr.kd_range[1])
    c.randomize_rfi_lim = int(bool(dr.randomize_rfi_lim))
    c.rfi_lim_range[0], c.rfi_lim_range[1] = float(dr.rfi_lim_range[0]), float(dr.rfi_lim_range[1])
    if "parallel_serial_pd" in dr and dr.parallel_serial_pd.get("enable", False):
        # legged_robot_base.py:607-613: kp / kd scales of the listed joints *= U(ratio) at every episodic DR (after randomize_pd_gain)
        pspd = dr.parallel_serial_pd
        L.ps_pd_idx = _joint_idx(pspd.joint_idx, D, "parallel_serial_pd")
        c.ps_pd, c.ps_pd_num = 1, len(L.ps_pd_idx)
        c.ps_pd_ratio[0], c.ps_pd_ratio[1] = float(pspd.ratio[0]), float(pspd.ratio[1])
    if "parallel_serial_tau" in dr and dr.parallel_serial_tau.get("enable", False):
        # legged_robot_base.py:621-623 (rao_scale += rao_lim randn, episodic) and 822-829 (torque += rfi_lim torque_limit randn, per step)
        pst = dr.parallel_serial_tau
        L.ps_tau_idx = _joint_idx(pst.joint_idx, D, "parallel_serial_tau")
        c.ps_tau, c.ps_tau_num = 1, len(L.ps_tau_idx)
        c.ps_tau_rao_lim, c.ps_tau_rfi_lim = float(pst.rao_lim), float(pst.rfi_lim)
    for i in range(K["PBHC_MAX_DOF"]):
        c.ps_pd_slot[i] = L.ps_pd_idx.index(i) if i in L.ps_pd_idx else -1
        c.ps_tau_slot[i] = L.ps_tau_idx.index(i) if i in L.ps_tau_idx else -1
    c.randomize_default_dof_pos = int(bool(dr.get("randomize_default_dof_pos", False)))     # legged_robot_base.py:632-635
    if c.randomize_default_dof_pos:
        c.dof_pos_range[0], c.dof_pos_range[1] = float(dr.dof_pos_range[0]), float(dr.dof_pos_range[1])


def _body_sets(c, L, rc, skel, mode):
    """the body index lists, the per-body flags and slots; returns the bodies terminate_by_body_z looks at ([] in mode 0)"""
    names, ext = skel.body_names, skel.body_names_ext
    L.feet = [names.index(s) for s in names if rc.foot_name in s]
    if len(L.feet) != 2:
        raise _lib.PbhcError(f"expected 2 feet, found {len(L.feet)}")
    for n in rc.penalize_contacts_on:
        L.penalised.extend([names.index(s) for s in names if n in s])
    motion = rc.motion
    L.upper = [ext.index(l) for l in motion.get("upper_body_link", [])]
    L.lower = [ext.index(l) for l in motion.get("lower_body_link", [])]
    L.track = [ext.index(l) for l in motion.get("motion_tracking_link", [])]
    body_z = []
    if mode == 1:
        L.key = [ext.index(l) for l in rc.key_bodies]                         # general_tracking.py:94-95
        anchor_link = motion.get("anchor_link", "pelvis_link")
        c.anchor_index = (names.index(anchor_link) if anchor_link in names else -1) + 1      # find_rigid_body_indice(...) + 1, sic (:97-98)
        body_z = [4, 10, 24, 25, 26]                                          # hard-coded in the reference (:253)
    for array, indices in (("feet", L.feet), ("penalised", L.penalised), ("upper", L.upper), ("lower", L.lower), ("track", L.track), ("key", L.key)):
        _set_indices(c, "num_" + array, array, indices)
    for b in range(skel.num_bodies_ext):
        c.body_flags[b] = ((1 if b in L.upper else 0) | (2 if b in L.lower else 0) | (4 if b in L.track else 0) | (8 if b in L.feet else 0)
                           | (16 if b in L.key else 0) | (32 if b in body_z else 0))
        c.track_slot[b] = L.track.index(b) if b in L.track else -1
        c.key_slot[b] = L.key.index(b) if b in L.key else -1
    return body_z


def _terminations(c, L, ec, rc, names, body_z, D, Bx, mode):
    """termination switches, scales and curricula; the noise on the reset state; the env options that are refused.  Returns the initial
    dof-far threshold (0 when the switch is off)."""
    term = ec.termination
    tc = ec.termination_curriculum
    scales = ec.termination_scales
    dof_far_thr = 0.0
    if mode == 0 and term.get("terminate_when_dof_far", False):
        # motion_tracking.py:343-349 reduces torch.any(norm(dif_joint_angles) > threshold) over the ENV axis: one env past the threshold resets
        # all of them.  The decision is the pre-pass k_dof_far_any; general tracking never reads the switch (accepted and ignored, as there).
        dcur = tc.terminate_when_dof_far_curriculum
        c.terminate_when_dof_far = 1
        dof_far_thr = float(dcur.init)                                # :128-130, whether or not the curriculum is enabled
        c.dof_far_curriculum = int(bool(dcur.get("enable", False)))
        if c.dof_far_curriculum:                                      # :283-292
            c.dof_far_degree, c.dof_far_down, c.dof_far_up = float(dcur.degree), float(dcur.level_down_threshold), float(dcur.level_up_threshold)
            c.dof_far_min, c.dof_far_max = float(dcur.min), float(dcur.max)
    level = float(ec.get("noise_to_initial_level", 0) or 0)
    if level != 0.0:
        # motion_tracking.py:470-545 / general_tracking.py:405-485 (custom_origins False: the plane-terrain branch every fixture runs): noise on
        # the state an env is reset to, scale x level as the reference multiplies its python floats (the rotation's max angle with its 3.14 / 180)
        ns = ec.init_noise_scale
        c.reset_noise = 1
        c.rn_root_pos, c.rn_root_vel, c.rn_root_ang_vel = (float(ns.root_pos * level), float(ns.root_vel * level), float(ns.root_ang_vel * level))
        c.rn_root_rot = float(ns.root_rot * 3.14 / 180 * level)
        c.rn_dof_pos, c.rn_dof_vel = float(ns.dof_pos * level), float(ns.dof_vel * level)
    if ec.get("use_teleop_control", False):
        raise NotImplementedError("use_teleop_control (a ROS subscriber feeding marker coordinates, motion_tracking.py:112-118)")
    sdc = ec.get("soft_dynamic_correction", None)
    if sdc is not None and sdc.get("enable", False):
        # motion_tracking.py:806-860 blends the SIMULATOR's state towards the reference between physics sub-steps: it acts on the physics, which
        # the replay stub does not have (the states it hands out are whatever the replay holds)
        raise NotImplementedError("soft_dynamic_correction (acts inside the simulator's physics sub-steps; the replay stub has none)")
    # legged_robot_base.py:449-479 + isaacgym.py:387-388: probabilistic terminations near the joint limits (one uniform per gate and STEP)
    prob = ec.get("termination_probality", {})
    c.terminate_close_pos = int(bool(term.get("terminate_when_close_to_dof_pos_limit", False)))
    c.terminate_close_vel = int(bool(term.get("terminate_when_close_to_dof_vel_limit", False)))
    c.terminate_close_tau = int(bool(term.get("terminate_when_close_to_torque_limit", False)))
    if c.terminate_close_pos:
        c.term_close_prob[0] = float(prob.terminate_when_close_to_dof_pos_limit)
        for i in range(D):
            c.dof_pos_limits_termination[i][0], c.dof_pos_limits_termination[i][1] = _scaled_limits(
                rc.dof_pos_lower_limit_list[i], rc.dof_pos_upper_limit_list[i], scales.termination_close_to_dof_pos_limit)
    if c.terminate_close_vel:
        c.term_close_prob[1] = float(prob.terminate_when_close_to_dof_vel_limit)
        c.term_close_vel_scale = float(scales.termination_close_to_dof_vel_limit)
    if c.terminate_close_tau:
        c.term_close_prob[2] = float(prob.terminate_when_close_to_torque_limit)
        c.term_close_tau_scale = float(scales.termination_close_to_torque_limit)
    c.terminate_by_contact = int(bool(term.get("terminate_by_contact", False)))              # legged_robot_base.py:434-436
    for n in rc.get("terminate_after_contacts_on", []):                                     # base_task.py:178-180,195-197
        L.termination_contact.extend([names.index(s) for s in names if n in s])
    if c.terminate_by_contact and len(L.termination_contact) > K["PBHC_MAX_IDX"]:
        raise _lib.PbhcError("too many terminate_after_contacts_on bodies")
    _set_indices(c, "num_term_contact", "term_contact", L.termination_contact if c.terminate_by_contact else [])    # (the kernel gets the list only when the switch is on)
    c.terminate_by_low_height = int(bool(term.get("terminate_by_low_height", False)))        # :442-444
    c.termination_min_base_height = float(scales.get("termination_min_base_height", 0.0))
    c.terminate_by_gravity = int(bool(term.terminate_by_gravity))
    c.termination_gravity = float(scales.termination_gravity)
    c.terminate_when_motion_far = int(bool(term.terminate_when_motion_far))
    c.terminate_when_motion_end = int(bool(term.terminate_when_motion_end))
    if mode == 1:                                                             # general_tracking.py:241-254
        c.terminate_by_ref_pos_z = int(bool(term.get("terminate_by_ref_pos_z", False)))
        c.terminate_by_ref_ori = int(bool(term.get("terminate_by_ref_ori", False)))
        c.terminate_by_body_z = int(bool(term.get("terminate_by_body_z", False)))
        c.ref_pos_z_threshold = float(scales.get("terminate_by_ref_pos_z_threshold", 0.25))
        c.ref_ori_threshold = float(scales.get("terminate_by_ref_ori_threshold", 0.8))
        c.body_z_threshold = float(scales.get("terminate_by_body_z_threshold", 0.25))
        if c.terminate_by_body_z and max(body_z) >= Bx:
            raise IndexError(f"terminate_by_body_z indexes body {max(body_z)} of {Bx}")      # the reference would raise the same way
        # (terminate_when_local_motion_far is read by nobody in the reference either)
    elif any(term.get(k, False) for k in ("terminate_by_ref_pos_z", "terminate_by_ref_ori", "terminate_by_body_z")):
        raise NotImplementedError("general-tracking terminations need env._target_ ...general_tracking.LeggedRobotGeneralTracking")
    c.motion_far_curriculum = int(bool(tc.terminate_when_motion_far_curriculum))
    c.motion_far_degree = float(tc.terminate_when_motion_far_curriculum_degree)
    c.motion_far_down = float(tc.terminate_when_motion_far_curriculum_level_down_threshold)
    c.motion_far_up = float(tc.terminate_when_motion_far_curriculum_level_up_threshold)
    c.motion_far_min = float(tc.terminate_when_motion_far_threshold_min)
    c.motion_far_max = float(tc.terminate_when_motion_far_threshold_max)
    return dof_far_thr


def _rewards(c, L, rw, ec, ob, dt, mode):
    """the reward terms (ids, scales x dt, sum columns, sigmas in use) and the penalty / noise / soft-limit curricula"""
    L.reward_scales = {name: v * dt for name, v in rw.reward_scales.items() if v != 0}
    L.reward_names = [name for name in L.reward_scales if name != "termination"]
    L.sum_names = list(L.reward_scales.keys())
    c.num_terms = len(L.reward_names)
    if c.num_terms > min(K["PBHC_MAX_TERMS"], 31):
        raise _lib.PbhcError("too many reward terms")
    c.use_vec_reward = int(bool(ec.use_vec_reward))
    c.num_rew_cols = L.num_rew_fn = c.num_terms + 1 if ec.use_vec_reward else 1
    pen_names = set(rw.reward_penalty_reward_names)
    for i, name in enumerate(L.reward_names):
        if name == "feet_max_height_for_this_air":
            # legged_robot_base.py:1022 applies `~` to self.last_contacts_filt, which _init_buffers (:68) creates as a FLOAT tensor and
            # _post_compute_observations_callback (:405) only ever writes in place: torch raises TypeError on the term's first evaluation
            raise NotImplementedError("reward term 'feet_max_height_for_this_air': the reference's env cannot run it (its first evaluation raises "
                                      "TypeError: `~` on the float tensor last_contacts_filt, legged_robot_base.py:68,1022)")
        term_id = "PBHC_R_" + name.upper()
        if term_id not in K or (mode == 0 and name in V2_ONLY_TERMS) or (mode == 1 and name in V1_ONLY_TERMS):
            raise NotImplementedError(f"reward term {name!r} has no HIP implementation")
        c.term_id[i] = K[term_id]
        if name in ("feet_heading_alignment", "feet_heading_alignment_contact", "penalty_feet_ori", "penalty_feet_ori_contact"):
            c.foot_ori_terms = 1
        c.term_scale[i] = float(L.reward_scales[name])
        c.term_penalty[i] = int(name in pen_names and bool(rw.reward_penalty_curriculum))
        c.term_sum_col[i] = L.sum_names.index(name)
        for sigma in TERM_SIGMAS.get(name, []):
            c.sigma_active[sigma] = 1
    c.radial_terms = (1 if "teleop_radial_body_velocity_extend" in L.reward_names else 0) | (2 if "teleop_radial_joint_velocity" in L.reward_names else 0)
    c.has_termination = int("termination" in L.reward_scales)
    if c.has_termination:
        c.termination_scale = float(L.reward_scales["termination"])
        c.termination_sum_col = L.sum_names.index("termination")
    c.num_sum_cols = len(L.sum_names)
    c.only_positive_rewards = int(bool(rw.only_positive_rewards))
    c.body_pos_lower_weight = float(rw.get("teleop_body_pos_lowerbody_weight", 1.0))
    c.body_pos_upper_weight = float(rw.get("teleop_body_pos_upperbody_weight", 1.0))
    c.desired_feet_air_time = float(rw.get("desired_feet_air_time", 0.0))
    c.max_contact_force = float(rw.get("locomotion_max_contact_force", 0.0))
    ats = rw.get("adaptive_tracking_sigma", {})
    c.adaptive_sigma = int(bool(ats.get("enable", False)))
    atype = ats.get("type", "origin")
    if atype not in ("origin", "mean", "scale"):           # the reference's if/elif chain leaves sigma untouched (only the EMA moves)
        raise NotImplementedError(f"adaptive_tracking_sigma.type {ats.get('type')!r}")
    c.adaptive_type = {"origin": 0, "mean": 3 if mode == 1 else 1, "scale": 2}[atype]
    c.adaptive_scale = float(ats.get("scale", 1.0))
    c.adaptive_alpha = float(ats.get("alpha", 0.0))
    c.penalty_curriculum = int(bool(rw.reward_penalty_curriculum))
    c.penalty_degree = float(rw.reward_penalty_degree)
    c.penalty_down = float(rw.reward_penalty_level_down_threshold)
    c.penalty_up = float(rw.reward_penalty_level_up_threshold)
    c.penalty_min = float(rw.reward_min_penalty_scale)
    c.penalty_max = float(rw.reward_max_penalty_scale)
    c.noise_curriculum = int(bool(ob.get("add_noise_currculum", False)))
    if c.noise_curriculum:                                   # legged_robot_base.py:1117-1126 (the up-threshold is the penalty curriculum's)
        c.noise_degree = float(ob.soft_dof_pos_curriculum_degree)
        c.noise_down = float(ob.soft_dof_pos_curriculum_level_down_threshold)
        c.noise_up = float(rw.reward_penalty_level_up_threshold)
        c.noise_min = float(ob.noise_value_min)
        c.noise_max = float(ob.noise_value_max)
    c.num_compute_average_epl = int(rw.num_compute_average_epl)
    lc = rw.reward_limit.reward_limits_curriculum
    c.soft_pos_curriculum = int(bool(lc.soft_dof_pos_curriculum))
    c.soft_vel_curriculum = int(bool(lc.soft_dof_vel_curriculum))
    c.soft_tau_curriculum = int(bool(lc.soft_torque_curriculum))
    for q, pre in enumerate(("soft_dof_pos", "soft_dof_vel", "soft_torque")):       # legged_robot_base.py:902-939 (device rule in k_env_finalize)
        if lc[pre + "_curriculum"]:
            c.soft_cur_degree[q] = float(lc[pre + "_curriculum_degree"])
            c.soft_cur_down[q] = float(lc[pre + "_curriculum_level_down_threshold"])
            c.soft_cur_up[q] = float(lc[pre + "_curriculum_level_up_threshold"])
            c.soft_cur_min[q] = float(lc[pre + "_min_limit"])
            c.soft_cur_max[q] = float(lc[pre + "_max_limit"])
    c.soft_dof_vel_limit = float(rw.reward_limit.soft_dof_vel_limit)
    c.soft_torque_limit = float(rw.reward_limit.soft_torque_limit)


def _noise_process(c, npc, dt):
    """obs.noise_process: the OU process on the IMU observations.  True when it runs."""
    if npc is None or not npc.get("enable", False):
        return False
    # legged_robot_base.py:122-129 + utils/noise_tool.py: only OUProcess defines reset_part, which _reset_tasks_callback calls on every
    # reset (:593-597); the other types raise NotImplementedError there on the first reset, so the reference cannot train with them
    if npc.get("type") != "ou":
        raise NotImplementedError(f"obs.noise_process.type {npc.get('type')!r}: only 'ou' can run in the reference's env (WhiteNoise, EmptyNoise "
                                  "and PinkNoise define no reset_part, which the env calls on the first reset; utils/noise_tool.py)")
    kw = npc.get("kwargs", {})
    mu, sigma, theta = float(kw.mu), float(kw.sigma), float(kw.theta)
    if not theta > 0.0:
        raise ValueError(f"obs.noise_process.kwargs.theta must be > 0 (stationary std sigma / sqrt(2 theta)), got {theta}")
    c.noise_process = 1
    c.ou_mu, c.ou_theta, c.ou_sigma = mu, theta, sigma
    c.ou_sqrt_dt, c.ou_sqrt_2theta = float(np.sqrt(dt)), float(np.sqrt(2 * theta))
    c.ou_scale_rpy, c.ou_scale_ang_vel = float(npc.scale.rpy), float(npc.scale.base_ang_vel)
    return True


def _materialise(c, L, maps, runs, image, roles, helper_runs, device):
    """the maps, their runs, the compact image and the roles into device tensors and the struct: the only step that touches the device"""
    c.num_groups = len(maps)
    L.group_names = [m[0] for m in maps]
    L.group_roles = roles
    lds_off = 0
    for i, (_, dst, src, scale, noise, clip, pitch) in enumerate(maps):
        tensors = (torch.tensor(dst, dtype=torch.int32, device=device), torch.tensor(src, dtype=torch.int32, device=device),
                   torch.tensor(scale, dtype=torch.float32, device=device), torch.tensor(noise, dtype=torch.float32, device=device))
        L.map_tensors.append(tensors)
        g = c.groups[i]
        g.dim, g.clip, g.pitch, g.role = len(src), clip, pitch, roles[i]
        g.dst, g.src, g.scale, g.noise = (t.data_ptr() for t in tensors)
        g.num_runs = len(runs[i]) if runs[i] is not None else -1
        for r, (d, s, n, late, a, b) in enumerate(runs[i] or []):
            R = g.runs[r]
            R.dst, R.src, R.len, R.late, R.scale, R.noise = int(d), int(s), int(n), int(late) | (2 if (i, r) in helper_runs else 0), float(a), float(b)
            L.helper_elements += n if (i, r) in helper_runs else 0
        if image is not None:
            g.dst = None                                  # identity
            g.lds_off, g.map_words = lds_off, len(image[i])
            lds_off += len(image[i])
    c.map_lds_words = lds_off
    if image is not None:
        L.map_image = torch.from_numpy(np.concatenate(image).view(np.int32).copy()).to(device)
        assert L.map_image.numel() == lds_off
        c.map_image = L.map_image.data_ptr()


def _initial_globals(rw, ec, ob, dof_far_thr):
    """the PBHC_G_* globals an env starts from (float64; the env uploads them)"""
    g = np.zeros(K["PBHC_NUM_GLOBALS"], dtype=np.float64)
    for i, key in enumerate(SIGMA_KEYS):
        sigma = float(rw.reward_tracking_sigma.get(key, 1.0)) if "reward_tracking_sigma" in rw else 1.0
        g[K["PBHC_G_SIGMA"] + i] = sigma
        g[K["PBHC_G_EMA"] + i] = sigma
    g[K["PBHC_G_PENALTY_SCALE"]] = float(rw.reward_initial_penalty_scale) if rw.reward_penalty_curriculum else 1.0
    g[K["PBHC_G_AVG_EP_LEN"]] = 0.0
    tc = ec.termination_curriculum
    g[K["PBHC_G_MOTION_FAR_THR"]] = float(tc.terminate_when_motion_far_initial_threshold
                                           if (ec.termination.terminate_when_motion_far and tc.terminate_when_motion_far_curriculum)
                                           else ec.termination_scales.termination_motion_far_threshold)
    g[K["PBHC_G_DOF_FAR_THR"]] = dof_far_thr
    lc = rw.reward_limit.reward_limits_curriculum
    g[K["PBHC_G_SOFT_POS_VAL"]] = float(lc.soft_dof_pos_initial_limit)
    g[K["PBHC_G_SOFT_VEL_VAL"]] = float(lc.soft_dof_vel_initial_limit)
    g[K["PBHC_G_SOFT_TAU_VAL"]] = float(lc.soft_torque_initial_limit)
    g[K["PBHC_G_NOISE_CURRICULUM"]] = float(ob.noise_initial_value) if ob.get("add_noise_currculum", False) else 1.0
    return g


RECORD_KEYS = ("root_trans_offset", "pose_aa", "dof", "root_rot", "actor_obs", "action", "terminate", "root_lin_vel", "root_ang_vel", "dof_vel",
               "contact_mask", "motion_times")


def record_layout(ec, L, D, Bx, mode):
    """env.config.save_motion (opt/record.yaml; motion_tracking.py:140-170): the evaluation recorder's part of the layout, or None when the
    key is absent or false.  It stays out of PbhcEnvConfig on purpose — the step kernel and its specialised builds are baked from that
    struct and must not change with the recorder.  `rows`: per key the trailing shape of one frame ([N, T, *rows[key]] buffers)."""
    if not ec.get("save_motion", False):
        return None
    if mode == 1:
        # general_tracking.py's class derives from LeggedRobotBase, not from LeggedRobotMotionTracking: it has no _init_save_motion and
        # never reads the key
        raise NotImplementedError("env.config.save_motion: LeggedRobotGeneralTracking has no recorder in the reference (only "
                                  "LeggedRobotMotionTracking records); it would be ignored there — refused here instead")
    if "dump_motion_name" in ec:
        raise NotImplementedError("env.config.dump_motion_name (motion_tracking.py:154-155 raises on it as well)")
    T = int(ec.save_total_steps)
    if T < 1:
        raise _lib.PbhcError(f"env.config.save_total_steps must be >= 1, got {T}")
    if "actor_obs" not in L.group_names[:-1]:
        raise _lib.PbhcError("env.config.save_motion records obs group 'actor_obs', which this config does not have")
    obs_dim = L.group_dims["actor_obs"]
    rows = dict(root_trans_offset=(3,), pose_aa=(Bx, 3), dof=(D,), root_rot=(4,), actor_obs=(obs_dim,), action=(D,), terminate=(),
                root_lin_vel=(3,), root_ang_vel=(3,), dof_vel=(D,), contact_mask=(2,), motion_times=())
    return dict(total_steps=T, obs_group=L.group_names.index("actor_obs"), rows=rows, save_note=ec.get("save_note", None),
                eval_timestamp=ec.get("eval_timestamp", None), ckpt_dir=ec.get("ckpt_dir", None))


CLIP_SAMPLING_DEFAULTS = dict(decay=0.5, prior_episodes=1.0, uniform_floor=0.1)       # a maintainer's choice, untrained


def clip_options(ec):
    """env.config.clip_statistics / env.config.clip_sampling -> plain dict(statistics, sampling, decay, prior_episodes, uniform_floor); both
    keys absent: everything off.  clip_sampling.enable implies clip_statistics.  Like the recorder this stays out of PbhcEnvConfig and of
    the layout: the step kernel and its specialised builds do not change with it."""
    out = dict(statistics=bool(ec.get("clip_statistics", False)), sampling=False, **CLIP_SAMPLING_DEFAULTS)
    cs = ec.get("clip_sampling", None)
    if cs is None:
        return out
    if not hasattr(cs, "get"):
        raise _lib.PbhcError(f"env.config.clip_sampling must be a mapping (enable, decay, prior_episodes, uniform_floor), got {cs!r}")
    unknown = sorted(set(cs.keys()) - {"enable", *CLIP_SAMPLING_DEFAULTS})
    if unknown:
        raise _lib.PbhcError(f"env.config.clip_sampling: unknown keys {unknown}")
    for k in CLIP_SAMPLING_DEFAULTS:
        try:
            out[k] = float(cs.get(k, CLIP_SAMPLING_DEFAULTS[k]))
        except (TypeError, ValueError):
            raise _lib.PbhcError(f"env.config.clip_sampling.{k} must be a number, got {cs.get(k)!r}") from None
    if not 0.0 <= out["decay"] <= 1.0:                     # (a NaN fails every one of these comparisons)
        raise _lib.PbhcError(f"env.config.clip_sampling.decay must lie in [0, 1], got {out['decay']}")
    if not (out["prior_episodes"] > 0.0 and out["prior_episodes"] < float("inf")):
        raise _lib.PbhcError(f"env.config.clip_sampling.prior_episodes must be > 0 and finite, got {out['prior_episodes']}")
    if not 0.0 <= out["uniform_floor"] <= 1.0:
        raise _lib.PbhcError(f"env.config.clip_sampling.uniform_floor must lie in [0, 1], got {out['uniform_floor']}")
    out["sampling"] = bool(cs.get("enable", False))
    out["statistics"] = out["statistics"] or out["sampling"]
    return out


START_SAMPLING_DEFAULTS = dict(bins=32, decay=0.9, prior_episodes=1.0, uniform_floor=0.1, lookahead_bins=4, lookahead_decay=0.8,
                               update_every_rollouts=1)                                # a maintainer's choice, untrained
_START_INT_KEYS = ("bins", "lookahead_bins", "update_every_rollouts")


def start_options(ec):
    """env.config.start_statistics / env.config.start_sampling -> plain dict(statistics, sampling, bins, decay, prior_episodes, uniform_floor,
    lookahead_bins, lookahead_decay, update_every_rollouts); both keys absent: everything off.  start_sampling.enable implies
    start_statistics.  lookahead_bins is clamped to bins only where it was NOT given (the default 4 with fewer than 4 bins); a given value
    above bins is refused.  Like clip_options this stays out of PbhcEnvConfig and of the layout."""
    out = dict(statistics=bool(ec.get("start_statistics", False)), sampling=False, **START_SAMPLING_DEFAULTS)
    cs = ec.get("start_sampling", None)
    if cs is None:
        return out
    if not hasattr(cs, "get"):
        raise _lib.PbhcError(f"env.config.start_sampling must be a mapping (enable, {', '.join(START_SAMPLING_DEFAULTS)}), got {cs!r}")
    unknown = sorted(set(cs.keys()) - {"enable", *START_SAMPLING_DEFAULTS})
    if unknown:
        raise _lib.PbhcError(f"env.config.start_sampling: unknown keys {unknown}")
    for k in START_SAMPLING_DEFAULTS:
        v = cs.get(k, START_SAMPLING_DEFAULTS[k])
        try:
            if isinstance(v, (bool, str)):
                raise TypeError
            out[k] = float(v)
        except (TypeError, ValueError):
            raise _lib.PbhcError(f"env.config.start_sampling.{k} must be a number, got {v!r}") from None
    for k in _START_INT_KEYS:
        if not abs(out[k]) < float("inf") or out[k] != int(out[k]):                        # (a NaN fails the first comparison)
            raise _lib.PbhcError(f"env.config.start_sampling.{k} must be a whole number, got {out[k]}")
        out[k] = int(out[k])
    max_bins = _lib.K["PBHC_START_MAX_BINS"]
    if not 1 <= out["bins"] <= max_bins:
        raise _lib.PbhcError(f"env.config.start_sampling.bins must lie in [1, {max_bins}], got {out['bins']}")
    if "lookahead_bins" not in cs:
        out["lookahead_bins"] = min(out["lookahead_bins"], out["bins"])
    if not 1 <= out["lookahead_bins"] <= out["bins"]:
        raise _lib.PbhcError(f"env.config.start_sampling.lookahead_bins must lie in [1, bins = {out['bins']}], got {out['lookahead_bins']}")
    if out["update_every_rollouts"] < 1:
        raise _lib.PbhcError(f"env.config.start_sampling.update_every_rollouts must be >= 1, got {out['update_every_rollouts']}")
    for k in ("decay", "uniform_floor", "lookahead_decay"):
        if not 0.0 <= out[k] <= 1.0:                       # (a NaN fails every one of these comparisons)
            raise _lib.PbhcError(f"env.config.start_sampling.{k} must lie in [0, 1], got {out[k]}")
    if not (out["prior_episodes"] > 0.0 and out["prior_episodes"] < float("inf")):
        raise _lib.PbhcError(f"env.config.start_sampling.prior_episodes must be > 0 and finite, got {out['prior_episodes']}")
    out["sampling"] = bool(cs.get("enable", False))
    out["statistics"] = out["statistics"] or out["sampling"]
    return out
