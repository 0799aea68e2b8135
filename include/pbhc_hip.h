/* pbhc_hip.h — C ABI of libpbhc_hip.so: the MI355X (gfx950) hot path of the PBHC / KungfuBot
 * humanoidverse motion-tracking agent.
 *
 * The reference (kyungminn/PBHC) is pure Python/PyTorch and has no FFI of its own; its plugin
 * boundary is three Hydra `_target_` classes (simulator / env / algo).  This library is the native
 * layer underneath our drop-in classes for those targets (pbhc_amd/...), and every entry point
 * names the reference code it replaces.  Conventions:
 *   - plain C, no torch types; all tensor arguments are raw DEVICE pointers owned by the caller
 *     (fp32 row-major unless stated; int64 / bool where the reference's tensors are);
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never synchronised;
 *   - return 0 on success, a negative PBHC_E* code otherwise; nothing throws across the boundary;
 *   - quaternions are xyzw (Isaac Gym order) except MJCF / extend_config tables, which are wxyz.
 */
#ifndef PBHC_HIP_H
#define PBHC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBHC_ABI_VERSION 16
/* The layout of PbhcEnvConfig and PbhcStepIO, the value of PbhcEnvConfig.abi_version.  It moves only when one of those two structs changes:
 * the config-specialised step kernel is compiled from the text of a filled PbhcEnvConfig, and saved training states carry its fingerprint,
 * so a change elsewhere in the ABI (version 16: PbhcFloatingParams) leaves both as they are. */
#define PBHC_ENV_CONFIG_VERSION 15

#define PBHC_OK 0
#define PBHC_EINVAL (-22)   /* bad argument / size over a compile-time maximum */
#define PBHC_ENOMEM (-12)
#define PBHC_EHIP (-5)      /* a HIP runtime call failed; see pbhc_last_error() */

#define PBHC_MAX_BODIES 36   /* bodies incl. extended (hands, head) */
#define PBHC_MAX_DEPTH 12    /* longest root->body chain */
#define PBHC_MAX_DOF 32
#define PBHC_MAX_FEET 2
#define PBHC_MAX_TERMS 32    /* reward terms (vector-reward heads - 1) */
#define PBHC_MAX_IDX 36
#define PBHC_MAX_GROUPS 8    /* observation groups + the history write-back map */
#define PBHC_MAX_QUEUE 8     /* control-delay queue depth */
#define PBHC_NUM_SIGMA 20
#define PBHC_NUM_GLOBALS 128
#define PBHC_MAX_FUTURE 32   /* future reference steps of the general-tracking observations */
#define PBHC_MAX_BODY_Z 8
#define PBHC_NUM_LOG 32

/* ---- skeleton (reference: Humanoid_Batch.__init__/from_mjcf,
 *      humanoidverse/utils/motion_lib/torch_humanoid_batch.py:44-165) ---------------------- */
typedef struct PbhcSkeleton {
  int32_t num_bodies;      /* B  : real bodies                                   */
  int32_t num_bodies_ext;  /* Bx : B + extended bodies                           */
  int32_t num_dof;         /* D  : dof d drives body d+1 (one hinge per body)    */
  int32_t max_depth;
  int32_t parent[PBHC_MAX_BODIES];
  int32_t depth[PBHC_MAX_BODIES];
  float offset[PBHC_MAX_BODIES][3];
  float local_rot_wxyz[PBHC_MAX_BODIES][4];
  float dof_axis[PBHC_MAX_DOF][3];
  /* chain[b][0..chain_len[b]-1]: the non-root bodies on the path root -> b (for an extended body: root -> its parent) */
  int32_t chain_len[PBHC_MAX_BODIES];
  int32_t chain[PBHC_MAX_BODIES][PBHC_MAX_DEPTH];
} PbhcSkeleton;

/* ---- reward term ids (reference: `_reward_<name>` in legged_robot_base.py:944-1087 and
 *      envs/motion_tracking/motion_tracking.py:1154-1328) ------------------------------------ */
enum PbhcRewardTerm {
  PBHC_R_TELEOP_CONTACT_MASK = 0,
  PBHC_R_TELEOP_MAX_JOINT_POSITION,
  PBHC_R_TELEOP_BODY_POSITION_EXTEND,
  PBHC_R_TELEOP_VR_3POINT,
  PBHC_R_TELEOP_BODY_POSITION_FEET,
  PBHC_R_TELEOP_BODY_ROTATION_EXTEND,
  PBHC_R_TELEOP_BODY_ANG_VELOCITY_EXTEND,
  PBHC_R_TELEOP_BODY_VELOCITY_EXTEND,
  PBHC_R_TELEOP_JOINT_POSITION,
  PBHC_R_TELEOP_JOINT_VELOCITY,
  PBHC_R_PENALTY_TORQUES,
  PBHC_R_PENALTY_DOF_VEL,
  PBHC_R_PENALTY_DOF_ACC,
  PBHC_R_PENALTY_ACTION_RATE,
  PBHC_R_PENALTY_ORIENTATION,
  PBHC_R_FEET_AIR_TIME,
  PBHC_R_PENALTY_FEET_CONTACT_FORCES,
  PBHC_R_PENALTY_STUMBLE,
  PBHC_R_PENALTY_SLIPPAGE,
  PBHC_R_FOOT_SLIP_PENALTY,
  PBHC_R_LIMITS_DOF_POS,
  PBHC_R_LIMITS_DOF_VEL,
  PBHC_R_LIMITS_TORQUE,
  PBHC_R_COLLISION,
  PBHC_R_ALIVE,
  /* general tracking (reference: envs/motion_tracking/general_tracking.py:1088-1279) */
  PBHC_R_TELEOP_CONTACT_MASK_V2,
  PBHC_R_TELEOP_KEY_BODY_POSITION,
  PBHC_R_TELEOP_ANCHOR_BODY_POSITION,
  PBHC_R_TELEOP_ANCHOR_BODY_ROTATION,
  PBHC_R_LOCAL_KEY_BODY_POSITION,
  PBHC_R_LOCAL_KEY_BODY_ROTATION,
  PBHC_R_KEY_BODY_VELOCITY,
  PBHC_R_KEY_BODY_ANG_VELOCITY,
  PBHC_R_TELEOP_ROOT_VEL,
  PBHC_R_TELEOP_ROOT_POSE,
  /* foot orientation terms of the base env (legged_robot_base.py:1030-1075; no shipped yaml weights them) */
  PBHC_R_FEET_HEADING_ALIGNMENT,
  PBHC_R_FEET_HEADING_ALIGNMENT_CONTACT,
  PBHC_R_PENALTY_FEET_ORI,
  PBHC_R_PENALTY_FEET_ORI_CONTACT,
  /* motion_tracking.py:78-94,1238-1244,1286-1292 (v1 env only): radial_velocity_potential of the flattened body / joint velocities,
   * exp(-(1 - cos) / 0.75) r exp(0.4 (1 - r^2.5)), r = |cur| / |ref|; no sigma.  |ref| = 0 gives NaN, as there (inf x 0) */
  PBHC_R_TELEOP_RADIAL_BODY_VELOCITY_EXTEND,
  PBHC_R_TELEOP_RADIAL_JOINT_VELOCITY,
  PBHC_R_NUM_TERMS
};

/* ---- tracking-sigma slots (reference: rewards.reward_tracking_sigma keys) ------------------ */
enum PbhcSigma {
  PBHC_S_MAX_JOINT_POS = 0, PBHC_S_UPPER_BODY_POS, PBHC_S_LOWER_BODY_POS, PBHC_S_VR_3POINT_POS,
  PBHC_S_FEET_POS, PBHC_S_BODY_ROT, PBHC_S_BODY_VEL, PBHC_S_BODY_ANG_VEL, PBHC_S_JOINT_POS, PBHC_S_JOINT_VEL,
  /* general tracking */
  PBHC_S_KEY_BODY_POS, PBHC_S_ANCHOR_BODY_POS, PBHC_S_ANCHOR_BODY_ROT, PBHC_S_LOCAL_KEY_BODY_POS, PBHC_S_LOCAL_KEY_BODY_ROT,
  PBHC_S_KEY_BODY_VEL, PBHC_S_KEY_BODY_ANG_VEL, PBHC_S_ROOT_VEL, PBHC_S_ROOT_POSE
};

/* ---- feature ids: the per-env scalars/vectors an observation key can read
 *      (reference getters `_get_obs_<key>`: legged_robot_base.py:1114-1215,
 *      motion_tracking.py:944-1015).  feat_off[id] is the offset inside the feature row. ------- */
enum PbhcFeature {
  PBHC_F_BASE_LIN_VEL = 0, PBHC_F_BASE_ANG_VEL, PBHC_F_PROJECTED_GRAVITY, PBHC_F_DOF_POS, PBHC_F_DOF_VEL,
  PBHC_F_ACTIONS, PBHC_F_REF_MOTION_PHASE, PBHC_F_DIF_LOCAL_RIGID_BODY_POS, PBHC_F_LOCAL_REF_RIGID_BODY_POS,
  PBHC_F_VR_3POINT_POS, PBHC_F_DR_BASE_COM, PBHC_F_DR_LINK_MASS, PBHC_F_DR_KP, PBHC_F_DR_KD, PBHC_F_DR_FRICTION,
  PBHC_F_DR_CTRL_DELAY, PBHC_F_RELYAW, PBHC_F_BASE_POS_Z, PBHC_F_DIF_JOINT_ANGLES, PBHC_F_DIF_JOINT_VELOCITIES,
  PBHC_F_LOCAL_REF_RIGID_BODY_VEL, PBHC_F_GLOBAL_REF_RIGID_BODY_VEL, PBHC_F_HISTORY, PBHC_F_ZERO,
  /* general tracking (getters general_tracking.py:821-954): per-body tables [Bx,3] / [Bx,6], the observation maps pick the key bodies;
   * future targets [S,dim] (general_tracking.py:500-565) */
  PBHC_F_ROLL_PITCH, PBHC_F_CONTACT_MASK, PBHC_F_DR_BASE_MASS, PBHC_F_LOCAL_BODY_POS, PBHC_F_LOCAL_BODY_ROT, PBHC_F_ANCHOR_REF_POS,
  PBHC_F_ANCHOR_REF_ROT, PBHC_F_DIF_ROOT_VELOCITY, PBHC_F_DIF_ROOT_ROT, PBHC_F_DIF_ROOT_HEIGHT, PBHC_F_REF_CONTACT_MASK,
  PBHC_F_FUT_ROOT_HEIGHT, PBHC_F_FUT_ROLL_PITCH, PBHC_F_FUT_BASE_LIN_VEL, PBHC_F_FUT_BASE_ANG_VEL, PBHC_F_FUT_DOF_POS, PBHC_F_FUT_LOCAL_KEY_POS,
  /* obs.noise_process (legged_robot_base.py:356-372): base_ang_vel_noise / projected_gravity_noise, the two root-frame quantities of
   * PBHC_F_BASE_ANG_VEL / PBHC_F_PROJECTED_GRAVITY rotated by the Ornstein-Uhlenbeck-perturbed base orientation.  (Appended, so that every
   * other id keeps its value; with the process off the two names read the clean slots instead.) */
  PBHC_F_BASE_ANG_VEL_NOISE, PBHC_F_PROJECTED_GRAVITY_NOISE,
  /* a constant one (indicator_guider); the feet rows of the contact forces [F,3] (feet_contact_force, legged_robot_base.py:1117-1118);
   * local_ref_rigid_body_pos_relyaw [Bx,3]: the reference body VELOCITIES rotated by the inverse of the relative yaw (motion_tracking.py:
   * 720-721 — not positions, whatever the name says); the v1 look-ahead joint rows [S,D] at (episode_length + 1 + i) dt + start
   * (motion_tracking.py:562-599), pre-reset values */
  PBHC_F_ONE, PBHC_F_FEET_CONTACT_FORCE, PBHC_F_REF_VEL_RELYAW, PBHC_F_FUT_REF_DOF_POS, PBHC_F_FUT_REF_DOF_VEL,
  PBHC_F_NUM
};

/* ---- device-resident globals (what the reference keeps as Python floats on the env object:
 *      adaptive sigma + EMA motion_tracking.py:1030-1048, penalty curriculum
 *      legged_robot_base.py:882-900, average_episode_length :875-879, motion-far threshold
 *      motion_tracking.py:309-317).  double[PBHC_NUM_GLOBALS]. -------------------------------- */
enum PbhcGlobal {
  PBHC_G_SIGMA = 0,                       /* [PBHC_NUM_SIGMA] */
  PBHC_G_EMA = 20,                        /* [PBHC_NUM_SIGMA] */
  PBHC_G_PENALTY_SCALE = 40,
  PBHC_G_AVG_EP_LEN = 41,
  PBHC_G_MOTION_FAR_THR = 42,
  PBHC_G_SOFT_POS_VAL = 43,
  PBHC_G_SOFT_VEL_VAL = 44,
  PBHC_G_SOFT_TAU_VAL = 45,
  PBHC_G_STEP_COUNTER = 46,
  PBHC_G_NOISE_CURRICULUM = 47,
  PBHC_G_DOF_FAR_THR = 48,                /* terminate_when_dof_far threshold (motion_tracking.py:128-130,283-292) */
  PBHC_G_DOF_FAR_HIT = 49,                /* 1.0 when k_dof_far_any found an env past the threshold in this step, else 0.0; set by the pre-pass,
                                           * read by k_env_step, cleared by k_env_finalize */
  PBHC_G_LOG = 64                         /* [PBHC_NUM_LOG] per-step log means, see PbhcLog */
};

enum PbhcLog {
  PBHC_L_UPPER_BODY_DIFF_NORM = 0, PBHC_L_LOWER_BODY_DIFF_NORM, PBHC_L_VR_3POINT_DIFF_NORM, PBHC_L_JOINT_POS_DIFF_NORM,
  PBHC_L_ACTION_CLIP_FRAC, PBHC_L_RESET_FRAC, PBHC_L_TERM_GRAVITY, PBHC_L_TERM_MOTION_FAR, PBHC_L_TERM_TIME_OUT,
  PBHC_L_TERM_MOTION_END, PBHC_L_END_TIME_RATIO, PBHC_L_END_TIME_RATIO_STD, PBHC_L_NUM_RESETS, PBHC_L_REW_MEAN,
  PBHC_L_KEY_BODY_DIFF_NORM, PBHC_L_LOCAL_UPPER_BODY_DIFF_NORM, PBHC_L_LOCAL_LOWER_BODY_DIFF_NORM, PBHC_L_LOCAL_VR_3POINT_DIFF_NORM,
  PBHC_L_LOCAL_KEY_BODY_DIFF_NORM, PBHC_L_TERM_REF_POS_Z, PBHC_L_TERM_REF_ORI, PBHC_L_TERM_BODY_Z,
  PBHC_L_TERM_CONTACT, PBHC_L_TERM_LOW_HEIGHT,
  PBHC_L_TERM_DOF_POS_LIMIT, PBHC_L_TERM_DOF_VEL_LIMIT, PBHC_L_TERM_TORQUE_LIMIT,
  PBHC_L_TERM_DOF_FAR, PBHC_L_DOF_FAR_THR,  /* terminate_by_dof_far; the threshold this step's termination test used */
  PBHC_L_NUM
};

/* ---- one output map: out[n][j] = clip((feat[src[j]] + U(-1,1)*noise[j]) * scale[j]) --------
 * (reference: helpers.parse_observation helpers.py:128-152 + sorted-key concat
 *  legged_robot_base.py:787-793 + clip :326-328; group PBHC_MAX_GROUPS-1 is conventionally the
 *  history write-back, history_handler.py:40-44, not clipped) */
/* The same map as RUNS: `len` consecutive output elements dst.. read `len` consecutive feature words src.. with one scale and one noise
 * scale (an observation key is a run; adjacent keys with equal scales merge).  The config-specialised step kernel (pbhc_env_step_spec.hip)
 * unrolls the run list into straight-line code — per element one LDS read at an immediate offset, the scale as a literal, one store —
 * where the generic kernel walks the per-element map. */
#define PBHC_MAX_RUNS 96
typedef struct PbhcObsRun {
  int32_t dst, src, len;
  int32_t late;              /* 1: reads a post-reset feature (written after the reset phase for a terminated env) */
  float scale, noise;
} PbhcObsRun;

typedef struct PbhcOutMap {
  int32_t dim;               /* number of elements this map writes */
  int32_t clip;              /* 1: clip to +-clip_observations */
  int32_t pitch;             /* floats per env row of the output tensor */
  int32_t role;              /* which half of a k_env_step workgroup writes this row: 0 = the dynamics waves (after their reward phase),
                              * 1 = the reference / observation waves; balanced by row width on the host */
  const int32_t* dst;        /* device [dim] position inside the row, or NULL = identity */
  const int32_t* src;        /* device [dim] index into the feature row */
  const float* scale;        /* device [dim] */
  const float* noise;        /* device [dim] noise scale (0 = none) */
  /* compact form (PbhcEnvConfig.map_image): word offset and size of this group's block
   * [seg_scale 16 floats][seg_noise 16 floats][nn_early][nn_late][n_early][n_late][u16 pair index x (n_early + n_late), padded to a word]
   * [noisy entries: j | word[j] << 16, early then late][u16 word[j] x dim, padded to a pair], word[j] = src[j] | seg[j] << 12.
   * A row is written in element pairs (2p, 2p+1): "late" pairs read a post-reset feature, a pair holding a noisy element is in neither
   * list (both of its elements are noise entries) */
  int32_t lds_off;
  int32_t map_words;
  int32_t num_runs;          /* runs[0..num_runs) cover the row exactly once; -1: too many runs for the table (the specialised kernel then
                              * walks the per-element map like the generic one) */
  PbhcObsRun runs[PBHC_MAX_RUNS];
} PbhcOutMap;
#define PBHC_MAX_SEGS 16

/* ---- static configuration of the env (tracking_mode 0: LeggedRobotMotionTracking, 1: LeggedRobotGeneralTracking) -----
 * Filled by the host from the reference's YAML config tree (same keys); copied to the device by
 * pbhc_env_create. */
typedef struct PbhcEnvConfig {
  int32_t abi_version;                      /* PBHC_ENV_CONFIG_VERSION */
  int32_t num_envs;
  PbhcSkeleton skel;
  /* extended bodies: skel entries B..Bx-1 (parent, offset, local_rot) */
  /* timing (base_task.py:37-39) */
  float dt;
  float max_episode_length;
  /* control (legged_robot_base.py:795-838): control_type 0 "P" (position targets), 1 "V" (velocity targets: kp (a - qd) - kd (qd - last_qd) / sim_dt),
   * 2 "T" (scaled actions are the torques), :809-817; sim_dt = 1 / simulator fps (base_task.py:34) */
  int32_t control_type;
  float sim_dt;
  int32_t foot_ori_terms;                    /* 1: a feet_heading_alignment* / penalty_feet_ori* term is configured (per-foot heading and tilt are computed) */
  float p_gains[PBHC_MAX_DOF], d_gains[PBHC_MAX_DOF], action_scale[PBHC_MAX_DOF], default_dof_pos[PBHC_MAX_DOF];
  float torque_limits[PBHC_MAX_DOF], dof_vel_limits[PBHC_MAX_DOF];
  float hard_dof_pos_limits[PBHC_MAX_DOF][2], soft_dof_pos_limits[PBHC_MAX_DOF][2];
  float action_clip_value;
  int32_t clip_torques, randomize_torque_rfi, use_rao, randomize_ctrl_delay, queue_len;
  float rfi_lim;
  /* domain randomisation ranges used on reset (legged_robot_base.py:599-635) */
  int32_t randomize_pd_gain, randomize_rfi_lim;
  /* domain_rand.randomize_default_dof_pos (legged_robot_base.py:632-635): at every reset default_dof_pos[env] = raw default + U(dof_pos_range);
   * needs PbhcStepIO.default_dof_pos (the per-env defaults, read by the torques and the dof_pos observation) */
  int32_t randomize_default_dof_pos;
  float dof_pos_range[2];
  float kp_range[2], kd_range[2], rfi_lim_range[2], rao_lim;
  int32_t ctrl_delay_range[2];
  /* body index sets (base_task.py:169-205, motion_tracking.py:203-232) */
  int32_t num_feet, feet[PBHC_MAX_FEET];
  int32_t num_penalised, penalised[PBHC_MAX_IDX];
  int32_t num_upper, upper[PBHC_MAX_IDX];
  int32_t num_lower, lower[PBHC_MAX_IDX];
  int32_t num_track, track[PBHC_MAX_IDX];
  int32_t body_flags[PBHC_MAX_BODIES];       /* bit0 upper, bit1 lower, bit2 tracked(vr 3-point), bit3 foot, bit4 key body, bit5 body_z list */
  int32_t track_slot[PBHC_MAX_BODIES];       /* position of the body inside `track`, or -1 */
  /* termination (legged_robot_base.py:408-489, motion_tracking.py:330-357) */
  int32_t terminate_by_gravity, terminate_when_motion_far, terminate_when_motion_end, motion_far_curriculum;
  float termination_gravity;
  float motion_far_degree, motion_far_down, motion_far_up, motion_far_min, motion_far_max;
  /* rewards (legged_robot_base.py:167-233,715-761) */
  int32_t num_terms;                         /* columns 0..num_terms-1; rew_buf has num_terms+1 columns if use_vec_reward */
  int32_t use_vec_reward, num_rew_cols;
  int32_t term_id[PBHC_MAX_TERMS];
  float term_scale[PBHC_MAX_TERMS];          /* reward_scales[name] * dt */
  int32_t term_penalty[PBHC_MAX_TERMS];      /* in reward_penalty_reward_names and curriculum on */
  int32_t term_sum_col[PBHC_MAX_TERMS];      /* column in episode_sums */
  int32_t term_src[PBHC_MAX_TERMS];          /* filled by pbhc_env_create (kernel-internal slot of the term's raw value, or -1) */
  int32_t sum_col_term[32];                  /* filled by pbhc_env_create: the term that accumulates into episode_sums column i, or -1 */
  int32_t has_termination, termination_sum_col, only_positive_rewards, num_sum_cols;
  float termination_scale;
  float body_pos_lower_weight, body_pos_upper_weight, desired_feet_air_time, max_contact_force;
  int32_t adaptive_sigma;                    /* rewards.adaptive_tracking_sigma.enable */
  int32_t adaptive_type;                     /* 0 "origin" (min(ema, sigma)), 1 "mean" (v1: (min+ema)/2 motion_tracking.py:1040-1045; v2: ema
                                                general_tracking.py:988-989), 2 "scale" (min(ema*scale, sigma)) */
  float adaptive_scale;
  int32_t sigma_active[PBHC_NUM_SIGMA];      /* 1 if a configured reward term updates this sigma */
  float adaptive_alpha;
  int32_t penalty_curriculum;
  float penalty_degree, penalty_down, penalty_up, penalty_min, penalty_max;
  /* obs.add_noise_currculum (legged_robot_base.py:591-592,1117-1126): PBHC_G_NOISE_CURRICULUM scales every observation noise amplitude and
   * moves by (1 -/+ degree) when the average episode length is below `noise_down` / above `noise_up` (the reference reads the latter from
   * rewards.reward_penalty_level_up_threshold), clipped to [noise_min, noise_max] */
  int32_t noise_curriculum;
  float noise_degree, noise_down, noise_up, noise_min, noise_max;
  int32_t num_compute_average_epl;
  int32_t soft_pos_curriculum, soft_vel_curriculum, soft_tau_curriculum;
  /* rewards.reward_limit.reward_limits_curriculum (legged_robot_base.py:902-939), [0] dof_pos, [1] dof_vel, [2] torque: at every step that
   * resets an env the value PBHC_G_SOFT_{POS,VEL,TAU}_VAL moves by (1 +/- degree) when the average episode length is below `down` / above `up`
   * — the limits WIDEN while episodes are short — and is clipped to [min, max] (the shipped yamls have min == max: a constant) */
  float soft_cur_degree[3], soft_cur_down[3], soft_cur_up[3], soft_cur_min[3], soft_cur_max[3];
  float soft_dof_vel_limit, soft_torque_limit;
  float max_episode_length_s;
  /* observations */
  float clip_observations;
  int32_t feat_off[PBHC_F_NUM];              /* features no observation reads share one scratch region at the end of the row */
  int32_t feat_dim;
  int32_t hist_dim;                          /* floats of history state per env */
  int32_t num_groups;
  PbhcOutMap groups[PBHC_MAX_GROUPS];
  /* compact observation maps, staged in LDS once per workgroup when they fit without costing occupancy (requires identity dst,
   * feat_dim <= 4096 and at most PBHC_MAX_SEGS distinct (scale, noise) pairs per group): the concatenated group blocks */
  int32_t map_lds_words;                     /* 0: none */
  int32_t pad3_;
  const uint32_t* map_image;                 /* device [map_lds_words] */
  int32_t has_contact_mask;
  float ref_init_yaw;
  int32_t dr_link_mass_dim;
  /* general tracking (general_tracking.py:86-98,226-262,500-507) */
  int32_t tracking_mode;
  int32_t num_key, key[PBHC_MAX_IDX];        /* robot.key_bodies as indices into the extended body list */
  int32_t key_slot[PBHC_MAX_BODIES];         /* position of the body inside `key`, or -1 */
  int32_t anchor_index;                      /* find_rigid_body_indice(anchor_link) + 1, sic */
  int32_t future_num_steps, future_steps[PBHC_MAX_FUTURE];   /* linspace(1, future_max_steps, future_num_steps) as long */
  int32_t terminate_by_ref_pos_z, terminate_by_ref_ori, terminate_by_body_z;
  float ref_pos_z_threshold, ref_ori_threshold, body_z_threshold;
  /* legged_robot_base.py:434-444: any |contact force| > 1 N on robot.terminate_after_contacts_on bodies; root height below a minimum */
  int32_t terminate_by_contact, terminate_by_low_height;
  int32_t num_term_contact, term_contact[PBHC_MAX_IDX];
  float termination_min_base_height;
  /* legged_robot_base.py:449-479: with probability term_close_prob[g] PER STEP (one draw for all envs) an env terminates when any joint is beyond
   * its termination position limit (isaacgym.py:387-388), |dof_vel| > dof_vel_limits * term_close_vel_scale, |torque| > torque_limits * term_close_tau_scale */
  int32_t terminate_close_pos, terminate_close_vel, terminate_close_tau;
  float term_close_prob[3];
  float dof_pos_limits_termination[PBHC_MAX_DOF][2];
  float term_close_vel_scale, term_close_tau_scale;
  /* termination.terminate_when_dof_far (motion_tracking.py:343-349, v1 only): EVERY env resets in a step where any env's
   * |ref dof_pos - dof_pos| exceeds PBHC_G_DOF_FAR_THR (a batch-global decision: the pre-pass k_dof_far_any, launched before k_env_step).
   * termination_curriculum.terminate_when_dof_far_curriculum (:283-292): the threshold moves by (1 +/- degree) against the average episode
   * length at every step that resets an env, clipped to [min, max] */
  int32_t terminate_when_dof_far, dof_far_curriculum;
  float dof_far_degree, dof_far_down, dof_far_up, dof_far_min, dof_far_max;
  /* noise on the reset state (motion_tracking.py:470-545, general_tracking.py:405-485), init_noise_scale.* x noise_to_initial_level folded in:
   * root position / linear / angular velocity + N(0,1) x scale, root rotation <- small_random_quaternion(max angle rn_root_rot) (x) rotation,
   * dof position / velocity + N(0,1) x scale (tracking_mode 1: + U[0,1) x scale, as the reference's rand_like).  reset_noise = 0: no draws */
  int32_t reset_noise;
  float rn_root_pos, rn_root_rot, rn_root_vel, rn_root_ang_vel, rn_dof_pos, rn_dof_vel;
  /* obs.noise_process, type ou (utils/noise_tool.py OUProcess; legged_robot_base.py:122-129,356-372,593-597): a per-env state x [6]
   * (PbhcStepIO.ou_state) stepped once per control step before termination, x += theta (mu - x) dt + sigma sqrt(dt) N(0,1), and re-drawn
   * from its stationary law mu + sigma / sqrt(2 theta) N(0,1) for the envs that reset (after the step's features: the redraw first shows in
   * the next step).  x[0:3] x ou_scale_rpy x pi / 180 perturb the base's euler angles, x[3:6] x ou_scale_ang_vel the
   * world-frame angular velocity, of the two PBHC_F_*_NOISE features.  dt is the control dt; ou_sqrt_dt = sqrt(dt), ou_sqrt_2theta =
   * sqrt(2 theta) as the reference's numpy scalars (float32).  noise_process = 0: no state, no draws */
  int32_t noise_process;
  float ou_mu, ou_theta, ou_sigma, ou_sqrt_dt, ou_sqrt_2theta, ou_scale_rpy, ou_scale_ang_vel;
  /* domain_rand.parallel_serial_pd (legged_robot_base.py:607-613): at every episodic DR of an env, after the randomize_pd_gain draws, the
   * gain scales of the listed joints are MULTIPLIED by U(ps_pd_ratio) (kp, then kd; they compound across episodes when randomize_pd_gain is
   * off).  domain_rand.parallel_serial_tau (:621-623, 822-829): at every episodic DR rao_scale of the listed joints += ps_tau_rao_lim N(0,1)
   * (accumulating; it reaches the torque only through use_rao), and every control step torque += ps_tau_rfi_lim x torque_limit x N(0,1) on
   * them, after the RFI term, before rao and clipping.  ps_*_slot[d]: column of dof d in the joint_idx list (the [N,J] draws), -1 if absent */
  int32_t ps_pd, ps_pd_num, ps_pd_slot[PBHC_MAX_DOF];
  float ps_pd_ratio[2];
  int32_t ps_tau, ps_tau_num, ps_tau_slot[PBHC_MAX_DOF];
  float ps_tau_rao_lim, ps_tau_rfi_lim;
  /* which of the optional features an observation reads (the step computes no other): bit 0 PBHC_F_ONE, bit 1 PBHC_F_FEET_CONTACT_FORCE,
   * bit 2 PBHC_F_REF_VEL_RELYAW (needs PBHC_F_RELYAW in the row).  future_ref_steps: obs.future_ref_steps when PBHC_F_FUT_REF_DOF_* are
   * read, else 0 (tracking_mode 0).  radial_terms: bit 0 / bit 1 the body / joint radial-velocity term is configured. */
  int32_t obs_extra, future_ref_steps, radial_terms, pad5_;
  int32_t pad2_;
  uint64_t seed;
} PbhcEnvConfig;

/* ---- reference-motion table (reference: MotionLibBase.load_motions / get_motion_state,
 *      motion_lib_base.py:123-259,261-391).  One packed row per frame:
 *      [dof_pos D | dof_vel D | contact 2 | pos Bx*3 | rot Bx*4 | vel Bx*3 | ang Bx*3]. ---------- */
typedef struct PbhcMotionTable {
  const float* frames;          /* device [total_frames, row] */
  int32_t row;                  /* 2D + 2 + 13 Bx */
  int32_t num_motions;
  const int32_t* length_starts; /* device [M] first row of each clip   */
  const int32_t* num_frames;    /* device [M]                           */
  const float* motion_dt;       /* device [M] 1/fps                     */
  const float* motion_len;      /* device [M] (F-1)/fps                 */
  /* when num_motions == 1 the clip's meta also travels by value (saves a dependent load in the step kernel) */
  int32_t single_num_frames;
  float single_dt, single_len;
} PbhcMotionTable;

/* ---- per-step tensors of the fused env step ------------------------------------------------ */
/* Extent, alignment and pitch of the caller-owned buffers (N = PbhcEnvConfig.num_envs, D dofs, B bodies, Bx bodies with the extended ones,
 * Q = queue_len, F = num_feet, T = num_frames), from the loads and stores the kernels issue (k_env_step generic and specialised,
 * k_dof_far_any, k_env_finalize; held by tests/test_gpu_step_memory.py, table in DESIGN.md "Memory contract of the per-step entries"):
 *   extent     exactly the shape given at the field, dense (row pitch = row length) except `obs[g]` and `hist`.  Nothing is read or written
 *              outside it: the last workgroup of a batch that is no multiple of the 4 envs of a workgroup clamps its loads onto env N - 1
 *              and stores nothing for the missing envs; a frame is read at index `frame_index` (or *frame_cursor) of [0, T) only.
 *   alignment  float, int32 and uint8 buffers: the element's own (4, 4, 1 bytes) — a base 4, 8 or 12 bytes behind a 16-byte boundary is
 *              fine.  int64 buffers (episode_length_buf, last_episode_length_buf, reset_buf, action_delay_idx, motion_ids, ovr_delay):
 *              8 bytes, else PBHC_EINVAL.  `hist` under a specialised kernel that reads history rows 16 bytes per lane: 16 bytes, else
 *              PBHC_EINVAL.  totals_out (and the `totals` of pbhc_env_finalize), doubles: 8 bytes, else PBHC_EINVAL.
 *   pitch      obs[g]: obs_pitch[g] floats between rows, 0 = dense, at least PbhcEnvConfig.groups[g].pitch (= the group's dimension),
 *              N x pitch < 2^30; columns [0, dim) of a row are written.  The generic kernel stores elements in PAIRS when the pitch is even
 *              and the base 8-byte aligned: with an odd dim and pitch > dim the float in column `dim` is written too (the only padding
 *              float any entry touches; callers that pad rows own their padding).  Any other pitch / base: element by element.
 *              hist (and obs[num_groups - 1], its write-back): hist_pitch floats, 0 = dense, >= hist_dim; under such a specialised
 *              kernel a multiple of 4 and >= hist_dim rounded up to 4 — the last 16-byte read of a row may take in up to 3 floats of its
 *              padding, whose values reach no result.
 *   NULL       where the field says "may be NULL"; the ovr_* draws and u_rfi: NULL -> in-kernel Philox.
 * Index-typed inputs are trusted, not clamped: motion_ids in [0, num_motions), action_delay_idx / ovr_delay in [0, Q), *frame_cursor and
 * frame_index < T. */
typedef struct PbhcStepIO {
  /* inputs */
  const float* actions_in;        /* [N,D]   policy actions                                    */
  /* replay window of the sim-stub: frame k = frame_cursor[0] % num_frames lands this step; the cursor lives on the device and is
   * advanced by the step itself (pointer bump without a host round trip, so a rollout can be captured in a hipGraph). */
  const float* frame_root;        /* [T,N,13]                                                  */
  const float* frame_dof_pos;     /* [T,N,D]                                                   */
  const float* frame_dof_vel;     /* [T,N,D]                                                   */
  const float* frame_contact;     /* [T,N,B,3] net contact forces                              */
  int32_t* frame_cursor;          /* device int32[1]                                           */
  int32_t num_frames;             /* T                                                         */
  int32_t frame_index;            /* >= 0: the host names the frame (saves the kernel a dependent load; the device cursor is still
                                     advanced); < 0: read the device cursor (hipGraph replay)  */
  /* optional injected random draws (NULL -> in-kernel Philox) */
  const float* u_rfi;             /* [N,D] uniforms of the torque RFI noise                    */
  const float* ovr_start_time;    /* [N]   values consumed by resetting envs                   */
  const float* ovr_kp; const float* ovr_kd; const float* ovr_rfi_lim; const float* ovr_rao; /* [N,D] */
  const float* ovr_dof_pos_bias;                                                          /* [N,D] the U(dof_pos_range) draw of randomize_default_dof_pos */
  const int64_t* ovr_delay;       /* [N]                                                       */
  const float* ovr_gate_u;        /* [3]   the per-step uniforms of the terminate_when_close_to_* gates (pos, vel, torque) */
  /* reset-state noise draws (PbhcEnvConfig.reset_noise), in the reference's call order: ovr_reset_root [N,13] = randn pos (3), randn axis (3),
   * rand angle (1), randn lin vel (3), randn ang vel (3); ovr_reset_dof_pos / ovr_reset_dof_vel [N,D] = randn (tracking_mode 1: rand) */
  const float* ovr_reset_root; const float* ovr_reset_dof_pos; const float* ovr_reset_dof_vel;
  /* obs.noise_process / parallel_serial_* draws, raw N(0,1) / ratios: ovr_ou_step [N,6] the OU step's normals (every env), ovr_ou_reset [N,6]
   * the stationary redraw's normals (envs that reset), ovr_ps_kp / ovr_ps_kd [N,J_pd] the U(ratio) factors, ovr_ps_rao [N,J_tau] the episodic
   * normals (envs with an episodic DR), ovr_ps_tau [N,J_tau] the per-step torque normals (every env) */
  const float* ovr_ou_step; const float* ovr_ou_reset; const float* ovr_ps_kp; const float* ovr_ps_kd; const float* ovr_ps_rao; const float* ovr_ps_tau;
  /* simulator-surface state (reference names; simulator/isaacgym/isaacgym.py:574-618) */
  float* root_states;             /* [N,13] */
  float* dof_state;               /* [N,D,2] (pos, vel) */
  float* rigid_body_state;        /* [N,B,13] pos3 rot4 vel3 ang3, may be NULL: nothing on the training path reads it — the replay stub hands NULL and
                                   * re-derives it on first access (pbhc_sim_fk of the same replay frame: the same arithmetic) */
  float* contact_forces;          /* [N,B,3], may be NULL (a copy of the replay frame's contact forces) */
  /* env state (reference names; legged_robot_base.py:39-131, motion_tracking.py:251-263) */
  float* actions; float* last_actions; float* actions_after_delay; float* action_queue; /* [N,D] x3, [N,Q,D] */
  float* last_dof_pos; float* last_dof_vel; float* torques;                              /* [N,D] */
  float* feet_air_time; float* contacts; float* contacts_filt; float* last_contacts; float* last_contacts_filt; /* [N,F] */
  float* kp_scale; float* kd_scale; float* rfi_lim_scale; float* rao_scale;              /* [N,D] */
  float* default_dof_pos;                                                                 /* [N,D] or NULL: per-env default joint angles (randomize_default_dof_pos); NULL -> PbhcEnvConfig.default_dof_pos */
  float* motion_start_times; float* motion_len; float* end_time_ratio_buf;               /* [N] */
  float* episode_sums;            /* [N,num_sum_cols] */
  float* hist;                    /* [N,hist_dim] */
  float* ou_state;                /* [N,6] Ornstein-Uhlenbeck state of obs.noise_process (read and written by the step); NULL when it is off */
  int64_t* episode_length_buf; int64_t* last_episode_length_buf; int64_t* reset_buf; int64_t* action_delay_idx; /* [N] */
  const int64_t* motion_ids;      /* [N] slot -> clip */
  uint8_t* time_out_buf;          /* [N] bool */
  const float* env_origins;       /* [N,3] */
  const float* dr_base_com; const float* dr_link_mass; const float* dr_friction;        /* [N,3] [N,L] [N,1] */
  const float* dr_base_mass;      /* [N,1] (general tracking priv_obs), may be NULL -> 1.0 */
  /* outputs */
  float* obs[PBHC_MAX_GROUPS];    /* [N,dim_g]; group num_groups-1 may alias `hist` semantics (see PbhcOutMap) */
  float* rew_buf;                 /* [N,num_rew_cols] */
  float* ref_body_pos_extend;     /* [N,Bx,3] may be NULL: extras["ref_body_pos_extend"] is read by evaluation callbacks only — the env hands NULL and */
  float* ref_body_rot_extend;     /* [N,Bx,4] may be NULL  re-derives both on first access from ref_time_out (pbhc_motion_state: the same lerp / slerp) */
  float* ref_time_out;            /* [N] may be NULL: the motion time of this step's reference lookup, (episode_length + 1) dt + start BEFORE a reset */
  float* episode_rew_out;         /* [N,num_sum_cols] episode_sums / max_episode_length_s of envs reset this step (else unchanged), may be NULL */
  /* Data-parallel runs: NULL -> the step finalizes its batch statistics itself.  Non-NULL -> device double[PBHC_NUM_TOTALS]: the step
   * only writes this shard's batch sums there (and advances the RNG counter / frame cursor); the caller sums them over ranks and calls
   * pbhc_env_finalize, so adaptive sigma, average episode length, the curricula and the logged means are those of ONE batch of
   * all ranks' envs (the reference is single-process: motion_tracking.py:1030-1048, legged_robot_base.py:875-900). */
  double* totals_out;
  /* row pitches in floats (0 = dense).  Rows padded to a multiple of 32 floats start on 128-B lines: no cache line is shared by two envs,
   * so no line is written twice by different workgroups. */
  int32_t obs_pitch[PBHC_MAX_GROUPS];
  int32_t hist_pitch;
  /* 1: re-draw the episodic domain randomisation (gain / torque-noise scales, control delay + action queue, default joint angles) of EVERY
   * env in this step, after its torques and before its observations — `_update_tasks_callback` with domain_rand.reinit_epis_rand > 0
   * (legged_robot_base.py:390-395 -> _episodic_domain_randomization(all env ids) :599-635).  Same draws as a reset's (Philox streams / ovr_*). */
  int32_t redraw_all;
  /* reserved: callers leave it 0, the library ignores it (it keeps the struct's size and the kernel-argument offsets of ABI version 11) */
  int32_t reserved0;
} PbhcStepIO;

/* The evaluation recorder (env.config.save_motion, motion_tracking.py:140-170,861-938): device-resident [N,T,...] buffers, T = total_steps =
 * save_total_steps, one frame per env and control step, each env's frames contiguous.  Not part of PbhcEnvConfig: the step kernel and its
 * specialised builds do not know the recorder exists. */
/* Contract: every buffer dense with exactly the extent given at the field, float / int32 buffers 4-byte aligned, `terminate` (int64) and the
 * PbhcStepIO int64 buffers it reads 8-byte aligned (else PBHC_EINVAL); actor_obs is read through PbhcStepIO.obs_pitch[obs_group] and
 * written dense.  A launch whose counter word 0 is < 3 or >= T + 3 stores nothing into the [N,T,...] buffers; of the counter only word 0
 * and the ticket words named below are ever written, and the ticket words are 0 again when the launch ends. */
#define PBHC_REC_SHARDS 128
#define PBHC_REC_COUNTER_WORDS 4160   /* 32 * (2 + PBHC_REC_SHARDS) */
typedef struct PbhcRecordIO {
  int32_t total_steps;            /* T */
  int32_t obs_group;              /* index of actor_obs in PbhcStepIO.obs */
  /* device int32 [PBHC_REC_COUNTER_WORDS], zeroed by the caller.  Word 0: control steps seen so far — read by every workgroup, advanced
   * (saturating at T + 3) by the one that finishes last; values 0..2 and >= T + 3 record nothing, value k writes frame k - 3 (the reference
   * drops its first three records).  Words 32 and 32 * (2 + s), s < PBHC_REC_SHARDS, each on a 128-byte line of its own: the workgroups'
   * two-level arrival ticket of the current launch (all back to 0 when the launch ends) */
  int32_t* counter;
  float* root_trans_offset;       /* [N,T,3]  root position - env origin */
  float* root_rot;                /* [N,T,4]  xyzw */
  float* root_lin_vel; float* root_ang_vel;   /* [N,T,3] */
  float* dof; float* dof_vel;     /* [N,T,D] */
  float* contact_mask;            /* [N,T,2]  contacts_filt */
  float* pose_aa;                 /* [N,T,Bx,3] row 0: rotation vector of the root quaternion (scipy as_rotvec), rows 1..D: dof_axis * dof, rest 0 */
  float* action;                  /* [N,T,D]  env.actions */
  float* actor_obs;               /* [N,T,dim of group obs_group], dense */
  int64_t* terminate;             /* [N,T]    reset_buf */
  float* motion_times;            /* [N,T]    episode_length_buf * dt + motion_start_times */
} PbhcRecordIO;

typedef struct PbhcEnv PbhcEnv;   /* opaque */

int pbhc_abi_version(void);
const char* pbhc_last_error(void);
int pbhc_sizeof_env_config(void);
int pbhc_sizeof_step_io(void);
int pbhc_sizeof_record_io(void);

/* Load-time FK + filtered velocities of one clip -> packed frame rows.
 * Replaces Humanoid_Batch.fk_batch / _compute_velocity / _compute_angular_velocity
 * (torch_humanoid_batch.py:168-290).  pose_aa [F,Bx,3], trans [F,3], contact [F,2] or NULL (device);
 * out_rows [F,row] device; scratch >= F*Bx*14 floats device. */
int pbhc_motion_build(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact,
                      int num_frames, float dt, float* out_rows, float* scratch, void* stream);

/* The same for a whole library in ONE launch set (the reference runs the FK once per env slot in a Python loop over clips,
 * motion_lib_base.py:403-472): the clips' frames concatenated — pose_aa [total_frames,Bx,3], trans [total_frames,3], contact [total_frames,2]
 * or NULL — with frame_clip [total_frames] (clip of every frame), clip_start [num_clips+1] (first frame of every clip, then the total) and
 * clip_dt [num_clips] (1 / fps), all device int32 / float.  Velocities and the Gaussian filter stop at clip boundaries.
 * out_rows [total_frames,row]; scratch >= total_frames*Bx*14 floats. */
int pbhc_motion_build_batch(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int total_frames, int num_clips,
                            const int32_t* frame_clip, const int32_t* clip_start, const float* clip_dt, float* out_rows, float* scratch, void* stream);

/* Lead-in / lead-out frames between a default pose and every clip of a library, BEFORE the build (reference: the offline step
 * robot_motion_process/motion_interpolation_pkl.py, one clip and 23 joints at a time; here any joint count, the whole library in ONE launch,
 * k_motion_extend).  default_dof: device float [D]. */
typedef struct PbhcMotionExtend {
  int32_t start_frames, end_frames;   /* frames added in front of / behind every clip; 0: nothing at that end */
  int32_t knee_modify;                /* the legs (dofs 0..5, 6..11) move one after the other, the knees (dofs 3, 9) through 1.0 rad */
  float default_height;               /* root z of the default pose */
  float default_quat_xyzw[4];         /* its root rotation: pitch and roll are used, the yaw is the clip's */
  const float* default_dof;
  float contact_fill;                 /* contact mask of a synthetic frame without knee_modify */
} PbhcMotionExtend;
/* The clips' raw arrays concatenated as for pbhc_motion_build_batch — pose_aa [total_in,Bx,3], trans [total_in,3], contact [total_in,2] or NULL
 * (then out_contact is NULL too and is not touched) — with in_start / out_start [num_clips+1] device int32: first frame of every clip in the
 * input / output (+ the totals), out_start[c+1] - out_start[c] = in_start[c+1] - in_start[c] + start_frames + end_frames, so
 * total_out = total_in + num_clips * (start_frames + end_frames).  Output frames inside a clip are copied bit for bit; the synthetic ones
 * are computed as csrc/pbhc_motion_extend.hip states.  With knee_modify: D >= 12 and frame counts N of 0 or 2 (N / 2 / 2) + 1 == N / 2. */
int pbhc_motion_extend_batch(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int total_in, int num_clips,
                             const int32_t* in_start, const int32_t* out_start, int total_out, PbhcMotionExtend params, float* out_pose_aa,
                             float* out_trans, float* out_contact, void* stream);

/* Mirrored and time-scaled copies of every clip of a library, BEFORE the extension and the build (no counterpart in the reference, which
 * ships seven clips; config key robot.motion.augmentation), the whole library in ONE launch, k_motion_augment.  A library of num_clips clips
 * becomes num_clips * num_variants clips; output clip src * num_variants + v is variant v of source clip src, v = speed index * (mirror ? 2 : 1)
 * + mirrored, speed index 0 = speed 1.0, index i > 0 = speeds[i - 1]; variant 0 is the source, bit for bit. */
#define PBHC_MAX_SPEEDS 8
typedef struct PbhcMotionAugment {
  int32_t num_variants;               /* V = (1 + num_speeds) * (mirror ? 2 : 1) */
  int32_t num_speeds;                 /* playback speeds besides 1.0, <= PBHC_MAX_SPEEDS */
  int32_t mirror;                     /* every speed also reflected across the x-z plane */
  int32_t pad;
  double speeds[PBHC_MAX_SPEEDS];     /* each in [0.25, 4]; the clip keeps its fps */
} PbhcMotionAugment;
/* Raw arrays as for pbhc_motion_extend_batch, in_start [num_clips+1], out_start [num_clips*V+1] device int32 (first frame of every clip in the
 * input / output, then the totals).  A variant of speed s of a clip of F frames has F' = floor((F - 1) / s) + 1 frames (formed in double, one
 * less if (F' - 1) s > F - 1); output frame k samples the source at x = k s: i0 = floor(x), t = x - i0; t == 0 copies frame i0 bit for bit,
 * otherwise translation and joint rows are a + t (b - a) in double rounded once, the root row is the short-way slerp of the two root rotations
 * in double, the contact mask is that of the nearer frame (i0 for t < 0.5).  The mirror, applied after the resampling: translation
 * (x, -y, z), pose_aa row b = (-x, y, -z) of row perm[b], contact columns swapped.  perm: device int32 [Bx], an involution with perm[0] = 0
 * (NULL without mirror).  total_out must lie in the range the frame-count formula allows for total_in frames in num_clips clips; an output
 * clip whose out_start entries disagree with the formula is left unwritten by the kernel. */
int pbhc_motion_augment_batch(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, const float* contact, int total_in, int num_clips,
                              const int32_t* in_start, const int32_t* out_start, int total_out, PbhcMotionAugment params, const int32_t* perm,
                              float* out_pose_aa, float* out_trans, float* out_contact, void* stream);

/* Contact masks and a stability screen for the SOURCE clips of a library, before the augmentation, the extension and the build (reference:
 * the offline steps motion_source/count_pkl_contact_mask.py foot_detect and smpl_retarget/motion_filter/utils/motion_filter.py
 * compute_com_cop / compute_diff / check_conditions, the latter restated in robot space; config keys robot.motion.contact_detection and
 * robot.motion.screening; semantics: csrc/pbhc_motion_screen.hip and DESIGN §8). */
typedef struct PbhcMotionScreen {
  int32_t foot[2];                    /* extended-body indices of the two feet: mask column 0 and 1 */
  int32_t epsilon_stab_frames;        /* N of check_conditions */
  int32_t pad;
  double vel_threshold;               /* squared displacement per FRAME below which a foot is still */
  double height_threshold;            /* foot z below which it is down */
  double epsilon_stab;                /* a frame is stable iff its distance is finite and below this */
  double cop_w, cop_k;                /* pressure weight exp(-cop_w z) above the ground, 1 - cop_k z below it */
} PbhcMotionScreen;
#define PBHC_SCREEN_REPORT 8          /* floats per clip: stable, first_dist, last_dist, max_dist, unstable_share, max_gap, 2 x reserved (0) */
/* Per-frame half: the FK of every frame of the concatenated raw arrays (pose_aa [total,Bx,3], trans [total,3], in_start [num_clips+1] device
 * int32 as for pbhc_motion_extend_batch), one launch that leaves ground[c] = the lowest real-body origin z of clip c's first frame, then
 * one wave per frame.  foot_pos [total,2,3] (NULL: no contact half; the params' foot indices are then not read) receives the world
 * positions of the two feet; dist [total] (NULL: no stability half; body_mass, body_com and ground may then be NULL) the horizontal
 * distance between the mass-weighted centre of the real bodies (body_mass [B], body_com [B,3] in the body frame) and the pressure-weighted
 * centre of their origins.  ground: device float [num_clips], scratch.  A clip whose in_start entries do not describe the input is left
 * unwritten. */
int pbhc_motion_screen_frames(const PbhcSkeleton* skel, const float* pose_aa, const float* trans, int total, int num_clips, const int32_t* in_start,
                              PbhcMotionScreen params, const float* body_mass, const float* body_com, float* ground, float* foot_pos, float* dist,
                              void* stream);
/* Per-clip half, one workgroup per clip.  mask [total,2] (with foot_pos; both NULL: no contact half): rows of the clips with derive[c] != 0
 * (device int32 [num_clips]) are written — frame 0 of a clip 1, frame f >= 1: 1 iff |p_f - p_(f-1)|^2 < vel_threshold and p_f.z <
 * height_threshold, else 0 — the rows of the others are not touched.  report [num_clips,PBHC_SCREEN_REPORT] (with dist; both NULL: no
 * stability half): stable = first and last frame stable and, if the clip has more than N frames, no two consecutive stable frames N or more
 * apart; max_gap = the largest such distance (0 with fewer than two stable frames); max_dist is +inf if a distance is not finite. */
int pbhc_motion_screen_clips(const float* foot_pos, const float* dist, int total, int num_clips, const int32_t* in_start, const int32_t* derive,
                             PbhcMotionScreen params, float* mask, float* report, void* stream);

/* Phase lookup + lerp/slerp.  Replaces MotionLibBase.get_motion_state (motion_lib_base.py:123-259).
 * ids [N] int64, times [N], offset [N,3] or NULL -> out [N,row] packed like a frame row
 * (positions include the offset).
 * Contract: all dense; float buffers 4-byte aligned, ids 8-byte aligned (else PBHC_EINVAL); ids in [0, tbl->num_motions) (trusted).  Of the
 * table only rows length_starts[id] .. length_starts[id] + num_frames[id] - 1 are read: a time at or beyond the clip's length reads its LAST
 * row twice, never the row behind it (the next clip's first row, or the end of `frames`); a negative time reads rows 0 and 1 with
 * blend 0. */
int pbhc_motion_state(const PbhcMotionTable* tbl, int num_bodies_ext, int num_dof, const int64_t* ids, const float* times,
                      const float* offset, int n, float* out, void* stream);

/* Rigid-body pose + twist from (root state, q, q-dot): what Isaac Gym's rigid-body state tensor
 * supplied in the reference (isaacgym.py:574-605).  out [N,B,13].
 * Contract: root_states [N,13] and out [N,B,13] dense; dof_pos / dof_vel: element (env, d) at float index (env * D + d) * dof_stride, i.e.
 * [N,D] dense with dof_stride 1, or the two columns of one [N,D,2] dof_state (dof_vel = dof_pos + 1) with dof_stride 2 — the last float
 * read is index (N * D - 1) * dof_stride.  4-byte alignment throughout. */
int pbhc_sim_fk(const PbhcSkeleton* skel, const float* root_states, const float* dof_pos, const float* dof_vel,
                int dof_stride, int n, float* out_body_state, void* stream);
/* Test-only: the same chain for every body INCLUDING the extended ones (motion_tracking.py:619-643), out [N,Bx,13], by method 0 — the walk
 * pbhc_sim_fk runs — or 1 — the pointer-jumping form the fused step runs for robots of <= 32 bodies (csrc/pbhc_env_step.h: fk_jump_wave).
 * dof_pos / dof_vel [N,D] dense. */
int pbhc_debug_fk(const PbhcSkeleton* skel, const float* root_states, const float* dof_pos, const float* dof_vel, int n, int method,
                  float* out_body_state_ext, void* stream);

/* Env object: owns the device copy of the config, the globals and the reduction scratch. */
/* `globals`: caller-owned device double[PBHC_NUM_GLOBALS] (see enum PbhcGlobal), initialised by the caller. */
int pbhc_env_create(const PbhcEnvConfig* cfg, const PbhcMotionTable* tbl, double* globals, PbhcEnv** out);
void pbhc_env_destroy(PbhcEnv* env);

/* Config-specialised step kernel (new; nothing of the reference to match — its counterpart there is TorchScript specialising the
 * rotation helpers per call site, isaac_utils/rotations.py `@torch.jit.script`).  k_env_step reads ~100 config scalars; compiled with the
 * env's config as compile-time constants (csrc/pbhc_env_step_spec.hip, -DPBHC_STATIC_CFG) the same source is 40 % shorter and ~19 % faster.
 *   pbhc_env_get_config          the config as pbhc_env_create finalised it: the text a specialised build is generated from
 *   pbhc_env_attach_specialised  load `so_path` (a build of pbhc_env_step_spec.hip) and use its kernel for this env's steps; refused with
 *                                PBHC_EINVAL unless the config baked into the object equals this env's member by member (run-time members —
 *                                pointers, num_envs, seed, ref_init_yaw — excepted: the kernel reads those from the env).  NULL detaches.
 *   pbhc_env_is_specialised      1 while a specialised kernel is attached
 *   pbhc_env_config_finalize     the same finalisation without an env or a device (validation + derived members): lets a build step
 *                                generate the specialised kernels of known configs ahead of time */
int pbhc_env_get_config(PbhcEnv* env, PbhcEnvConfig* out);
int pbhc_env_config_finalize(const PbhcEnvConfig* cfg, PbhcEnvConfig* out);
/* Dynamic LDS (bytes) of one k_env_step workgroup — 4 envs: state, bodies, reference frame, feature row, skeleton constants, compact
 * observation maps — for this config; < 0: -(error code).  160 KB per CU / this = resident workgroups per CU (no reference counterpart). */
int pbhc_env_config_lds_bytes(const PbhcEnvConfig* cfg);
int pbhc_env_attach_specialised(PbhcEnv* env, const char* so_path);
int pbhc_env_is_specialised(PbhcEnv* env);
/* One LeggedRobotBase.step (legged_robot_base.py:239-338) for all envs: 2 launches (step + finalize). */
int pbhc_env_step(PbhcEnv* env, const PbhcStepIO* io, void* stream);
/* The same step as its two launches, for a caller that keeps the one-workgroup reduction off its critical chain (the rollout of
 * mh_ppo.py:270-342 is step -> policy forward -> step: only the fused launch has to precede the policy forward).  `launch` = the fused
 * per-env kernel on `stream`; `finish` = the reduction of its partial sums into the globals (or into io->totals_out) on a stream of the
 * caller's choice, ordered by the caller after the launch and before the next launch / pbhc_policy_sample (which reads the step counter). */
int pbhc_env_step_launch(PbhcEnv* env, const PbhcStepIO* io, void* stream);
int pbhc_env_step_finish(PbhcEnv* env, const PbhcStepIO* io, void* stream);
/* One frame of the evaluation recorder: k_record_motion on `stream`, to be called right after pbhc_env_step / pbhc_env_step_launch of the same
 * `io` on the same stream (it reads the post-reset state that step left: root_states, dof_state, actions, contacts_filt, reset_buf,
 * episode_length_buf, motion_start_times and the observation row obs[rec->obs_group]).  A plain launch with no host-side state: a stream
 * capture may record it, the frame index lives in rec->counter. */
int pbhc_record_motion(PbhcEnv* env, const PbhcStepIO* io, const PbhcRecordIO* rec, void* stream);
/* Per-clip episode statistics and failure-weighted clip sampling (env.config.clip_statistics / clip_sampling; pbhc_clip_stats.hip).  Raw
 * device pointers, no PbhcEnv: the step kernel does not know about them.  NULL or sizes < 1 return PBHC_EINVAL without touching the GPU.
 * pbhc_clip_stats: k_clip_stats on `stream`, to follow the step that left reset_buf, time_out_buf (u8), end_time_ratio_buf and
 *   last_episode_length_buf [N].  For every env with reset_buf != 0 and slot_clip[env] in [0, M): window[slot_clip[env]] += (1, time_out == 0,
 *   llrintf(end_time_ratio * 2^24), last_episode_length); window [M,4] int64.  Integer atomics only: the table does not depend on arrival
 *   order.  A plain launch with no host-side state: a stream capture may record it.
 * pbhc_clip_sampling_update: one workgroup.  Per clip, in double, with the window's episodes e and failures f:
 *   E <- f32(decay E + e) (sampling_history), F <- f32(decay F + f) (termination_history), r = (F + prior) / (E + prior),
 *   success_rate = E > 0 ? 1 - F / E : 0, sampling_prob = f32((1 - floor) r / sum(r) + floor / M); cdf [M] double = the inclusive prefix sum
 *   of double(sampling_prob); the window is cleared.  decay and uniform_floor in [0, 1], prior_episodes > 0, else PBHC_EINVAL.
 * pbhc_clip_sample_slots: slot j of slot_clip [N] <- the first i with cdf[i] > u * cdf[M-1] (clamped to M-1),
 *   u = u01(philox4x32(seed; j, draw_index, 20, 0)[0]): a multinomial draw with replacement that never returns a clip of probability 0.
 *   cdf [M] double: as pbhc_clip_sampling_update left it (any non-decreasing prefix sum of non-negative weights). */
int pbhc_clip_stats(const int64_t* reset_buf, const uint8_t* time_out_buf, const float* end_time_ratio_buf, const int64_t* last_episode_length_buf,
                    const int64_t* slot_clip, int N, int M, int64_t* window, void* stream);
int pbhc_clip_sampling_update(int64_t* window, float* sampling_history, float* termination_history, float* success_rate, float* sampling_prob,
                              double* cdf, int M, double decay, double prior_episodes, double uniform_floor, void* stream);
int pbhc_clip_sample_slots(const double* cdf, int M, uint64_t seed, uint32_t draw_index, int64_t* slot_clip, int N, void* stream);
/* Failure-weighted start-time sampling (env.config.start_statistics / start_sampling; pbhc_start_sampling.hip): K phase bins of equal width
 * per clip.  Raw device pointers, no PbhcEnv: the step kernel does not know about them, it reads start_time through
 * PbhcStepIO.ovr_start_time.  NULL (where not allowed below), N < 1, M < 1, K outside [1, PBHC_START_MAX_BINS] or a bad rule parameter
 * return PBHC_EINVAL without touching the GPU.
 * pbhc_start_stats: k_start_stats on `stream`, to follow the step that left reset_buf, time_out_buf (u8), end_time_ratio_buf and
 *   last_episode_length_buf [N]; clip_len [M]: the table's motion_len; dt > 0: the control step.  For every env with reset_buf != 0 and
 *   c = slot_clip[env] in [0, M), in double: pe = end_time_ratio, ps = pe - (last_episode_length * dt) / clip_len[c],
 *   e = clamp(floor(pe K), 0, K-1), s = clamp(floor(ps K), 0, e); a non-finite phase adds nothing.  window[c][s][0] += 1,
 *   window[c][e+1][0] -= 1 if e+1 < K (the prefix sum over the bins = episodes that visited each bin), window[c][e][1] += (time_out == 0).
 *   window [M,K,2] int64.  Integer atomics only: the table does not depend on arrival order.  A plain launch with no host-side state.
 * pbhc_start_sampling_update: one workgroup per clip.  Per bin b, in double, v_b = the prefix sum of column 0, f_b = column 1:
 *   V_b <- f32(decay V_b + v_b), F_b <- f32(decay F_b + f_b) (hist_V, hist_F [M,K] float32), r_b = (F_b + prior) / (V_b + prior),
 *   w_b = sum_{u=0}^{H-1} lambda^u r_{b+u} over b+u <= K-1 (H = lookahead_bins, lambda = lookahead_decay; no wrap-around),
 *   prob[c][b] = f32((1 - floor) w_b / sum_b w_b + floor / K); cdf [M,K] double = per clip the inclusive prefix sum of double(prob); the
 *   window is cleared.  decay, uniform_floor, lookahead_decay in [0, 1], prior_episodes > 0, 1 <= lookahead_bins <= K.
 * pbhc_start_draw: k_start_draw on `stream`; env j if reset_buf is NULL or reset_buf[j] != 0, with c = slot_clip[j] in [0, M):
 *   (u1, u2) = u01 of words 0 and 1 of philox4x32(seed; j, (uint32)counter[0], 21, salt) (counter: a device double, read not advanced — the
 *   env globals' step counter; salt: 0 for the per-step launch, the count of redraw-all calls otherwise), or ovr_u[j][0..1] when ovr_u
 *   [N,2] is not NULL (tests); bin = the first b with cdf[c][b] > u1 cdf[c][K-1], clamped to K-1 — never a bin of probability 0;
 *   start_time[j] = min(f32(((bin + u2) / K) clip_len[c]) formed in double, the largest float below clip_len[c]).  Other entries of
 *   start_time are not written.  A plain launch with no host-side state: a replayed graph draws afresh, the counter having moved. */
#define PBHC_START_MAX_BINS 128
int pbhc_start_stats(const int64_t* reset_buf, const uint8_t* time_out_buf, const float* end_time_ratio_buf, const int64_t* last_episode_length_buf,
                     const int64_t* slot_clip, const float* clip_len, double dt, int N, int M, int K, int64_t* window, void* stream);
int pbhc_start_sampling_update(int64_t* window, float* hist_V, float* hist_F, float* prob, double* cdf, int M, int K, double decay,
                               double prior_episodes, double uniform_floor, int lookahead_bins, double lookahead_decay, void* stream);
int pbhc_start_draw(const double* cdf, const float* clip_len, const int64_t* slot_clip, const int64_t* reset_buf, const float* ovr_u, int N, int M,
                    int K, uint64_t seed, const double* counter, uint32_t salt, float* start_time, void* stream);
/* Per-clip tracking error of the library sweep (env.library_sweep; pbhc_clip_track.hip).  Raw device pointers, no PbhcEnv: the step kernel
 * does not know about it.  k_clip_track on `stream`, to follow the step (and pbhc_clip_stats) that left root_states [N,13], dof_state
 * [N,D,2], ref_time [N] (PbhcStepIO.ref_time_out) and reset_buf [N]; motion_ids [N] and `tbl`: the table entries and the table that step
 * used, env_origins [N,3].  For every env with slot_clip[env] in [0, M):
 *   reset_buf != 0: no frame (the post-step state is the new episode's: the terminal frame is not scored); retire[env] = -1 unless retire is
 *     NULL.  retire may alias slot_clip: the env is then scored on its first episode only.
 *   otherwise: track_window[slot_clip[env]] += (1, llrintf(e_g 2^20), llrintf(e_l 2^20), llrintf(e_j 2^20)); track_window [M,4] int64, e_g =
 *     mean_b |p_b - r_b|, e_l = mean_b |(p_b - p_0) - (r_b - r_0)| over the B real bodies (p: the FK pbhc_sim_fk runs, r: the lookup
 *     pbhc_motion_state runs at ref_time, offset by the origin), e_j = |q - q_ref|_2 — the per-frame E_gmpbpe, E_mpbpe, E_mpjpe of
 *     measure_traj.py:147-222.  A frame with a non-finite error is not counted.  motion_ids outside the table: skipped.
 * Integer atomics only: the table does not depend on arrival order.  NULL (retire excepted), N < 1, M < 1, a skeleton beyond the kernel
 * maxima or a table row that does not fit it return PBHC_EINVAL without touching the GPU. */
int pbhc_clip_track(const PbhcSkeleton* skel, const PbhcMotionTable* tbl, const float* root_states, const float* dof_state, const float* ref_time,
                    const float* env_origins, const int64_t* motion_ids, const int64_t* reset_buf, const int64_t* slot_clip, int64_t* retire,
                    int N, int M, int64_t* track_window, void* stream);
/* Second half of a step launched with io->totals_out: `totals` = the element-wise sum over ranks of every shard's totals_out,
 * `num_envs_total` = the number of envs of all ranks.  Must run before the next pbhc_env_step of this env. */
#define PBHC_NUM_TOTALS 64
int pbhc_env_finalize(PbhcEnv* env, const double* totals, double num_envs_total, void* stream);

/* Measurement aid: when enabled, k_env_step of each following pbhc_env_step carries a pair of HIP
 * events attached to its dispatch (kernel begin / end) on the launch stream (ring of PBHC_PROFILE_RING pairs).  pbhc_env_profile_read synchronises on the
 * recorded events and returns the most recent durations in milliseconds (oldest first). */
#define PBHC_PROFILE_RING 512
int pbhc_env_profile(PbhcEnv* env, int enable);
int pbhc_env_profile_read(PbhcEnv* env, float* ms_out, int max_count, int* count);
/* What the dispatch-attached event pair reads BEYOND a kernel's execution (queue-side start / stop handling): measured with a one-wave kernel
 * that spins for exactly 20 us of the 100 MHz wall clock (median of 33 launches minus 0.020 ms).  Subtract it from pbhc_env_profile_read's values
 * to compare with a profiler's kernel durations. */
int pbhc_env_profile_overhead(PbhcEnv* env, void* stream, float* overhead_ms);

/* Rollout-side fusions of MHPPO._rollout_step (mh_ppo.py:270-342).
 * pbhc_policy_sample: a ~ Normal(mu, std) (Philox keyed by seed / counter[0] / env), log-prob, and the writes of one rollout-buffer
 * step: actions, action_mean, action_sigma [N,A], actions_log_prob [N], values [N,R] (copied from `value`; both may be NULL when the
 * critic runs on another stream and stores its own output).
 * counter: device double, read (not advanced) — pass the env globals' step counter. */
int pbhc_policy_sample(const float* mu, const float* std, const float* value, int N, int A, int R, uint64_t seed, const double* counter,
                       float* actions, float* action_mean, float* action_sigma, float* logp, float* values_out, void* stream);
/* pbhc_rollout_post: rewards_stored = rew + gamma * values * time_out (bootstrap, :300-305), dones = reset_buf != 0, and the
 * episode book-keeping (:311-323) kept on the device: cur_reward_sum/cur_episode_length [N], ep_stats double[3] +=
 * (sum of finished returns, sum of finished lengths, count).
 * pbhc_rollout_post2: the same with `values` NULL allowed — rewards_stored = rew, the caller adds the bootstrap once the values exist (the
 * critic evaluated over all steps' slabs at once) — and the step's time-out flags copied to time_outs_out [N] (may be NULL) for that. */
int pbhc_rollout_post(const float* rew, const float* values, const int64_t* reset_buf, const uint8_t* time_outs, int N, int R, float gamma,
                      float* rewards_out, uint8_t* dones_out, float* cur_reward_sum, float* cur_episode_length, double* ep_stats, void* stream);
int pbhc_rollout_post2(const float* rew, const float* values, const int64_t* reset_buf, const uint8_t* time_outs, int N, int R, float gamma,
                       float* rewards_out, uint8_t* dones_out, float* cur_reward_sum, float* cur_episode_length, double* ep_stats, uint8_t* time_outs_out,
                       void* stream);

/* GAE + returns + normalised advantages.  Replaces MHPPO._compute_returns (mh_ppo.py:348-395).
 * rewards/values/returns [T,N,R], dones [T,N] bool, last_values [N,R], advantages [T,N].
 * stats: device scratch of 2 * ceil(T*N / 256) + 2 doubles: per-block partial sums, then the mean and the unbiased std of the unnormalised
 * advantages at stats[2 * ceil(T*N / 256)] and the element behind it (the data-parallel path re-normalises with them). */
int pbhc_gae(const float* rewards, const float* values, const uint8_t* dones, const float* last_values, int T, int N, int R,
             float gamma, float lam, float* returns, float* advantages, double* stats, void* stream);

/* Fused forward + backward of the MHPPO losses (mh_ppo.py:433-480,509-511) on the network outputs of one minibatch.
 * mu [B,A], std [A] (the actor's `std` parameter), value [B,R]; batch tensors as the reference's storage keys
 * (actions [B,A], old_logp [B], old_mu/old_sigma [B,A], adv [B], returns/old_values [B,R]).
 * Out: grad_mu = d(actor_loss)/d(mu) [B,A], grad_value = d(critic_loss)/d(value) [B,R], grad_std [A] (surrogate part and the
 * entropy bonus), scalars[4] = {surrogate loss, value loss, entropy, mean KL}.  adapt_lr bit 0: apply the adaptive-KL rule
 * (mh_ppo.py:455-466) to lr[0] (actor) and lr[1] (critic) on the device; bit 1: the KL of ppo_mimic.py:621-628
 * (log(sigma / (old_sigma + 1e-5)) instead of log(sigma / old_sigma + 1e-5)).  `std` is the sigma vector the distribution used
 * (mh_ppo: the parameter; ppo_mimic: clamp(std, min_sigma, max_sigma), the caller masks grad_std accordingly).
 * scalars_acc (may be NULL): float[4], scalars_acc[i] += scalars[i] — the running sums behind the iteration's mean losses
 * (mh_ppo.py:412-417 `mean_value_loss += ...`) without a launch of their own.  scratch: pbhc_ppo_loss_scratch_floats(B) floats. */
int pbhc_ppo_loss(const float* mu, const float* std, const float* value, const float* actions, const float* old_logp, const float* old_mu,
                  const float* old_sigma, const float* adv, const float* returns, const float* old_values, int B, int A, int R, float clip,
                  float value_coef, float entropy_coef, int use_clipped_value_loss, float desired_kl, int adapt_lr, float* grad_mu, float* grad_value,
                  float* grad_std, float* scalars, float* scalars_acc, float* lr, float* scratch, void* stream);
int pbhc_ppo_loss_scratch_floats(int B);
/* pbhc_ppo_loss's first stage alone: grad_mu, grad_value and *num_partials partial rows of the loss sums in `scratch`; its second stage
 * (grad_std, scalars, the learning rates) then runs inside the backward's finishing launch, pbhc_colsum_final_ppo_reduce below.
 * kl_form2: pbhc_ppo_loss's adapt_lr bit 1. */
int pbhc_ppo_loss_partials(const float* mu, const float* std, const float* value, const float* actions, const float* old_logp, const float* old_mu,
                           const float* old_sigma, const float* adv, const float* returns, const float* old_values, int B, int A, int R, float clip,
                           float value_coef, int use_clipped_value_loss, int kl_form2, float* grad_mu, float* grad_value, float* scratch,
                           int* num_partials, void* stream);
/* The same learning-rate rule on a KL mean already on the device (data-parallel update: the mean over all ranks, after the all-reduce):
 * lr[i] <- rule(lr[i], *kl_mean) for i < n.  Reference: mh_ppo.py:455-466. */
int pbhc_kl_lr_rule(float* lr, int n, const float* kl_mean, float desired_kl, void* stream);

/* Backward of one MLP activation fused with the bias gradient of the layer below it (what autograd runs as elu_backward /
 * silu_backward + a column sum, agents/modules/modules.py:47-63 under torch.autograd): dz = dy * act'(saved), grad_bias = colsum(dz).
 * act: 0 none (bias gradient of the output layer), 1 ELU from the activation output, 2 SiLU from the pre-activation, 3 ReLU from the
 * output.  dy/saved/dz [B,n] row-major (dz may alias dy), grad_bias [n], scratch >= PBHC_ACT_MAX_BLOCKS * n floats. */
#define PBHC_ACT_MAX_BLOCKS 1024
int pbhc_act_bwd_bias(const float* dy, const float* saved, int B, int n, int act, float* dz, float* grad_bias, float* scratch, void* stream);
/* The same in two halves, so that a whole network's bias gradients are finished by ONE launch: pbhc_act_bwd_partials does the slab pass
 * and leaves per-row-block column sums in `scratch` (returns their count in *num_row_blocks); pbhc_colsum_final sums up to
 * PBHC_MAX_COLSUM_JOBS such scratch areas into their grad_bias vectors (fixed order, deterministic). */
#define PBHC_MAX_COLSUM_JOBS 16
typedef struct PbhcColsumJob {
  const float* part;   /* [num_row_blocks, n] */
  float* out;          /* [n] */
  int32_t num_row_blocks;
  int32_t n;
} PbhcColsumJob;
int pbhc_act_bwd_partials(const float* dy, const float* saved, int B, int n, int act, float* dz, float* scratch, int* num_row_blocks, void* stream);
int pbhc_colsum_final(const PbhcColsumJob* jobs, int num_jobs, void* stream);
/* Backward of a stack's narrow OUTPUT Linear (y = h W^T + b, A = out_features <= 32, K = in_features in {64, 128, 192, 256}) in one pass over the
 * rows — what autograd runs as mm (weight gradient), a column sum (bias gradient), mm (input gradient) and the activation backward of the layer
 * below (agents/modules/modules.py:47-63 under torch.autograd; mh_ppo.py:513-517):
 *   dh[M,K] = (dy[M,A] . w[A,K]) * act'(saved)       saved = the lower layer's activation OUTPUT (ELU, ReLU; NULL: = h) or PRE-activation (SiLU)
 *   part_dw[b, A*K], part_db[b, A], part_cs[b, K]    partial rows b < *num_row_blocks (<= PBHC_ACT_MAX_BLOCKS) of dW = dy^T h, db = colsum(dy) and
 *                                                    colsum(dh); finish each with a pbhc_colsum_final job (n = A*K, A, K). */
int pbhc_linear_out_bwd(const float* dy, const float* h, const float* saved, const float* w, int M, int A, int K, int act, float* dh, float* part_dw,
                        float* part_db, float* part_cs, int* num_row_blocks, void* stream);
/* test / measurement aid.  bits 0-7: 0 = the streaming VALU form of pbhc_linear_out_bwd for every shape (default 1: K = 128 runs on the matrix
 * cores); bits 8-15: 32-row tiles per workgroup of the matrix-core form (0 / 1: one — measured in the update: 28.85 / 28.84 / 29.1 ms per update
 * at 1 / 2 / 3, i.e. fewer partial rows buy nothing) */
void pbhc_debug_out_bwd_variant(int mfma);
/* pbhc_colsum_final with pbhc_ppo_loss's second stage as one more workgroup of the same launch (same sums in the same order as there): nothing
 * needs grad_std, scalars[4], scalars_acc or lr before the optimiser pass that follows the backward's finishing launch.  num_jobs may be 0. */
typedef struct PbhcPpoReduce {
  const float* scratch;        /* as left by pbhc_ppo_loss_partials; 16-byte aligned */
  const float* std;
  float* grad_std;
  float* scalars;
  float* scalars_acc;          /* may be NULL */
  float* lr;
  int32_t num_partials, B, A, adapt_lr;      /* num_partials from pbhc_ppo_loss_partials; adapt_lr bit 0 as pbhc_ppo_loss */
  float entropy_coef, desired_kl;
} PbhcPpoReduce;
int pbhc_colsum_final_ppo_reduce(const PbhcColsumJob* jobs, int num_jobs, const PbhcPpoReduce* red, void* stream);
/* pbhc_colsum_final_ppo_reduce that also leaves the sum of squares of the gradients, so that the optimiser pass needs no norm pass of its own
 * (pbhc_adam_clip2_parts below).  Outputs are bit for bit those of pbhc_colsum_final (jobs) + pbhc_colsum_final_ppo_reduce (red).
 * Up to two flat gradient segments (actor, critic; n == 0: unused).  Every workgroup adds, in double, the squares of the floats it stores and
 * writes that ONE sum to its own slot of seg[s].part, s = the segment that contains the job's `out` (in no segment: no slot; straddling a
 * segment's end: PBHC_EINVAL); workgroup 0 does the same for grad_std and advances step[0] and step[1] by one (as pbhc_adam_clip2's norm
 * pass does).  range_off / range_len: the parts of the segment that NO job of this call (nor grad_std) writes, in floats from `base`,
 * ascending and disjoint — the caller's statement; rider workgroups of the launch square them, PBHC_SQ_RANGE_FLOATS per workgroup (4-byte
 * alignment is enough).  Slots per segment, in order: grad_std, the jobs' workgroups in job order, the riders; every slot is written exactly
 * once per call, nothing needs zeroing.  num_jobs <= PBHC_SQ_MAX_JOBS (both exports): each PBHC_MAX_COLSUM_JOBS jobs are a launch, the slots are numbered across
 * them, the last launch carries `red` and the riders.  pbhc_colsum_final_ppo_reduce_sqnorm_slots: slots[s] = the slot count of segment s for
 * the same arguments (launches nothing; part may be NULL and part_cap 0 there); part_cap (doubles) must be at least that.
 * The sum of a segment's slots is ||g||^2 in a fixed order, reproducible run to run, but grouped differently from pbhc_adam_clip2's strided
 * norm pass: the float norm can land on the adjacent float of that one's. */
#define PBHC_SQ_MAX_RANGES 16
#define PBHC_SQ_MAX_JOBS 256
#define PBHC_SQ_RANGE_FLOATS 4096
typedef struct PbhcSqSegment {
  const float* base;           /* the segment's gradients */
  double* part;                /* part_cap doubles */
  int32_t n, part_cap, num_ranges;
  int32_t range_off[PBHC_SQ_MAX_RANGES], range_len[PBHC_SQ_MAX_RANGES];
} PbhcSqSegment;
typedef struct PbhcSqnorm {
  PbhcSqSegment seg[2];
  float* step;                 /* float[2] */
} PbhcSqnorm;
int pbhc_colsum_final_ppo_reduce_sqnorm(const PbhcColsumJob* jobs, int num_jobs, const PbhcPpoReduce* red, const PbhcSqnorm* sq, void* stream);
int pbhc_colsum_final_ppo_reduce_sqnorm_slots(const PbhcColsumJob* jobs, int num_jobs, const PbhcPpoReduce* red, const PbhcSqnorm* sq, int32_t* slots);


/* One Linear of a training-time Linear / activation stack on the fp32 matrix cores with its activation folded into the GEMM epilogue
 * (agents/modules/modules.py:47-63: `nn.Linear` followed by `nn.ELU` / `nn.SiLU` / `nn.ReLU`; replaces torch.addmm + the activation pass):
 *   y[M,N] = act(x[M,K] . w[N,K]^T + bias[N])        act: 0 none, 1 ELU (alpha 1), 2 SiLU, 3 ReLU;  bias may be NULL
 *   pre[M,N] (may be NULL) = x . w^T + bias            the pre-activation, which SiLU's derivative needs
 * x, w row-major, contiguous (rows need 4-byte alignment only).  f32 in, f32 accumulate (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain). */
int pbhc_linear_act_fwd(const float* x, const float* w, const float* bias, float* y, float* pre, int M, int N, int K, int act, void* stream);
/* The stack's last hidden layer AND its narrow output layer in one launch (the tail `Linear(K,128) - act - Linear(128,NO)` of modules.py:47-63's
 * nn.Sequential: 23 action means / 20 value heads): y, pre as above with N = 128, and out[M, NO] = y . w_out[NO,128]^T + b_out[NO] (b_out may be
 * NULL) computed from the tile's activated rows while they are in LDS (32-row tiles hold whole rows) — replaces the library addmm of the
 * output layer (14 / 9 us of launch for 0.14 GFLOP at 24 576 rows).  NO <= 32, K >= 4; out rows contiguous. */
int pbhc_linear_act_fwd_out(const float* x, const float* w, const float* bias, float* y, float* pre, int M, int N, int K, int act, const float* w_out,
                            const float* b_out, int NO, float* out, void* stream);
/* pbhc_linear_act_fwd_out for TWO stacks' tails in one launch (the same 32 x 128 tile code on a shared grid; the problem with the longer K
 * takes the leading workgroups): each problem's y / pre / out are bit for bit those of its own pbhc_linear_act_fwd_out call.  Both argument
 * sets are checked as there; the two M need not be equal. */
int pbhc_linear_act_fwd_out_pair(const float* x0, const float* w0, const float* bias0, float* y0, float* pre0, int M0, int N0, int K0, int act0, const float* w_out0,
                                 const float* b_out0, int NO0, float* out0, const float* x1, const float* w1, const float* bias1, float* y1, float* pre1, int M1,
                                 int N1, int K1, int act1, const float* w_out1, const float* b_out1, int NO1, float* out1, void* stream);
/* pbhc_linear_act_fwd for TWO wide layers in one launch: two problems that the single entry each runs on 64 x 128 tiles of the LDS-DMA kernel
 * share a grid (the problem with more tile work takes the leading workgroups); y / pre are bit for bit the single call's, no output layer rides.
 * pbhc_linear_act_fwd_pairable(M, N, K): 1 if pbhc_linear_act_fwd itself runs the problem on those tiles — its own tile choice or a shape
 * forced with pbhc_gemm_debug_force_shape, K >= 4, no measurement setting active — else 0.  The pair entry refuses (PBHC_EINVAL, nothing
 * launched) unless that holds for BOTH problems, so pairing never changes the tiles a layer runs on.  The two M need not be equal. */
int pbhc_linear_act_fwd_pairable(int M, int N, int K);
int pbhc_linear_act_fwd_pair(const float* x0, const float* w0, const float* bias0, float* y0, float* pre0, int M0, int N0, int K0, int act0, const float* x1,
                             const float* w1, const float* bias1, float* y1, float* pre1, int M1, int N1, int K1, int act1, void* stream);
/* The same with row strides and a batch: batch b computes y[b] = act(x[b] . w^T + bias) with x[b] = x + b * x_batch_stride (rows lda floats
 * apart, lda >= K), y[b] = y + b * y_batch_stride (rows ldc floats apart, ldc >= N), one weight matrix for all — e.g. the L output positions of
 * nn.Conv1d(C -> O, kernel k, stride s) on time-major activations [B, T, C] (encoder_modules.py:60-107): window l is the [B, k*C] matrix at
 * x + l*s*C with lda = T*C, written to out[:, l, :] of [B, L, O] (y + l*O, ldc = L*O).  K >= 4. */
int pbhc_linear_act_fwd_strided(const float* x, int lda, long long x_batch_stride, const float* w, const float* bias, float* y, float* pre, int ldc,
                                long long y_batch_stride, int batches, int M, int N, int K, int act, void* stream);
/* The WHOLE Linear / activation stack of a no-grad forward (the rollout's policy and critic evaluation, `BaseModule.forward`,
 * agents/modules/modules.py:47-63 as called from mh_ppo.py:286-290 / ppo_mimic.py:392-400) in one launch: a workgroup carries 16 rows through
 * every layer, activations stay in LDS.  y[M, dims[L]] = W_L-1 act(... act(W_0 x + b_0) ...) + b_L-1 (no activation after the last layer).
 * x rows ldx floats apart, y rows ldy apart; weights[l] = the PACKED copy (pbhc_mlp_pack, pbhc_mlp_packed_floats(dims[l+1], dims[l]) floats,
 * 16-byte aligned) of nn.Linear.weight [dims[l+1], dims[l]] — the MFMA operand fragments laid out 1 KiB-contiguous per wave-instruction;
 * the caller repacks when the weights change (once per rollout: they are constant over its steps).  biases[l] may be NULL; act as
 * pbhc_linear_act_fwd.  pbhc_mlp_fwd_lds_bytes: the launch's dynamic LDS (<= 160 KB or the call is refused): two images of 16 rows, image
 * (l & 1) at the widest pitch ceil16(dims[l]) + 4 of its layers' inputs l < L and of the output row dims[L]. */
#define PBHC_MLP_MAX_LAYERS 8
/* pbhc_mlp_fwd_sample: the policy's stack with pbhc_policy_sample folded into the last layer's epilogue (mh_ppo.py:286-296: the rollout's
 * act() + log-prob + buffer writes): mu = the stack's output [M, A] (A = dims[L] <= 32, else PBHC_EINVAL and nothing launched), actions = mu + std * z with z from the Philox call
 * pbhc_policy_sample makes — keyed by seed / (uint32)counter[0] + counter_offset / row / column — action_mean = mu, action_sigma = std,
 * logp[M] = the row's Normal log-density.  `counter`: a device double the caller keeps constant over a rollout (a snapshot of the env's step
 * counter at its start) with counter_offset = the step index, so that the launch does not wait for the previous step's reduction. */
typedef struct PbhcMlpSample {
  const float* std;            /* [A] */
  const double* counter;
  uint64_t seed;
  int32_t counter_offset;
  int32_t pad_;
  float* actions;              /* [M, A] */
  float* action_mean;          /* [M, A] */
  float* action_sigma;         /* [M, A] */
  float* logp;                 /* [M] */
} PbhcMlpSample;
int pbhc_mlp_fwd_sample(const float* x, int ldx, const float* const* weights, const float* const* biases, const int* dims, int num_layers, int act, int M,
                        const PbhcMlpSample* sample, void* stream);
/* pbhc_mlp_fwd_cat: the same stack on input rows given as up to PBHC_MLP_MAX_SEGS column segments laid side by side — `module(torch.cat([obs,
 * motion_embedding, latent], -1))` of the general-tracking actor (agent_modules.py:75-84 of the reference) without materialising the concatenation;
 * sum(width) == dims[0], ld[i] >= width[i] (floats).  y may be NULL when `sample` is given (then the sampling epilogue of pbhc_mlp_fwd_sample runs);
 * both may be given.  16-byte loads are used when every segment allows them (16-byte aligned base, ld % 4 == 0, inner widths % 4 == 0). */
#define PBHC_MLP_MAX_SEGS 3
typedef struct PbhcMlpInput {
  const float* x[PBHC_MLP_MAX_SEGS];
  int32_t ld[PBHC_MLP_MAX_SEGS];
  int32_t width[PBHC_MLP_MAX_SEGS];
  int32_t nseg;
} PbhcMlpInput;
int pbhc_mlp_fwd_cat(const PbhcMlpInput* in, const float* const* weights, const float* const* biases, const int* dims, int num_layers, int act, float* y, int ldy,
                     int M, const PbhcMlpSample* sample, void* stream);
/* Riders: the small per-step kernels of the rollout as EXTRA WORKGROUPS of the policy launch, so that the dependent chain
 * env step -> policy forward -> env step stays on one queue with no branch beside it (the policy forward of step t reads nothing the previous
 * step's reduction writes: its sampler is keyed by the counter snapshot, see PbhcMlpSample).  Behind the ceil(M / 16) workgroups of the stack:
 *   has_finalize: ONE workgroup runs the single-process form of pbhc_env_step_finish's reduction (the same additions in the same order, the
 *                 same scalar chains: the globals come out equal bit for bit) — fill this half with pbhc_env_finalize_rider, which launches
 *                 nothing; the launch that carries it must follow the pbhc_env_step_launch it belongs to on its stream, and precede the next;
 *   has_post:     ceil(N / 16) workgroups run pbhc_rollout_post2's kernel body on 16 envs each (same arguments, same per-env arithmetic;
 *                 ep_stats is summed per 16 envs before its atomics instead of per 8).
 * pbhc_mlp_fwd_sample_riders / pbhc_mlp_fwd_cat_riders: pbhc_mlp_fwd_sample / pbhc_mlp_fwd_cat with `riders` (NULL, or both flags 0: exactly
 * those calls). */
typedef struct PbhcRider {
  const PbhcEnvConfig* cfg;          /* finalize half: the env's device-side config, globals and partial-sum rows */
  double* globals;
  const float* partials;
  int32_t* frame_cursor;
  int32_t num_partial_rows;          /* 2 * workgroups of the env step */
  int32_t num_frames;
  const float* rew;                  /* post half: the arguments of pbhc_rollout_post2 */
  const float* values;               /* may be NULL */
  const int64_t* reset_buf;
  const uint8_t* time_outs;
  float* rewards_out;
  uint8_t* dones_out;
  float* cur_reward_sum;
  float* cur_episode_length;
  double* ep_stats;
  uint8_t* time_outs_out;            /* may be NULL */
  int32_t N, R;
  float gamma;
  int32_t has_finalize, has_post;
  int32_t pad_;
} PbhcRider;
int pbhc_env_finalize_rider(PbhcEnv* env, const PbhcStepIO* io, PbhcRider* rider);
/* test aid: the stand-alone reduction kernel on a rider's finalize half (any partial rows / globals / cursor), to hold the rider workgroup to it */
int pbhc_debug_env_finalize(const PbhcRider* rider, void* stream);
int pbhc_mlp_fwd_sample_riders(const float* x, int ldx, const float* const* weights, const float* const* biases, const int* dims, int num_layers, int act, int M,
                               const PbhcMlpSample* sample, const PbhcRider* riders, void* stream);
int pbhc_mlp_fwd_cat_riders(const PbhcMlpInput* in, const float* const* weights, const float* const* biases, const int* dims, int num_layers, int act, float* y,
                            int ldy, int M, const PbhcMlpSample* sample, const PbhcRider* riders, void* stream);
/* pbhc_conv_encoder_fwd: the general-tracking `ConvEncoder` (agents/modules/encoder_modules.py:22-107 of the reference: Linear(d -> H) + ReLU
 * per time step, Conv1d(H -> O1, k1, s1) + act, Conv1d(O1 -> O2, k2, s2) + act, Linear(L2 * O2 -> E)) under no_grad in ONE launch, 16 rows per
 * workgroup through all four layers (the rollout: 4 096 rows per control step).  x [M, T * d] with row pitch ldx >= (T - 1) * d + ceil16(d)
 * (a rollout slab's padded rows: the kernel reads whole 16-float k-steps, so the last step's read ends inside the padding, but the result
 * depends on columns [0, T * d) only — the padding may hold anything, NaN included), y [M, E] with row pitch ldy >= E.  Weights packed by pbhc_mlp_pack from row-major matrices: w1 [H, d]; wc1 [O1, k1 * H] and wc2
 * [O2, k2 * O1] with the kernel tap OUTER (conv.weight.permute(0, 2, 1)); wo [E, L2 * O2] with its columns in (position, channel) order.
 * act: 1 ELU, 2 SiLU, 3 ReLU (the conv layers; layer 1 is ReLU, the output layer linear).  pbhc_conv_encoder_lds_bytes: the launch's LDS need
 * (<= 160 KB; the caller falls back to the per-layer kernels otherwise). */
typedef struct PbhcConvEncoder {
  const float* w1; const float* b1;
  const float* wc1; const float* bc1;
  const float* wc2; const float* bc2;
  const float* wo; const float* bo;
  int32_t T, d, H, O1, k1, s1, O2, k2, s2, E, act;
  int32_t pad_;
} PbhcConvEncoder;
size_t pbhc_conv_encoder_lds_bytes(const PbhcConvEncoder* e);
int pbhc_conv_encoder_fwd(const float* x, int ldx, const PbhcConvEncoder* e, float* y, int ldy, int M, void* stream);
size_t pbhc_mlp_packed_floats(int N, int K);
int pbhc_mlp_pack(const float* w, int N, int K, float* packed, void* stream);
size_t pbhc_mlp_fwd_lds_bytes(const int* dims, int num_layers);
int pbhc_mlp_fwd(const float* x, int ldx, const float* const* weights, const float* const* biases, const int* dims, int num_layers, int act, float* y, int ldy,
                 int M, void* stream);
/* The input gradient of that Linear with the activation backward of the layer BELOW folded in (what autograd runs as mm + elu_backward /
 * silu_backward + a column sum; replaces `dy @ w` + pbhc_act_bwd_partials):
 *   dx[M,N] = (dy[M,K] . w[K,N]) * act'(saved[M,N])   N = in_features, K = out_features; saved = the lower layer's activation OUTPUT
 *                                                     (ELU, ReLU) or PRE-activation (SiLU)
 *   scratch[b, :] = column sums of dx over row block b (*num_row_blocks of them, <= PBHC_ACT_MAX_BLOCKS; finish with pbhc_colsum_final)
 * scratch may be NULL (no column sums); act 0: saved unused. */
int pbhc_linear_dgrad_act(const float* dy, const float* w, const float* saved, float* dx, float* scratch, int* num_row_blocks, int M, int N, int K,
                          int act, void* stream);
/* pbhc_linear_dgrad_act for TWO layers in one launch on 32 x 128 tiles (the larger problem takes the leading workgroups; each problem has its
 * own scratch and row-block count = ceil(M / 32)): bit for bit the results of two pbhc_linear_dgrad_act calls that run on 32 x 128 tiles.
 * Refused for a problem that entry would not run so: needs 4 <= K <= 128 and N % 4 == 0.  The two M need not be equal.  When both K are exactly
 * 128 the pair runs the weight-stationary kernel (one persistent workgroup per CU holds a 128 x 128 slice of W in LDS), as the single entry
 * does for such a problem on 32 x 128 tiles; the results are the same bits either way. */
/* 1 if pbhc_linear_dgrad_act itself runs (M, N, K) on those tiles (its own tile choice; no test / measurement setting active), else 0:
 * ask this for BOTH problems before forming a pair, so that pairing never changes the tile height a layer runs on. */
int pbhc_linear_dgrad_act_pairable(int M, int N, int K);
int pbhc_linear_dgrad_act_pair(const float* dy0, const float* w0, const float* saved0, float* dx0, float* scratch0, int* num_row_blocks0, int M0, int N0, int K0,
                               int act0, const float* dy1, const float* w1, const float* saved1, float* dx1, float* scratch1, int* num_row_blocks1, int M1, int N1,
                               int K1, int act1, void* stream);
/* The weight gradient of that Linear (autograd's `dy.t() @ x`): dw[N,K] = sum over the M rows of dy[m,N]^T x[m,K], N = out_features,
 * K = in_features.  The rows are split over pbhc_linear_wgrad_parts(M, N, K) workgroup groups (0: shape not supported — N % 4, M % 32, K < 4 —
 * use the library) whose partial images go to `scratch` (parts * N * K floats) and are summed in a fixed order. */
int pbhc_linear_wgrad_parts(int M, int N, int K);
int pbhc_linear_wgrad(const float* dy, const float* x, float* dw, float* scratch, int M, int N, int K, void* stream);
/* test / measurement aid for the Linear entries above.  shape < 0: everything automatic.  Otherwise bits 0-7: tile shape (0: 128x128, 1: 96x128,
 * 2: 64x128, 3: 64x64 forward only, 0xff: automatic); bits 8-15: K-loop ablation flags (tools/gemm_ablation.py; results are wrong with parts
 * off); bits 16-23: staging version (0: automatic, 1: register-staged version 1, 2: LDS-DMA with BK 16 x 3 stages, 4: automatic except that
 * the K = 128 input gradients on 32 x 128 tiles stay on the ring kernel instead of the weight-stationary one — the pair entries and the
 * pairable queries read 4 as 0); bits 24-30: workgroups of a weight-stationary launch (0: one per CU; raised to one per 128-column slice
 * and capped at the number of tiles — no result depends on it). */
void pbhc_gemm_debug_force_shape(int shape);

/* The minibatch shuffle of one update (RolloutStorage.mini_batch_generator, agents/modules/data_utils.py:134-152: `tensor.flatten(0, 1)[indices]`
 * per stored key) for several keys in ONE launch: dst_j[i, :] = src_j[index[i], :] for every job j and row i < nrows.  src rows are src_pitch floats
 * apart (the rollout slabs are 128-byte-padded), dst is contiguous [nrows, width]; f32 only; index values in [0, source rows). */
#define PBHC_MAX_GATHER_JOBS 12
typedef struct PbhcGatherJob {
  const float* src;
  float* dst;
  int32_t width;
  int32_t src_pitch;
} PbhcGatherJob;
int pbhc_gather_rows(const PbhcGatherJob* jobs, int num_jobs, const int64_t* index, int nrows, void* stream);

/* The left <-> right mirror of observation / action rows (algo.config.symmetry; the tables: pbhc_amd/envs/obs_mirror.py) for several tensors in ONE
 * launch: dst_j[r * dst_pitch + c] = sign_j[c] * src_j[r * src_pitch + index_j[c]] for every job j, row r < nrows and column c < width.  index /
 * sign: device arrays of `width` entries, index values in [0, width) (larger ones are read as width - 1).  dst_pitch >= width: a job may write the
 * observation columns of an assembled first-layer input in place; the columns beyond `width` are not touched.  src and dst must not overlap.
 * f32 only; a sign flip and a copy, so bit-exact.  NULL pointers, width < 1 or > PBHC_MIRROR_MAX_WIDTH, a pitch below the width, nrows < 1 or more
 * than PBHC_MAX_MIRROR_JOBS jobs return PBHC_EINVAL without a launch. */
#define PBHC_MAX_MIRROR_JOBS 8
#define PBHC_MIRROR_MAX_WIDTH 4096
typedef struct PbhcMirrorJob {
  const float* src;
  float* dst;
  const int32_t* index;
  const float* sign;
  int32_t width;
  int32_t src_pitch;
  int32_t dst_pitch;
} PbhcMirrorJob;
int pbhc_mirror_rows(const PbhcMirrorJob* jobs, int num_jobs, int nrows, void* stream);
/* The mirror-symmetry term of the policy mean with a detached target (rsl_rl's form), mu / mu_m / grad_mu_m [B, A] contiguous, A <= PBHC_MAX_DOF:
 *   target[b, a] = act_sign[a] * mu[b, act_index[a]]          L = coef * mean over the B A elements of (mu_m - target)^2
 *   grad_mu_m = dL / dmu_m = (2 coef / (B A)) (mu_m - target)  (nothing flows into mu)
 * scalar_out[0] = L; acc_out (may be NULL): acc_out[0] += L.  The sum runs in two stages in a fixed order without atomics — thread t of block g adds up
 * its elements (g + i * blocks) * PBHC_SYM_THREADS + t for i = 0, 1, ..., blocks = min(ceil(B A / (PBHC_SYM_THREADS * PBHC_SYM_ELEMS)),
 * PBHC_SYM_MAX_BLOCKS); a block sums its threads by a 6-level butterfly per wave and then the waves in order; one block of PBHC_SYM_MAX_BLOCKS threads
 * sums the block partials the same way — so two runs agree bit for bit.  scratch: PBHC_SYM_MAX_BLOCKS floats. */
#define PBHC_SYM_THREADS 256
#define PBHC_SYM_ELEMS 4
#define PBHC_SYM_MAX_BLOCKS 512
int pbhc_symmetry_loss(const float* mu, const float* mu_m, const int32_t* act_index, const float* act_sign, int B, int A, float coef, float* grad_mu_m,
                       float* scratch, float* scalar_out, float* acc_out, void* stream);

/* nn.utils.clip_grad_norm_(max_norm) + torch.optim.Adam.step() (mh_ppo.py:519-524; weight_decay > 0: torch.optim.AdamW, decoupled,
 * ppo_mimic.py:184-190,682-686) over ONE flat fp32 segment of n
 * parameters (param/grad/exp_avg/exp_avg_sq flat views; lr and step are device scalars, step is incremented).
 * scratch: 512 doubles.  norm_out (may be NULL): the pre-clip gradient norm.
 * beta1 / beta2 act at their float values: beta2 = 0.999f is 0.99900001, so exp_avg_sq is 1.3e-5 (relative) below a double-beta Adam's while
 * the bias correction uses the same value and the parameter step agrees to rounding (tests/test_gpu_ppo_kernels.py). */
int pbhc_adam_clip(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int n, const float* lr, float* step, float max_norm, float beta1,
                   float beta2, float eps, float weight_decay, double* scratch, float* norm_out, void* stream);
/* Two consecutive segments (actor [0,n0), critic [n0,n0+n1): MHPPO's two clip_grad_norm_ + two Adam steps, mh_ppo.py:519-524) in ONE launch
 * pair: lr, step, norm_out are 2-element device arrays, scratch 2 x 512 doubles; each segment is clipped by its own norm.
 * zero_grad != 0: the gradient buffer is left ZEROED instead of holding the clipped gradients (the next optimiser step's
 * `optimizer.zero_grad()`, mh_ppo.py:513-514, done by the pass that read the gradients last: no fill launch of its own). */
int pbhc_adam_clip2(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int n0, int n1, const float* lr, float* step, float max_norm, float beta1,
                    float beta2, float eps, float weight_decay, int zero_grad, double* scratch, float* norm_out, void* stream);
/* pbhc_adam_clip2's optimiser pass ALONE, on norm partials that are already there: segment s is clipped by sqrt(sum of part_s[0 .. nparts_s)),
 * summed as pbhc_adam_clip2 sums its own partials (same kernel, same arithmetic).  No norm pass, and `step` is NOT advanced: whoever left the
 * partials has done that (pbhc_colsum_final_ppo_reduce_sqnorm).  nparts >= 1. */
int pbhc_adam_clip2_parts(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int n0, int n1, const float* lr, const float* step, float max_norm,
                          float beta1, float beta2, float eps, float weight_decay, int zero_grad, const double* part0, int nparts0, const double* part1,
                          int nparts1, float* norm_out, void* stream);

/* Test-only: the device functions of csrc/pbhc_math.h (the quaternion / rotation algebra every kernel inlines; SURVEY 8 row a1:
 * isaac_utils/rotations.py:28-669, utils/torch_utils.py:51-79,239-296) applied elementwise, so that they can be pinned directly against
 * the reference's own outputs.  a / b / c: device operand arrays of n elements ([n,4] xyzw quaternions, [n,3] vectors, [n] scalars,
 * [n,9] row-major matrices, as the function takes them); out: [n, width of the result]. */
enum PbhcDebugFn {
  PBHC_DBG_QUAT_ROTATE = 0,        /* a q, b v -> [n,3] */
  PBHC_DBG_QUAT_ROTATE_INVERSE,    /* a q, b v -> [n,3] */
  PBHC_DBG_QUAT_APPLY,             /* a q, b v -> [n,3] */
  PBHC_DBG_QUAT_MUL,               /* a q, b p -> [n,4] */
  PBHC_DBG_QUAT_CONJ,              /* a q -> [n,4] */
  PBHC_DBG_SLERP,                  /* a q0, b q1, c t -> [n,4] */
  PBHC_DBG_CALC_HEADING,           /* a q -> [n] */
  PBHC_DBG_CALC_HEADING_QUAT,      /* a q -> [n,4] */
  PBHC_DBG_CALC_HEADING_QUAT_INV,  /* a q -> [n,4] */
  PBHC_DBG_EULER_XYZ,              /* a q -> [n,3] roll pitch yaw */
  PBHC_DBG_QUAT_FROM_ANGLE_AXIS,   /* a angle [n], b axis -> [n,4] */
  PBHC_DBG_QUAT_ANGLE,             /* a q -> [n]: quat_to_angle_axis(q)[0] */
  PBHC_DBG_AXIS_ANGLE_TO_QUAT_WXYZ,/* a axis-angle [n,3] -> [n,4] wxyz */
  PBHC_DBG_QUAT_TO_MATRIX,         /* a q (xyzw) -> [n,9] */
  PBHC_DBG_MATRIX_TO_QUAT,         /* a [n,9] -> [n,4] xyzw */
  PBHC_DBG_YAW_QUAT,               /* a q -> [n,4] */
  PBHC_DBG_QUAT_TO_MAT6,           /* a q -> [n,6]: first two columns of R, row-major */
  PBHC_DBG_QUAT_UNIT,              /* a q -> [n,4] */
  PBHC_DBG_NUM
};
int pbhc_debug_rotations(int fn, const float* a, const float* b, const float* c, int n, float* out, void* stream);
/* Test-only, host code: csrc/pbhc_math.h rotvec_from_quat (the recorder's pose_aa row 0) on n xyzw quaternions given in double, evaluated
 * in double (out64 [n,3]) and — after rounding the quaternion to float — in float (out32 [n,3]); either output may be NULL. */
int pbhc_debug_rotvec_host(const double* quat_xyzw, int n, double* out64, float* out32);

/* The closed-loop joint-space simulator (pbhc_amd/simulator/joint_sim.py JointSpaceSim; k_joint_sim in csrc/pbhc_joint_sim.hip): ONE launch per control
 * step on the stepping stream, directly in front of pbhc_env_step / pbhc_env_step_launch with the SAME env handle and io.  It writes the one-frame replay
 * window the step then consumes through io->frame_* (io->num_frames must be 1, so frame_index 0 and the device cursor name the same frame):
 *   joints  from io->dof_state (what the previous step left, resets included) `decimation` sub-steps of h = sim_dt of decoupled second-order dynamics
 *           under the step's own PD law — the action clipped, the delayed action PEEKED from io->action_queue / action_delay_idx (the step still owns
 *           and shifts the queue), the torque formula of legged_robot_base.py:795-838 re-evaluated with the current (q, v) in every sub-step, the RFI /
 *           parallel_serial_tau draws of THIS control step (Philox streams 1 / 19 keyed with the globals' step counter, or io->u_rfi / io->ovr_ps_tau)
 *           held over the sub-steps:  v <- (v + h tau / I_d) / (1 + h b_d / I_d),  q <- q + h v,  and with enforce_limits q clamped to
 *           hard_dof_pos_limits with an outward v zeroed.  control_type "V" is refused.
 *   root    the clip's root body at (episode_length_buf + 2) dt + motion_start_times (the step's own reference time, from the pre-step counter) with
 *           pbhc_motion_state's lerp / slerp, + env_origins on the position.
 *   contact contact_force (N) on z of a foot body when the clip's lerped contact mask is > 0.5 — or, for a library without masks, when the foot's
 *           reference height is below foot_height_threshold — else 0; no other element of the contact frame is written (the caller zeroes it once).
 * No gravity, no coupling between joints, no contact dynamics.  tau0 (may be NULL): device [N,D], the first sub-step's torque.
 * NULL pointers, io->num_frames != 1, decimation outside [1, 64], an inertia <= 0 or a damping < 0 of a used dof return PBHC_EINVAL without a launch. */
typedef struct PbhcJointSimParams {
  float inertia[PBHC_MAX_DOF];    /* I_d  kg m^2 (armature included) */
  float damping[PBHC_MAX_DOF];    /* b_d  N m s / rad, passive, taken implicitly */
  float contact_force;
  float foot_height_threshold;
  int32_t enforce_limits;
  int32_t decimation;
  float* tau0;
} PbhcJointSimParams;
int pbhc_sizeof_joint_sim_params(void);
/* Memory contract of the three simulator step entries (pbhc_joint_sim_step, pbhc_articulated_sim_step, pbhc_floating_sim_step; 8 envs per
 * workgroup, loads of a ragged last workgroup clamped onto env N - 1, nothing stored for the missing envs).  Read, with the extents and
 * alignments of PbhcStepIO: actions_in, dof_state, action_queue, action_delay_idx, kp_scale, kd_scale, rfi_lim_scale, rao_scale,
 * episode_length_buf, motion_start_times, motion_ids, env_origins, u_rfi / ovr_ps_tau / default_dof_pos when non-NULL (the floating
 * simulator also root_states), and the motion table's rows of the env's clip.  Written: the ONE frame of the window — frame_root [1,N,13],
 * frame_dof_pos / frame_dof_vel [1,N,D] whole, of frame_contact [1,N,B,3] only z of the foot bodies (floating: all three components of the
 * bodies that own contact points) — and, when non-NULL, tau0 [N,D] and base_acc / root_acc [N,6].  PbhcFloatingParams.points:
 * [PBHC_ART_MAX_BODIES, PBHC_FLOAT_MAX_POINTS, 3] floats, read only.  The floating simulator's optional per-env operands, each NULL or whole:
 * read only env_inertial [N, PBHC_ART_MAX_BODIES, 4] floats (16-byte aligned, else PBHC_EINVAL; one 16-byte load per lane), env_friction [N]
 * floats and u_push [N,3] floats; read AND written push_counter [N] int32 and push_interval [N] int32 (every env, every step), push_vel [N,2]
 * floats (written for the envs whose push fires, never read), stored by lane 0 of the env alone.  Everything dense, float and int32
 * buffers 4-byte aligned, the int64 buffers 8-byte aligned (else PBHC_EINVAL). */
int pbhc_joint_sim_step(PbhcEnv* env, const PbhcStepIO* io, const PbhcJointSimParams* params, void* stream);

/* The articulated rigid-body simulator (pbhc_amd/simulator/articulated_sim.py ArticulatedSim; k_articulated_sim in csrc/pbhc_articulated_sim.hip): the
 * same place in the step, the same one-frame window, root, contact, torque law and draws as pbhc_joint_sim_step — only the joint law differs.  The robot's
 * tree (kinematics exactly pbhc_sim_fk's: R_b = R_parent local_rot_b Rot(axis_{b-1}, q_{b-1}), p_b = p_parent + R_parent offset_b, hinge d drives body
 * d + 1 about an axis through that body's origin) carries link masses, centres of mass and inertia tensors (body frame, about the centre of mass, the six
 * words xx yy zz xy xz yz).  The base is prescribed (the root row the kernel writes; constant over the sub-steps): R_0, w_0 and, with base_acceleration,
 * a_0 = (v(tref) - v(tref - dt)) / dt and alpha_0 likewise from the angular velocity (else 0); gravity enters as a_0 - g.  Every sub-step, h = sim_dt:
 *   tau from the current (q, v) by the step's torque law;  (M(q) + diag(armature + h b)) dv = h (tau - b v - c(q, v; R_0, w_0, alpha_0, a_0 - g));
 *   v <- v + dv;  q <- q + h v;  with enforce_limits the clamp of pbhc_joint_sim_step.
 * M: the joint-space inertia matrix at THIS sub-step's q; c: the inverse dynamics at q'' = 0.  No free root, no contact dynamics.
 * tau0 (may be NULL): device [N,D], the first sub-step's torque.  base_acc (may be NULL): device [N,6], the a_0 and alpha_0 the kernel used.
 * NULL pointers, io->num_frames != 1, B > PBHC_ART_MAX_BODIES, decimation outside [1, 64], a negative armature, damping or mass, control type "V"
 * return PBHC_EINVAL without a launch. */
#define PBHC_ART_MAX_BODIES 32
typedef struct PbhcArticulatedParams {
  float mass[PBHC_ART_MAX_BODIES];          /* m_b  kg; the root's entry is not used (the base is prescribed) */
  float com[PBHC_ART_MAX_BODIES][3];        /* c_b  m, body frame */
  float inertia[PBHC_ART_MAX_BODIES][6];    /* I_b  kg m^2 about the centre of mass, body frame: xx yy zz xy xz yz */
  float armature[PBHC_MAX_DOF];             /* kg m^2, added to the diagonal of M */
  float damping[PBHC_MAX_DOF];              /* b_d  N m s / rad, passive, taken implicitly */
  float gravity[3];                         /* m / s^2, world */
  int32_t base_acceleration;
  float contact_force;
  float foot_height_threshold;
  int32_t enforce_limits;
  int32_t decimation;
  float* tau0;
  float* base_acc;
} PbhcArticulatedParams;
int pbhc_sizeof_articulated_params(void);
int pbhc_articulated_sim_step(PbhcEnv* env, const PbhcStepIO* io, const PbhcArticulatedParams* params, void* stream);
/* Test-only: `steps` sub-steps of h seconds of the SAME device function as k_articulated_sim under a constant torque, n independent robots.
 * base [n,13]: R_0 as a quaternion xyzw, w_0, alpha_0, a_0 (gravity is taken from params); q, v, tau [n,D]; limits: HOST [D,2], read only with
 * enforce_limits; out_q, out_v [n,D] the final state, out_qdd0 [n,D] the first sub-step's dv / h.  steps outside [1, 4096], h <= 0, NULL pointers,
 * a skeleton over the maxima, a negative armature, damping or mass return PBHC_EINVAL without a launch. */
int pbhc_debug_articulated_substeps(const PbhcSkeleton* skel, const PbhcArticulatedParams* params, const float* base, const float* q, const float* v,
                                    const float* tau, int n, int steps, float h, int enforce_limits, const float* limits, float* out_q, float* out_v,
                                    float* out_qdd0, void* stream);

/* The floating-base simulator (pbhc_amd/simulator/floating_sim.py FloatingBaseSim; k_floating_sim in csrc/pbhc_floating_sim.hip): the same place in the
 * step, the same one-frame window, delayed-action peek, torque law, draws, tau0 and limits clamp as pbhc_articulated_sim_step, the same tree, link
 * inertias and kinematics — but the root is FREE (six more degrees of freedom of the tree; the root link's own mass, centre of mass and inertia count)
 * and the ground pushes back at contact points fixed to the links.  The clip's root, its contact mask and a contact_force are not read.
 * State: io->root_states [N,13] (position, quaternion xyzw, WORLD linear velocity v_0 of the root's origin, world angular velocity w_0) and io->dof_state,
 * both what the previous step left, resets included.  Every sub-step, h = sim_dt:
 *   1. tau from the current (q, v) by the step's torque law.
 *   2. contact, explicitly from the state at the start of the sub-step: point k is r_k in the frame of body b_k; z_k its world height,
 *      xd_k = v_0 + (velocity of b_k's origin relative to the root's) + w_b x R_b r_k its world velocity; delta = ground_height - z_k.
 *      delta > 0:  f_n = max(0, stiffness delta - normal_damping xd_z),  f_t = -friction f_n xd_t / max(|xd_t|, slip_velocity)  (Coulomb, linear below
 *      the slip velocity; xd_t the horizontal part);  else f = 0.
 *   3. H(q) [a_0; alpha_0; q''] = [0; 0; tau - b v] - C(q, v, w_0) + sum_k J_k^T f_k + H [g; 0; 0],  diag(armature + h b) added to the joint block of
 *      the (6 + D) x (6 + D) inertia matrix H of the free-floating tree; a_0 = d v_0 / dt, alpha_0 = d w_0 / dt.
 *   4. v_0 += h a_0;  w_0 += h alpha_0;  v += h q'';  p_0 += h v_0;  R_0 <- exp(h w_0) R_0 (world-frame exponential map, renormalised);  q += h v;
 *      with enforce_limits the clamp of pbhc_joint_sim_step.
 * Frame: frame_root the integrated root state, frame_dof_pos / frame_dof_vel the integrated joints, frame_contact — for every body that owns contact
 * points — all three components of the sum of its points' forces at the LAST sub-step (no other element is written: the caller zeroes it once).
 * points: DEVICE [PBHC_ART_MAX_BODIES][PBHC_FLOAT_MAX_POINTS][3] (body frame, m; the whole table is read), of which body b uses the first
 * num_points[b].  tau0 (may be NULL): device [N,D], the
 * first sub-step's torque.  root_acc (may be NULL): device [N,6], the LAST sub-step's a_0 and alpha_0.
 * Per-env domain randomisation (every pointer may be NULL: the feature is off and the kernel runs the path it ran without it):
 *   env_inertial  DEVICE [N][PBHC_ART_MAX_BODIES][4], 16-byte aligned: row (n, b) = (mass, com_x, com_y, com_z) of body b in env n, which
 *                 replaces mass[b] and com[b] there (the inertia tensor about the centre of mass stays `inertia`); rows b >= B are 0.  The
 *                 values are the caller's statement (masses >= 0, the root's > 0): a device table is not read by the entry.
 *   env_friction  DEVICE [N], replaces `friction` in env n.
 *   push_counter  DEVICE int32 [N], push_interval DEVICE int32 [N] (whole seconds), push_vel DEVICE [N,2]: push_robots.  NULL together or
 *                 set together.  In front of the sub-steps of a control step, per env, dt the env's control step:
 *                   fire = push_counter == (int)((float)push_interval / dt);
 *                   fire: push_counter = 0;  push_interval = min(push_lo + (int)floor(u0 (push_hi - push_lo)), push_hi - 1);
 *                         push_vel = ((2 u1 - 1) max_push_vel_xy, (2 u2 - 1) max_push_vel_xy);  unless the previous step reset the env
 *                         (episode_length_buf == 0): v_0.xy += push_vel with push_fixed, v_0.xy = push_vel without;
 *                   push_counter += 1.
 *                 (u0, u1, u2): u_push [N,3] when non-NULL, else Philox stream 22 keyed (seed, env, step counter, 22, 0), words 0..2.
 *                 push_lo < push_hi, both >= 0, and max_push_vel_xy >= 0, else PBHC_EINVAL.  pbhc_debug_floating_substeps has no control
 *                 step: it honours env_inertial and env_friction for its n robots and refuses a non-NULL push_counter.
 * NULL pointers (io->root_states, points included), io->num_frames != 1, B > PBHC_ART_MAX_BODIES, decimation outside [1, 64], a negative mass,
 * armature, damping, stiffness, normal_damping or friction, slip_velocity <= 0, a root mass <= 0, num_points outside [0, PBHC_FLOAT_MAX_POINTS] or
 * not 0 for a body >= B, control type "V" return PBHC_EINVAL without a launch. */
#define PBHC_FLOAT_MAX_POINTS 4
typedef struct PbhcFloatingParams {
  float mass[PBHC_ART_MAX_BODIES];          /* m_b  kg, the root's included */
  float com[PBHC_ART_MAX_BODIES][3];        /* c_b  m, body frame */
  float inertia[PBHC_ART_MAX_BODIES][6];    /* I_b  kg m^2 about the centre of mass, body frame: xx yy zz xy xz yz */
  float armature[PBHC_MAX_DOF];             /* kg m^2, added to the diagonal of the joint block */
  float damping[PBHC_MAX_DOF];              /* b_d  N m s / rad, passive, taken implicitly */
  float gravity[3];                         /* m / s^2, world */
  float stiffness;                          /* N / m */
  float normal_damping;                     /* N s / m */
  float friction;
  float slip_velocity;                      /* m / s */
  float ground_height;                      /* m, world z of the plane */
  int32_t enforce_limits;
  int32_t decimation;
  int32_t num_points[PBHC_ART_MAX_BODIES];
  const float* points;
  float* tau0;
  float* root_acc;
  const float* env_inertial;
  const float* env_friction;
  int32_t* push_counter;
  int32_t* push_interval;
  float* push_vel;
  const float* u_push;
  int32_t push_lo;                          /* push_interval is drawn from {push_lo, ..., push_hi - 1}  s */
  int32_t push_hi;
  float max_push_vel_xy;                    /* m / s */
  int32_t push_fixed;                       /* != 0: the push is added to v_0.xy; 0: it replaces it */
} PbhcFloatingParams;
int pbhc_sizeof_floating_params(void);
int pbhc_floating_sim_step(PbhcEnv* env, const PbhcStepIO* io, const PbhcFloatingParams* params, void* stream);
/* Test-only: `steps` sub-steps of h seconds of the SAME device function as k_floating_sim under a constant torque, n independent robots.
 * root [n,13] as io->root_states; q, v, tau [n,D]; limits: HOST [D,2], read only with enforce_limits.  out_root [n,13], out_q, out_v [n,D] the final
 * state; out_acc0 [n,6+D] the FIRST sub-step's [a_0, alpha_0, q'']; out_force [n,B,PBHC_FLOAT_MAX_POINTS,3] the first sub-step's force on every point
 * (0 for a point a body does not have).  steps outside [1, 4096], h <= 0, NULL pointers and what pbhc_floating_sim_step refuses of the params
 * return PBHC_EINVAL without a launch. */
int pbhc_debug_floating_substeps(const PbhcSkeleton* skel, const PbhcFloatingParams* params, const float* root, const float* q, const float* v,
                                 const float* tau, int n, int steps, float h, int enforce_limits, const float* limits, float* out_root, float* out_q,
                                 float* out_v, float* out_acc0, float* out_force, void* stream);

/* Retargeting at ingestion (pbhc_amd/motion_retarget.py; csrc/pbhc_retarget.hip; definition: DESIGN §8 "Retargeting"; reference:
 * smpl_retarget/phc_retarget/fit_smpl_motion.py:137-179).  M clips concatenated: `starts` is the HOST array int32 [M + 1] (checked before any
 * launch), `d_starts` its device copy; every other array is a device pointer.  keypoints [total, P, 3] world-frame targets of the bodies
 * pick[0..P-1] (indices into the extended body list), trans [total, 3], dof [total, D], root_rot [total, 3] rotation vectors, root_off [M, 3].
 *   loss of clip c   = mean over (frame, pick) of |p_pick - target|, body positions by pbhc_motion_build's FK of
 *                      pose_aa = [root_rot, dof_axis[d] * dof[d], 0 for the extended bodies] rooted at trans + root_off[c].
 *   pbhc_retarget_loss_grad   loss_out [M] and the analytic gradients g_dof [total, D], g_root_rot [total, 3], g_root_off [M, 3]; no update.
 *                             body_pos_out [total, Bx, 3] or NULL; scratch: 4 * total floats.
 *   pbhc_retarget_fit         `iterations` iterations from the state it is handed, all enqueued on `stream` with no synchronisation: dof takes
 *                             torch's Adadelta step (dof_lr, rho, adadelta_eps), root_rot and root_off torch's Adam step (root_lr, beta1, beta2,
 *                             adam_eps), dof is clamped to `limits` and smoothed along time by `filter_taps` (5, or 0 = off) Gaussian taps of
 *                             `filter_sigma` frames, edge-replicated inside the clip.  loss_history [iterations, M]: the loss before each
 *                             update.  state->step (Adam's step count) advances by `iterations`: k, then n - k iterations equal n.
 *                             state->scratch: (D + 4) * total floats.
 *   pbhc_retarget_finish      clamps state->dof once more and writes pose_aa_out [total, Bx, 3], root_trans_out = trans + root_off [total, 3],
 *                             root_quat_out [total, 4] xyzw.
 * Sums run in pick order inside a frame and in an order fixed by the clip's own frame count across frames, with no atomics: a clip fitted
 * alone and inside a batch gives the same bits.  num_picks outside 1..PBHC_MAX_BODIES, a pick outside [0, Bx), filter_taps not 0 or 5, a
 * limit with lo > hi, total != starts[M], a clip of 0 frames, iterations < 1, NULL pointers return PBHC_EINVAL without a launch. */
typedef struct PbhcRetargetParams {
  int32_t num_picks;
  int32_t pick[PBHC_MAX_BODIES];
  float dof_lr;
  float root_lr;
  float rho;
  float adadelta_eps;
  float beta1;
  float beta2;
  float adam_eps;
  int32_t filter_taps;
  float filter_sigma;
  float limits[PBHC_MAX_DOF][2];
} PbhcRetargetParams;
typedef struct PbhcRetargetState {
  float* dof;        /* [total, D] */
  float* dof_sq;     /* [total, D] Adadelta square_avg */
  float* dof_acc;    /* [total, D] Adadelta acc_delta */
  float* root_rot;   /* [total, 3] */
  float* root_m;     /* [total, 3] Adam exp_avg */
  float* root_v;     /* [total, 3] Adam exp_avg_sq */
  float* root_off;   /* [M, 3] */
  float* off_m;      /* [M, 3] */
  float* off_v;      /* [M, 3] */
  float* scratch;    /* [(D + 4) * total] */
  int32_t step;      /* Adam steps taken so far */
} PbhcRetargetState;
int pbhc_sizeof_retarget_params(void);
int pbhc_sizeof_retarget_state(void);
int pbhc_retarget_loss_grad(const PbhcSkeleton* skel, const PbhcRetargetParams* params, const float* keypoints, const float* trans,
                            const float* dof, const float* root_rot, const float* root_off, int total, int num_clips, const int32_t* starts,
                            const int32_t* d_starts, float* loss_out, float* g_dof, float* g_root_rot, float* g_root_off, float* body_pos_out,
                            float* scratch, void* stream);
int pbhc_retarget_fit(const PbhcSkeleton* skel, const PbhcRetargetParams* params, const float* keypoints, const float* trans, int total,
                      int num_clips, const int32_t* starts, const int32_t* d_starts, PbhcRetargetState* state, int iterations,
                      float* loss_history, void* stream);
int pbhc_retarget_finish(const PbhcSkeleton* skel, const PbhcRetargetParams* params, const float* trans, int total, int num_clips,
                         const int32_t* starts, const int32_t* d_starts, PbhcRetargetState* state, float* pose_aa_out, float* root_trans_out,
                         float* root_quat_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
