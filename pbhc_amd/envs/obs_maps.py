"""The observation maps as host data: which features the observations read, where they sit in the feature row, every output element as
(dst, src, scale, noise), the same as runs and as the compact block image, and which waves write which row.  Python / numpy only — no
device, no pointer: pbhc_amd/envs/env_config.py (`build`, `_materialise`) turns the results into tensors and struct members.
"""
import numpy as np

from .. import _lib

K = _lib.K

# ---- observation key -> feature.  A new feature is added HERE: its key below, its width in feature_dims, its readiness class in
# FEATURE_CLASS0 / FEATURE_CLASS2 (and PBHC_F_<NAME> in the header)
OBS_FEATURES = {
    "base_lin_vel": "BASE_LIN_VEL", "base_ang_vel": "BASE_ANG_VEL", "projected_gravity": "PROJECTED_GRAVITY", "dof_pos": "DOF_POS",
    "dof_vel": "DOF_VEL", "actions": "ACTIONS", "ref_motion_phase": "REF_MOTION_PHASE",
    "dif_local_rigid_body_pos": "DIF_LOCAL_RIGID_BODY_POS", "local_ref_rigid_body_pos": "LOCAL_REF_RIGID_BODY_POS",
    "vr_3point_pos": "VR_3POINT_POS", "dr_base_com": "DR_BASE_COM", "dr_link_mass": "DR_LINK_MASS", "dr_kp": "DR_KP", "dr_kd": "DR_KD",
    "dr_friction": "DR_FRICTION", "dr_ctrl_delay": "DR_CTRL_DELAY", "relyaw": "RELYAW", "base_pos_z": "BASE_POS_Z",
    "dif_joint_angles": "DIF_JOINT_ANGLES", "dif_joint_velocities": "DIF_JOINT_VELOCITIES",
    "local_ref_rigid_body_vel": "LOCAL_REF_RIGID_BODY_VEL", "global_ref_rigid_body_vel": "GLOBAL_REF_RIGID_BODY_VEL",
    # legged_robot_base.py:1136-1146.  dof_pos_noise / dof_vel_noise are the clean joint values (live views of the simulator's, :370-371),
    # so they read the clean features; the two root-frame names read features of their own while obs.noise_process runs, and the clean
    # ones when it is off (:373-379 aliases them): see NOISE_PROCESS_FEATURES
    "base_ang_vel_noise": "BASE_ANG_VEL", "projected_gravity_noise": "PROJECTED_GRAVITY", "dof_pos_noise": "DOF_POS", "dof_vel_noise": "DOF_VEL",
}
# both envs: legged_robot_base.py:1117-1118; motion_tracking.py:950-952 / general_tracking.py:837-839 (the reference body VELOCITIES rotated by
# the relative-yaw inverse heading, whatever the name says)
OBS_FEATURES.update({"feet_contact_force": "FEET_CONTACT_FORCE", "local_ref_rigid_body_pos_relyaw": "REF_VEL_RELYAW"})
# the v1 env only (motion_tracking.py:977-990): constants and the look-ahead joint rows
OBS_FEATURES_V1 = {"indicator_guider": "ONE", "indicator_learner": "ZERO", "zero_vector": "ZERO",
                   "future_ref_dof_pos": "FUT_REF_DOF_POS", "future_ref_dof_vel": "FUT_REF_DOF_VEL"}
NOISE_PROCESS_FEATURES = {"base_ang_vel_noise": "BASE_ANG_VEL_NOISE", "projected_gravity_noise": "PROJECTED_GRAVITY_NOISE"}
# general tracking getters (general_tracking.py:821-954): plain features ...
OBS_FEATURES_V2 = {
    "roll_pitch": "ROLL_PITCH", "root_height": "BASE_POS_Z", "contact_mask": "CONTACT_MASK", "ref_contact_mask": "REF_CONTACT_MASK",
    "dr_base_mass": "DR_BASE_MASS", "anchor_ref_pos": "ANCHOR_REF_POS", "anchor_ref_rot": "ANCHOR_REF_ROT",
    "dif_root_velocity": "DIF_ROOT_VELOCITY", "dif_root_rot": "DIF_ROOT_ROT", "dif_root_height": "DIF_ROOT_HEIGHT",
}
# ... and keys that are gathers out of per-body / per-step feature tables: key -> features they read
OBS_GATHERS_V2 = {
    "local_key_body_pos": ["LOCAL_BODY_POS"], "local_key_body_rot": ["LOCAL_BODY_ROT"], "dif_local_key_body_pos": ["DIF_LOCAL_RIGID_BODY_POS"],
    "local_ref_key_body_pos": ["LOCAL_REF_RIGID_BODY_POS"], "future_motion_root_height": ["FUT_ROOT_HEIGHT"], "future_motion_roll_pitch": ["FUT_ROLL_PITCH"],
    "future_motion_base_lin_vel": ["FUT_BASE_LIN_VEL"], "future_motion_base_ang_vel": ["FUT_BASE_ANG_VEL"], "future_motion_base_yaw_vel": ["FUT_BASE_ANG_VEL"],
    "future_motion_dof_pos": ["FUT_DOF_POS"], "future_motion_local_ref_key_body_pos": ["FUT_LOCAL_KEY_POS"],
    "next_step_ref_motion": ["FUT_ROOT_HEIGHT", "FUT_ROLL_PITCH", "FUT_BASE_LIN_VEL", "FUT_BASE_ANG_VEL", "FUT_DOF_POS", "FUT_LOCAL_KEY_POS"],
}


def feature_dims(D, Bx, num_track, num_feet, S, Kb, Sr, link_mass_dim, hist_dim):
    """width of every feature.  The ORDER of this table is load-bearing: the features in use are laid out in the feature row in this
    order (feature_layout), so it decides every feat_off — append, never reorder."""
    return {
        "BASE_LIN_VEL": 3, "BASE_ANG_VEL": 3, "PROJECTED_GRAVITY": 3, "DOF_POS": D, "DOF_VEL": D, "ACTIONS": D, "REF_MOTION_PHASE": 1,
        "DIF_LOCAL_RIGID_BODY_POS": 3 * Bx, "LOCAL_REF_RIGID_BODY_POS": 3 * Bx, "VR_3POINT_POS": 3 * max(num_track, 1),
        "DR_BASE_COM": 3, "DR_LINK_MASS": max(link_mass_dim, 1), "DR_KP": D, "DR_KD": D, "DR_FRICTION": 1, "DR_CTRL_DELAY": 1,
        "RELYAW": 1, "BASE_POS_Z": 1, "DIF_JOINT_ANGLES": D, "DIF_JOINT_VELOCITIES": D, "LOCAL_REF_RIGID_BODY_VEL": 3 * Bx,
        "GLOBAL_REF_RIGID_BODY_VEL": 3 * Bx, "HISTORY": hist_dim, "ZERO": 1,
        "ROLL_PITCH": 2, "CONTACT_MASK": 2, "DR_BASE_MASS": 1, "LOCAL_BODY_POS": 3 * Bx, "LOCAL_BODY_ROT": 6 * Bx, "ANCHOR_REF_POS": 3,
        "ANCHOR_REF_ROT": 6, "DIF_ROOT_VELOCITY": 3, "DIF_ROOT_ROT": 4, "DIF_ROOT_HEIGHT": 1, "REF_CONTACT_MASK": 2,
        "FUT_ROOT_HEIGHT": max(S, 1), "FUT_ROLL_PITCH": max(2 * S, 1), "FUT_BASE_LIN_VEL": max(3 * S, 1), "FUT_BASE_ANG_VEL": max(3 * S, 1),
        "FUT_DOF_POS": max(S * D, 1), "FUT_LOCAL_KEY_POS": max(S * Kb * 3, 1),
        "BASE_ANG_VEL_NOISE": 3, "PROJECTED_GRAVITY_NOISE": 3,
        "ONE": 1, "FEET_CONTACT_FORCE": 3 * num_feet, "REF_VEL_RELYAW": 3 * Bx, "FUT_REF_DOF_POS": max(Sr * D, 1), "FUT_REF_DOF_VEL": max(Sr * D, 1),
    }


# readiness class of every feature word (see the compact maps, compact_image): which phase of the step kernel produces it.  0: before the
# dynamics chain ends, 2: post-reset; every feature in neither set is class 1
FEATURE_CLASS0 = {"HISTORY", "ZERO", "ONE", "BASE_LIN_VEL", "BASE_ANG_VEL", "PROJECTED_GRAVITY", "BASE_ANG_VEL_NOISE", "PROJECTED_GRAVITY_NOISE", "REF_MOTION_PHASE", "RELYAW", "ROLL_PITCH", "DR_BASE_COM",
                  "DR_LINK_MASS", "DR_FRICTION", "DR_BASE_MASS", "REF_CONTACT_MASK", "FUT_ROOT_HEIGHT", "FUT_ROLL_PITCH", "FUT_BASE_LIN_VEL",
                  "FUT_BASE_ANG_VEL", "FUT_DOF_POS", "FUT_LOCAL_KEY_POS"}
FEATURE_CLASS2 = {"DOF_POS", "DOF_VEL", "ACTIONS", "DR_KP", "DR_KD", "DR_CTRL_DELAY", "BASE_POS_Z", "CONTACT_MASK"}


def plain_key(key):
    return key[:-4] if key.endswith("_raw") else key


def history_layout(ob, dims):
    """(keys, frames per key, offset per key, width) of the history block: every key of obs_auxiliary with its longest history"""
    hist_len = {}
    for aux_cfg in ob.obs_auxiliary.values():
        for key, n in aux_cfg.items():
            hist_len[key] = max(hist_len.get(key, 0), int(n))
    hist_keys = sorted(hist_len.keys())
    hist_off, width = {}, 0
    for key in hist_keys:
        hist_off[key] = width
        width += hist_len[key] * dims[key]
    return hist_keys, hist_len, hist_off, max(width, 1)


def feature_layout(ob, feats, fdim, hist_keys, mode):
    """which features the observation maps read, and the feature row -> (used, offset of EVERY feature, readiness class per row word)"""
    # which features do the observation maps read?  the kernel skips the others (feat_off = -1)
    used = {"HISTORY", "ZERO"}
    for key in [plain_key(key) for keys in ob.obs_dict.values() for key in keys] + hist_keys:
        if key in feats:
            used.add(feats[key])
            if feats[key] == "REF_VEL_RELYAW":
                used.add("RELYAW")                   # the kernel derives the rotation from the relative yaw in the row
        elif mode == 1 and key in OBS_GATHERS_V2:
            used.update(OBS_GATHERS_V2[key])
    row_off, end = {}, 0
    for name, n in fdim.items():
        if name in used and name != "HISTORY":
            row_off[name] = end
            end += n
    trash = end                       # features nobody reads share one scratch region at the end of the row
    for name, n in fdim.items():
        if name not in used:
            row_off[name] = trash
            end = max(end, trash + n)
    # HISTORY is the LAST block of the feature index space: a specialised kernel keeps it out of the LDS feature row (csrc/pbhc_env_step.h:
    # step_lds_plan — the old history waits in registers and is staged over dead arrays once the termination flags are known)
    row_off["HISTORY"] = end
    end += fdim["HISTORY"]
    feat_class = np.ones(end, dtype=np.int64)
    for name in row_off:
        if name in used:
            feat_class[row_off[name]:row_off[name] + fdim[name]] = 0 if name in FEATURE_CLASS0 else (2 if name in FEATURE_CLASS2 else 1)
    return used, row_off, feat_class


def group_maps(ob, dims, L, feats, D, S, Sr, mode):
    """every output element as (dst, src, scale, noise): per observation group, then the history write-back ->
    [(name, dst, src, scale, noise, clip, pitch)].  `L`: the layout so far (feat_off, feat_dim_each, hist_*, key, group_dims)"""
    feat_off, fdim, hist_off, key_ids = L.feat_off, L.feat_dim_each, L.hist_off, L.key

    def key_sources(key):
        """feature-row indices of observation key `key` (flat, in the reference's element order)."""
        if key in ob.obs_auxiliary:                      # _get_obs_history_* (motion_tracking.py:993-1015)
            idx = []
            for hk, frames in sorted(ob.obs_auxiliary[key].items()):
                base = feat_off["HISTORY"] + hist_off[hk]
                idx.extend(range(base, base + int(frames) * dims[hk]))
            return idx
        if mode == 1 and key in OBS_GATHERS_V2:
            fo = lambda f: feat_off[f]
            per_body = lambda f, w: [fo(f) + w * b + j for b in key_ids for j in range(w)]
            if key == "local_key_body_pos":
                idx = per_body("LOCAL_BODY_POS", 3)
            elif key == "local_key_body_rot":
                idx = per_body("LOCAL_BODY_ROT", 6)
            elif key == "dif_local_key_body_pos":
                idx = per_body("DIF_LOCAL_RIGID_BODY_POS", 3)
            elif key == "local_ref_key_body_pos":
                idx = per_body("LOCAL_REF_RIGID_BODY_POS", 3)
            elif key == "future_motion_base_yaw_vel":
                idx = [fo("FUT_BASE_ANG_VEL") + 3 * st + 2 for st in range(S)]
            elif key == "next_step_ref_motion":                       # step-0 slices, general_tracking.py:554-564
                idx = ([fo("FUT_ROOT_HEIGHT")] + [fo("FUT_ROLL_PITCH") + j for j in range(2)] + [fo("FUT_BASE_LIN_VEL") + j for j in range(3)]
                       + [fo("FUT_BASE_ANG_VEL") + 2] + [fo("FUT_DOF_POS") + j for j in range(D)] + [fo("FUT_LOCAL_KEY_POS") + j for j in range(3 * len(key_ids))])
            else:
                f = OBS_GATHERS_V2[key][0]
                idx = list(range(fo(f), fo(f) + fdim[f]))
            if (key.startswith("future_") or key == "next_step_ref_motion") and not S:
                raise _lib.PbhcError(f"observation {key!r} needs obs.future_num_steps > 0")
            if len(idx) != dims[key] * (S if (key.startswith("future_motion_") and S) else 1):       # future keys list their PER-STEP dim
                raise _lib.PbhcError(f"obs_dims[{key}]={dims[key]} does not match the {len(idx)} values the env produces")
            return idx
        if key not in feats:
            raise NotImplementedError(f"observation {key!r} has no HIP implementation")
        f = feats[key]
        if key == "zero_vector":                         # obs_dims.zero_vector zeros (motion_tracking.py:983-984)
            return [feat_off["ZERO"]] * dims[key]
        if key in ("future_ref_dof_pos", "future_ref_dof_vel"):
            if not Sr:
                raise _lib.PbhcError(f"observation {key!r} needs obs.future_ref_steps > 0")
            if dims[key] != Sr * D:
                raise _lib.PbhcError(f"obs_dims[{key}]={dims[key]} does not match future_ref_steps x dofs = {Sr * D}")
        if dims[key] > fdim[f]:
            raise _lib.PbhcError(f"obs_dims[{key}]={dims[key]} exceeds the feature size {fdim[f]}")
        idx = list(range(feat_off[f], feat_off[f] + dims[key]))
        if key == "dof_vel" and mode == 1 and ob.get("masked_dof_vel", False):       # general_tracking.py:821-829
            for j in (4, 5, 10, 11):
                idx[j] = feat_off["ZERO"]
        return idx

    if len(ob.obs_dict) + 1 > K["PBHC_MAX_GROUPS"]:            # + history write-back
        raise _lib.PbhcError("too many observation groups")
    maps = []
    for group, keys in ob.obs_dict.items():
        src, scale, noise = [], [], []
        for key in sorted(keys):
            k = plain_key(key)
            key_scale, key_noise = float(ob.obs_scales[k]), (0.0 if key.endswith("_raw") else float(ob.noise_scales[k]))
            idx = key_sources(k)
            src.extend(idx); scale.extend([key_scale] * len(idx)); noise.extend([key_noise] * len(idx))
        assert len(src) == L.group_dims[group], (group, len(src), L.group_dims[group])
        maps.append((group, list(range(len(src))), src, scale, noise, 1, L.group_dims[group]))
    # history write-back: new[k][0] = parse(current k), new[k][t] = old[k][t-1]  (history_handler.py:40-44)
    dst, src, scale, noise = [], [], [], []
    for hk in L.hist_keys:
        cur = key_sources(hk)
        o0 = hist_off[hk]
        dst.extend(range(o0, o0 + len(cur))); src.extend(cur); scale.extend([float(ob.obs_scales[hk])] * len(cur)); noise.extend([float(ob.noise_scales[hk])] * len(cur))
        n_old = (L.hist_len[hk] - 1) * dims[hk]
        base = feat_off["HISTORY"] + o0
        dst.extend(range(o0 + dims[hk], o0 + dims[hk] + n_old)); src.extend(range(base, base + n_old)); scale.extend([1.0] * n_old); noise.extend([0.0] * n_old)
    if not src:
        dst, src, scale, noise = [0], [feat_off["ZERO"]], [1.0], [0.0]
    maps.append(("__history__", dst, src, scale, noise, 0, L.hist_dim))
    for group, _, src, *_ in maps:
        if not src:
            raise _lib.PbhcError(f"observation group {group} has no non-history element")
    return maps


def run_length(group_map, feat_class, history_off):
    """a map as runs of consecutive (dst, src) with one scale / noise / readiness class (PbhcObsRun: [dst, src, len, late, scale, noise]):
    what the config-specialised kernel unrolls into straight-line code.  None when there are more than PBHC_MAX_RUNS (num_runs = -1 in
    the struct)"""
    _, dst, src, scale, noise, _, _ = group_map
    runs = []
    for j in range(len(src)):
        late = int(feat_class[src[j]]) == 2
        last = runs[-1] if runs else None
        if last and last[0] + last[2] == dst[j] and last[1] + last[2] == src[j] and last[3] == late \
                and last[4] == scale[j] and last[5] == noise[j] and src[j] != history_off:        # (no run straddles the history block)
            last[2] += 1
        else:
            runs.append([dst[j], src[j], 1, late, scale[j], noise[j]])
    return runs if len(runs) <= K["PBHC_MAX_RUNS"] else None


def compact_image(maps, feat_class):
    """compact form of the maps (16 bits per element, staged in LDS by the kernel): one uint32 block per group, or None.  Possible when
    every group writes its row in order and has at most PBHC_MAX_SEGS distinct (scale, noise) pairs"""
    seg_tables = [sorted(set(zip(scale, noise))) for _, _, _, scale, noise, _, _ in maps]
    if len(feat_class) > 4096 or any(dst != list(range(len(dst))) or len(pairs) > K["PBHC_MAX_SEGS"]
                                      for (_, dst, *_), pairs in zip(maps, seg_tables)):
        return None
    image = []
    for (_, _, src, scale, noise, _, _), pairs in zip(maps, seg_tables):
        seg_of = {p: seg for seg, p in enumerate(pairs)}
        packed = np.array([s | (seg_of[(a, b)] << 12) for s, a, b in zip(src, scale, noise)] + [0] * (len(src) % 2), dtype=np.uint16)
        tabs = np.zeros(32, dtype=np.float32)
        for seg, (a, b) in enumerate(pairs):
            tabs[seg], tabs[16 + seg] = a, b
        if len(src) >= 65536:
            raise _lib.PbhcError("observation group too wide for the compact maps")
        # The kernel writes a row in element PAIRS (one 8-byte store), in two passes by readiness of the pair's sources (feat_class):
        # "early" = everything but the post-reset features (history, DR, per-env scalars, reference / future targets, difference
        # features), written while the dynamics chain still runs; "late" = pairs that read a post-reset feature.  A pair that holds a
        # noisy element belongs to neither: both of its elements go to the noise list, which the kernel visits last.
        n_el = len(src)
        npair = (n_el + 1) // 2
        pair_noisy = [any(noise[j] != 0.0 for j in (2 * p, 2 * p + 1) if j < n_el) for p in range(npair)]
        pair_late = [any(int(feat_class[src[j]]) == 2 for j in (2 * p, 2 * p + 1) if j < n_el) for p in range(npair)]
        early = [p for p in range(npair) if not pair_noisy[p] and not pair_late[p]]
        late = [p for p in range(npair) if not pair_noisy[p] and pair_late[p]]
        plist = np.array(early + late + [0] * ((len(early) + len(late)) % 2), dtype=np.uint16)
        noisy_e = [j | (int(packed[j]) << 16) for j in range(n_el) if pair_noisy[j // 2] and not pair_late[j // 2]]
        noisy_l = [j | (int(packed[j]) << 16) for j in range(n_el) if pair_noisy[j // 2] and pair_late[j // 2]]
        if noisy_e:
            noisy_e += [noisy_e[-1]] * ((-len(noisy_e)) % 4)      # early list padded to a Philox quad (repeats rewrite the same value)
        noisy = np.array(noisy_e + noisy_l, dtype=np.uint32)
        hdr = np.array([len(noisy_e), len(noisy_l), len(early), len(late)], dtype=np.uint32)
        image.append(np.concatenate([tabs.view(np.uint32), hdr, plist.view(np.uint32), noisy, packed.view(np.uint32)]))
    return image


def assign_roles(maps, runs, feat_off, fdim, role0_handicap, row_help_share, mode):
    """who writes which row -> (role per group, {(group, run)} handed to the dynamics waves).  Role 0: dynamics waves, free once their
    reward phase is done; role 1: reference / observation waves.  Greedy by width, role 0 handicapped by the work of its reward / reset
    phases; a row that reads future targets — produced by role 1 while role 0 already writes — stays with role 1."""
    fut_lo = min([feat_off[f] for f in feat_off if f.startswith("FUT_")] or [1 << 30])
    fut_hi = max([feat_off[f] + fdim[f] for f in feat_off if f.startswith("FUT_")] or [-1])
    elements = sum(len(m[2]) for m in maps)
    # Round 4: v1 hands EVERY row to role 1 (role0_handicap 1e9) — with them the history block leaves the LDS feature row (step_lds_plan: a
    # fifth workgroup per CU), and role 0, the chain that sets a workgroup's duration, ends with its reward / reset phases.
    load = [role0_handicap * elements, 0.0]
    roles = [0] * len(maps)
    for i in sorted(range(len(maps)), key=lambda i_: -len(maps[i_][2])):
        reads_future = any(fut_lo <= s < fut_hi for s in maps[i][2])
        roles[i] = 1 if (reads_future or load[1] <= load[0]) else 0
        load[roles[i]] += len(maps[i][2])
    # ... of which the dynamics waves take the share that balances the two roles after bar2 (they idle for ~2.3 k cycles after their reward /
    # reset phases while the reference waves write 1 010 elements): whole runs that read no history (that block is staged by the reference
    # waves), largest first, marked in PbhcObsRun.late bit 1.  The specialised kernel honours the marks in the builds whose history block
    # lives outside the feature row (step_lds_plan); every other build lets the reference waves write all runs.
    # Measured (profiles/round4_k_env_step_variants.txt (h)): shares of 0.15 / 0.23 / 0.32 give 18.3-18.6 us against 18.2 at 4096 envs and nothing
    # at 32 768 — the launch's tail is the chip-wide store drain, not the reference waves' instruction stream — so the default share is 0.
    helper_runs = set()
    if mode == 0 and row_help_share > 0.0 and all(r == 1 for r in roles) and all(rs is not None for rs in runs):
        candidates = sorted(((rs[r][2], i, r) for i, rs in enumerate(runs) for r in range(len(rs)) if rs[r][1] + rs[r][2] <= feat_off["HISTORY"]), reverse=True)
        budget = row_help_share * elements
        for n, i, r in candidates:
            if n <= budget:
                helper_runs.add((i, r))
                budget -= n
    return roles, helper_runs
