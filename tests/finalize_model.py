"""A plain model of the env step's one-workgroup reduction (csrc/pbhc_env_finalize.h): what the reference does on the host after every step,
restated as straight-line scalar numpy code on the 64 column totals of the step's partial rows.

    finalize_model(totals, cfg, globals, cursor, num_frames, n) -> (globals, cursor)

`totals` [PBHC_NUM_TOTALS] float64 column totals; `cfg` a mapping of the config fields the reduction reads (`cfg_from_struct` makes one from a
`PbhcEnvConfig`, so that the model sees the fp32 values the kernel sees); `globals` the env's double vector before the step; `n` the number of
envs the totals were taken over.  Python floats / float64 wherever the reference computes with Python floats, `np.float32` exactly where it
holds an fp32 value: the batch mean of an error (`error.mean().item()`) and the average episode length (a 0-dim fp32 tensor).

The rules, from the reference:
  adaptive sigma            motion_tracking.py:1030-1048 (v1: "scale", "mean" = (min(ema, sigma) + ema) / 2, "origin"),
                            general_tracking.py:970-991 (v2: "mean" = ema)
  average episode length    legged_robot_base.py:875-879, called from _reset_buffers_callback (:684) for a non-empty set of reset envs only
  penalty curriculum        legged_robot_base.py:882-900
  soft-limit curricula      legged_robot_base.py:902-939
  noise curriculum          legged_robot_base.py:637-645 (_update_obs_noise_curriculum, from _reset_tasks_callback :591-592; its up threshold
                            is rewards.reward_penalty_level_up_threshold)
  end time ratio, motion-far / dof-far threshold curricula      motion_tracking.py:272-317 (only when an env was reset: :266-267)
  per-cause termination means                                    legged_robot_base.py (_update_reset_buf): mean(cause) / (mean(reset_buf) + 1e-15)

Column and slot indices are read from the header (`_lib.K`) and from csrc/pbhc_partials.h; nothing is retyped here.

Where the device deliberately differs from the reference (pinned by tests/test_gpu_env_finalize.py):
  * `end_time_ratio_std` of ONE env: torch's unbiased std() of one element is NaN; the kernel (and this model) writes 0 when the variance
    estimate is not positive — 0 / 0 included.
  * the termination means and the end-time-ratio statistics are formed in double from exact column totals, the reference forms them in fp32.
"""
import math
import os
import re

import numpy as np

from pbhc_amd import _lib

K = _lib.K
f32 = np.float32


def _partial_columns():
    text = _lib._strip_comments(open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "pbhc_partials.h")).read())
    body = re.search(r"enum\s*\{(.*?)\}", text, flags=re.S).group(1)
    out, val = {}, -1
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        if "=" in item:
            name, v = [x.strip() for x in item.split("=")]
            val = int(eval(v, {}, dict(K, **out)))
        else:
            name, val = item, val + 1
        out[name] = val
    return out


P = _partial_columns()
assert P["P_NUM"] <= K["PBHC_NUM_TOTALS"] and P["P_UPPER_NORM"] == K["PBHC_NUM_SIGMA"]

CFG_FIELDS = ["num_envs", "adaptive_sigma", "adaptive_type", "adaptive_scale", "adaptive_alpha", "penalty_curriculum", "penalty_degree", "penalty_down",
              "penalty_up", "penalty_min", "penalty_max", "noise_curriculum", "noise_degree", "noise_down", "noise_up", "noise_min", "noise_max",
              "num_compute_average_epl", "soft_pos_curriculum", "soft_vel_curriculum", "soft_tau_curriculum", "terminate_when_motion_far",
              "motion_far_curriculum", "motion_far_degree", "motion_far_down", "motion_far_up", "motion_far_min", "motion_far_max", "tracking_mode",
              "terminate_when_dof_far", "dof_far_curriculum", "dof_far_degree", "dof_far_down", "dof_far_up", "dof_far_min", "dof_far_max"]
CFG_ARRAYS = ["sigma_active", "soft_cur_degree", "soft_cur_down", "soft_cur_up", "soft_cur_min", "soft_cur_max"]


def cfg_from_struct(c):
    """the fields the reduction reads, out of a `PbhcEnvConfig` (ints stay ints, floats are the struct's fp32 values as Python floats)"""
    cfg = {k: getattr(c, k) for k in CFG_FIELDS}
    cfg.update({k: list(getattr(c, k)) for k in CFG_ARRAYS})
    cfg["num_dof"] = c.skel.num_dof
    return cfg


def _clip(v, lo, hi):
    return min(max(v, lo), hi)                           # np.clip of a Python float


def _move(v, avg, down, up, degree, lo, hi, widen_when_short):
    """one curriculum: the value moves by (1 +/- degree) when the fp32 average episode length is below `down` / above `up`, then is clipped.
    widen_when_short: (1 + degree) below `down` (limits, thresholds); else (1 - degree) below `down` (penalty scale, noise)"""
    if avg < f32(down):
        v = v * (1.0 + degree) if widen_when_short else v * (1.0 - degree)
    elif avg > f32(up):
        v = v * (1.0 - degree) if widen_when_short else v * (1.0 + degree)
    return _clip(v, lo, hi)


def finalize_model(totals, cfg, globals, cursor, num_frames, n, advance=True):
    """-> (globals after the step, cursor after the step).  advance=False: the data-parallel apply (`pbhc_env_finalize`), which leaves the step
    counter and the replay cursor to the reduce half."""
    t = [float(x) for x in np.asarray(totals, np.float64)]
    g = np.array(globals, np.float64, copy=True)
    n = float(n)
    G = lambda name: K["PBHC_G_" + name]
    L = lambda name: K["PBHC_G_LOG"] + K["PBHC_L_" + name]

    # ---- adaptive sigma: motion_tracking.py:1030-1048, general_tracking.py:970-991
    if cfg["adaptive_sigma"]:
        alpha, scale, kind = float(cfg["adaptive_alpha"]), float(cfg["adaptive_scale"]), cfg["adaptive_type"]
        for i in range(K["PBHC_NUM_SIGMA"]):
            if not cfg["sigma_active"][i]:
                continue
            mean = float(f32(t[P["P_ERR"] + i] / n))                      # error.mean().item(): an fp32 value
            ema = float(g[G("EMA") + i]) * (1.0 - alpha) + mean * alpha
            sigma = float(g[G("SIGMA") + i])
            if kind == 2:                                                  # "scale"
                sigma = min(ema * scale, sigma)
            elif kind == 1:                                                # v1 "mean"
                sigma = (min(ema, sigma) + ema) / 2
            elif kind == 3:                                                # v2 "mean"
                sigma = ema
            else:                                                          # "origin"
                sigma = min(ema, sigma)
            g[G("EMA") + i], g[G("SIGMA") + i] = ema, sigma

    # ---- logged means
    nreset = t[P["P_RESET_CNT"]]
    rfrac = nreset / n
    g[L("UPPER_BODY_DIFF_NORM")] = t[P["P_UPPER_NORM"]] / n
    g[L("LOWER_BODY_DIFF_NORM")] = t[P["P_LOWER_NORM"]] / n
    g[L("VR_3POINT_DIFF_NORM")] = t[P["P_VR_NORM"]] / n
    g[L("JOINT_POS_DIFF_NORM")] = t[P["P_JOINT_NORM"]] / n
    g[L("ACTION_CLIP_FRAC")] = t[P["P_CLIP_CNT"]] / (n * float(cfg["num_dof"]))
    g[L("RESET_FRAC")] = rfrac
    g[L("NUM_RESETS")] = nreset
    g[L("REW_MEAN")] = t[P["P_REW_SUM"]] / n
    cause = lambda col: (t[P[col]] / n) / (rfrac + 1e-15)
    g[L("TERM_GRAVITY")] = cause("P_TERM_GRAVITY")
    g[L("TERM_MOTION_FAR")] = cause("P_TERM_FAR")
    g[L("TERM_TIME_OUT")] = cause("P_TERM_TIMEOUT")
    g[L("TERM_MOTION_END")] = cause("P_TERM_END")
    g[L("TERM_CONTACT")] = cause("P_TERM_CONTACT")
    g[L("TERM_LOW_HEIGHT")] = cause("P_TERM_LOWH")
    g[L("TERM_DOF_POS_LIMIT")] = cause("P_TERM_POSLIM")
    g[L("TERM_DOF_VEL_LIMIT")] = cause("P_TERM_VELLIM")
    g[L("TERM_TORQUE_LIMIT")] = cause("P_TERM_TAULIM")
    if cfg["terminate_when_dof_far"]:                    # a batch-wide flag: its env-mean is the flag; cleared for the next step's pre-pass
        g[L("TERM_DOF_FAR")] = float(g[G("DOF_FAR_HIT")]) / (rfrac + 1e-15)
        g[G("DOF_FAR_HIT")] = 0.0
        g[L("DOF_FAR_THR")] = g[G("DOF_FAR_THR")]        # the threshold this step's test used (logged before the curriculum moves it)
    if cfg["tracking_mode"]:
        g[L("TERM_REF_POS_Z")] = cause("P_TERM_REFZ")
        g[L("TERM_REF_ORI")] = cause("P_TERM_REFORI")
        g[L("TERM_BODY_Z")] = cause("P_TERM_BODYZ")
        g[L("KEY_BODY_DIFF_NORM")] = t[P["P_KEY_NORM"]] / n
        g[L("LOCAL_UPPER_BODY_DIFF_NORM")] = t[P["P_LUP_NORM"]] / n
        g[L("LOCAL_LOWER_BODY_DIFF_NORM")] = t[P["P_LLO_NORM"]] / n
        g[L("LOCAL_VR_3POINT_DIFF_NORM")] = t[P["P_LVR_NORM"]] / n
        g[L("LOCAL_KEY_BODY_DIFF_NORM")] = t[P["P_LKEY_NORM"]] / n

    if nreset > 0.0:                                     # everything below hangs on reset_envs_idx of a non-empty set
        # ---- legged_robot_base.py:875-879: fp32 throughout (a 0-dim fp32 tensor times Python floats)
        cur = f32(t[P["P_RESET_EPLEN"]] / nreset)
        frac = nreset / float(cfg["num_compute_average_epl"])
        avg = f32(f32(g[G("AVG_EP_LEN")]) * f32(1.0 - frac)) + f32(cur * f32(frac))
        avg = f32(avg)
        g[G("AVG_EP_LEN")] = float(avg)
        if cfg["penalty_curriculum"]:                    # legged_robot_base.py:882-900
            g[G("PENALTY_SCALE")] = _move(float(g[G("PENALTY_SCALE")]), avg, cfg["penalty_down"], cfg["penalty_up"], float(cfg["penalty_degree"]),
                                          float(cfg["penalty_min"]), float(cfg["penalty_max"]), widen_when_short=False)
        for q, (on, slot) in enumerate((("soft_pos_curriculum", "SOFT_POS_VAL"), ("soft_vel_curriculum", "SOFT_VEL_VAL"), ("soft_tau_curriculum", "SOFT_TAU_VAL"))):
            if cfg[on]:                                  # legged_robot_base.py:902-939
                g[G(slot)] = _move(float(g[G(slot)]), avg, cfg["soft_cur_down"][q], cfg["soft_cur_up"][q], float(cfg["soft_cur_degree"][q]),
                                   float(cfg["soft_cur_min"][q]), float(cfg["soft_cur_max"][q]), widen_when_short=True)
        if cfg["noise_curriculum"]:                      # legged_robot_base.py:637-645
            g[G("NOISE_CURRICULUM")] = _move(float(g[G("NOISE_CURRICULUM")]), avg, cfg["noise_down"], cfg["noise_up"], float(cfg["noise_degree"]),
                                             float(cfg["noise_min"]), float(cfg["noise_max"]), widen_when_short=False)
        if cfg["terminate_when_motion_far"] and cfg["motion_far_curriculum"]:      # motion_tracking.py:309-317
            g[G("MOTION_FAR_THR")] = _move(float(g[G("MOTION_FAR_THR")]), avg, cfg["motion_far_down"], cfg["motion_far_up"], float(cfg["motion_far_degree"]),
                                           float(cfg["motion_far_min"]), float(cfg["motion_far_max"]), widen_when_short=True)
        if cfg["terminate_when_dof_far"] and cfg["dof_far_curriculum"]:            # motion_tracking.py:298-307
            g[G("DOF_FAR_THR")] = _move(float(g[G("DOF_FAR_THR")]), avg, cfg["dof_far_down"], cfg["dof_far_up"], float(cfg["dof_far_degree"]),
                                        float(cfg["dof_far_min"]), float(cfg["dof_far_max"]), widen_when_short=True)
        # ---- motion_tracking.py:275-276: mean and unbiased std of end_time_ratio_buf over ALL envs
        mean = t[P["P_ETR_SUM"]] / n
        num, den = t[P["P_ETR_SQ"]] - n * mean * mean, n - 1.0
        var = num / den if den != 0.0 else (math.nan if num == 0.0 else math.copysign(math.inf, num))
        g[L("END_TIME_RATIO")] = mean
        g[L("END_TIME_RATIO_STD")] = math.sqrt(var) if var > 0.0 else 0.0

    if advance:
        g[G("STEP_COUNTER")] += 1.0
        cursor = (int(cursor) + 1) % int(num_frames)
    return g, cursor
