// pbhc_partials.h — the columns of the partial-sum rows k_env_step writes (two rows per workgroup) and the env's reduction adds up
// (pbhc_env_finalize.h).  Expects include/pbhc_hip.h before it.
#pragma once

#define PBHC_NP 64   // partial sums per workgroup

// ------------------------------------------------------------------------------------------------
// partial-sum columns written per workgroup by k_env_step, reduced by k_env_finalize
enum {
  P_ERR = 0,            // [PBHC_NUM_SIGMA] tracking errors (adaptive sigma)
  P_UPPER_NORM = PBHC_NUM_SIGMA, P_LOWER_NORM, P_VR_NORM, P_JOINT_NORM, P_CLIP_CNT, P_RESET_CNT, P_TERM_GRAVITY, P_TERM_FAR,
  P_TERM_TIMEOUT, P_TERM_END, P_RESET_EPLEN, P_ETR_SUM, P_ETR_SQ, P_REW_SUM,
  P_KEY_NORM, P_LUP_NORM, P_LLO_NORM, P_LVR_NORM, P_LKEY_NORM, P_TERM_REFZ, P_TERM_REFORI, P_TERM_BODYZ,      // general tracking
  P_TERM_CONTACT, P_TERM_LOWH, P_TERM_POSLIM, P_TERM_VELLIM, P_TERM_TAULIM,
  P_NUM
};
static_assert(P_NUM <= PBHC_NP, "partials");
static_assert(PBHC_NP == PBHC_NUM_TOTALS, "totals");
