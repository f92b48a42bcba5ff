/* libtftfund: entry points added after library version 103 (tff_version() >= 104).  Included by tftfund.h; including it alone works too.
 * The algorithm, the contract and the refusals of the adaptive robust call are stated in tftfund.h, under "the same with an early stop per scene". */
#ifndef TFTFUND_ADAPTIVE_H
#define TFTFUND_ADAPTIVE_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

int tff_robust_pose_scenes_adaptive_dev(tff_ctx* ctx, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int32_t ns_max,
                                        int64_t S, const double* calm, int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold,
                                        int32_t n_cand, int32_t lo_rounds, double confidence, int32_t first_round, double* Rt2, double* Rt3, double* T,
                                        uint8_t* mask, int32_t* info, int32_t* used, int32_t* status);
int tff_robust_pose_scenes_adaptive_host(tff_ctx* ctx, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t S, const double* calm,
                                         int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand,
                                         int32_t lo_rounds, double confidence, int32_t first_round, double* Rt2, double* Rt3, double* T, uint8_t* mask,
                                         int32_t* info, int32_t* used, int32_t* status);
/* The round ends and thresholds the adaptive call uses: ends[r - 1] = e_r, qmin[r - 1] = qmin_r for r = 1 .. *rounds (room for 32 each).  No context; any
 * n_hyp >= 1.  TFF_E_INVALID: the confidence, first_round, a null pointer, more than 32 rounds. */
int tff_robust_round_plan(double confidence, int64_t n_hyp, int32_t first_round, int64_t* ends, double* qmin, int32_t* rounds);

#ifdef __cplusplus
}
#endif
#endif
