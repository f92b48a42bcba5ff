/* libtftfund: entry points added after library version 104 (tff_version() >= 105).  Included by tftfund.h; including it alone works too.
 *
 * ---- quality-guided (PROSAC) sampling for the robust estimators ------------------------------------------------------------------------------------------
 * Match lists come with a score per match.  PROSAC (Chum & Matas, CVPR 2005) draws the early hypotheses from the best-ranked matches and widens the pool
 * as the hypothesis index grows; after `growth` draws the sampling is the uniform one.  The pool is a function of the hypothesis index alone, so the sampler
 * stays counter-based and every bitwise contract of the robust calls (a scene alone = a scene in a list, any chunk, any round, used[] reproduces) holds.
 *
 * THE DEFINITION, for one scene of N correspondences, the sample size m = n_sample and G = growth (1 <= G <= 2^31 - 2^25: PROSAC's T_N); the numpy twins
 * api.guided_pool_ends and api.sample_indices_guided_reference compute the same, index for index:
 *   T(n) for n = m .. N, in double, each n on its own: T = (double)G; for i = 0 .. m-1: T = T * (double)(n - i) / (double)(N - i) -- multiply, then divide,
 *     in that order.  No other operation is used, so nothing can be contracted into an FMA.
 *   ends[m] = 1; ends[n + 1] = ends[n] + (int)ceil(T(n + 1) - T(n)), in integers from there on.  ends[N] <= G + N.
 *   pool(t) for the 1-based hypothesis t = h + 1: the smallest n in [m, N] with ends[n] >= t; if t > ends[N] the draw is uniform.
 *   Ranks of hypothesis h: with a pool n, the m - 1 ranks the sampler of tff_sample_indices_dev gives for (seed, h, m - 1, n - 1) -- distinct, in
 *     [0, n - 1) -- followed by rank n - 1 as the last entry (so h = 0 draws the ranks 0 .. m-1); when uniform, that sampler's ranks for (seed, h, m, N),
 *     exactly the draw of the calls without a ranking.
 *   Indices: order[rank], where order is the scene's ranking, best first, as local indices 0 .. N-1.  An entry of order outside [0, N) makes every
 *     hypothesis that draws it a row of -1, which the pose kernels treat as "no hypothesis" (TFF_ST_TOO_FEW, never a candidate); such an entry is never used
 *     as an address.  Duplicates in order are no error: they only produce degenerate samples.
 *
 * tff_robust_pose_scenes_guided_dev / _host: the arguments of the adaptive call (tftfund.h, tftfund_adaptive.h) plus order -- n_total int32 packed like the
 * scenes (the ranking of scene s at order[scene_offsets[s] ..]); a device pointer for _dev, a host pointer for _host -- and growth, both after first_round.
 * Scene s draws with seed + s.  confidence == 0 means a fixed n_hyp and no rounds: first_round is not read, used may be null, and if given every entry is
 * filled with n_hyp.  With a confidence the rounds and the stop rule are the EXISTING ones, unchanged: the rule is evaluated on the whole scene and stays
 * valid (conservative) under guided sampling.  PROSAC's own termination criterion is deliberately out of scope.  Everything after the sampler -- the pose
 * kernels, the counts, the selection, the re-draw of the candidates from their keys (by the same function of h), the refits, the masks -- is that of
 * tff_robust_pose_scenes_*.
 * THE CONTRACT: the outputs of scene s are bit for bit those of the same call on that scene alone (S = 1, its ranking, the seed seed + s), and with a
 * confidence those of the fixed guided call with n_hyp = used[s].
 * TFF_E_INVALID, before any work, each with a tff_last_error text: a null context; a null order; growth outside [1, 2^31 - 2^25]; everything the adaptive
 * call refuses (with confidence == 0: everything tff_robust_pose_scenes_* refuses).  _host validates the offsets as the other _host forms do.
 * _dev: no host synchronisation and no device-to-host copy.  Workspace beyond the other calls', reserved before anything goes on the stream: 4 n_total
 * bytes for the pool tables (8 n_total for _host, which stages the ranking).
 *
 * tff_sample_indices_guided_dev: the twin of tff_sample_indices_dev -- row b of sample_idx (B x n int32) = the indices of hypothesis first + b of one scene
 * of Ns correspondences ranked by order (Ns int32, device).  The scene's table is computed on the stream first.  1 <= n <= 16, n <= Ns <= 2^24. */
#ifndef TFTFUND_GUIDED_H
#define TFTFUND_GUIDED_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

int tff_robust_pose_scenes_guided_dev(tff_ctx* ctx, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int32_t ns_max,
                                      int64_t S, const double* calm, int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold,
                                      int32_t n_cand, int32_t lo_rounds, double confidence, int32_t first_round, const int32_t* order, int64_t growth,
                                      double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* used, int32_t* status);
int tff_robust_pose_scenes_guided_host(tff_ctx* ctx, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t S, const double* calm,
                                       int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand,
                                       int32_t lo_rounds, double confidence, int32_t first_round, const int32_t* order, int64_t growth, double* Rt2,
                                       double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* used, int32_t* status);
int tff_sample_indices_guided_dev(tff_ctx* ctx, uint64_t seed, int64_t first, int64_t B, int32_t n, int32_t Ns, const int32_t* order, int64_t growth,
                                  int32_t* sample_idx);

#ifdef __cplusplus
}
#endif
#endif
