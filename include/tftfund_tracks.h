/* libtftfund: entry points added after library version 107 (tff_version() >= 108).  Included by tftfund.h; including it alone works too.
 *
 * ---- bundle adjustment over tracks: per-point visibility for M = 2 .. 6 views ---------------------------------------------------------------------------------
 * The header comment of the reference's BundleAdjustment.m (:4-22) says: "The points do not need to be seen in all cameras but at least in two ... If point n
 * is not seen in image m, then Corresp(2*m-1:2*m,n)=[NaN;NaN]".  Its code cannot do that (Normalize2Ddata.m:34-35 takes `mean` over the view, so one NaN
 * drops the whole view; tff_bundle_adjust_views_batch_* reproduce exactly that).  These two calls do what the comment says.  Arguments, layouts and outputs are
 * those of tff_bundle_adjust_views_batch_* (tftfund.h) plus `used`.  DEFINITION (tests/ba_tracks_oracle.py restates it in numpy):
 *   1. Observation (v, i) exists iff both of its coordinates are finite (a NaN or an Inf in either one: not seen).
 *   2. Point i takes part iff it has at least two observations.  Any other point is dropped before everything else: it enters no normalisation, no
 *      triangulation, no residual and no norm; its column of reconst is NaN, also when reconst0 was given.  used[b] = the number of points taking part.
 *   3. View v is normalised as Normalize2Ddata.m:33-39 does, over its n_v observations of points taking part: centroid and mean distance over n_v, not N.
 *      n_v = 0: the view is unseen, its camera keeps its initial angles and translation (its translation is scaled by 1/|t2| like every other).
 *      n_v >= 1 and a normalisation that is not finite (one observation, or coincident ones): status TFF_ST_NONFINITE, NaN in every output, iter 0.
 *   4. used == 0 (fewer than two seen views implies it): status TFF_ST_TOO_FEW, NaN in every output, iter 0.
 *   5. Without reconst0 every point is triangulated from the views that see it (:59-77).  Change of coordinates, Euler angles and variables as :80-100;
 *      residuals and Jacobian as :128-204, an observation that does not exist contributing zero rows.
 *   6. The Levenberg-Marquardt loop of every tff_bundle_adjust_* call; the norms of its step test run over all camera parameters and the points taking part.
 *   7. Rt(1:3,:) = eye(3,4), scale 1/|t2|, repr_err = |f| in normalised coordinates over the observations that exist.
 * An all-NaN column is inert (rule 2): appending such columns changes no bit of Rt, iter, repr_err, used, status or of the other columns of reconst.  Problems
 * of different N therefore go into one call padded with NaN columns; that is the ragged form of this call.  An item's outputs do not depend on the other items
 * of the batch.  On fully visible input the result agrees with tff_bundle_adjust_views_batch_* to rounding (the sums are the same, their code is not).
 * Every output pointer except Rt may be NULL.  TFF_E_INVALID, before any work: what tff_bundle_adjust_views_batch_* refuse (a null context, M outside 2 .. 6,
 * negative B or N, N = 0 with B > 0, a null calm, Rt_in, corresp or Rt, a calm_stride other than 0 or 9 M).  LDS: that of the whole-view call, 48 N bytes plus
 * a fixed part; nothing is kept per point beyond that (the visibility is read from the observations).  Workspace of the _host form: its staging, 4 B bytes more.
 * Losses for M views: tftfund_tracks_loss.h; covariances for M views: tftfund_tracks_cov.h.  Not here: more than six views, a loss in the polish of tff_robust_pose_scenes_* over
 * tracks, merging of tracks. */
#ifndef TFTFUND_TRACKS_H
#define TFTFUND_TRACKS_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

int tff_bundle_adjust_tracks_batch_dev(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                       int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                       int32_t* used, int32_t* status);
int tff_bundle_adjust_tracks_batch_host(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                        int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                        int32_t* used, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif
