/* libtftfund: entry points added after library version 108 (tff_version() >= 109).  Included by tftfund.h; including it alone works too.
 *
 * ---- robust losses (Huber, Cauchy) for the bundle adjustment over tracks, M = 2 .. 6 views ------------------------------------------------------------------
 * tff_bundle_adjust_tracks_batch_* (tftfund_tracks.h) are plain least squares: on raw matches a track of five good observations and one wrong one is
 * the normal case, and that one observation pulls every camera.  These two calls take the arguments of tff_bundle_adjust_tracks_batch_* followed by
 * `int32_t loss, double scale, double* weight`.  Everything not named here is what tftfund_tracks.h rules 1 - 7 say.  DEFINITION
 * (tests/ba_tracks_loss_oracle.py restates it in numpy):
 *   1. The loss is PER OBSERVATION, not per point.  With s_v the isotropic scale of view v's normalisation (over its own n_v observations, rule 3 of
 *      tftfund_tracks.h; an unseen view has s_v = 1 and contributes no rows) the pixel residual of observation (v, i) is e_{v,i} = r_{v,i} / s_v, a
 *      2-vector, and F = sum over the observations that exist of rho(|e_{v,i}|^2).  rho, rho' and the loss codes TFF_LOSS_HUBER, TFF_LOSS_CAUCHY with
 *      the scale c > 0 in pixels are those of tftfund_loss.h.  This differs on purpose from the three-view call of that header, which weighs a whole
 *      correspondence: in a track the unit that goes wrong is one observation.
 *   2. Reweighting: at the current parameters w_{v,i} = rho'(|e_{v,i}|^2); the two residual rows of observation (v, i) and the same rows of both
 *      Jacobians are multiplied by sqrt(w_{v,i}) / s_v before anything is accumulated (the point blocks, the Schur sums, the gradient, the
 *      back-substitution of the points).  The weights are those of the current point; there is no second-order term.
 *   3. Gauge: the step is freed of its component along v = (0 for all angles; t_j for every camera j that is seen; X_i for every point taking part),
 *      step -= v (v . step) / (v . v), as in the three-view loss loop.  An unseen camera is not in v: it keeps its start exactly, as in the plain call.
 *   4. The P x P Schur system (P = 6 (M - 1)) is solved without the plain call's pivot floor; a zero or non-finite pivot gives TFF_ST_NONFINITE.  The
 *      diagonal of an unseen camera's block is 1, as in the plain call.
 *   5. Damping floor: after a successful step lambda = max(lambda / 10, 1e-3).  Everything else in the loop is the plain one: start 0.01, x10 on a
 *      rejected trial, both tolerances 1e-6, at most 400 iterations, the same step test, the same stop at lambda > 1e16.  Why: in pixels the matrix is
 *      about 1e9 and its rounding about 1e-7; the gauge direction's pivot is the damping alone, and a slowly converging Huber run (linear convergence,
 *      a hundred successes) would otherwise carry lambda below the rounding within ten successes.
 *   6. The costs that steer acceptance and the function tolerance are F at the current and at the trial parameters.  repr_err = sqrt(F) at the end:
 *      pixels, robustified.  Poses and points leave in the scale |t2| = 1.
 *   7. weight: B x N x M doubles, [b][i][v] next to the layout of corresp; may be NULL.  w_{v,i} at the final parameters where the observation exists
 *      and the point takes part; NaN where the observation does not exist, over a dropped point, and over a whole item whose status is not 0.
 *   8. loss == TFF_LOSS_NONE: the call IS tff_bundle_adjust_tracks_batch_*, bit for bit -- the same kernel instance, the normalised metric, no floor,
 *      scale is not read --, and weight is 1 where rule 7 writes a weight and NaN elsewhere, filled by a small kernel of its own.
 *   9. TFF_E_INVALID, before any work, each with a tff_last_error text: everything tff_bundle_adjust_tracks_batch_* refuse; a loss other than the three
 *      codes; with a loss, a scale that is not a positive finite number.
 * An all-NaN column is inert (rule 2 of tftfund_tracks.h): appending such columns changes no bit of Rt, iter, repr_err, used, status, of the other
 * columns of reconst or of the other rows of weight.  Problems of different N therefore go into one call padded with NaN columns; that is the ragged form
 * of this call.  An item's outputs do not depend on the other items of the batch.  Every output pointer except Rt may be NULL.  LDS: that of the plain
 * tracks call; the loss keeps nothing per point.  Workspace of the _host form beyond that of tff_bundle_adjust_tracks_batch_host: 8 B N M bytes for the
 * staged weights.  Covariances for M views: tftfund_tracks_cov.h.  Not here: more than six views, a loss in the polish of tff_robust_pose_scenes_* over tracks. */
#ifndef TFTFUND_TRACKS_LOSS_H
#define TFTFUND_TRACKS_LOSS_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

int tff_bundle_adjust_tracks_loss_batch_dev(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                            int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                            int32_t* used, int32_t* status, int32_t loss, double scale, double* weight);
int tff_bundle_adjust_tracks_loss_batch_host(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                             int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                             int32_t* used, int32_t* status, int32_t loss, double scale, double* weight);

#ifdef __cplusplus
}
#endif
#endif
