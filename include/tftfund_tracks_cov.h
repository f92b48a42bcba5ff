/* libtftfund: entry points added after library version 109 (tff_version() >= 110).  Included by tftfund.h; including it alone works too.
 *
 * ---- pose and point covariances of the bundle adjustment over tracks, M = 2 .. 6 views ------------------------------------------------------------------------
 * tff_ba_covariance_* (tftfund_cov.h) give the covariance of the three-view adjustment: P = 12, full visibility, a loss per correspondence, camera 1 = [I|0]
 * given.  The adjustment that real data ends up in is the one over tracks (tftfund_tracks.h, tftfund_tracks_loss.h): M = 2 .. 6 views, per-point
 * visibility, a Huber or Cauchy loss per observation.  These four calls give its covariance.  Everything not said here is rules 1 - 7 of tftfund_tracks.h and
 * rules 1 - 2 of tftfund_tracks_loss.h.  DEFINITION (tests/ba_tracks_cov_oracle.py restates it in numpy):
 *   1. Parameters: x = (angles of cameras 2..M, translations of cameras 2..M, X_i of the points taking part), P = 6 (M - 1) camera parameters in that
 *      order, in the output frame: camera 1 = [I|0], |t2| = 1.  The angles are those of R = Rx(a) Ry(b) Rz(c), as in tftfund_cov.h.
 *   2. J, r: what the tracks kernels accumulate at x.  TFF_LOSS_NONE: the residual in the per-view normalised frame.  With a loss: the pixel residual of
 *      observation (v, i), both rows times sqrt(w_{v,i}) / s_v, w_{v,i} = rho'(|e_{v,i}|^2) PER OBSERVATION.  An observation that does not exist has no
 *      rows; a dropped point has no columns.
 *   3. A camera j >= 2 is ESTIMATED iff its view is seen (n_v > 0); C_s is the number of estimated cameras.  An unseen camera is a constant: its 6 rows
 *      and columns of cov are exactly 0 and it is absent from the gauge vector (rule 3 of tftfund_tracks_loss.h).  If view 2 is unseen the output scale
 *      rests on a quantity that was not estimated: cov, sigma0 and point_cov of that item are NaN.
 *   4. Gauge: N = J'J is singular along v = (0 for angles; t_j of the estimated cameras; X_i).  h = the gradient of |t2| = 1: t2 in camera 2's
 *      translation slots, 0 elsewhere.  Q = the top-left block of inv([[N, h], [h', 0]]) over the estimated parameters.
 *   5. dof = 2 n_obs - (6 C_s + 3 m - 1), n_obs the observations of the m points taking part (three fully visible views: 3 m - 11, as tftfund_cov.h).
 *      sigma0^2 = r'r / dof: normalised units without a loss, pixels with one.  cov = sigma0^2 Q_cameras: P x P doubles, row-major, symmetric TO THE BIT,
 *      cov h_P = 0.  point_cov = sigma0^2 x the 3 x 3 diagonal block of Q of every point taking part, six doubles xx xy xz yy yz zz at [b][i]; NaN over a
 *      dropped point.
 *   6. NaN in cov, sigma0 and point_cov of an item: dof <= 0; a non-finite input pose or a non-finite point taking part; what the adjustment answers with a
 *      status other than 0 (TFF_ST_TOO_FEW, a TFF_ST_NONFINITE normalisation); view 2 unseen; a pivot that is not positive; a non-finite result.  There
 *      is no new status code.
 *   7. Device route: the dense matrix is never formed.  S is the Schur complement of the point blocks at damping 0 -- the sums of the tracks kernels as
 *      they are --; an unseen camera's block gets a unit diagonal for the solve and is zeroed afterwards; with h_P, v_P the camera parts of h and v,
 *          Q_c = inv(S + alpha h_P h_P') - v_P v_P' / (alpha (h_P'v_P)^2),  alpha = trace(S) / (6 C_s),
 *          Q_Xi = inv(V_i) + inv(V_i) B_i' Q_c B_i inv(V_i);
 *      the inverse is P solves against the unit vectors, the result symmetrised (A_ij + A_ji) / 2.
 *   8. Input poses are taken as the tracks call takes Rt_in: first camera free, any common scale; reconst is in the same frame and scale.  The kernel
 *      performs the same change of coordinates (BundleAdjustment.m:80-86) and converts to |t2| = 1 exactly.  Fed the adjustment's own outputs that
 *      change of coordinates is the identity.
 *   9. An all-NaN column is inert: appending such columns changes no bit of cov, sigma0 or of the other rows of point_cov; that is the ragged form of
 *      this call.  An item does not depend on its neighbours in the batch.
 *
 * tff_ba_tracks_covariance_batch_*: the covariance AT the given poses and points; no iteration is run.  Rt B x 12 M (3M x 4 column-major), corresp
 * B x N x 2M, reconst B x 3N (required), cov B x P x P, sigma0 B, point_cov B x 6N or NULL.  loss, scale as tff_bundle_adjust_tracks_loss_batch_*.
 * tff_bundle_adjust_tracks_cov_batch_*: the argument list of tff_bundle_adjust_tracks_loss_batch_* followed by cov, sigma0, point_cov.  It IS that
 * adjustment followed by the call above on its outputs, on one stream: every adjustment output has the bits of the call without a covariance, and cov,
 * sigma0, point_cov have the bits of tff_ba_tracks_covariance_* on those outputs.  With reconst == NULL a workspace of the context holds the points.
 * TFF_E_INVALID, before any work, each with a tff_last_error text: everything tff_bundle_adjust_tracks_loss_batch_* refuse; a null cov or sigma0; on the
 * stand-alone form a null reconst.  B = 0 does nothing.  LDS: a fixed amount per M (the Schur sums, the P x (P + 1) work matrix and two P x P matrices,
 * 31 KB at M = 6); the points are read from global memory.  Workspace: 24 B N bytes for the points in the frame of camera 1; the _host forms stage their
 * arrays in addition.  Not here: a ragged packed form (NaN padding is this call's ragged form), more than six views, cross-covariances between points, a
 * covariance from the polish of tff_robust_pose_scenes_* over tracks. */
#ifndef TFTFUND_TRACKS_COV_H
#define TFTFUND_TRACKS_COV_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

int tff_ba_tracks_covariance_batch_dev(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt, const double* corresp, int64_t B,
                                       int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov);
int tff_ba_tracks_covariance_batch_host(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt, const double* corresp, int64_t B,
                                        int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov);

int tff_bundle_adjust_tracks_cov_batch_dev(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                           int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                           int32_t* used, int32_t* status, int32_t loss, double scale, double* weight, double* cov, double* sigma0,
                                           double* point_cov);
int tff_bundle_adjust_tracks_cov_batch_host(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                            int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                            int32_t* used, int32_t* status, int32_t loss, double scale, double* weight, double* cov, double* sigma0,
                                            double* point_cov);

#ifdef __cplusplus
}
#endif
#endif
