/* libtftfund: entry points added after library version 106 (tff_version() >= 107).  Included by tftfund.h; including it alone works too.
 *
 * ---- pose and point covariances of the three-view bundle adjustment ---------------------------------------------------------------------------------------
 * A least-squares adjustment has a second output, the covariance of what it estimated.  DEFINITION (tests/ba_cov_oracle.py restates it in numpy): let
 *   x = (angles2, angles3, t2, t3, X_1 .. X_m)   the parameters of the adjustment, in the order of BundleAdjustment.m:100, in the output scale |t2| = 1,
 *   J, r                                         the Jacobian and the residual the kernel accumulates at x: for TFF_LOSS_NONE the residual in the per-view
 *                                                normalised frame; with a loss the pixel residual, its rows times sqrt(w_i) / s_v, w_i = rho'(|e_i|^2)
 *                                                (include/tftfund_loss.h),
 *   N = J'J                                      singular along the scale gauge v = (0, 0, t2, t3, X): the residual does not change along it,
 *   h = (0, 0, t2, 0, 0 ..)                      the gradient of the gauge |t2| = 1 that the output is in.
 * The COFACTOR MATRIX Q is the top-left (12 + 3m)^2 block of inv([[N, h], [h', 0]]), equivalently P N^+ P' with P = I - v h' / (h'v), and
 *   sigma0^2 = r'r / (3m - 11)                   6m residuals, 11 + 3m free parameters; sigma0 is in normalised units for TFF_LOSS_NONE, in pixels with a loss,
 *   cov       = sigma0^2 Q[0:12, 0:12]           144 doubles, row-major, symmetric to the bit, rank 11: cov h12 = 0 (the length of t2 is fixed, not estimated),
 *   point_cov = sigma0^2 times the 3 x 3 diagonal block of Q of every point, six doubles xx xy xz yy yz zz (cross-covariances between points are not given).
 * The angles are those of R = Rx(a) Ry(b) Rz(c) (BundleAdjustment.m:92-94).  The device never forms the dense matrix: with S the Schur complement of the
 * point blocks (the 78 sums of the adjustment's own sweeps at damping 0) and h12, v12 the camera parts of h, v,
 *   Q_c  = inv(S + alpha h12 h12') - v12 v12' / (alpha (h12'v12)^2),     alpha = trace(S) / 12,
 *   Q_Xi = inv(V_i) + inv(V_i) B_i' Q_c B_i inv(V_i),                    V_i = Jp_i' Jp_i,  B_i = Jc_i' Jp_i.
 * alpha brings the border to the size of S; without it the pixel metric (S ~ 1e8) costs up to 2e-2 of the result.
 * NaN in cov, sigma0 and point_cov of an item: m <= 3 (no redundancy), a non-finite input pose, a pivot of the 12 x 12 factorisation that is not positive,
 * a non-finite result.  There is no status output and no new status code.
 *
 * The poses and points may come in any common scale; the result is that of the scale |t2| = 1.  What tff_bundle_adjust_* return is in that scale.
 *
 * tff_ba_covariance_batch_dev / _host: the covariance AT the given poses Rt2, Rt3 (B x 12, 3 x 4 column-major, camera 1 = [I|0]) and points reconst
 * (B x 3N, required) for the correspondences corresp (B x 6N) and calibration calm (27 doubles, calm_stride 0 shared or 27), as tff_bundle_adjust_batch_*
 * take and return them; loss, scale as tff_bundle_adjust_loss_*.  No iteration is run.  cov B x 144, sigma0 B, point_cov B x 6N or NULL.
 * tff_ba_covariance_ragged_dev / _host: the packed form, with the arguments of tff_bundle_adjust_ragged_*: corresp (6 n_total), offsets (B + 1), an optional
 * mask (n_total bytes, non-zero selects), reconst packed like corresp (3 n_total, read where selected); point_cov is packed like corresp (6 n_total): NaN
 * where the mask deselects and over the range of an item that has nothing selected.  THE RAGGED CONTRACT of this library holds: item b gets, bit for bit,
 * what the fixed call with B = 1 gives on its selected correspondences in packed order; no host synchronisation and no device-to-host copy on the _dev path;
 * nothing is read or written outside [0, n_total).  The kernel keeps no points in LDS, so there is no TFF_BA_MAX_N limit here.  An item with bad offsets
 * gets NaN cov and sigma0 (it has no range: its point_cov is not written); so does an item whose poses are NaN, as the adjustment leaves them for an item
 * that failed.  The _host form refuses offsets that decrease or begin below 0 (TFF_E_INVALID).
 * tff_bundle_adjust_cov_batch_dev / _host, tff_bundle_adjust_cov_ragged_dev / _host: the argument lists of tff_bundle_adjust_loss_batch_* and
 * tff_bundle_adjust_loss_ragged_* followed by cov, sigma0, point_cov.  Each IS the adjustment followed by the covariance call above on its outputs, on one
 * stream: every output of the adjustment has the bits of the call without a covariance, and cov, sigma0, point_cov the bits of tff_ba_covariance_* on them.
 * With reconst == NULL a workspace of the context holds the points (24 bytes per correspondence).
 * TFF_E_INVALID, before any work: a null context, what check of the loss refuses, a null cov, sigma0 or reconst (tff_ba_covariance_*), everything the
 * adjustment's own call refuses.  Workspace: 8 + 208 B bytes for a ragged call, under a mask 76 bytes per correspondence more (124 with point_cov). */
#ifndef TFTFUND_COV_H
#define TFTFUND_COV_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

int tff_ba_covariance_batch_dev(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2, const double* Rt3, const double* corresp,
                                int64_t B, int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov);
int tff_ba_covariance_batch_host(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2, const double* Rt3, const double* corresp,
                                 int64_t B, int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov);
int tff_ba_covariance_ragged_dev(tff_ctx* ctx, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                 int64_t calm_stride, const double* Rt2, const double* Rt3, const double* reconst, int64_t B, int32_t loss, double scale,
                                 double* cov, double* sigma0, double* point_cov);
int tff_ba_covariance_ragged_host(tff_ctx* ctx, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm,
                                  int64_t calm_stride, const double* Rt2, const double* Rt3, const double* reconst, int64_t B, int32_t loss, double scale,
                                  double* cov, double* sigma0, double* point_cov);

int tff_bundle_adjust_cov_batch_dev(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                    const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3, double* reconst,
                                    int32_t* iter, double* repr_err, int32_t* status, int32_t loss, double scale, double* weight, double* cov,
                                    double* sigma0, double* point_cov);
int tff_bundle_adjust_cov_batch_host(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                     const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3, double* reconst,
                                     int32_t* iter, double* repr_err, int32_t* status, int32_t loss, double scale, double* weight, double* cov,
                                     double* sigma0, double* point_cov);
int tff_bundle_adjust_cov_ragged_dev(tff_ctx* ctx, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                     int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2,
                                     double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss,
                                     double scale, double* weight, double* cov, double* sigma0, double* point_cov);
int tff_bundle_adjust_cov_ragged_host(tff_ctx* ctx, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm,
                                      int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2,
                                      double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss,
                                      double scale, double* weight, double* cov, double* sigma0, double* point_cov);

#ifdef __cplusplus
}
#endif
#endif
