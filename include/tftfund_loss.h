/* libtftfund: entry points added after library version 105 (tff_version() >= 106).  Included by tftfund.h; including it alone works too.
 *
 * ---- robust losses (Huber, Cauchy) for the three-view bundle adjustment -----------------------------------------------------------------------------------
 * tff_bundle_adjust_batch_* and tff_bundle_adjust_ragged_* are plain least squares: one wrong match among the selected ones pulls the pose as hard as it
 * likes.  With a loss the adjustment minimises F = sum_i rho(|e_i|^2) over the PIXEL residual e_i of correspondence i: e_{i,v} = r_{i,v} / s_v, where r is
 * the residual in the per-view normalised frame of Normalize2Ddata the plain call works in and s_v that frame's isotropic scale.  With the scale c > 0 in
 * pixels:
 *   TFF_LOSS_HUBER    rho(s) = s for s <= c^2, otherwise 2 c sqrt(s) - c^2;   rho'(s) = 1, otherwise c / sqrt(s)
 *   TFF_LOSS_CAUCHY   rho(s) = c^2 log1p(s / c^2);                            rho'(s) = 1 / (1 + s / c^2)
 * THE LOOP is that of the plain call (damping 0.01, x10 / /10, both tolerances 1e-6, at most 400 iterations, the same step test), reweighted: at the
 * current parameters w_i = rho'(|e_i|^2), and the residual rows of correspondence i in view v and the same rows of both Jacobians are multiplied by
 * sqrt(w_i) / s_v before anything is accumulated (the point blocks, the Schur sums, the gradient, the back-substitution of the points).  The weights are
 * those of the current point, not of the trial point; there is no second-order correction.  The cost does not change along the common scale of t2, t3 and the
 * points, so the step has no component along that direction v = (0, t2, t3, X) of the variables; rounding would put one there (in pixels only the
 * damping stands in it), and the step is therefore freed of it: step -= v (v . step) / (v . v).  For the same reason the 12 x 12 Schur system is solved
 * without the plain call's pivot floor (1e-10 of the largest entry; the damping lies below it): any positive finite pivot is taken.  A system that is
 * singular beyond its damping therefore does not end the item with TFF_ST_NONFINITE as in the plain call: it yields a step that the cost test rejects, the
 * damping grows, and the item ends at the damping limit with status 0 and its last accepted parameters; a zero or non-finite pivot still gives
 * TFF_ST_NONFINITE.  The costs that steer acceptance and the function tolerance are
 * sum_i rho(|e_i|^2) at the current and at the trial parameters, without frozen weights.  repr_err is sqrt(F) at the end: pixels, robustified.  The poses
 * and the points leave in the scale |t2| = 1, as from the plain calls.  tests/ba_loss_oracle.py restates all this in numpy.
 *
 * tff_bundle_adjust_loss_batch_dev / _host: the arguments of tff_bundle_adjust_batch_* plus, at the end, loss, scale and weight -- B x N doubles (a device
 * pointer for _dev, a host pointer for _host), may be NULL: w_i at the final parameters, NaN over an item whose status is not 0.
 * tff_bundle_adjust_loss_ragged_dev / _host: the arguments of tff_bundle_adjust_ragged_* plus the same three; weight is packed like the correspondences
 * (n_total doubles): w_i at the selected positions, NaN where the mask deselects the correspondence and over the range of an item that failed (an item
 * with TFF_ST_BAD_OFFSETS has no range: nothing is written for it).
 * loss == TFF_LOSS_NONE: the call IS the existing one, bit for bit -- the same kernel instance, scale is not read --, and weight is filled with 1 at the
 * selected positions.  TFF_E_INVALID, before any work, each with a tff_last_error text: a null context; a loss other than the three below; with a loss, a
 * scale that is not a positive finite number; everything the plain call refuses.
 * THE RAGGED CONTRACT carries over word for word: item b equals, bit for bit -- weight, iter, repr_err and status included --, the fixed-N loss call with
 * B = 1 on its selected correspondences; no host synchronisation and no device-to-host copy on the _dev path; the per-item statuses are unchanged;
 * nothing is read or written outside [0, n_total); the plan and its launch classes are unchanged.  Workspace beyond the plain call's: 8 n_total bytes for
 * the compact weights of a masked call with a weight output (and the staged weights of a _host call). */
#ifndef TFTFUND_LOSS_H
#define TFTFUND_LOSS_H
#include "tftfund.h"
#ifdef __cplusplus
extern "C" {
#endif

#define TFF_LOSS_NONE 0
#define TFF_LOSS_HUBER 1
#define TFF_LOSS_CAUCHY 2

int tff_bundle_adjust_loss_batch_dev(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                     const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3, double* reconst,
                                     int32_t* iter, double* repr_err, int32_t* status, int32_t loss, double scale, double* weight);
int tff_bundle_adjust_loss_batch_host(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                      const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3, double* reconst,
                                      int32_t* iter, double* repr_err, int32_t* status, int32_t loss, double scale, double* weight);
int tff_bundle_adjust_loss_ragged_dev(tff_ctx* ctx, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                      int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2,
                                      double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss,
                                      double scale, double* weight);
int tff_bundle_adjust_loss_ragged_host(tff_ctx* ctx, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm,
                                       int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2,
                                       double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss,
                                       double scale, double* weight);

#ifdef __cplusplus
}
#endif
#endif
