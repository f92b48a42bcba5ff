/*
 * tftfund.h -- C ABI of the MI355X-native batched trifocal-tensor /
 * fundamental-matrix pose estimators (libtftfund.so, built by hipcc for gfx950).
 *
 * This is the drop-in boundary for the hot path of LauraFJulia/TFT_vs_Fund.
 * The reference has no FFI layer; its "operator API" is the MATLAB calling
 * convention of the method handles
 *     [R_t_2,R_t_3,Reconst,T,iter] = Method(Corresp,CalM)
 * (experiments.m:51-59,108; experiments_real.m:53-61,126; example.m:32-42).
 * Each tff_*_pose_batch entry point below replaces one such method for a batch
 * of B independent triplets; the MEX shim in matlab/ and the ctypes binding in
 * tft_vs_fund_amd/api.py bind exactly these symbols.
 *
 * Data layout (all IEEE double, MATLAB column-major, caller owns every buffer):
 *   corresp  B x (6 x N): triplet b, correspondence n = 6 contiguous doubles
 *            [x1 y1 x2 y2 x3 y3] at corresp[(b*N + n)*6]          (Corresp, 6xN)
 *   calm     27 doubles per triplet = 9x3 column-major [K1;K2;K3]; calm_stride
 *            is 27 (one per triplet) or 0 (one shared by the batch)   (CalM, 9x3)
 *   Rt2,Rt3  B x 12: 3x4 column-major [R|t], camera 1 = [I|0], |t2| = 1
 *   T        B x 27: T(j,k,i) at j + 3k + 9i, unit Frobenius norm, global sign free
 *   reconst  B x (3 x N) or NULL                                   (Reconst, 3xN)
 *   iter     B int32 or NULL  (0 for the linear methods, GH iterations otherwise)
 *   status   B int32 or NULL  (replaces MATLAB exceptions, see TFF_ST_*)
 * Ragged batches (tff_pose_batch_ragged_*): triplets with different correspondence counts, packed:
 *   offsets  B + 1 int64; triplet b owns correspondences offsets[b] .. offsets[b+1]-1, n_b = offsets[b+1] - offsets[b]
 *   corresp  correspondence n of triplet b = [x1 y1 x2 y2 x3 y3] at corresp[(offsets[b] + n)*6]
 *   reconst  3 doubles per correspondence at reconst[(offsets[b] + n)*3] or NULL;  calm, Rt2, Rt3, T, iter, status as above
 *
 * Every function returns 0 on success or a negative code (-hipError_t for HIP
 * failures, TFF_E_* otherwise); tff_last_error() gives a thread-local message.
 * `_dev` variants take device pointers valid on the context's device and only
 * enqueue work on the context's stream (no synchronisation).  The context owns device
 * workspaces (status scratch when status == NULL, the records and spill slices of the
 * iterative methods) that grow on demand: a call with a larger B or N than any earlier
 * call of that method may hipMalloc / hipFree.  Inside a hipGraph capture use a `_dev`
 * entry point only after a warm-up call with the same method and B, N at least as large.
 * `_host` variants take host pointers and perform H2D, compute, D2H and a stream
 * synchronisation.
 * A context is bound to one device.  Its entry points are serialised by an internal lock
 * (the workspaces are shared state) and its work by its stream; when the stream is changed
 * (tff_ctx_set_stream) work on the new stream waits, on the device, for the work already
 * enqueued on the old one.  For concurrent streams or threads use one context each:
 * different contexts are independent.  No global state.
 */
#ifndef TFTFUND_H
#define TFTFUND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tff_ctx tff_ctx;

/* per-triplet status codes */
#define TFF_ST_OK 0
#define TFF_ST_TOO_FEW 1    /* N < 7 (TFT) or N < 8 (F): experiments.m:99, linearF.m:35-37 */
#define TFF_ST_NONFINITE 2  /* NaN/Inf in the result: Gauss_Helmert.m:53-55,63-65 */
#define TFF_ST_NO_POSE 3    /* no candidate with score >= 0: R_f unassigned in R_t_from_TFT.m:91-104 */
#define TFF_ST_NO_PARAM 5   /* PiColPoseEstimation.m:84-89: error('The minimal param could not be found') */
#define TFF_ST_RANK 4       /* Nordberg: P2(:,1:3) or P3(:,1:3) of rank < 2 (NordbergTFT...m:58,60 would fail: null() returns two columns) */
#define TFF_ST_BAD_OFFSETS 6 /* ragged calls (_dev): offsets[b+1] < offsets[b], offsets[b] < 0, or n_b > n_max -- NaN poses for that item only */
#define TFF_ST_TOO_LARGE 7   /* ragged BA: more selected correspondences than TFF_BA_MAX_N */

/* error codes (besides -hipError_t) */
#define TFF_E_INVALID (-10001)
#define TFF_E_NOMEM (-10002)

/* options for tff_ctx_set_option */
#define TFF_OPT_SOLVER 1    /* 0 (default): fast tiers (Gram matrix + Cholesky inverse iteration, certified sign-only cheirality votes) with
                             * the exact kernel (Householder QR of the explicit design matrix, one-sided Jacobi fall-backs: the accuracy
                             * of the reference's svd() calls) over the triplets they could not finish or certify; 1: exact kernel for all */
#define TFF_OPT_EXACT_BELOW 5 /* batches with N < value go to the exact kernel as a whole (default 12: minimal samples, where the two smallest
                             * singular values of the design matrix often nearly coincide); 0 = only the flagged triplets */
#define TFF_OPT_STAGE_LDS 2 /* -1 auto (default: staged in LDS while that costs no occupancy, N <= 200 for the TFT kernels, N <= 48 for LinearF),
                             * 0 re-read correspondences through L2, 1 stage them in LDS */

#define TFF_OPT_GH_EXACT 4  /* Gauss-Helmert methods: 1 = always form pinv(W) through per-block eigen-decompositions -- an A/B switch: it carries the
                             * 1e-6 .. 1e-4 noise of any fp64 pinv(W) (default 0: deflated block pseudo-inverse + factored strong direction, which
                             * reproduce a 50-digit evaluation of the reference's iteration to 1e-11 for Ressl, Nordberg and Pi) */
#define TFF_OPT_SPILL 6     /* per-correspondence state of the iterative methods: 0 (default) it leaves the LDS for the context's global slices whenever that lets
                             * more workgroups share a CU (measured faster, at the price of HBM traffic); 1 = only when the LDS cannot hold it (large N) */
#define TFF_OPT_KERNEL 3    /* Kernel variants of the iterative TFT methods: 0 automatic (default: a workgroup per triplet for the iteration -- two wavefronts
                             * for Ressl / Nordberg / Pi / PiCol, four for FaugPapa -- at every N since round 4);
                             * 1 the fused single-wavefront kernels (one wavefront per triplet from start to end);
                             * 2 workgroup kernels always (the same as 0 now) */
#define TFF_OPT_ROWS 7      /* LinearTFT / LinearF pose kernels, and the linear stage + pose tail of the iterative methods: 1 four triplets per wavefront,
                             * one per row of 16 lanes (csrc/tft_rows_kernel.h, f_rows_kernel.h, gh_rows_kernel.h, optimf_rows_kernel.h); 0 one triplet
                             * per wavefront (csrc/tft_kernel.h, f_kernel.h: the lowest latency for batches under ~1 000 triplets, ~16 us less per call); 2 (default)
                             * = 1 for every method and every batch size since the end of round 5.  (Before, the two linear methods went by batch size;
                             * the two routes agree to 1e-14 but not bit for bit, so a triplet's last bits depended on the batch it arrived in.)  With the
                             * default the same triplet gives the same bits -- and, for the iterative methods, the same `iter` -- in a batch of one, of 1 023
                             * or of a million, through the *_sampled_dev entry points in chunks of any size, and in any shard of a multi-GPU call.
                             * Whatever the route: a triplet with status != 0 has NaN in every output (T, R_t_2, R_t_3, Reconst) */
#define TFF_OPT_PRE 10      /* trifocal row kernels (TFF_OPT_ROWS route): where the three Normalize2Ddata calls and the 96 moment sums of linearTFT's system are
                             * computed.  0 (default) = inside the row kernels (two passes over the correspondences); 1 = in a kernel of their own, one triplet
                             * per wavefront, the correspondences read from HBM once and parked in LDS (csrc/tft_moments_kernel.h), the row kernels starting
                             * from its 112-double record; 2 = that kernel from N >= 48.  An A/B switch: measured slower than the fused passes on MI355X
                             * (profiles/r5_ab_pre.txt) -- the path is bound by fp64 issue, not by those passes' memory waits.  Results agree to rounding */
#define TFF_OPT_COUNT_ROWS 11 /* tff_inlier_count_batch_dev on many hypotheses of one scene: 1 (default) four hypotheses per wavefront, one per row of 16 lanes
                             * (the cameras composed once per row, 25 trips of 16 over a 400-correspondence scene); 0 one hypothesis per wavefront.  Identical counts */
#define TFF_OPT_BA_CLASSES 12 /* tff_bundle_adjust_ragged_*: how the items are launched.  0 (default): by batch size -- up to 256 items (every item resident at once
                             * even at one wavefront per CU) one launch sized for TFF_BA_MAX_N, larger batches three launch classes by LDS need; 1 = one
                             * launch always; 2 = three classes always (A/B switch, tools/bench_ba_ragged.py).  Identical results */
#define TFF_OPT_SCORE 13    /* what tff_inlier_count_batch_dev / tff_inlier_count_scenes_dev write and tff_robust_pose_* rank by: 0 (default) the inlier
                             * count; 1 the MSAC score, an int32 sum of per-inlier weights in [1, TFF_SCORE_UNITS] (formula at tff_inlier_count_batch_dev).
                             * Any other value: TFF_E_INVALID.  Masks, their row sums, the refit batches and info[0] stay hard counts under either value */
#define TFF_SCORE_UNITS 64  /* the MSAC weight of a perfect inlier: count <= score <= TFF_SCORE_UNITS * count */
#define TFF_OPT_DEBUG_FP_HANDOVER 8 /* test hook: 1 = FaugPapa's block kernel hands every third triplet back to the generic workgroup kernel, as it does when its
                             * pseudo-inverse reports a failure (exercises that production fall-back; results must not depend on it beyond the
                             * generic kernel's LAPACK-level noise) */
#define TFF_OPT_DEBUG_ADAPTIVE 9 /* profiling hook: 1 = the *_debug_dev entry points of the linear methods keep the production vote logic (main candidates only,
                             * scale sums during the votes) instead of evaluating all four cheirality scores for the debug record */
#define TFF_DEBUG_STRIDE 128 /* doubles per triplet written by the *_debug_dev entry points */

int tff_version(void);
const char* tff_last_error(void);

/* Context: device ordinal; owns a stream unless one is supplied. */
int tff_ctx_create(tff_ctx** out, int device);
void tff_ctx_destroy(tff_ctx* ctx);
int tff_ctx_set_stream(tff_ctx* ctx, void* hip_stream); /* borrow the caller's hipStream_t; NULL is the device's null stream */
int tff_ctx_use_own_stream(tff_ctx* ctx);               /* back to the context's own non-blocking stream */
void* tff_ctx_get_stream(tff_ctx* ctx);
int tff_ctx_set_option(tff_ctx* ctx, int option, long value);
int tff_ctx_synchronize(tff_ctx* ctx);

/* LinearTFTPoseEstimation (TFT_methods/LinearTFTPoseEstimation.m:44-62):
 * Normalize2Ddata x3 -> linearTFT -> transform_TFT -> R_t_from_TFT -> (Reconst). */
int tff_linear_tft_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                  int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                  int32_t* iter, int32_t* status);
int tff_linear_tft_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                   int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                   int32_t* iter, int32_t* status);
/* same, additionally writing B x TFF_DEBUG_STRIDE intermediates (unconstrained tensor,
 * epipoles, constrained tensor, cheirality votes, t3 scale, solver iterations, normalisation) */
int tff_linear_tft_pose_batch_debug_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                        int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                        int32_t* iter, int32_t* status, double* dbg);

/* the same record for LinearFPoseEstimation (phase stamps at dbg[80 ..], iteration counts of the two view pairs at dbg[69], dbg[70]) */
int tff_linear_f_pose_batch_debug_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                      int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                      int32_t* iter, int32_t* status, double* dbg);

/* ResslTFTPoseEstimation (TFT_methods/ResslTFTPoseEstimation.m:47-177): linearTFT, Ressl's 20-parameter /
 * 2-constraint minimal parameterisation, Gauss-Helmert refinement (Optimization/Gauss_Helmert.m:38-83),
 * then transform_TFT -> R_t_from_TFT -> (Reconst).  iter = Gauss-Helmert iterations.  Any N (the per-correspondence state spills to a
 * global workspace when it exceeds the LDS). */
int tff_ressl_tft_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                 int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                 int32_t* iter, int32_t* status);
int tff_ressl_tft_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                  int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                  int32_t* iter, int32_t* status);
int tff_ressl_tft_pose_batch_debug_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                       int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                       int32_t* iter, int32_t* status, double* dbg);

/* NordbergTFTPoseEstimation (TFT_methods/NordbergTFTPoseEstimation.m:47-222): three orthogonal matrices in
 * axis-angle form + a 10-entry sparse tensor (19 parameters, 1 constraint), Gauss-Helmert refinement.
 * The projective fix-up for rank-deficient P2/P3 (:56-62) is applied (rank by sigma_3 = |det| / (sigma_1 sigma_2)). */
int tff_nordberg_tft_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                    int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                    int32_t* iter, int32_t* status);
int tff_nordberg_tft_pose_batch_debug_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                          int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                          int32_t* iter, int32_t* status, double* dbg);
int tff_nordberg_tft_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                     int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                     int32_t* iter, int32_t* status);

/* FaugPapaTFTPoseEstimation (TFT_methods/FaugPapaTFTPoseEstimation.m:48-159): all 27 tensor entries as
 * parameters, 12 algebraic constraints (3 determinants + 9 extended-rank), Gauss-Helmert refinement. */
int tff_faugpapa_tft_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                    int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                    int32_t* iter, int32_t* status);
int tff_faugpapa_tft_pose_batch_debug_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                          int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                          int32_t* iter, int32_t* status, double* dbg);
int tff_faugpapa_tft_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                     int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                     int32_t* iter, int32_t* status);

/* PiPoseEstimation (TFT_methods/PiPoseEstimation.m:50-182): Ponce-Hebert Pi matrices from the linear solution
 * (27 parameters, 9 constraints), 3 epipolar equations + 1 trilinearity per correspondence, Gauss-Helmert.
 * PiColPoseEstimation (TFT_methods/PiColPoseEstimation.m:50-218): the variant for collinear camera centres
 * (11 constraints, 3 + 2 equations per correspondence); TFF_ST_NO_PARAM where the reference raises
 * 'The minimal param could not be found'. */
int tff_pi_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                          int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                          int32_t* iter, int32_t* status);
int tff_pi_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                           int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                           int32_t* iter, int32_t* status);
int tff_picol_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                             int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                             int32_t* iter, int32_t* status);
int tff_picol_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                              int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                              int32_t* iter, int32_t* status);

/* Pi / PiCol (collinear != 0) with the start of the Gauss-Helmert iteration exposed: init_p (B x 27, the vector `pi`
 * of PiPoseEstimation.m:86 / PiColPoseEstimation.m:113) and init_x (B x 6N, `x_est`).  The Pi matrices depend on sign
 * and basis choices the reference leaves to svd (null(P), null(M.')); PiCol's result depends on them
 * (PiColPoseEstimation.m:93-94 is not covariant), so parity for it is checked from this common start. */
int tff_pi_pose_batch_debug_dev(tff_ctx* ctx, int32_t collinear, const double* corresp, const double* calm,
                                int64_t calm_stride, int64_t B, int32_t N, double* Rt2, double* Rt3, double* T,
                                double* reconst, int32_t* iter, int32_t* status, double* init_p, double* init_x);

/* OptimFPoseEstimation (F_methods/OptimFPoseEstimation.m:44-73): two fundamental matrices, each refined by
 * optimF (F_methods/optimF.m:34-109: linearF start, 9 parameters, constraints det F = 0 and |F| = 1, one
 * epipolar equation per correspondence, Gauss-Helmert) -> recover_R_t x2 -> t3 scale -> (Reconst) ->
 * T = TFT_from_P.  iter = it1 + it2.  Needs N >= 8. */
int tff_optim_f_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                               int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                               int32_t* iter, int32_t* status);
int tff_optim_f_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                int32_t* iter, int32_t* status);

/* LinearFPoseEstimation (F_methods/LinearFPoseEstimation.m:42-109): Normalize2Ddata x3 ->
 * linearF x2 (F_methods/linearF.m:32-62) -> recover_R_t x2 -> t3 scale -> (Reconst) ->
 * T = TFT_from_P (TFT_methods/TFT_from_P.m:25-33).  Needs N >= 8 (status TFF_ST_TOO_FEW otherwise). */
int tff_linear_f_pose_batch_dev(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                int32_t* iter, int32_t* status);
int tff_linear_f_pose_batch_host(tff_ctx* ctx, const double* corresp, const double* calm, int64_t calm_stride,
                                 int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst,
                                 int32_t* iter, int32_t* status);

/* ---- building blocks (device pointers; all arrays MATLAB column-major) ------------------------- */

/* triangulation3D (auxiliar_functions/triangulation3D.m:32-64): M = 2 or 3 cameras (3x4 each, cam_stride 12*M per
 * item or 0 = shared), pts B x (2M x N); X B x (4 x N) unit-norm homogeneous points, sign free, not dehomogenised. */
int tff_triangulate_batch_dev(tff_ctx* ctx, const double* cams, int64_t cam_stride, const double* pts, int64_t B,
                              int32_t M, int32_t N, double* X);

/* ReprError (auxiliar_functions/ReprError.m:39-65) for three views: RMS over the 3N reprojected points; pts3d
 * (B x 3 x N) or NULL to triangulate first (ReprError.m:43-44).  corresp_stride 6*N or 0 (one shared scene). */
int tff_repr_error_batch_dev(tff_ctx* ctx, const double* cams, int64_t cam_stride, const double* corresp,
                             int64_t corresp_stride, const double* pts3d, int64_t B, int32_t N, double* err);

/* Inlier count of pose hypotheses against ONE shared scene (6 x Ns): cameras K1[I|0], K2 Rt2[b], K3 Rt3[b];
 * a correspondence is an inlier when all six reprojection residuals after triangulation are <= threshold in
 * absolute value (experiments_real.m:94-98).  counts B int32; err (B, RMS) optional.
 * TFF_OPT_SCORE = 1 (MSAC): counts[b] is the hypothesis's score instead, on every route of this call (with or without err): the sum over its
 * inliers -- the same rule decides who is one -- of the weight
 *     w = 1 + (int)(63.0 * fmax(0.0, 1.0 - ss * c)),   c = 1 / (6 threshold^2) computed once by the host in double,
 *     ss = (dx_0^2 + dy_0^2) + (dx_1^2 + dy_1^2) + (dx_2^2 + dy_2^2) of the six residuals the rule compares, added in that order,
 * each dx^2 + dy^2 evaluated as fma(dx, dx, dy * dy) and 1 - ss * c as fma(-ss, c, 1.0), so that every route gives the same integer.  An outlier
 * weighs 0, an inlier at the rim of the threshold box 1, a perfect one TFF_SCORE_UNITS: count <= score <= 64 * count <= 2^30 (Ns <= 2^24). */
int tff_inlier_count_batch_dev(tff_ctx* ctx, const double* scene, int32_t Ns, const double* calm, const double* Rt2,
                               const double* Rt3, int64_t B, double threshold, int32_t* counts, double* err);

/* transform_TFT (TFT_methods/transform_TFT.m:32-49), inverse = 0 or 1; M1..M3 3x3, m_stride 9 or 0 (shared). */
int tff_transform_tft_batch_dev(tff_ctx* ctx, const double* T, const double* M1, const double* M2, const double* M3,
                                int64_t m_stride, int64_t B, int32_t inverse, double* Tout);

/* R_t_from_TFT (TFT_methods/R_t_from_TFT.m:40-106): pixel-coordinate tensor + CalM + Corresp -> poses. */
int tff_rt_from_tft_batch_dev(tff_ctx* ctx, const double* T, const double* calm, int64_t calm_stride,
                              const double* corresp, int64_t B, int32_t N, double* Rt2, double* Rt3, int32_t* status);

/* linearTFT (TFT_methods/linearTFT.m:33-91) on points used as given (rows x1;y1;x2;y2;x3;y3 of corresp):
 * T (27, unit norm), P2, P3 (3x4 each, P1 = [I|0]; both NULL to skip). */
int tff_linear_tft_batch_dev(tff_ctx* ctx, const double* corresp, int64_t B, int32_t N, double* T, double* P2,
                             double* P3, int32_t* status);

/* linearF (F_methods/linearF.m:32-62; refine = 0) or optimF (F_methods/optimF.m:34-78; refine = 1) for the view
 * pairs (1,2) and (1,3) of each item: F21, F31 (B x 9, 3x3 column-major, x2' F21 x1 = 0).  linearF normalises its
 * inputs itself; iter (optimF: it1 + it2) may be NULL.  Needs N >= 8. */
int tff_linear_f_batch_dev(tff_ctx* ctx, const double* corresp, int64_t B, int32_t N, int32_t refine, double* F21,
                           double* F31, int32_t* iter, int32_t* status);

/* BundleAdjustment (Optimization/BundleAdjustment.m:49-216) for three views: refines the poses (Rt2_in, Rt3_in: B x 12,
 * camera 1 = [I|0]) and the space points (reconst0: B x 3N, or NULL to triangulate them first, :59-77) by Levenberg-Marquardt on
 * the reprojection residual in per-view normalised coordinates.  Outputs: poses with |t2| = 1, points (NULL to skip),
 * successful LM iterations, repr_err = norm of the final residual vector (normalised units, as BundleAdjustment.m:105).
 * MATLAB's lsqnonlin is closed source: the loop follows its documented LM defaults (see csrc/ba_kernel.h); results are
 * comparable at the converged optimum.  All correspondences must be visible in all three views. */
int tff_bundle_adjust_batch_dev(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2_in,
                                const double* Rt3_in, const double* corresp, int64_t B, int32_t N, const double* reconst0,
                                double* Rt2, double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* status);
int tff_bundle_adjust_batch_host(tff_ctx* ctx, const double* calm, int64_t calm_stride, const double* Rt2_in,
                                 const double* Rt3_in, const double* corresp, int64_t B, int32_t N, const double* reconst0,
                                 double* Rt2, double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* status);

/* ---- ragged, masked BundleAdjustment: one call for items with different correspondence counts, e.g. the polish of tff_robust_pose_scenes_* ------------
 * corresp, offsets: packed as in tff_pose_batch_ragged_* (item b owns the n_b correspondences offsets[b] .. offsets[b+1]-1; offsets on the device for
 * _dev).  n_total (host, in [0, 2^31 - 1]) bounds every offset and sizes the workspaces.  mask: NULL, or n_total bytes, the byte of correspondence n of
 * item b at offsets[b] + n, non-zero = use it -- exactly the `mask` tff_robust_pose_scenes_* writes.  m_b = the number of selected correspondences of
 * item b (n_b without a mask).  calm, Rt2_in, Rt3_in, Rt2, Rt3, iter, repr_err, status: per item, as tff_bundle_adjust_batch_dev.  reconst0, reconst
 * (each may be NULL): 3 doubles per packed correspondence at (offsets[b] + n) * 3; reconst0 is read at selected positions only, reconst gets NaN at the
 * unselected positions of a valid item.  used (B int32, may be NULL) receives m_b.
 * THE CONTRACT: the outputs of item b -- Rt2, Rt3, reconst at the selected positions, iter, repr_err, status -- are bit for bit those of
 * tff_bundle_adjust_batch_dev called with B = 1, N = m_b, the item's selected correspondences in packed order, its poses, its CalM, its selected reconst0
 * triples and the same context options: one kernel serves both calls, with the same instruction stream per item.  Nothing depends on B, on the
 * neighbouring items or on the order in which the launch plan lists the items.
 * Per-item failures (statuses, the offsets of _dev being device data); the item gets NaN poses and repr_err, iter 0 and used 0, its neighbours are
 * unaffected: a negative or decreasing offset or one above n_total gives TFF_ST_BAD_OFFSETS and leaves the item's reconst range untouched; m_b = 0 gives
 * TFF_ST_TOO_FEW; m_b > TFF_BA_MAX_N gives TFF_ST_TOO_LARGE (the points of an item live in LDS); the last two write NaN over the item's reconst range.
 * Whatever the offsets hold, no kernel reads or writes outside [0, n_total) of the packed arrays.  (Items whose ranges overlap -- only malformed offsets
 * make them -- share positions of reconst: their points are in bounds and otherwise unspecified; with a mask, an item whose selection would not fit the
 * n_total slots of the compact workspace after the items before it is TFF_ST_BAD_OFFSETS.)
 * The launch plan: the kernel needs 13 872 + 48 m bytes of LDS and runs four wavefronts per CU while an item needs at most 40 KiB, two up to 80 KiB, one
 * up to 160 KiB.  The items are sorted on the device into three classes by m_b (tff_bundle_adjust_ragged_class_bounds: the largest m of each class,
 * bounds[2] = TFF_BA_MAX_N) and every class gets its own launch with its own LDS size, so a few large items do not cost the small ones their occupancy.
 * The class launches follow one another on the stream, so a batch of at most 256 items, all resident at once anyway, takes ONE launch sized for
 * TFF_BA_MAX_N instead (TFF_OPT_BA_CLASSES; B is a host value).  The results do not depend on the plan.
 * TFF_E_INVALID: a null required pointer, B < 0, n_total outside [0, 2^31 - 1], a calm_stride other than 0 or 27; _host only: decreasing or negative
 * offsets, before any work.  B = 0 returns 0.
 * _dev: no host synchronisation and no device-to-host copy.  _host: host pointers (n_total is offsets[B]), one synchronisation.
 * Workspaces of the context, growing on demand: 24 B bytes for the plan; with a mask, 100 bytes x n_total for the compact copies (correspondences,
 * reconst0, points, source indices); status == NULL borrows the status scratch. */
#define TFF_BA_MAX_N 3124    /* largest N whose 13 872 + 48 N bytes of LDS fit the 160 KiB limit (checked against the kernel's ba_lds_bytes at compile time) */
int tff_bundle_adjust_ragged_dev(tff_ctx* ctx, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                 int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2,
                                 double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status);
int tff_bundle_adjust_ragged_host(tff_ctx* ctx, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm,
                                  int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2,
                                  double* Rt3, double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status);
int tff_bundle_adjust_ragged_class_bounds(int32_t bounds[3]);
/* Declared in tftfund_loss.h, which this header includes at its end: robust losses (Huber, Cauchy) for the three-view bundle adjustment.
 * tff_bundle_adjust_loss_batch_dev / _host and tff_bundle_adjust_loss_ragged_dev / _host take the arguments of the four tff_bundle_adjust_batch_* and
 * tff_bundle_adjust_ragged_* calls above plus `int32_t loss, double scale, double* weight` at the end.  With TFF_LOSS_NONE they are those calls, bit for bit. */
/* Declared in tftfund_cov.h, included at the end as well: the covariance of the adjusted poses and points.  tff_ba_covariance_batch_* / _ragged_* evaluate it at
 * given poses and points; tff_bundle_adjust_cov_batch_* / _ragged_* are the loss forms followed by it, with `double* cov, double* sigma0, double* point_cov`. */

/* BundleAdjustment (Optimization/BundleAdjustment.m:49-216) as the reference writes it, for M = 2 .. 6 views, in MATLAB's own
 * array layouts so that a gateway passes its arguments through: calm = CalM (3M x 3, column-major; calm_stride 0 = shared, 9M =
 * one per item), Rt_in = R_t_0 (3M x 4 column-major per item, camera 1 included and NOT required to be [I|0]: the change of
 * coordinates of :80-86 is done on the device, after the optional initial triangulation of :59-77 in the given frame),
 * corresp = Corresp (2M x N column-major per item), reconst0 = Reconst0 (3 x N per item) or NULL.  Outputs: Rt = R_t (3M x 4
 * column-major per item, R_t(1:3,:) = eye(3,4), |t2| = 1), reconst (3 x N per item, or NULL), iter, repr_err, status.
 * Missing observations (:28-29, :165): a NaN entry is handled as the reference's code handles it -- Normalize2Ddata.m:34-37 turns
 * every point of that VIEW into NaN, :165 then skips the whole view: its camera keeps the initial angles and translation, the
 * other views are adjusted.  Without reconst0, fewer than two complete views: status TFF_ST_TOO_FEW and NaN outputs (the
 * reference stops with an error at :73-74).  Same Levenberg-Marquardt loop as tff_bundle_adjust_batch_dev.
 * Per-POINT visibility, as the reference's header comment documents it (:4-22), is tff_bundle_adjust_tracks_batch_* of tftfund_tracks.h, included at the end. */
int tff_bundle_adjust_views_batch_dev(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in,
                                      const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt,
                                      double* reconst, int32_t* iter, double* repr_err, int32_t* status);
int tff_bundle_adjust_views_batch_host(tff_ctx* ctx, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in,
                                       const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt,
                                       double* reconst, int32_t* iter, double* repr_err, int32_t* status);

/* Minimal-sample hypotheses (BASELINE.json config 4): hypothesis b = the n correspondences
 * sample_idx[b*n .. b*n+n) of one shared scene (6 x Ns); n >= 7 (TFT) / 8 (F); shared CalM (27). */
int tff_linear_tft_pose_sampled_dev(tff_ctx* ctx, const double* scene, int32_t Ns, const double* calm,
                                    const int32_t* sample_idx, int64_t B, int32_t n, double* Rt2, double* Rt3,
                                    double* T, int32_t* status);
int tff_linear_f_pose_sampled_dev(tff_ctx* ctx, const double* scene, int32_t Ns, const double* calm,
                                  const int32_t* sample_idx, int64_t B, int32_t n, double* Rt2, double* Rt3,
                                  double* T, int32_t* status);

/* ---- matches with outliers: robust estimation over minimal samples of ONE scene (6 x Ns, shared CalM of 27 doubles) ------------------------------
 * tff_sample_indices_dev: row b of sample_idx (B x n int32) = n DISTINCT indices in [0, Ns), a function of (seed, first + b, n, Ns) only -- stateless and
 * counter-based, so any chunking or sharding of a hypothesis range draws the same samples.  1 <= n <= 16, Ns >= n, B >= 0, first >= 0 (else
 * TFF_E_INVALID).  One thread per hypothesis, exactly n draws: a Fisher-Yates shuffle of which only the n swaps are kept.  With wrapping uint64 arithmetic
 *     splitmix64(x): z = x + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)
 *     key = splitmix64(seed ^ ((first + b) * 0xD1342543DE82EF95))
 *     for i in 0 .. n-1:  u = splitmix64(key + i) >> 32;  r = i + ((u * (Ns - i)) >> 32);  out[i] = look(r);  record (r, look(i))
 *     look(p) = the value of the LAST record whose position is p, else p.            (numpy form: api.sample_indices_reference) */
int tff_sample_indices_dev(tff_ctx* ctx, uint64_t seed, int64_t first, int64_t B, int32_t n, int32_t Ns, int32_t* sample_idx);

/* Per-correspondence inlier flags of B pose hypotheses against the scene: mask (B x Ns, 0 / 1), counts (B, or NULL) = its row sums.  The rule and the
 * arithmetic per correspondence are those of tff_inlier_count_batch_dev (one shared device function), so the row sums equal that function's counts
 * (its counts at TFF_OPT_SCORE = 0: this call writes flags and hard row sums under either value of that option). */
int tff_inlier_mask_batch_dev(tff_ctx* ctx, const double* scene, int32_t Ns, const double* calm, const double* Rt2, const double* Rt3,
                              int64_t B, double threshold, uint8_t* mask, int32_t* counts);

/* RANSAC with local optimisation; method = TFF_METHOD_LINEAR_TFT or TFF_METHOD_LINEAR_F (ids below).  The algorithm, from the public pieces:
 *   1. idx = tff_sample_indices_dev(seed, 0, n_hyp, n_sample, Ns); hypotheses = the method's *_pose_sampled_dev on idx; count[h] = tff_inlier_count_batch_dev
 *      at `threshold` (pixels, per coordinate).  n_sample = 0: the method's minimum (7 / 8); at most 16.
 *   2. candidates: the n_cand hypotheses with status 0 that come first in the order (count descending, hypothesis index ascending); fewer successes, fewer
 *      candidates.
 *   3. lo_rounds times, for all candidates at once: each one's inlier mask -> its inliers in scene order, packed with device-side offsets -> ONE
 *      tff_pose_batch_ragged_dev call of `method` (n_max = Ns) -> the refits' counts.  A candidate adopts its refit iff the refit's status is 0 and its count
 *      is >= the candidate's: a fit to all of a pose's inliers is preferred to a minimal-sample pose of equal support, and a count never decreases.
 *   4. the winner: the largest count, ties to the earlier candidate.  Rt2, Rt3 (12 each), T (27), mask (Ns flags of that pose; their sum is info[0]),
 *      info = [inlier count, index of the hypothesis the winner started from, refits it adopted, number of candidates], status = TFF_ST_OK.
 *      No successful hypothesis: status TFF_ST_NO_POSE, NaN in the three arrays, zero mask, info = [0, -1, 0, 0].
 * TFF_OPT_SCORE = 1 (MSAC): "count" in steps 1 - 4 is the score tff_inlier_count_batch_dev writes under that option (w summed over the inliers, formula
 *   there): 1. score[h] per hypothesis (a failed hypothesis still -1, the selection keys (score + 1) << 32 | ... unchanged); 2. the order is (score
 *   descending, index ascending); 3. the masks, the packed refit batch and its offsets come from the hard rule as before, the refits are scored, and a
 *   candidate adopts its refit iff the refit's status is 0 and its score is >= the candidate's: a refit of equal support that fits its inliers worse is
 *   refused; 4. the winner has the largest score.  mask and info[0] are unchanged in meaning: the flags of the returned pose and their number.  The score
 *   of the returned pose is one tff_inlier_count_batch_dev call away and is not part of info.
 * The result is a function of the arguments (seed included) and the context's options only.  Hypotheses are processed in chunks of 262 144 (their pose records,
 * 107 MB, the counts of all n_hyp hypotheses and K * Ns * 49 bytes for the refits are workspaces of the context); the result does not depend on the chunk size.
 * _dev: device pointers, no host synchronisation and no device-to-host copy (selection, compaction and offsets are kernels).  _host: host pointers, one
 * synchronisation.  Ns at most 2^24 (the ragged call's n_max).
 * TFF_E_INVALID: another method, n_sample outside [minimum, 16], Ns < n_sample, n_hyp < 1 (or above 2^31 - 1), n_cand outside [1, 64], lo_rounds outside
 * [0, 8], a threshold that is not a positive finite number, a null pointer, and what the ragged call refuses (TFF_OPT_ROWS = 0, TFF_OPT_KERNEL = 1). */
int tff_robust_pose_dev(tff_ctx* ctx, int32_t method, const double* scene, int32_t Ns, const double* calm, uint64_t seed, int64_t n_hyp,
                        int32_t n_sample, double threshold, int32_t n_cand, int32_t lo_rounds, double* Rt2, double* Rt3, double* T,
                        uint8_t* mask, int32_t* info, int32_t* status);
int tff_robust_pose_host(tff_ctx* ctx, int32_t method, const double* scene, int32_t Ns, const double* calm, uint64_t seed, int64_t n_hyp,
                         int32_t n_sample, double threshold, int32_t n_cand, int32_t lo_rounds, double* Rt2, double* Rt3, double* T,
                         uint8_t* mask, int32_t* info, int32_t* status);

/* ---- robust estimation for a batch of scenes in one call: the triplet lists of a dataset (experiments_real.m) ----------------------------------------------
 * scenes: packed 6 x n_total doubles as in tff_pose_batch_ragged_*; scene_offsets: S + 1 int64 (on the device for _dev), scene s owns the correspondences
 * scene_offsets[s] .. scene_offsets[s+1]-1, n_s of them.  n_total (host, at most 2^31 - 1) bounds every offset and sizes `mask` and the workspaces; ns_max
 * (host, at most 2^24) bounds every n_s and is the refit's n_max.  calm: 27 doubles shared (calm_stride 0) or one CalM per scene (27).
 * Outputs: Rt2, Rt3 (S x 12), T (S x 27), mask (n_total bytes, the flags of scene s at mask[scene_offsets[s] ..]), info (S x 4), status (S).
 * THE CONTRACT: the outputs of scene s are bit for bit those of tff_robust_pose_dev on that scene alone -- its n_s correspondences, its CalM, the seed
 * seed + s in wrapping uint64 arithmetic, the same remaining arguments and context options.  Nothing depends on S, on the neighbouring scenes, or on where a
 * chunk of hypotheses (g = s * n_hyp + h, 262 144 per chunk) ends.  (There is one implementation: tff_robust_pose_* is this call for S = 1, the scene
 * [0, Ns) and the shared CalM, behind its own argument checks.  The sentence above says that a scene's result is independent of the list it stands in.)
 * Per-scene failures (the offsets of _dev are device data, so these are statuses, as in the ragged calls): n_s < n_sample gives TFF_ST_TOO_FEW; a decreasing
 * or negative offset, an offset above n_total or n_s > ns_max gives TFF_ST_BAD_OFFSETS; both with NaN poses, info = [0, -1, 0, 0] and zero flags, the
 * neighbours unaffected.  No successful hypothesis: TFF_ST_NO_POSE as above.  Whatever the offsets hold, no kernel reads or writes outside [0, n_total) of the
 * packed arrays; the whole mask is zeroed first.  (Scenes whose ranges overlap -- only malformed offsets make them -- share bytes of the mask: their
 * results are in bounds and otherwise unspecified.)
 * TFF_E_INVALID: what tff_robust_pose_dev refuses (the scene size apart), S < 0, S * n_hyp above 2^31 - 1, S * n_cand above the ragged call's 2^28 - 1 items,
 * a calm_stride other than 0 or 27, n_total or ns_max out of range; _host: decreasing or negative offsets, before any work.  S = 0 returns 0.
 * _dev: no host synchronisation and no device-to-host copy.  _host: host pointers (n_total and ns_max come from the offsets), one synchronisation.
 * Workspaces of the context, growing on demand: one chunk of hypotheses (51 doubles each, 78 with one CalM per scene), 4 * S * n_hyp bytes of counts, 49 * n_cand * n_total bytes for the
 * candidates' flags and packed refits (NOT S * n_cand * ns_max). */
int tff_robust_pose_scenes_dev(tff_ctx* ctx, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int32_t ns_max, int64_t S,
                               const double* calm, int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand,
                               int32_t lo_rounds, double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* status);
int tff_robust_pose_scenes_host(tff_ctx* ctx, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t S, const double* calm,
                                int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand, int32_t lo_rounds,
                                double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* status);
/* ---- the same with an early stop per scene: hypotheses in rounds, up to a cap, until a confidence is reached -------------------------------------------------
 * Arguments beyond tff_robust_pose_scenes_*: confidence c, 0 < c < 1; first_round, a multiple of 4 and >= 4; n_hyp is now the CAP per scene; used (S int32).
 *   Round ends: e_r = min(n_hyp, first_round << (r - 1)) for r = 1 .. R, until e_R = n_hyp; e_0 = 0.  At most 32 rounds.
 *   Thresholds: one per round, computed by the host in double: qmin_r = -expm1(log1p(-c) / e_r).  (A sample of n_sample correspondences is all-inlier with
 *   probability about w^n_sample at an inlier ratio w; e_r such samples all miss with probability (1 - w^n_sample)^e_r <= 1 - c iff w^n_sample >= qmin_r.)
 *   Round r draws the hypotheses h in [e_(r-1), e_r) of every scene that is still live.  Hypothesis h of scene s is what it is in the fixed call: a function of
 *   (seed + s, h).
 *   The stop rule, after round r, for each live scene of n_s correspondences: best = the largest of the scene's counts so far, a failed hypothesis counting
 *   -1.  I = best (TFF_OPT_SCORE = 0) or best / TFF_SCORE_UNITS in integer division (TFF_OPT_SCORE = 1: a lower bound on that hypothesis's inlier count, so
 *   MSAC never stops earlier than the count would for the same hypothesis).  w = (double)I / (double)n_s; q = w multiplied by itself n_sample - 1 times, in
 *   that order, in double.  The scene stops iff I >= 1 and q >= qmin_r.  No log and no pow runs on the device: given qmin_r from tff_robust_round_plan, the
 *   same few lines of numpy reproduce every decision exactly.
 *   used[s] = e_r for a scene that stops after round r, n_hyp for one that never stops, 0 for a scene that is TFF_ST_TOO_FEW or TFF_ST_BAD_OFFSETS (it never
 *   runs).
 *   After the rounds, steps 2 - 4 of tff_robust_pose_dev run unchanged on the scene-major counts (stride n_hyp): the whole array is -1 before round 1, so a
 *   hypothesis that was never drawn is never selected.
 * THE CONTRACT: the outputs of scene s are bit for bit those of tff_robust_pose_dev on that scene alone with n_hyp = used[s] and the seed seed + s, under the
 * same context options.  S, the neighbouring scenes, the chunking of a round's S * (e_r - e_(r-1)) rows (262 144 per chunk) and first_round do not matter
 * beyond what used[s] says.  first_round >= n_hyp is one round: the fixed call, with used = n_hyp for the valid scenes.
 * What the early stop saves: the hypotheses of a scene that has stopped get sample indices -1, their inlier counts are skipped, and with n_sample below
 * TFF_OPT_EXACT_BELOW (the default n_sample of 7 / 8 is) a wavefront of the pose kernel whose four hypotheses are all of that kind leaves at once -- whole
 * wavefronts are, as first_round and the chunk size are multiples of 4, a last round of odd length apart.  With n_sample >= TFF_OPT_EXACT_BELOW the fast-tier
 * pose kernels serve the call and are unchanged: there such a hypothesis still costs a pose (whose outputs are NaN / TFF_ST_TOO_FEW as before), and only
 * the counting is saved.
 * TFF_E_INVALID: what tff_robust_pose_scenes_* refuses; a confidence outside (0, 1) or NaN; first_round < 4 or not a multiple of 4; more than 32 rounds;
 * a null `used`.  _dev: no host synchronisation and no device-to-host copy; every workspace is reserved before the first launch.  Workspaces beyond the fixed
 * call's: 4 bytes per row of a chunk and 12 S bytes. */
/* Declared in tftfund_adaptive.h, which this header includes at its end: tff_robust_pose_scenes_adaptive_dev / _host (the arguments of
 * tff_robust_pose_scenes_*, plus `double confidence, int32_t first_round` after lo_rounds and `int32_t* used` before status) and tff_robust_round_plan. */
/* Declared in tftfund_guided.h, included at the end as well: quality-guided (PROSAC) sampling.  tff_robust_pose_scenes_guided_dev / _host take the adaptive
 * call's arguments plus `const int32_t* order, int64_t growth` after first_round: per scene a ranking of its correspondences, best first; the early
 * hypotheses draw from the best-ranked ones, and after `growth` draws the sampling is the uniform one.  tff_sample_indices_guided_dev is the sampler alone.
 * The definition and the refusals are stated in that header.  Without a ranking every call above computes what it always did. */

/* Inlier counts of S * per_scene pose hypotheses, hypothesis b against scene b / per_scene with that scene's CalM: counts[b] is what
 * tff_inlier_count_batch_dev returns for that pose against that scene alone (the same rule per correspondence; the same scores at TFF_OPT_SCORE = 1).  The hypotheses of a scene whose offsets are
 * negative, decreasing or above n_total count -1.  Four hypotheses per wavefront; a workgroup serves one scene at a time, staged in LDS when it fits 48 KB. */
int tff_inlier_count_scenes_dev(tff_ctx* ctx, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int64_t S, const double* calm,
                                int64_t calm_stride, const double* Rt2, const double* Rt3, int64_t per_scene, double threshold, int32_t* counts);

/* ---- multi-GPU (one process, one host thread + stream per device) ----------------------------------
 * The reference runs its triplets one after the other in one MATLAB thread (experiments.m:91-108); they are independent,
 * so a batch is cut into contiguous shards of ceil(B / G) triplets, shard g on device g, with no collective on the data
 * path.  tff_pose_batch_host_multi lands every shard directly in the caller's host arrays (same argument meaning as the
 * single-device `_host` entry points).  tff_pose_batch_dev_multi works on device-resident shards and gathers the
 * fixed-size result records (51 doubles per triplet: Rt2 | Rt3 | T) of all shards onto every device with one
 * ncclAllGather (RCCL over xGMI; librccl.so is opened on first use). */
typedef struct tff_multi tff_multi;
#define TFF_METHOD_LINEAR_TFT 0   /* method ids: the order of experiments.m:51-59 */
#define TFF_METHOD_RESSL_TFT 1
#define TFF_METHOD_NORDBERG_TFT 2
#define TFF_METHOD_FAUGPAPA_TFT 3
#define TFF_METHOD_PI 4
#define TFF_METHOD_PICOL 5
#define TFF_METHOD_LINEAR_F 6
#define TFF_METHOD_OPTIM_F 7
int tff_multi_create(tff_multi** out, const int32_t* devices, int32_t n_devices);   /* devices NULL: 0..n-1; n_devices <= 0: all visible */
void tff_multi_destroy(tff_multi* m);
int32_t tff_multi_size(const tff_multi* m);
tff_ctx* tff_multi_ctx(tff_multi* m, int32_t rank);                                  /* per-device context (options, synchronisation) */
void tff_multi_shard(const tff_multi* m, int64_t B, int32_t rank, int64_t* begin, int64_t* end);   /* [rank*chunk, min(B,(rank+1)*chunk)), chunk = ceil(B/G) */
int tff_pose_batch_host_multi(tff_multi* m, int32_t method, const double* corresp, const double* calm, int64_t calm_stride,
                              int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst, int32_t* iter,
                              int32_t* status);
/* corresp[g], calm[g]: shard g on device g.  records[g]: G * chunk * 51 doubles on device g; afterwards block r of EVERY
 * device = [Rt2 (chunk x 12) | Rt3 (chunk x 12) | T (chunk x 27)] of shard r.  status[g] (or status == NULL): G * chunk int32. */
int tff_pose_batch_dev_multi(tff_multi* m, int32_t method, const double* const* corresp, const double* const* calm,
                             int64_t calm_stride, int64_t B, int32_t N, double* const* records, int32_t* const* status);

/* ---- ragged batches: one call for triplets with different correspondence counts (layout at the top) -------------------------------
 * Each triplet's outputs are bit-identical to those of the fixed-N entry point of the method called on that triplet alone, under the same
 * context options: triplet b takes the kernels the fixed-N call takes for n_b (TFF_ST_TOO_FEW below 7 / 8 correspondences, the exact tiers
 * below TFF_OPT_EXACT_BELOW or with TFF_OPT_SOLVER = 1, the exact fix-up of what the fast tiers flag), and writes what that call writes,
 * its Reconst range included.  Methods: TFF_METHOD_LINEAR_TFT, TFF_METHOD_LINEAR_F and TFF_METHOD_OPTIM_F (others: TFF_E_INVALID).
 * TFF_OPT_PRE is ignored (the moments come from the row kernels' own passes, the default); TFF_OPT_ROWS = 0 and TFF_OPT_KERNEL = 1 give
 * TFF_E_INVALID.
 * TFF_METHOD_OPTIM_F: an item with n_b < max(8, TFF_OPT_EXACT_BELOW), or any item with TFF_OPT_SOLVER = 1, is done whole by the one-triplet
 * exact kernel (TFF_ST_TOO_FEW below 8); the others take the three staged kernels of the fixed-N call (linear stage, Gauss-Helmert
 * refinement, pose tail), then the exact kernel over what those flag; iter = it1 + it2.  The refinement runs as up to three launches by n_b:
 * observations and estimates in LDS up to bounds[0], the estimates alone in LDS up to bounds[1], the estimates in global slices beyond
 * (tff_optim_f_ragged_bounds; TFF_OPT_SPILL moves bounds[1] as it does for the fixed-N call).  Every item takes the storage route its
 * fixed-N call takes, whatever n_max and its neighbours are.  Workspaces, grown on demand: a record of 32 doubles per item, the slices
 * (only when n_max exceeds bounds[1]: one of 4 n_max + 16 doubles per resident wavefront), the plan and the retry list (B + 2 int32).
 * _dev: device pointers, offsets included; n_max (host) bounds every n_b (at most 2^24) and sizes the plan's workspace: the plan keeps
 * three int32 per n in 0 .. n_max and scans them in one workgroup, so its cost grows with n_max, not with B (n_max = 2^24: ~200 MB and a
 * scan of 16 M buckets per call) -- pass a bound close to the largest n_b; an item that breaks
 * it, or whose offsets decrease or are negative, gets TFF_ST_BAD_OFFSETS and NaN poses while its neighbours are unaffected.  No host
 * synchronisation and no device-to-host copy: after a warm-up call with the same method, B and n_max at least as large, a call can be
 * captured in a hipGraph.  B = 0 returns 0; at most 2^28 - 1 triplets per call. */
int tff_pose_batch_ragged_dev(tff_ctx* ctx, int32_t method, const double* corresp, const int64_t* offsets, int32_t n_max,
                              const double* calm, int64_t calm_stride, int64_t B, double* Rt2, double* Rt3, double* T,
                              double* reconst, int32_t* iter, int32_t* status);
/* host pointers; n_max is computed; decreasing or negative offsets give TFF_E_INVALID before any work.  The packed range
 * offsets[0] .. offsets[B] of corresp is read and the same range of reconst written. */
int tff_pose_batch_ragged_host(tff_ctx* ctx, int32_t method, const double* corresp, const int64_t* offsets, const double* calm,
                               int64_t calm_stride, int64_t B, double* Rt2, double* Rt3, double* T, double* reconst, int32_t* iter,
                               int32_t* status);
/* TFF_METHOD_OPTIM_F in a ragged call: bounds[0] = the largest n whose refinement keeps the normalised observations in LDS (the largest n with
 * optimf_refine_lds_bytes(n, true) + 512 <= 160 KiB / 8, where optimf_refine_lds_bytes(n, staged) = 8 (F + 4 n + 2 + (staged ? 6 n : 0)) for a
 * fixed part of F doubles), bounds[1] = the largest n whose estimates stay in LDS under the default options (the largest n with
 * 160 KiB / (optimf_refine_lds_bytes(n, false) + 512) >= 8).  Computed from the expressions the launchers use; 0 < bounds[0] < bounds[1]. */
int tff_optim_f_ragged_bounds(int32_t bounds[2]);

#ifdef __cplusplus
}
#endif
#include "tftfund_adaptive.h"   /* entry points added after library version 103 */
#include "tftfund_guided.h"     /* entry points added after library version 104 */
#include "tftfund_tracks.h"     /* entry points added after library version 107 */
#include "tftfund_tracks_loss.h" /* entry points added after library version 108 (its loss codes are those of the last header below) */
#include "tftfund_tracks_cov.h" /* entry points added after library version 109 (its loss codes are those of the last header below) */
#include "tftfund_cov.h"        /* entry points added after library version 106 (its loss codes are those of the header below) */
#include "tftfund_loss.h"       /* entry points added after library version 105 */
#endif
