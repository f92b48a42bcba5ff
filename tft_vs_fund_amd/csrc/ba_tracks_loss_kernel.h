// BundleAdjustment over tracks with a robust loss (include/tftfund_tracks_loss.h; tests/ba_tracks_loss_oracle.py is the definition in numpy):
// k_bundle_adjust_tracks_loss<M, LOSS>, M = 2 .. 6 views, LOSS Huber or Cauchy, one wavefront per problem.
//
// This is k_bundle_adjust_tracks<M> (ba_tracks_kernel.h) with the reweighted loop of k_bundle_adjust_loss<LOSS> (ba_kernel.h), the loss taken PER
// OBSERVATION -- in a track the unit that goes wrong is one observation, not the whole point:
//   * e_{v,i} = r_{v,i} / s_v in pixels, F = sum over the observations that exist of rho(|e_{v,i}|^2); w_{v,i} = rho'(|e_{v,i}|^2) at the current
//     parameters, and the two rows of observation (v, i) of the residual and of both Jacobians are multiplied by sqrt(w_{v,i}) / s_v inside the point
//     function's caller, from the residual the lane already holds, before anything is accumulated (batl_weigh).  c and the M values 1 / s_v are
//     wave-uniform registers: no LDS per point beyond the 6N doubles of the plain kernel;
//   * the step is freed of its component along the scale gauge v = (0; t_j of every camera that is seen; X_i of every point taking part): one wave
//     reduction of v . step and a second, cheap pass that applies it and evaluates the trial cost (ba_kernel.h does the same for three views);
//   * the Schur system is solved without a pivot floor (in pixels the gauge's pivot is the damping alone), and the damping does not fall below
//     BATL_LAMBDA_FLOOR: the matrix is about 1e9 in pixels and its rounding about 1e-7, a slowly converging Huber run would otherwise carry the damping
//     below the rounding within ten successes;
//   * `weight` (B x N x M, next to the layout of corresp): w_{v,i} at the final parameters; NaN where the observation does not exist, over a dropped
//     point and over an item whose status is not 0.
// The sweep and the trial pass are restated here rather than shared through a template parameter, so that ba_tracks_kernel.h, ba_views_kernel.h and
// ba_kernel.h stay as they are and every existing instance compiles to what it was.  bat_load, bat_normalise, bat_point, bav_vinv, bav_chunk,
// bav_prepare, wave_solve_gj and BaLoss / ba_rho / ba_rho1 are used as they stand.
#pragma once
#include "ba_tracks_kernel.h"

namespace tff {

constexpr double BATL_LAMBDA_FLOOR = 1e-3;

struct BatLossArgs {
    BatArgs t;                                             // the arguments of the plain tracks call
    double scale;                                          // c, in pixels
    double* weight;                                        // B x N x M or null
};
template <int M, int LOSS> struct BatLoss { BaLoss<LOSS> l; double is[M]; };           // c, c^2, 1 / c^2 (l.is is not used); 1 / s_v

// |e_{v,.}|^2 of one observation from its normalised residual (0 for one that does not exist: its rows are zero)
template <int M, int LOSS>
__device__ __forceinline__ double batl_e2(const BatLoss<M, LOSS>& ls, const double (&r)[2 * M], int v) {
    const double ex = r[2 * v] * ls.is[v], ey = r[2 * v + 1] * ls.is[v];
    return ex * ex + ey * ey;
}
// the rows of r, Jp, Jc of every observation times sqrt(w_{v,i}) / s_v (the rows of a missing observation are zero and stay zero)
template <int M, int LOSS>
__device__ __forceinline__ void batl_weigh(const BatLoss<M, LOSS>& ls, double (&r)[2 * M], double (&Jp)[2 * M][3], double (&Jc)[M - 1][2][6]) {
#pragma unroll
    for (int v = 0; v < M; ++v) {
        const double f = sqrt(ba_rho1<LOSS>(ls.l, batl_e2<M, LOSS>(ls, r, v))) * ls.is[v];
#pragma unroll
        for (int row = 2 * v; row < 2 * v + 2; ++row) {
            r[row] *= f;
#pragma unroll
            for (int k = 0; k < 3; ++k) Jp[row][k] *= f;
            if (v > 0) {
#pragma unroll
                for (int k = 0; k < 6; ++k) Jc[v - 1][row - 2 * v][k] *= f;
            }
        }
    }
}
// sum over the observations of a point that exist of rho(|e|^2)
template <int M, int LOSS>
__device__ __forceinline__ double batl_rho_sum(const BatLoss<M, LOSS>& ls, const double (&r)[2 * M], unsigned mask) {
    double S = 0.0;
#pragma unroll
    for (int v = 0; v < M; ++v)
        if (mask >> v & 1u) S += ba_rho<LOSS>(ls.l, batl_e2<M, LOSS>(ls, r, v));
    return S;
}

// bat_sweep with the rows weighed
template <int M, int LOSS, int SW>
__device__ inline void batl_sweep(BavLds<M>* L, const double* pts, const double* Xs, int N, double lambda, const BatLoss<M, LOSS>& ls) {
    const int lane = lane_id();
    double acc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int i = lane; i < N; i += WAVE) {
        PtV<M> x;
        const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
        if (!bat_takes_part(mask)) continue;
        const double X[3] = {Xs[3 * i], Xs[3 * i + 1], Xs[3 * i + 2]};
        double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6], Vi[6];
        bat_point<M, true>(L, &L->cur, x, mask, X, r, Jp, Jc);
        batl_weigh<M, LOSS>(ls, r, Jp, Jc);
        bav_vinv<M>(Jp, lambda, Vi);
        double g3[3] = {0.0, 0.0, 0.0}, u[3], s[2 * M];                      // s = r - Jp inv(V) Jp' r
#pragma unroll
        for (int row = 0; row < 2 * M; ++row) { g3[0] += Jp[row][0] * r[row]; g3[1] += Jp[row][1] * r[row]; g3[2] += Jp[row][2] * r[row]; }
        sym3_mul(Vi, g3, u);
#pragma unroll
        for (int row = 0; row < 2 * M; ++row) s[row] = r[row] - (Jp[row][0] * u[0] + Jp[row][1] * u[1] + Jp[row][2] * u[2]);
        bav_chunk<M, 30 * SW>(Jp, Jc, Vi, s, acc);
    }
    const double tot = wave_reduce_scatter<32>(acc);
    const int idx = reduce32_index(lane);
    if ((lane & 1) == 0 && idx < 30) L->H[30 * SW + idx] = tot;
}
template <int M, int LOSS, int SW = 0>
__device__ inline void batl_sweeps(BavLds<M>* L, const double* pts, const double* Xs, int N, double lambda, const BatLoss<M, LOSS>& ls) {
    if constexpr (SW < BavDims<M>::SWEEPS) {
        batl_sweep<M, LOSS, SW>(L, pts, Xs, N, lambda, ls);
        batl_sweeps<M, LOSS, SW + 1>(L, pts, Xs, N, lambda, ls);
    }
}

// F = sum rho(|e|^2) of parameter set `cam` with points Xs
template <int M, int LOSS>
__device__ inline double batl_cost(const BavLds<M>* L, const BavCams<M>* cam, const double* pts, const double* Xs, int N, const BatLoss<M, LOSS>& ls) {
    double S = 0.0;
    for (int i = lane_id(); i < N; i += WAVE) {
        PtV<M> x;
        const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
        if (!bat_takes_part(mask)) continue;
        const double X[3] = {Xs[3 * i], Xs[3 * i + 1], Xs[3 * i + 2]};
        double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6];
        bat_point<M, false>(L, cam, x, mask, X, r, Jp, Jc);
        S += batl_rho_sum<M, LOSS>(ls, r, mask);
    }
    return wave_sum(S);
}

// NaN over the weights of item b
template <int M>
__device__ inline void batl_weight_nan(double* weight, long b, int N) {
    const double qnan = __builtin_nan("");
    if (weight) for (long e = lane_id(); e < (long)M * N; e += WAVE) weight[b * M * (long)N + e] = qnan;
}

template <int M, int LOSS>
__global__ void __launch_bounds__(64, 1) k_bundle_adjust_tracks_loss(const BatLossArgs q) {
    static_assert(LOSS == BA_LOSS_HUBER || LOSS == BA_LOSS_CAUCHY, "the plain call is k_bundle_adjust_tracks");
    using D = BavDims<M>;
    constexpr int C = D::C, P = D::P;
    const BavArgs& a = q.t.v;
    TFF_DYNAMIC_LDS(double, smem);
    BavLds<M>* L = reinterpret_cast<BavLds<M>*>(smem);
    double* Xc = smem + bav_lds_doubles<M>();                                // current points (3N), then trial points (3N)
    const int lane = lane_id();
    const double qnan = __builtin_nan("");
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int N = opaque_int(a.N);
        double* Xt = Xc + 3 * N;
        const double* pts = a.corresp + b * 2 * M * (long)N;
        const double* calm = a.calm + b * a.calm_stride;
        const double* Rt0 = a.Rt_in + b * 12 * M;                            // R_t_0(3j + r, c) = Rt0[3j + r + 3M c]
        wave_sync();
        bool bad_norm;
        const int used = bat_normalise<M>(pts, N, L->nrm, L->seen, &bad_norm);      // :52-54
        if (lane == 0 && q.t.used) q.t.used[b] = used;
        if (used == 0 || bad_norm) {                                         // nothing to adjust / a view of one observation or of coincident ones
            bav_store_nan<M>(a, b, N);
            batl_weight_nan<M>(q.weight, b, N);
            if (lane == 0 && a.status) a.status[b] = (used == 0) ? ST_TOO_FEW : ST_NONFINITE;
            continue;
        }
        BatLoss<M, LOSS> ls;
#pragma unroll
        for (int v = 0; v < M; ++v) ls.is[v] = wave_uniform(1.0 / L->nrm[3 * v]);   // (an unseen view: 1)
        ls.l.c = q.scale; ls.l.c2 = q.scale * q.scale; ls.l.ic2 = 1.0 / ls.l.c2;
        for (int e = lane; e < 9 * M; e += WAVE) {                           // CalM(3j-2:3j,:) = Normal * CalM(...)   (:55)
            const int v = e / 9, r = (e % 9) / 3, c = e % 3;
            const Mat3 Nm = normal_matrix(L->nrm, v);
            const double k0 = calm[(3 * v + 0) + 3 * M * c], k1 = calm[(3 * v + 1) + 3 * M * c], k2 = calm[(3 * v + 2) + 3 * M * c];
            L->K[v][3 * r + c] = Nm.m[r][0] * k0 + Nm.m[r][1] * k1 + Nm.m[r][2] * k2;
        }
        if (lane < 12) {                                                     // change_coord = R_t_0(1:3,:)   (:80)
            const int r = lane % 3, c = lane / 3;
            const double v = Rt0[r + 3 * M * c];
            if (c < 3) L->R1[3 * r + c] = v; else L->t1[r] = v;
        }
        wave_sync();
        int status = ST_OK;
        if (a.reconst0) {
            for (int e = lane; e < 3 * N; e += WAVE) Xc[e] = a.reconst0[b * 3 * (long)N + e];
        } else {                                                             // initial triangulation from the views that see the point   (:59-77)
            for (int e = lane; e < 12 * M; e += WAVE) {                      // cameras{j} = CalM(3j-2:3j,:) * R_t_0(3j-2:3j,:)
                const int j = e / 12, r = (e % 12) >> 2, c = e & 3;
                L->P0[j][e % 12] = L->K[j][3 * r] * Rt0[3 * j + 0 + 3 * M * c] + L->K[j][3 * r + 1] * Rt0[3 * j + 1 + 3 * M * c] +
                                   L->K[j][3 * r + 2] * Rt0[3 * j + 2 + 3 * M * c];
            }
            wave_sync();
            bool conv_all = true;
            for (int i = lane; i < N; i += WAVE) {
                PtV<M> x;
                const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
                if (!bat_takes_part(mask)) continue;
                double S[4][4], X[4];
                tri_zero(S);
#pragma unroll
                for (int v = 0; v < M; ++v) {
                    if (!(mask >> v & 1u)) continue;                         // :65-67
                    double Pv[12];
#pragma unroll
                    for (int c = 0; c < 12; ++c) Pv[c] = L->P0[v][c];
                    tri_accum(S, Pv, x.v[2 * v], x.v[2 * v + 1]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = r + 1; c < 4; ++c) S[r][c] = S[c][r];
                bool conv;
                spd_min_eigvec<4>(S, X, 200, &conv);                         // V(:,4) of svd(ls_matrix)   (triangulation3D.m:61-62)
                conv_all = conv_all && conv;
                const double iw = 1.0 / X[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) Xc[3 * i + k] = X[k] * iw;       // Reconst0(:,i) = X(1:3)/X(4)   (:75)
            }
            if (wave_any(!conv_all)) status = ST_NONFINITE;                  // two coincident smallest singular values: no defined start
        }
        wave_sync();
        // ---- change of coordinates so that the first pose is [Id 0] (:80-86), angles (:92-94) and translations (:95) ----
        if (lane < C) {
            const int j = lane + 1;
            double Rj[9], tj[3], Rn[9];
            for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) Rj[3 * r + c] = Rt0[3 * j + r + 3 * M * c]; tj[r] = Rt0[3 * j + r + 3 * M * 3]; }
            double w1[3];                                                    // change_coord(:,1:3).' * change_coord(:,4)
            for (int k = 0; k < 3; ++k) w1[k] = L->R1[0 + k] * L->t1[0] + L->R1[3 + k] * L->t1[1] + L->R1[6 + k] * L->t1[2];
            for (int r = 0; r < 3; ++r) {
                tj[r] = tj[r] - (Rj[3 * r] * w1[0] + Rj[3 * r + 1] * w1[1] + Rj[3 * r + 2] * w1[2]);
                for (int c = 0; c < 3; ++c) Rn[3 * r + c] = Rj[3 * r] * L->R1[3 * c] + Rj[3 * r + 1] * L->R1[3 * c + 1] + Rj[3 * r + 2] * L->R1[3 * c + 2];
            }
            const double R12 = Rn[5], R22 = Rn[8], R02 = Rn[2], R01 = Rn[1], R00 = Rn[0];
            L->cur.c[3 * lane + 0] = -atan2(R12, R22);
            L->cur.c[3 * lane + 1] = -atan2(-R02, sqrt(R12 * R12 + R22 * R22));
            L->cur.c[3 * lane + 2] = -atan2(R01, R00);
            for (int k = 0; k < 3; ++k) L->cur.c[3 * C + 3 * lane + k] = tj[k];
        }
        for (int i = lane; i < N; i += WAVE) {                               // Reconst0 = R1 * Reconst0 + t1   (:86); a dropped point's column is not read again
            const double X0 = Xc[3 * i], X1 = Xc[3 * i + 1], X2 = Xc[3 * i + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) Xc[3 * i + r] = L->R1[3 * r] * X0 + L->R1[3 * r + 1] * X1 + L->R1[3 * r + 2] * X2 + L->t1[r];
        }
        wave_sync();
        bav_prepare<M>(L, &L->cur);
        // ---- Levenberg-Marquardt, reweighted (tests/ba_tracks_loss_oracle.py) ----
        double lambda = BA_INIT_DAMPING;
        double S = batl_cost<M, LOSS>(L, &L->cur, pts, Xc, N, ls);
        int it = 0;
#pragma unroll 1
        while (it < BA_MAX_ITER && status == ST_OK) {
            batl_sweeps<M, LOSS>(L, pts, Xc, N, lambda, ls);
            wave_sync();
            for (int e = lane; e < P * (P + 1); e += WAVE) {                 // (sum Jc'Jc - W inv(V) W' + lambda I) dc = -sum Jc' s
                const int r = e / (P + 1), c = e % (P + 1);
                double v;
                if (c == P) v = L->H[D::NT + r];
                else {
                    const int hi = (r > c) ? r : c, lo = (r > c) ? c : r;
                    v = L->H[hi * (hi + 1) / 2 + lo];
                    if (r == c) {                                            // a camera nobody sees has an all-zero block: dc = 0 for it, whatever lambda is
                        const int cam = (r < 3 * C) ? r / 3 : (r - 3 * C) / 3;
                        v = (L->seen[cam + 1] != 0.0) ? v + lambda : 1.0;
                    }
                }
                L->Mx[e] = v;
            }
            wave_sync();
            const bool ok = wave_solve_gj<P>(L->Mx, L->dc, 0.0);             // no pivot floor: any positive finite pivot is taken
            if (!ok) { status = ST_NONFINITE; break; }
            // dX_i = -inv(V_i) Jp_i' (r_i + Jc_i dc), v . step over the points, |X|^2
            double St = 0.0, step2 = 0.0, x2 = 0.0, vs = 0.0;
            for (int i = lane; i < N; i += WAVE) {
                PtV<M> x;
                const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
                if (!bat_takes_part(mask)) continue;
                const double X[3] = {Xc[3 * i], Xc[3 * i + 1], Xc[3 * i + 2]};
                double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6], Vi[6];
                bat_point<M, true>(L, &L->cur, x, mask, X, r, Jp, Jc);
                batl_weigh<M, LOSS>(ls, r, Jp, Jc);
                bav_vinv<M>(Jp, lambda, Vi);
#pragma unroll
                for (int cj = 0; cj < C; ++cj)
#pragma unroll
                    for (int row = 0; row < 2; ++row) {
                        double e = 0.0;
#pragma unroll
                        for (int m = 0; m < 3; ++m) e += Jc[cj][row][m] * wave_uniform(L->dc[3 * cj + m]) + Jc[cj][row][3 + m] * wave_uniform(L->dc[3 * C + 3 * cj + m]);
                        r[2 + 2 * cj + row] += e;
                    }
                double g3[3] = {0.0, 0.0, 0.0}, dX[3];
#pragma unroll
                for (int row = 0; row < 2 * M; ++row) { g3[0] += Jp[row][0] * r[row]; g3[1] += Jp[row][1] * r[row]; g3[2] += Jp[row][2] * r[row]; }
                sym3_mul(Vi, g3, dX);
#pragma unroll
                for (int k = 0; k < 3; ++k) { Xt[3 * i + k] = X[k] - dX[k]; x2 += X[k] * X[k]; vs -= X[k] * dX[k]; }
            }
            // The cost does not change along v = (0; t_j of the cameras that are seen; X), the common scale: the step has no component along v, and what
            // rounding leaves there (in pixels only the damping stands in that direction) is taken out: step -= v (v . step) / (v . v).  A camera nobody
            // sees is not in v: its step is exactly zero and stays so.
            vs = wave_sum(vs); x2 = wave_sum(x2);
            double vv = x2;
            for (int k = 0; k < 3 * C; ++k) {
                if (wave_uniform(L->seen[k / 3 + 1]) == 0.0) continue;
                const double tk = wave_uniform(L->cur.c[3 * C + k]);
                vs += tk * wave_uniform(L->dc[3 * C + k]); vv += tk * tk;
            }
            const double beta = vs / vv;
            wave_sync();
            if (lane < P) {
                const bool in_v = lane >= 3 * C && L->seen[(lane - 3 * C) / 3 + 1] != 0.0;
                const double d = L->dc[lane] - (in_v ? beta * L->cur.c[lane] : 0.0);
                L->dc[lane] = d;
                L->trial.c[lane] = L->cur.c[lane] + d;
            }
            wave_sync();
            bav_prepare<M>(L, &L->trial);
            for (int i = lane; i < N; i += WAVE) {                           // the trial points without the gauge component, and the trial cost
                PtV<M> x;
                const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
                if (!bat_takes_part(mask)) continue;
                double Xn[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double Xk = Xc[3 * i + k];
                    Xn[k] = Xt[3 * i + k] - beta * Xk;
                    Xt[3 * i + k] = Xn[k];
                    step2 += (Xn[k] - Xk) * (Xn[k] - Xk);
                }
                double rt[2 * M], Jp2[2 * M][3], Jc2[M - 1][2][6];
                bat_point<M, false>(L, &L->trial, x, mask, Xn, rt, Jp2, Jc2);
                St += batl_rho_sum<M, LOSS>(ls, rt, mask);
            }
            St = wave_sum(St); step2 = wave_sum(step2);
            for (int k = 0; k < P; ++k) { const double dk = wave_uniform(L->dc[k]), ck = wave_uniform(L->cur.c[k]); step2 += dk * dk; x2 += ck * ck; }
            const bool small_step = sqrt(step2) < BA_TOL_X * (1.4901161193847656e-08 + sqrt(x2));
            if (St < S) {                                                    // successful step
                ++it;
                const bool done = fabs(St - S) <= BA_TOL_FUN * S || small_step;
                for (int i = lane; i < N; i += WAVE) {                       // (a dropped point has no trial value)
                    PtV<M> x;
                    if (!bat_takes_part(bat_load_raw<M>(pts, i, x))) continue;
#pragma unroll
                    for (int k = 0; k < 3; ++k) Xc[3 * i + k] = Xt[3 * i + k];
                }
                if (lane < P) L->cur.c[lane] = L->trial.c[lane];
                wave_sync();
                bav_prepare<M>(L, &L->cur);
                S = St;
                lambda = fmax(lambda / 10.0, BATL_LAMBDA_FLOOR);
                if (done) break;
            } else {
                lambda = lambda * 10.0;
                if (small_step || lambda > 1e16) break;
            }
        }
        // ---- outputs: R = Rx*Ry*Rz, scale 1/|t2| (:108-122) ----
        wave_sync();
        const double t2x = L->cur.c[3 * C], t2y = L->cur.c[3 * C + 1], t2z = L->cur.c[3 * C + 2];
        const double scale = rsqrt(t2x * t2x + t2y * t2y + t2z * t2z);
        double* out = a.Rt + b * 12 * M;                                     // R_t(3j + r, c) = out[3j + r + 3M c]
        if (lane < 12) { const int r = lane % 3, c = lane / 3; out[r + 3 * M * c] = (r == c) ? 1.0 : 0.0; }
        if (lane < C) {
            const double* ang = L->cur.c + 3 * lane;
            const double cx = cos(ang[0]), sx = sin(ang[0]), cy = cos(ang[1]), sy = sin(ang[1]), cz = cos(ang[2]), sz = sin(ang[2]);
            Mat3 Rx{{{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}}}, Ry{{{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}}, Rz{{{cz, -sz, 0}, {sz, cz, 0}, {0, 0, 1}}};
            const Mat3 R = mat3_mul(mat3_mul(Rx, Ry), Rz);
            const int j = lane + 1;
            for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) out[3 * j + r + 3 * M * c] = R.m[r][c]; out[3 * j + r + 3 * M * 3] = scale * L->cur.c[3 * C + 3 * lane + r]; }
        }
        const bool bad = !(fabs(S) <= 1.79e308);
        if (bad && status == ST_OK) status = ST_NONFINITE;
        if (a.reconst || q.weight) {
            for (int i = lane; i < N; i += WAVE) {                           // a dropped point's column is NaN, also when Reconst0 was given
                PtV<M> x;
                const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
                const bool take = bat_takes_part(mask);
                if (a.reconst) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) a.reconst[b * 3 * (long)N + 3 * i + k] = take ? scale * Xc[3 * i + k] : qnan;
                }
                if (q.weight) {                                              // w_{v,i} at the final parameters
                    double w[M];
#pragma unroll
                    for (int v = 0; v < M; ++v) w[v] = qnan;
                    if (take && status == ST_OK) {
                        const double X[3] = {Xc[3 * i], Xc[3 * i + 1], Xc[3 * i + 2]};
                        double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6];
                        bat_point<M, false>(L, &L->cur, x, mask, X, r, Jp, Jc);
#pragma unroll
                        for (int v = 0; v < M; ++v)
                            if (mask >> v & 1u) w[v] = ba_rho1<LOSS>(ls.l, batl_e2<M, LOSS>(ls, r, v));
                    }
#pragma unroll
                    for (int v = 0; v < M; ++v) q.weight[(b * (long)N + i) * M + v] = w[v];
                }
            }
        }
        if (lane == 0) {
            if (a.iter) a.iter[b] = it;
            if (a.repr_err) a.repr_err[b] = sqrt(S);                         // sqrt(F): pixels, robustified
            if (a.status) a.status[b] = status;
        }
    }
}

// loss == TFF_LOSS_NONE: the plain kernel ran and knows no weights.  1 where the observation exists and the point takes part, NaN elsewhere and over an
// item whose status is not 0.  One thread per point.
struct BatOnesArgs { double* weight; const double* corresp; const int* status; long B; int N; int M; };   // status may be null
__global__ void __launch_bounds__(256) k_bat_weight_ones(const BatOnesArgs a) {
    const double qnan = __builtin_nan("");
    const long total = a.B * (long)a.N;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const double* p = a.corresp + e * 2 * a.M;
        const bool item_ok = !a.status || a.status[e / a.N] == ST_OK;
        unsigned m = 0;
        for (int v = 0; v < a.M; ++v)
            if (bat_finite(p[2 * v]) && bat_finite(p[2 * v + 1])) m |= 1u << v;
        const bool take = bat_takes_part(m) && item_ok;
        for (int v = 0; v < a.M; ++v) a.weight[e * a.M + v] = (take && (m >> v & 1u)) ? 1.0 : qnan;
    }
}

}  // namespace tff
