// BundleAdjustment over tracks (include/tftfund_tracks.h; tests/ba_tracks_oracle.py is the definition in numpy): M = 2 .. 6 views, one wavefront per
// problem, a non-finite observation means "this point is not seen in this view" and nothing else -- what the header comment of the reference's
// BundleAdjustment.m:4-22 promises and its code (Normalize2Ddata.m:34-35: `mean` over the view) cannot do.
//
// This is k_bundle_adjust_views<M> (ba_views_kernel.h) with its wave-uniform seen[v] turned into a per-lane mask, one bit per view, derived from the loaded
// observation every time it is needed (no LDS per point beyond the 6N doubles of the points and their trial values):
//   * a point with fewer than two observations is dropped before everything else: it enters no sum, no triangulation, no norm, and its Reconst column is NaN;
//   * the normalisation of view v (Normalize2Ddata.m:33-39) runs over the n_v observations of the points that take part, with its own count;
//   * a missing observation contributes exact zeros to the residual and to both Jacobians (a branch on the lane's bit, never NaN * 0);
//   * the Schur entries (bav_entry / bav_chunk), the 3 x 3 point blocks (bav_vinv), the camera set-up (bav_prepare) and the solve (wave_solve_gj) are those
//     of ba_views_kernel.h, which this file leaves as it is.
// The lane of point i is i % 64 and a dropped point adds nothing, so appending all-NaN columns changes no bit of any other output: problems of different N
// go into one batch padded with NaN columns.
#pragma once
#include "ba_views_kernel.h"

namespace tff {

struct BatArgs {
    BavArgs v;                                             // the arguments of the whole-view call, same layouts
    int* used;                                             // B: points taking part (at least two observations), or null
};

constexpr double BAT_FINITE_MAX = 1.7976931348623157e308;
__device__ __forceinline__ bool bat_finite(double x) { return fabs(x) <= BAT_FINITE_MAX; }       // false for NaN and +-Inf
__device__ __forceinline__ bool bat_takes_part(unsigned m) { return (m & (m - 1)) != 0; }          // at least two bits

// the raw observation of point i in every view and the views that see it (both coordinates finite)
template <int M>
__device__ __forceinline__ unsigned bat_load_raw(const double* pts, int i, PtV<M>& p) {
    const double2* q = reinterpret_cast<const double2*>(pts + 2 * M * (long)i);
    unsigned m = 0;
#pragma unroll
    for (int v = 0; v < M; ++v) {
        const double2 a = q[v];
        p.v[2 * v] = a.x; p.v[2 * v + 1] = a.y;
        if (bat_finite(a.x) && bat_finite(a.y)) m |= 1u << v;
    }
    return m;
}
template <int M>
__device__ __forceinline__ unsigned bat_load(const double* pts, int i, const double* nrm, PtV<M>& p) {   // ... normalised   (:54)
    const unsigned m = bat_load_raw<M>(pts, i, p);
#pragma unroll
    for (int v = 0; v < M; ++v) {
        p.v[2 * v] = nrm[3 * v] * p.v[2 * v] + nrm[3 * v + 1];
        p.v[2 * v + 1] = nrm[3 * v] * p.v[2 * v + 1] + nrm[3 * v + 2];
    }
    return m;
}

// Normalize2Ddata.m:33-39 per view over the observations of the points taking part.  seen[v] = 1 iff n_v > 0; an unseen view gets the identity.
// Returns the number of points taking part; *bad: some view with n_v >= 1 has a normalisation that is not finite.
template <int M>
__device__ inline int bat_normalise(const double* pts, int N, double* nrm, double* seen, bool* bad) {
    const int lane = lane_id();
    double s[2 * M];
    int cnt[M], used = 0;
#pragma unroll
    for (int k = 0; k < 2 * M; ++k) s[k] = 0.0;
#pragma unroll
    for (int v = 0; v < M; ++v) cnt[v] = 0;
    for (int i = lane; i < N; i += WAVE) {
        PtV<M> x;
        const unsigned m = bat_load_raw<M>(pts, i, x);
        if (!bat_takes_part(m)) continue;
        ++used;
#pragma unroll
        for (int v = 0; v < M; ++v)
            if (m >> v & 1u) { s[2 * v] += x.v[2 * v]; s[2 * v + 1] += x.v[2 * v + 1]; ++cnt[v]; }
    }
    used = wave_sum_i(used);
    double c[2 * M], nv[M];
#pragma unroll
    for (int v = 0; v < M; ++v) {
        nv[v] = (double)wave_sum_i(cnt[v]);
        c[2 * v] = wave_sum(s[2 * v]) / nv[v];                               // points0 = mean(points,2) over the view's own observations
        c[2 * v + 1] = wave_sum(s[2 * v + 1]) / nv[v];
    }
    double d[M];
#pragma unroll
    for (int v = 0; v < M; ++v) d[v] = 0.0;
    for (int i = lane; i < N; i += WAVE) {
        PtV<M> x;
        const unsigned m = bat_load_raw<M>(pts, i, x);
        if (!bat_takes_part(m)) continue;
#pragma unroll
        for (int v = 0; v < M; ++v)
            if (m >> v & 1u) {
                const double dx = x.v[2 * v] - c[2 * v], dy = x.v[2 * v + 1] - c[2 * v + 1];
                d[v] += sqrt(dx * dx + dy * dy);
            }
    }
    const double r2 = sqrt(2.0);
    bool any_bad = false;
#pragma unroll
    for (int v = 0; v < M; ++v) {
        const double norm0 = wave_sum(d[v]) / nv[v];                         // :35
        const bool has = nv[v] > 0.0;
        const double sc = r2 / norm0, ox = -r2 * c[2 * v] / norm0, oy = -r2 * c[2 * v + 1] / norm0;
        const bool fin = bat_finite(sc) && bat_finite(ox) && bat_finite(oy);
        any_bad = any_bad || (has && !fin);
        if (lane == 0) {
            nrm[3 * v + 0] = (has && fin) ? sc : 1.0; nrm[3 * v + 1] = (has && fin) ? ox : 0.0; nrm[3 * v + 2] = (has && fin) ? oy : 0.0;
            seen[v] = has ? 1.0 : 0.0;
        }
    }
    wave_sync();
    *bad = any_bad;
    return used;
}

// bav_point with the visibility of THIS lane's point: an observation that does not exist contributes zero rows (:165-167)
template <int M, bool JAC>
__device__ __forceinline__ void bat_point(const BavLds<M>* L, const BavCams<M>* cam, const PtV<M>& x, unsigned mask, const double (&X)[3], double (&r)[2 * M],
                                          double (&Jp)[2 * M][3], double (&Jc)[M - 1][2][6]) {
#pragma unroll
    for (int v = 0; v < M; ++v) {
        if (!(mask >> v & 1u)) {
            r[2 * v] = 0.0; r[2 * v + 1] = 0.0;
            if (JAC) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { Jp[2 * v][k] = 0.0; Jp[2 * v + 1][k] = 0.0; }
                if (v > 0) {
#pragma unroll
                    for (int m = 0; m < 6; ++m) { Jc[v - 1][0][m] = 0.0; Jc[v - 1][1][m] = 0.0; }
                }
            }
            continue;
        }
        const double* A = (v == 0) ? L->K[0] : cam->KR[v - 1];
        double p[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = A[3 * k] * X[0] + A[3 * k + 1] * X[1] + A[3 * k + 2] * X[2] + ((v == 0) ? 0.0 : cam->Kt[v - 1][k]);
        const double iz = 1.0 / p[2];
        const double gx = p[0] * iz, gy = p[1] * iz;
        r[2 * v] = x.v[2 * v] - gx;                                          // Dist(point, Gamma(P*[Point;1]))   (:176-178)
        r[2 * v + 1] = x.v[2 * v + 1] - gy;
        if (JAC) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                Jp[2 * v][k] = -(A[k] - gx * A[6 + k]) * iz;                 // respect 3d point: P(:,1:3)   (:184)
                Jp[2 * v + 1][k] = -(A[3 + k] - gy * A[6 + k]) * iz;
            }
            if (v > 0) {
                const double* Kj = L->K[v];
#pragma unroll
                for (int m = 0; m < 3; ++m) {                                // respect rotation (angles)   (:191-192)
                    const double* D = cam->KdR[v - 1][m];
                    const double d0 = D[0] * X[0] + D[1] * X[1] + D[2] * X[2], d1 = D[3] * X[0] + D[4] * X[1] + D[5] * X[2],
                                 d2 = D[6] * X[0] + D[7] * X[1] + D[8] * X[2];
                    Jc[v - 1][0][m] = -(d0 - gx * d2) * iz;
                    Jc[v - 1][1][m] = -(d1 - gy * d2) * iz;
                    Jc[v - 1][0][3 + m] = -(Kj[m] - gx * Kj[6 + m]) * iz;    // respect translation: K   (:188)
                    Jc[v - 1][1][3 + m] = -(Kj[3 + m] - gy * Kj[6 + m]) * iz;
                }
            }
        }
    }
}

// one accumulation sweep over the points taking part: entries [30 SW, 30 SW + 30) of bav_entry
template <int M, int SW>
__device__ inline void bat_sweep(BavLds<M>* L, const double* pts, const double* Xs, int N, double lambda) {
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
template <int M, int SW = 0>
__device__ inline void bat_sweeps(BavLds<M>* L, const double* pts, const double* Xs, int N, double lambda) {
    if constexpr (SW < BavDims<M>::SWEEPS) {
        bat_sweep<M, SW>(L, pts, Xs, N, lambda);
        bat_sweeps<M, SW + 1>(L, pts, Xs, N, lambda);
    }
}

template <int M>
__device__ inline double bat_cost(const BavLds<M>* L, const BavCams<M>* cam, const double* pts, const double* Xs, int N) {
    double S = 0.0;
    for (int i = lane_id(); i < N; i += WAVE) {
        PtV<M> x;
        const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
        if (!bat_takes_part(mask)) continue;
        const double X[3] = {Xs[3 * i], Xs[3 * i + 1], Xs[3 * i + 2]};
        double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6];
        bat_point<M, false>(L, cam, x, mask, X, r, Jp, Jc);
#pragma unroll
        for (int k = 0; k < 2 * M; ++k) S += r[k] * r[k];
    }
    return wave_sum(S);
}

template <int M>
__global__ void __launch_bounds__(64, 1) k_bundle_adjust_tracks(const BatArgs q) {
    using D = BavDims<M>;
    constexpr int C = D::C, P = D::P;
    const BavArgs& a = q.v;
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
        if (lane == 0 && q.used) q.used[b] = used;
        if (used == 0 || bad_norm) {                                         // nothing to adjust / a view of one observation or of coincident ones
            bav_store_nan<M>(a, b, N);
            if (lane == 0 && a.status) a.status[b] = (used == 0) ? ST_TOO_FEW : ST_NONFINITE;
            continue;
        }
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
        // ---- Levenberg-Marquardt (oracle/ba_oracle.py: levenberg_marquardt) ----
        double lambda = BA_INIT_DAMPING;
        double S = bat_cost<M>(L, &L->cur, pts, Xc, N);
        int it = 0;
#pragma unroll 1
        while (it < BA_MAX_ITER && status == ST_OK) {
            bat_sweeps<M>(L, pts, Xc, N, lambda);
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
            const bool ok = wave_solve_gj<P>(L->Mx, L->dc);
            if (!ok) { status = ST_NONFINITE; break; }
            if (lane < P) L->trial.c[lane] = L->cur.c[lane] + L->dc[lane];
            wave_sync();
            bav_prepare<M>(L, &L->trial);
            // dX_i = -inv(V_i) Jp_i' (r_i + Jc_i dc); trial cost; norms for the step test, over the points taking part
            double St = 0.0, step2 = 0.0, x2 = 0.0;
            for (int i = lane; i < N; i += WAVE) {
                PtV<M> x;
                const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
                if (!bat_takes_part(mask)) continue;
                const double X[3] = {Xc[3 * i], Xc[3 * i + 1], Xc[3 * i + 2]};
                double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6], Vi[6];
                bat_point<M, true>(L, &L->cur, x, mask, X, r, Jp, Jc);
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
                double Xn[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) { Xn[k] = X[k] - dX[k]; Xt[3 * i + k] = Xn[k]; step2 += dX[k] * dX[k]; x2 += X[k] * X[k]; }
                double rt[2 * M], Jp2[2 * M][3], Jc2[M - 1][2][6];
                bat_point<M, false>(L, &L->trial, x, mask, Xn, rt, Jp2, Jc2);
#pragma unroll
                for (int k = 0; k < 2 * M; ++k) St += rt[k] * rt[k];
            }
            St = wave_sum(St); step2 = wave_sum(step2); x2 = wave_sum(x2);
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
                lambda = lambda / 10.0;
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
        if (a.reconst) {
            for (int i = lane; i < N; i += WAVE) {                           // a dropped point's column is NaN, also when Reconst0 was given
                PtV<M> x;
                const bool take = bat_takes_part(bat_load_raw<M>(pts, i, x));
#pragma unroll
                for (int k = 0; k < 3; ++k) a.reconst[b * 3 * (long)N + 3 * i + k] = take ? scale * Xc[3 * i + k] : qnan;
            }
        }
        const bool bad = !(fabs(S) <= 1.79e308);
        if (bad && status == ST_OK) status = ST_NONFINITE;
        if (lane == 0) {
            if (a.iter) a.iter[b] = it;
            if (a.repr_err) a.repr_err[b] = sqrt(S);                         // norm(func(variables)) over the observations that exist   (:105)
            if (a.status) a.status[b] = status;
        }
    }
}

}  // namespace tff
