// The covariance of the bundle adjustment over tracks (tff_ba_tracks_covariance_*, include/tftfund_tracks_cov.h; tests/ba_tracks_cov_oracle.py is the
// definition in numpy).
//
// k_ba_tracks_cov<M, LOSS>: M = 2 .. 6 views, LOSS none, Huber or Cauchy per observation, one wavefront per item, at GIVEN poses and points -- there is
// no Levenberg-Marquardt loop here.  It is k_ba_cov (ba_cov_kernel.h) on the pieces of the tracks kernels: it repeats what k_bundle_adjust_tracks and
// k_bundle_adjust_tracks_loss compute before their loop (bat_normalise, Normal * K, the change of coordinates to camera 1, the Euler angles by the same
// atan2 expressions, the loss constants), runs their accumulation sweeps at damping 0 -- bat_sweeps / batl_sweeps as they are --, which leaves the Schur
// complement S of the point blocks in BavLds::H, and then, with C_s the cameras whose view is seen, h = t2 in camera 2's translation slots the gradient
// of the output's gauge |t2| = 1 and v = (0 for angles; t_j of the seen cameras) the camera part of the scale gauge (S v = 0),
//     Q_c  = inv(S + alpha h h') - v v' / (alpha (h'v)^2),          alpha = trace(S) / (6 C_s),
//     Q_Xi = inv(V_i) + inv(V_i) B_i' Q_c B_i inv(V_i),             V_i = Jp_i' Jp_i,  B_i = Jc_i' Jp_i  (P x 3),
//     sigma0^2 = r'r / dof,  dof = 2 n_obs - (6 C_s + 3 m - 1),     cov = sigma0^2 Q_c,     point_cov_i = sigma0^2 Q_Xi  (xx xy xz yy yz zz).
// A camera nobody sees is a constant: its block of S is zero, gets a unit diagonal for the solve, and its rows and columns of Q_c are zeroed afterwards.
// The inverse is P solves of the P x P system against the unit vectors (wave_solve_gj, any positive pivot), their result symmetrised,
// (A_ij + A_ji) / 2, so that cov is symmetric TO THE BIT.
//
// The poses come as the tracks call takes Rt_in: first camera free, any common scale.  The change of coordinates (:80-86) is that of the tracks kernels
// -- the identity, bit for bit, on the adjustment's own outputs --; everything is evaluated at the scale given and converted to |t2| = 1 afterwards,
// exactly: with g = 1 / |t2|, Q_c(scale 1) = G Q_c G, G = diag(1 (3 C x), g (3 C x)), Q_Xi(scale 1) = g^2 Q_Xi; sigma0 is the same.
//
// The points are read from global memory.  The sweeps take an array of points in the frame of camera 1, so lane i % 64 writes the moved point i to
// `xwork` (3 per point, a workspace of the caller) and reads it back itself in every later pass: no lane reads what another wrote.  The LDS is
// therefore BavLds<M> plus two P x P matrices for every N, and the kernel needs no launch classes.  In the point pass B_i has non-zero rows only for the
// cameras that see the point: the products run over the lane's visibility bits, block by block, and neither W = B_i inv(V_i) (P x 3) nor the camera
// Jacobians are kept next to it -- Q_Xi = inv(V_i) + inv(V_i) (sum_ab B_a' Q_ab B_b) inv(V_i) from the 6 x 3 blocks B_a alone.
//
// NaN cov, sigma0 and point_cov: dof <= 0, a non-finite pose or point taking part, what the adjustment answers with a status other than 0 (no point
// taking part, a normalisation that is not finite), view 2 unseen, a pivot that is not positive, a result that is not finite.  point_cov is NaN over a
// dropped point.  The lane of point i is i % 64 and a dropped point adds nothing: appending all-NaN columns changes no bit of any other output.
#pragma once
#include "ba_tracks_loss_kernel.h"

namespace tff {

struct BatCovArgs {
    const double* calm; long calm_stride;                  // 9M doubles per set: MATLAB's 3M x 3 CalM, column-major
    const double* Rt;                                      // B x 12M: 3M x 4 column-major, first camera free, any common scale
    const double* corresp; long B; int N;                  // B x N x 2M
    const double* reconst;                                 // B x 3N: the points, in the frame and scale of Rt
    double scale;                                          // c of the loss, in pixels
    double* xwork;                                         // B x 3N: the points in the frame of camera 1 (workspace)
    double* cov; double* sigma0;                           // B x P x P, B
    double* point_cov;                                     // B x 6N, or null
};

template <int M> constexpr int batc_lds_doubles() { return bav_lds_doubles<M>() + 2 * BavDims<M>::P * BavDims<M>::P; }
template <int M> constexpr size_t batc_lds_bytes() { return (size_t)batc_lds_doubles<M>() * sizeof(double); }

// index in the parameter vector of column k (angles 0..2, translation 3..5) of camera a (0: view 2)
template <int M> __host__ __device__ constexpr int batc_param(int a, int k) { return (k < 3) ? 3 * a + k : 3 * (M - 1) + 3 * a + (k - 3); }

// B_a = Jc_a' Jp_a (6 x 3) of camera A, or zeros where the camera does not see the point
template <int M, int A>
__device__ __forceinline__ void batc_block(const double (&Jp)[2 * M][3], const double (&Jc)[M - 1][2][6], double (&Bm)[M - 1][6][3]) {
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int d = 0; d < 3; ++d) Bm[A][k][d] = Jc[A][0][k] * Jp[2 * (A + 1)][d] + Jc[A][1][k] * Jp[2 * (A + 1) + 1][d];
}
// T += B_A' Q_AB B_B over the 6 x 6 block (A, B) of Q_c (row-major P x P in LDS)
template <int M, int A, int B2>
__device__ __forceinline__ void batc_pair(const double* Qc, const double (&Bm)[M - 1][6][3], double (&T)[6]) {
    constexpr int P = BavDims<M>::P;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int l = 0; l < 6; ++l) {
            const double q = Qc[P * batc_param<M>(A, k) + batc_param<M>(B2, l)];
            u[0] += q * Bm[B2][l][0]; u[1] += q * Bm[B2][l][1]; u[2] += q * Bm[B2][l][2];
        }
        T[0] += Bm[A][k][0] * u[0]; T[1] += Bm[A][k][0] * u[1]; T[2] += Bm[A][k][0] * u[2];
        T[3] += Bm[A][k][1] * u[1]; T[4] += Bm[A][k][1] * u[2]; T[5] += Bm[A][k][2] * u[2];
    }
}
template <int M, int A, int B2 = 0>
__device__ __forceinline__ void batc_row(const double* Qc, const double (&Bm)[M - 1][6][3], unsigned mask, double (&T)[6]) {
    if constexpr (B2 < M - 1) {
        if (mask >> (B2 + 1) & 1u) batc_pair<M, A, B2>(Qc, Bm, T);
        batc_row<M, A, B2 + 1>(Qc, Bm, mask, T);
    }
}
template <int M, int A = 0>
__device__ __forceinline__ void batc_blocks(const double (&Jp)[2 * M][3], const double (&Jc)[M - 1][2][6], double (&Bm)[M - 1][6][3]) {
    if constexpr (A < M - 1) {
        batc_block<M, A>(Jp, Jc, Bm);                                        // (the rows of a missing observation are zero: so is its block)
        batc_blocks<M, A + 1>(Jp, Jc, Bm);
    }
}
template <int M, int A = 0>
__device__ __forceinline__ void batc_rows(const double* Qc, const double (&Bm)[M - 1][6][3], unsigned mask, double (&T)[6]) {
    if constexpr (A < M - 1) {
        if (mask >> (A + 1) & 1u) batc_row<M, A>(Qc, Bm, mask, T);
        batc_rows<M, A + 1>(Qc, Bm, mask, T);
    }
}
// Vi T Vi for symmetric 3 x 3 matrices packed xx xy xz yy yz zz, added to q
__device__ __forceinline__ void batc_sandwich(const double (&Vi)[6], const double (&T)[6], double (&q)[6]) {
    const double t0[3] = {T[0], T[1], T[2]}, t1[3] = {T[1], T[3], T[4]}, t2[3] = {T[2], T[4], T[5]};
    double y0[3], y1[3], y2[3];                                              // Y = Vi T, column by column (T symmetric: its columns are its rows)
    sym3_mul(Vi, t0, y0); sym3_mul(Vi, t1, y1); sym3_mul(Vi, t2, y2);
    const double r0[3] = {y0[0], y1[0], y2[0]}, r1[3] = {y0[1], y1[1], y2[1]}, r2[3] = {y0[2], y1[2], y2[2]};   // rows of Y
    double z0[3], z1[3], z2[3];                                              // row r of Y Vi = Vi (row r of Y)'
    sym3_mul(Vi, r0, z0); sym3_mul(Vi, r1, z1); sym3_mul(Vi, r2, z2);
    q[0] += z0[0]; q[1] += z0[1]; q[2] += z0[2]; q[3] += z1[1]; q[4] += z1[2]; q[5] += z2[2];
}

template <int M, int LOSS>
__global__ void __launch_bounds__(64, 1) k_ba_tracks_cov(const BatCovArgs a) {
    using D = BavDims<M>;
    constexpr int C = D::C, P = D::P;
    TFF_DYNAMIC_LDS(double, smem);
    BavLds<M>* L = reinterpret_cast<BavLds<M>*>(smem);
    double* Ai = smem + bav_lds_doubles<M>();                                // inv(S + alpha h h'): Ai[P j + k] = entry (k, j)
    double* Qc = Ai + P * P;                                                 // Q_c, row-major
    const int lane = lane_id();
    const double qnan = __builtin_nan("");
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int N = opaque_int(a.N);
        const double* pts = a.corresp + b * 2 * M * (long)N;
        const double* calm = a.calm + b * a.calm_stride;
        const double* Rt0 = a.Rt + b * 12 * M;                               // R_t(3j + r, c) = Rt0[3j + r + 3M c]
        const double* Xg = a.reconst + b * 3 * (long)N;
        double* Xw = a.xwork + b * 3 * (long)N;
        double* cov = a.cov + b * (long)(P * P);
        double* pc = a.point_cov ? a.point_cov + b * 6 * (long)N : nullptr;
        wave_sync();
        bool fin = true;
        for (int e = lane; e < 12 * M; e += WAVE) fin = fin && bat_finite(Rt0[e]);
        bool bad_norm;
        const int used = bat_normalise<M>(pts, N, L->nrm, L->seen, &bad_norm);      // :52-54
        // the observations of the points taking part, and whether those points are finite
        int nobs = 0;
        for (int i = lane; i < N; i += WAVE) {
            PtV<M> x;
            const unsigned mask = bat_load_raw<M>(pts, i, x);
            if (!bat_takes_part(mask)) continue;
            nobs += __builtin_popcount(mask);
            fin = fin && bat_finite(Xg[3 * i]) && bat_finite(Xg[3 * i + 1]) && bat_finite(Xg[3 * i + 2]);
        }
        nobs = wave_sum_i(nobs);
        int cs = 0;
#pragma unroll
        for (int v = 1; v < M; ++v) cs += (wave_uniform(L->seen[v]) != 0.0) ? 1 : 0;
        const int dof = 2 * nobs - (6 * cs + 3 * used - 1);
        const bool view2 = wave_uniform(L->seen[1]) != 0.0;
        if (used == 0 || bad_norm || !view2 || dof <= 0 || wave_any(!fin)) {
            for (int e = lane; e < P * P; e += WAVE) cov[e] = qnan;
            if (lane == 0) a.sigma0[b] = qnan;
            if (pc) for (int e = lane; e < 6 * N; e += WAVE) pc[e] = qnan;
            continue;
        }
        BatLoss<M, LOSS> ls;
        if constexpr (LOSS != BA_LOSS_NONE) {
#pragma unroll
            for (int v = 0; v < M; ++v) ls.is[v] = wave_uniform(1.0 / L->nrm[3 * v]);   // (an unseen view: 1)
            ls.l.c = a.scale; ls.l.c2 = a.scale * a.scale; ls.l.ic2 = 1.0 / ls.l.c2;
        }
        for (int e = lane; e < 9 * M; e += WAVE) {                           // CalM(3j-2:3j,:) = Normal * CalM(...)   (:55)
            const int v = e / 9, r = (e % 9) / 3, c = e % 3;
            const Mat3 Nm = normal_matrix(L->nrm, v);
            const double k0 = calm[(3 * v + 0) + 3 * M * c], k1 = calm[(3 * v + 1) + 3 * M * c], k2 = calm[(3 * v + 2) + 3 * M * c];
            L->K[v][3 * r + c] = Nm.m[r][0] * k0 + Nm.m[r][1] * k1 + Nm.m[r][2] * k2;
        }
        if (lane < 12) {                                                     // change_coord = R_t(1:3,:)   (:80)
            const int r = lane % 3, c = lane / 3;
            const double v = Rt0[r + 3 * M * c];
            if (c < 3) L->R1[3 * r + c] = v; else L->t1[r] = v;
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
        for (int i = lane; i < N; i += WAVE) {                               // Reconst = R1 * Reconst + t1   (:86); a dropped point's column is not read again
            const double X0 = Xg[3 * i], X1 = Xg[3 * i + 1], X2 = Xg[3 * i + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) Xw[3 * i + r] = L->R1[3 * r] * X0 + L->R1[3 * r + 1] * X1 + L->R1[3 * r + 2] * X2 + L->t1[r];
        }
        wave_sync();
        bav_prepare<M>(L, &L->cur);
        if constexpr (LOSS == BA_LOSS_NONE) bat_sweeps<M>(L, pts, Xw, N, 0.0);
        else batl_sweeps<M, LOSS>(L, pts, Xw, N, 0.0, ls);
        wave_sync();
        // ---- Q_c ----
        double tr = 0.0, tt = 0.0;
        for (int k = 0; k < P; ++k) tr += wave_uniform(L->H[k * (k + 1) / 2 + k]);       // (an unseen camera's diagonal is an exact zero)
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double tk = wave_uniform(L->cur.c[3 * C + k]); tt += tk * tk; }     // h'v = |t2|^2
        const double alpha = tr / (double)(6 * cs);
        for (int e = lane; e < P * (P + 1); e += WAVE) {
            const int r = e / (P + 1), c = e % (P + 1);
            double v = 0.0;
            if (c < P) {
                const int hi = (r > c) ? r : c, lo = (r > c) ? c : r;
                const double hr = (r >= 3 * C && r < 3 * C + 3) ? L->cur.c[r] : 0.0, hc = (c >= 3 * C && c < 3 * C + 3) ? L->cur.c[c] : 0.0;
                v = L->H[hi * (hi + 1) / 2 + lo] + alpha * hr * hc;
                if (r == c && L->seen[((r < 3 * C) ? r / 3 : (r - 3 * C) / 3) + 1] == 0.0) v = 1.0;
            }
            L->Mx[e] = v;
        }
        bool ok = true;
#pragma unroll 1
        for (int j = 0; j < P; ++j) {                                        // column j of the inverse
            wave_sync();
            if (lane < P) L->Mx[(P + 1) * lane + P] = (lane == j) ? 1.0 : 0.0;
            wave_sync();
            ok = wave_solve_gj<P>(L->Mx, Ai + P * j, 0.0) && ok;
        }
        const double ivv = 1.0 / (alpha * tt * tt);
        for (int e = lane; e < P * P; e += WAVE) {
            const int r = e / P, c = e % P;
            const bool sr = L->seen[((r < 3 * C) ? r / 3 : (r - 3 * C) / 3) + 1] != 0.0, sc = L->seen[((c < 3 * C) ? c / 3 : (c - 3 * C) / 3) + 1] != 0.0;
            const double vr = (r >= 3 * C && sr) ? L->cur.c[r] : 0.0, vc = (c >= 3 * C && sc) ? L->cur.c[c] : 0.0;
            const double q = (sr && sc) ? 0.5 * (Ai[P * c + r] + Ai[P * r + c]) - (vr * vc) * ivv : 0.0;
            Qc[e] = q;
            fin = fin && bat_finite(q);
        }
        wave_sync();
        // ---- r'r, and the point blocks ----
        double rr = 0.0;
#pragma unroll 1
        for (int i = lane; i < N; i += WAVE) {
            PtV<M> x;
            const unsigned mask = bat_load<M>(pts, i, L->nrm, x);
            if (!bat_takes_part(mask)) {
                if (pc) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) pc[6 * i + k] = qnan;
                }
                continue;
            }
            const double X[3] = {Xw[3 * i], Xw[3 * i + 1], Xw[3 * i + 2]};
            double r[2 * M], Jp[2 * M][3], Jc[M - 1][2][6];
            bat_point<M, true>(L, &L->cur, x, mask, X, r, Jp, Jc);
            if constexpr (LOSS != BA_LOSS_NONE) batl_weigh<M, LOSS>(ls, r, Jp, Jc);
#pragma unroll
            for (int k = 0; k < 2 * M; ++k) rr += r[k] * r[k];
            if (pc) {
                double Vi[6], Bm[M - 1][6][3], T[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                bav_vinv<M>(Jp, 0.0, Vi);
                batc_blocks<M>(Jp, Jc, Bm);
                batc_rows<M>(Qc, Bm, mask, T);
                double q[6] = {Vi[0], Vi[1], Vi[2], Vi[3], Vi[4], Vi[5]};
                batc_sandwich(Vi, T, q);
#pragma unroll
                for (int k = 0; k < 6; ++k) { pc[6 * i + k] = q[k]; fin = fin && bat_finite(q[k]); }
            }
        }
        rr = wave_sum(rr);
        const double s2 = rr / (double)dof;
        ok = ok && !wave_any(!(fin && bat_finite(s2)));
        // ---- outputs, at the scale |t2| = 1 ----
        const double g = 1.0 / sqrt(tt);
        for (int e = lane; e < P * P; e += WAVE) {
            const int r = e / P, c = e % P;
            const double gg = ((r >= 3 * C) ? g : 1.0) * ((c >= 3 * C) ? g : 1.0);
            cov[e] = ok ? (s2 * Qc[e]) * gg : qnan;
        }
        if (lane == 0) a.sigma0[b] = ok ? sqrt(s2) : qnan;
        if (pc) {                                                            // every lane rescales what it wrote itself
            const double f = s2 * (g * g);
            for (int i = lane; i < N; i += WAVE) {
#pragma unroll
                for (int k = 0; k < 6; ++k) pc[6 * i + k] = ok ? pc[6 * i + k] * f : qnan;
            }
        }
    }
}

}  // namespace tff
