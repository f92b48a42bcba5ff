// The covariance of the three-view bundle adjustment (tff_ba_covariance_*, include/tftfund_cov.h; tests/ba_cov_oracle.py is the definition in numpy).
//
// k_ba_cov<LOSS>: one wavefront per item, at GIVEN poses and points -- there is no Levenberg-Marquardt loop here.  It repeats what k_bundle_adjust_t
// (ba_kernel.h) computes before its loop (normalise3, Normal * K, the Euler angles by the same atan2 expressions, the loss constants), runs the three
// accumulation sweeps of that kernel at damping 0 -- ba_sweep, ba_point, ba_weigh and ba_vinv as they are --, which leaves the Schur complement S of the
// point blocks in BaLds::H, and then, with h = (0, 0, t2, 0) the gradient of the output's gauge |t2| = 1 and v = (0, 0, t2, t3) the camera part of the
// scale gauge (S v = 0),
//     Q_c  = inv(S + alpha h h') - v v' / (alpha (h'v)^2),          alpha = trace(S) / 12,
//     Q_Xi = inv(V_i) + inv(V_i) B_i' Q_c B_i inv(V_i),             V_i = Jp_i' Jp_i,  B_i = Jc_i' Jp_i  (12 x 3),
//     sigma0^2 = r'r / (3 m - 11),     cov = sigma0^2 Q_c,     point_cov_i = sigma0^2 Q_Xi  (xx xy xz yy yz zz).
// alpha puts the border into the metric of S (in pixels S is 1e8: with alpha = 1 the inverse loses what the sum S + h h' rounds away, 8e-4 .. 2e-2 of
// the result).  The inverse is twelve solves of the 12 x 12 system against the unit vectors (wave_solve_gj, any positive pivot), their result
// symmetrised, (A_ij + A_ji) / 2, so that cov is symmetric TO THE BIT.
//
// The poses may come in any scale: everything is evaluated at the scale given and converted to |t2| = 1 afterwards, exactly -- the residual does not
// change along the scale, so with g = 1 / |t2| the Jacobian's translation and point columns are those at scale 1 times g, and
// Q_c(scale 1) = G Q_c G, G = diag(1 (6 x), g (6 x)), Q_Xi(scale 1) = g^2 Q_Xi; sigma0 is the same.
//
// The points are read from global memory (four visits each: three sweeps and the pass below), so the LDS is the fixed PoseLds + BaLds of
// ba_lds_bytes(0) for every N and the kernel needs no launch classes.  NaN cov, sigma0 and point_cov: m <= 3 (no redundancy), a non-finite pose, a
// pivot that is not positive, a result that is not finite.
//
// Ragged form (item_n set): item b has item_n[b] correspondences, the first at index item_off[b] of corresp, reconst and point_cov -- the compact arrays
// of the plan of ba_ragged_kernel.h under a mask, the caller's otherwise; item_n[b] <= 0 is an item the plan failed: NaN cov and sigma0, nothing else
// touched.  The body is the same instruction stream for both forms: same item, same N, same bits.  k_ba_cov_scatter then puts point_cov in place.
#pragma once
#include "ba_ragged_kernel.h"

namespace tff {

struct BaCovArgs {
    const double* calm; long calm_stride;
    const double* Rt2; const double* Rt3;            // B x 12 (3x4 column-major), camera 1 = [I|0]
    const double* corresp; long B; int N;
    const double* reconst;                           // the points, 3 per correspondence
    double scale;                                    // c of the loss, in pixels
    double* cov; double* sigma0;                     // B x 144, B
    double* point_cov;                               // 6 per correspondence, or null
    const int* item_n = nullptr; const long* item_off = nullptr;
};

template <int LOSS>
__global__ void __launch_bounds__(64, 1) k_ba_cov(const BaCovArgs a) {
    TFF_DYNAMIC_LDS(double, smem);
    PoseLds* w = reinterpret_cast<PoseLds*>(smem);
    constexpr int base = (POSE_LDS_DOUBLES + 1) & ~1;
    BaLds* L = reinterpret_cast<BaLds*>(smem + base);
    double* Ai = w->Lp;                                                      // inv(S + alpha h h'): Ai[12 j + k] = entry (k, j)
    double* Qc = w->Lp + 144;                                                // Q_c, row-major
    const int lane = lane_id();
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        long first = 0;
        int N;
        if (a.item_n) {
            N = opaque_int(wave_uniform_i(a.item_n[b]));
            if (N > 0) first = a.item_off[b];                                // (the offset of a failed item is not defined)
        } else {
            N = opaque_int(a.N);
            first = b * (long)N;
        }
        const double* pts = a.corresp + 6 * first;
        const double* Xs = a.reconst + 3 * first;
        double* pc = a.point_cov ? a.point_cov + 6 * first : nullptr;
        bool fin = true;
        if (lane < 24) fin = fabs(((lane < 12) ? a.Rt2 : a.Rt3)[b * 12 + (lane % 12)]) <= 1.79e308;
        if (N <= 3 || wave_any(!fin)) {
            for (int e = lane; e < 144; e += WAVE) a.cov[b * 144 + e] = qnan;
            if (lane == 0) a.sigma0[b] = qnan;
            if (pc) for (int e = lane; e < 6 * N; e += WAVE) pc[e] = qnan;
            continue;
        }
        wave_sync();
        if (lane < 27) w->calm[lane] = a.calm[b * a.calm_stride + lane];
        wave_sync();
        normalise3(pts, N, w->nrm);                                          // BundleAdjustment.m:52-54
        BaLoss<LOSS> ls;
        if constexpr (LOSS != BA_LOSS_NONE) {
#pragma unroll
            for (int v = 0; v < 3; ++v) ls.is[v] = wave_uniform(1.0 / w->nrm[3 * v]);
            ls.c = a.scale; ls.c2 = a.scale * a.scale; ls.ic2 = 1.0 / ls.c2;
        }
        if (lane < 27) {                                                     // CalM(3j-2:3j,:) = Normal * CalM(...)   (:55)
            const int v = lane / 9, r = (lane % 9) / 3, c = lane % 3;
            const Mat3 Nm = normal_matrix(w->nrm, v);
            const Mat3 Km = load_K(w->calm, v);
            L->K[v][3 * r + c] = Nm.m[r][0] * Km.m[0][c] + Nm.m[r][1] * Km.m[1][c] + Nm.m[r][2] * Km.m[2][c];
        }
        if (lane < 2) {                                                      // angles (:92-94) and translations (:95) of cameras 2, 3
            const double* Rt = (lane == 0 ? a.Rt2 : a.Rt3) + b * 12;         // column-major 3x4: R(r,c) = Rt[r + 3c]
            const double R12 = Rt[1 + 6], R22 = Rt[2 + 6], R02 = Rt[0 + 6], R01 = Rt[0 + 3], R00 = Rt[0];
            L->cur.c[3 * lane + 0] = -atan2(R12, R22);
            L->cur.c[3 * lane + 1] = -atan2(-R02, sqrt(R12 * R12 + R22 * R22));
            L->cur.c[3 * lane + 2] = -atan2(R01, R00);
            for (int k = 0; k < 3; ++k) L->cur.c[6 + 3 * lane + k] = Rt[9 + k];
        }
        wave_sync();
        ba_prepare(L, &L->cur);
        ba_sweep<0, LOSS>(L, pts, w->nrm, Xs, N, 0.0, ls);
        ba_sweep<1, LOSS>(L, pts, w->nrm, Xs, N, 0.0, ls);
        ba_sweep<2, LOSS>(L, pts, w->nrm, Xs, N, 0.0, ls);
        wave_sync();
        // ---- Q_c ----
        double tr = 0.0, tt = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) tr += wave_uniform(L->H[k * (k + 1) / 2 + k]);
#pragma unroll
        for (int k = 6; k < 9; ++k) { const double tk = wave_uniform(L->cur.c[k]); tt += tk * tk; }     // h'v = |t2|^2
        const double alpha = tr / 12.0;
        for (int e = lane; e < 12 * 13; e += WAVE) {
            const int r = e / 13, c = e % 13;
            double v = 0.0;
            if (c < 12) {
                const int hi = (r > c) ? r : c, lo = (r > c) ? c : r;
                const double hr = (r >= 6 && r < 9) ? L->cur.c[r] : 0.0, hc = (c >= 6 && c < 9) ? L->cur.c[c] : 0.0;
                v = L->H[hi * (hi + 1) / 2 + lo] + alpha * hr * hc;
            }
            L->M[e] = v;
        }
        bool ok = true;
#pragma unroll 1
        for (int j = 0; j < 12; ++j) {                                       // column j of the inverse
            wave_sync();
            if (lane < 12) L->M[13 * lane + 12] = (lane == j) ? 1.0 : 0.0;
            wave_sync();
            ok = wave_solve_gj<12>(L->M, Ai + 12 * j, 0.0) && ok;
        }
        const double ivv = 1.0 / (alpha * tt * tt);
        for (int e = lane; e < 144; e += WAVE) {
            const int r = e / 12, c = e % 12;
            const double vr = (r >= 6) ? L->cur.c[r] : 0.0, vc = (c >= 6) ? L->cur.c[c] : 0.0;
            const double q = 0.5 * (Ai[12 * c + r] + Ai[12 * r + c]) - (vr * vc) * ivv;
            Qc[e] = q;
            fin = fin && fabs(q) <= 1.79e308;
        }
        wave_sync();
        // ---- r'r, and the point blocks ----
        double rr = 0.0;
#pragma unroll 1
        for (int i = lane; i < N; i += WAVE) {
            const Pt6 x = premap(load_pt(pts, i), w->nrm);
            const double X[3] = {Xs[3 * i], Xs[3 * i + 1], Xs[3 * i + 2]};
            double r[6], Jp[6][3], Jc[2][2][6];
            ba_point<true>(L, &L->cur, x, X, r, Jp, Jc);
            ba_weigh<LOSS>(ls, r, Jp, Jc);
#pragma unroll
            for (int k = 0; k < 6; ++k) rr += r[k] * r[k];
            if (pc) {
                double Vi[6], W[12][3];
                ba_vinv(Jp, 0.0, Vi);
#pragma unroll
                for (int p = 0; p < 12; ++p) {                               // W = B_i inv(V_i)
                    const int cp = ba_cam_of(p), lp = ba_col_of(p);
                    double bp[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) bp[k] = Jc[cp][0][lp] * Jp[2 + 2 * cp][k] + Jc[cp][1][lp] * Jp[3 + 2 * cp][k];
                    sym3_mul(Vi, bp, W[p]);
                }
                double q[6] = {Vi[0], Vi[1], Vi[2], Vi[3], Vi[4], Vi[5]};     // + W' Q_c W
#pragma unroll
                for (int p = 0; p < 12; ++p) {
                    double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
                    for (int c = 0; c < 12; ++c) {
                        const double qc = Qc[12 * p + c];
                        u[0] += qc * W[c][0]; u[1] += qc * W[c][1]; u[2] += qc * W[c][2];
                    }
                    q[0] += W[p][0] * u[0]; q[1] += W[p][0] * u[1]; q[2] += W[p][0] * u[2];
                    q[3] += W[p][1] * u[1]; q[4] += W[p][1] * u[2]; q[5] += W[p][2] * u[2];
                }
#pragma unroll
                for (int k = 0; k < 6; ++k) { pc[6 * i + k] = q[k]; fin = fin && fabs(q[k]) <= 1.79e308; }
            }
        }
        rr = wave_sum(rr);
        const double s2 = rr / (double)(3 * N - 11);
        ok = ok && !wave_any(!(fin && fabs(s2) <= 1.79e308));
        // ---- outputs, at the scale |t2| = 1 ----
        const double g = 1.0 / sqrt(tt);
        for (int e = lane; e < 144; e += WAVE) {
            const int r = e / 12, c = e % 12;
            const double gg = ((r >= 6) ? g : 1.0) * ((c >= 6) ? g : 1.0);
            a.cov[b * 144 + e] = ok ? (s2 * Qc[e]) * gg : qnan;
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

// ---- ragged: point_cov to its place (as k_ba_ragged_scatter does for the points) --------------------------------------------------------------------
struct BaCovScatter {
    BaRaggedPlan plan;
    const double* pc_ws;          // (mask only) k_ba_cov's point blocks in compact order, 6 x n_total
    double* point_cov;            // packed 6 x n_total
};
// one workgroup per item
__global__ void __launch_bounds__(BA_RAGGED_TILE) k_ba_cov_scatter(const BaCovScatter q) {
    const BaRaggedPlan& a = q.plan;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        long o0, o1;
        if (!ba_ragged_range(a, b, &o0, &o1)) continue;                      // ST_BAD_OFFSETS: the item's range is not defined
        const int m = a.m[b];
        if (m <= 0) {                                                        // the item failed: NaN over its range, unless the scan found it overlapping
            if (a.status[b] == ST_BAD_OFFSETS) continue;
            for (long e = 6 * o0 + (long)threadIdx.x; e < 6 * o1; e += BA_RAGGED_TILE) q.point_cov[e] = qnan;
            continue;
        }
        if (!a.mask) continue;                                               // k_ba_cov wrote the caller's array itself
        for (long i = o0 + (long)threadIdx.x; i < o1; i += BA_RAGGED_TILE)
            if (a.mask[i] == 0) {
#pragma unroll
                for (int e = 0; e < 6; ++e) q.point_cov[6 * i + e] = qnan;
            }
        const long c0 = a.coff[b];
        for (long k = (long)threadIdx.x; k < m; k += BA_RAGGED_TILE) {
            const long i = o0 + a.src[c0 + k];
#pragma unroll
            for (int e = 0; e < 6; ++e) q.point_cov[6 * i + e] = q.pc_ws[6 * (c0 + k) + e];
        }
    }
}

// the arguments of k_ba_cov for a plan whose count, scan and compact kernels have run (reconst0 of the plan: the points)
inline BaCovArgs ba_cov_ragged_args(const BaRaggedPlan& p, const double* calm, long calm_stride, const double* Rt2, const double* Rt3, double scale,
                                    double* cov, double* sigma0, double* pc_ws, double* point_cov) {
    BaCovArgs a{calm, calm_stride, Rt2, Rt3, p.mask ? p.packed : p.corresp, p.B, 0, p.mask ? p.rec0 : p.reconst0, scale, cov, sigma0,
                point_cov ? (p.mask ? pc_ws : point_cov) : nullptr};
    a.item_n = p.m;
    a.item_off = p.mask ? p.coff : p.offsets;
    return a;
}

constexpr size_t ba_cov_lds_bytes() { return ba_lds_bytes(0); }

}  // namespace tff
