// Robust three-view pose estimation (tff_robust_pose_*, tff_sample_indices_dev, tff_inlier_mask_batch_dev): RANSAC over minimal samples of one
// scene with local optimisation of the K best hypotheses.  The hypotheses, their inlier counts and the refits come from the existing kernels
// (the *_sampled route of the pose kernels, k_inlier_count_*, the ragged chain); this file holds what ties them together on the device:
//
//   k_sample_indices   n distinct indices per hypothesis, a function of (seed, hypothesis index, n, Ns) alone (counter-based)
//   k_inlier_mask      the inlier rule of k_repr_error per correspondence, written out as 0 / 1 flags (+ the row sums)
//   k_robust_mark      a failed hypothesis (status != 0) gets the count -1: it is never a candidate
//   k_robust_topk      one round of the top-K selection: the largest packed key (count, index) below the previous round's
//   k_robust_seed      the K keys -> candidate counts, hypothesis indices, validity
//   k_robust_offsets   the candidates' inlier counts -> offsets of the packed refit batch
//   k_robust_compact   a candidate's inliers, in scene order, into its range of the packed batch
//   k_robust_adopt     a candidate takes its refit iff that succeeded and has at least as many inliers
//   k_robust_finish    the winner (largest count, ties to the earlier candidate) -> the caller's outputs
//
// Hypotheses are processed in chunks of ROBUST_CHUNK (the pose records of a chunk, 51 doubles per hypothesis, are the only workspace that grows
// with the chunk: 107 MB); only the int32 counts of ALL hypotheses are kept, and the K winners are recomputed from their indices -- the sampler is
// counter-based and a sampled hypothesis has the same bits in a batch of any size, so the result does not depend on the chunk size.
#pragma once
#include "blocks_kernel.h"

namespace tff {

constexpr long ROBUST_CHUNK = 262144;        // hypotheses per chunk (api.ROBUST_CHUNK)
constexpr int ROBUST_MAX_SAMPLE = 16;        // the sampler's swap list lives in registers
constexpr int ROBUST_MAX_CAND = 64;

// ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    unsigned long long z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// the hypothesis index a selection key carries (k_robust_topk); key 0 = no hypothesis: index 0, flagged invalid elsewhere
__device__ __forceinline__ long robust_key_index(unsigned long long key) { return key ? (long)(0xFFFFFFFFULL - (key & 0xFFFFFFFFULL)) : 0; }
__device__ __forceinline__ int robust_key_count(unsigned long long key) { return (int)(key >> 32) - 1; }

struct SampleArgs {
    unsigned long long seed;
    long first;                              // row b is hypothesis first + b ...
    const unsigned long long* keys;          // ... or, when non-null, the hypothesis of selection key keys[b]
    long B;
    int n, Ns;                               // 1 <= n <= ROBUST_MAX_SAMPLE, Ns >= n
    int* out;                                // B x n
};
// One thread per hypothesis: a Fisher-Yates shuffle of the virtual array 0 .. Ns-1 of which only the n swaps are kept (position, value): exactly n
// draws, no memory proportional to Ns.  Both loops are unrolled over the 16 possible entries so that the list is indexed statically (registers).
// sample_draw: the n indices of hypothesis h under `seed`, each plus `base` (the scene's first correspondence in a packed array, robust_scenes_kernel.h)
__device__ __forceinline__ void sample_draw(const unsigned long long seed, const unsigned long long h, const int n, const int Ns, const int base, int* out) {
    const unsigned long long key = splitmix64(seed ^ (h * 0xD1342543DE82EF95ULL));
    int pos[ROBUST_MAX_SAMPLE], val[ROBUST_MAX_SAMPLE];
#pragma unroll
    for (int i = 0; i < ROBUST_MAX_SAMPLE; ++i) {
        if (i < n) {
            const unsigned long long u = splitmix64(key + (unsigned long long)i) >> 32;
            const int r = i + (int)((u * (unsigned long long)(Ns - i)) >> 32);
            int vr = r, vi = i;              // the value at a position: that of the LAST swap recorded there, else the position itself
#pragma unroll
            for (int j = 0; j < i; ++j) {
                vr = (pos[j] == r) ? val[j] : vr;
                vi = (pos[j] == i) ? val[j] : vi;
            }
            out[i] = base + vr;
            pos[i] = r; val[i] = vi;
        }
    }
}
__global__ void __launch_bounds__(256) k_sample_indices(const SampleArgs a) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const unsigned long long h = a.keys ? (unsigned long long)robust_key_index(a.keys[b]) : (unsigned long long)(a.first + b);
    sample_draw(a.seed, h, a.n, a.Ns, 0, a.out + b * a.n);
}

// ---- per-correspondence inlier flags ------------------------------------------------------------------------------------------------------------
struct InlierMaskArgs {
    const double* scene;     // 6 x Ns, shared
    const double* calm;      // 27, shared: cameras K1 [I|0], K2 Rt2[b], K3 Rt3[b]
    const double* Rt2; const double* Rt3;    // B x 12 column-major poses
    long B;
    int Ns;
    double thr;
    unsigned char* mask;     // B x Ns
    int* counts;             // B or null: the row sums
    const int* gate;         // null, or one int32: the kernel does nothing unless *gate == 0 (the estimator's status)
};
// One wavefront per hypothesis, the cameras composed and pinned as in k_repr_error, the rule per correspondence that of the count kernels
// (count_if_inlier): the row sums are their counts.
__global__ void __launch_bounds__(64, 4) k_inlier_mask(const InlierMaskArgs a) {
    __shared__ double cam[3][12];
    if (a.gate && *a.gate != 0) return;
    const int lane = lane_id();
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        wave_sync();
        if (lane < 3) {
            const Mat3 K = load_K(a.calm, lane);
            double Rt[12];                                                   // row-major pose of view `lane`
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int r = e >> 2, c = e & 3;
                Rt[e] = (lane == 0) ? ((r == c) ? 1.0 : 0.0) : ((lane == 1) ? a.Rt2[b * 12 + r + 3 * c] : a.Rt3[b * 12 + r + 3 * c]);
            }
            compose_camera_from_pose(K, Rt, cam[lane]);
        }
        wave_sync();
        double P[3][12], Zt[4][4];
        load_uniform12(cam[0], P[0]);
        load_uniform12(cam[1], P[1]);
        load_uniform12(cam[2], P[2]);
        inlier_threshold_form(P, a.thr, Zt);
        unsigned char* row = a.mask + b * (long)a.Ns;
        int cnt = 0;
#pragma unroll 1
        for (int i = lane; i < a.Ns; i += WAVE) {
            int in = 0;
            count_if_inlier(P, Zt, cam[0], cam[1], cam[2], load_pt(a.scene, i), a.thr, in);
            row[i] = (unsigned char)in;
            cnt += in;
        }
        cnt = wave_sum_i(cnt);
        if (lane == 0 && a.counts) a.counts[b] = cnt;
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------------------------
struct RobustMarkArgs { int* counts; const int* status; long B; };
__global__ void __launch_bounds__(256) k_robust_mark(const RobustMarkArgs a) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < a.B && a.status[b] != 0) a.counts[b] = -1;
}

// The order of the candidates is (count descending, hypothesis index ascending) = descending key (count + 1) << 32 | (2^32 - 1 - index); keys are
// distinct, so round r takes the largest key below the one round r - 1 took and nothing has to be marked.  A key of 0 = nothing left.
// blockIdx.y is the scene (one for tff_robust_pose_*): its counts at counts + y * n_hyp, its keys at sel + y * K, the keys built from h within the scene.
struct RobustTopkArgs {
    const int* counts;       // n_hyp per scene, -1 = failed
    long n_hyp;
    unsigned long long* sel; // K keys per scene, zero on entry
    int round;
    int K;
};
constexpr int ROBUST_TOPK_THREADS = 256;
__global__ void __launch_bounds__(ROBUST_TOPK_THREADS) k_robust_topk(const RobustTopkArgs a) {
    __shared__ unsigned long long part[ROBUST_TOPK_THREADS / 64];
    const int* counts = a.counts + (long)blockIdx.y * a.n_hyp;
    unsigned long long* sel = a.sel + (long)blockIdx.y * a.K;
    const unsigned long long below = a.round ? sel[a.round - 1] : ~0ULL;
    unsigned long long best = 0;
    if (below != 0) {
        for (long h = (long)blockIdx.x * blockDim.x + threadIdx.x; h < a.n_hyp; h += (long)gridDim.x * blockDim.x) {
            const int c = counts[h];
            const unsigned long long key = ((unsigned long long)(c + 1) << 32) | (0xFFFFFFFFULL - (unsigned long long)h);
            if (c >= 0 && key < below && key > best) best = key;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < ROBUST_TOPK_THREADS / 64; ++w) best = part[w] > best ? part[w] : best;
        if (best) atomicMax(sel + a.round, best);
    }
}

// The state of the K candidates, all device-resident
struct RobustState {
    const unsigned long long* sel;   // K selection keys
    long K;
    int Ns;
    int* cnt;                // K current inlier counts, -1 = no such candidate
    int* seed_idx;           // K hypothesis indices
    int* nref;               // K refits adopted
    double* pose;            // K x 51: Rt2 (K x 12) | Rt3 (K x 12) | T (K x 27), the current poses
    int* status;             // K status of the candidates' hypotheses (recomputed with their poses)
    double* ref_pose;        // K x 51, the refits, same layout
    int* ref_status;         // K
    int* ref_cnt;            // K
    const unsigned char* mask;   // K x Ns
    const int* mask_cnt;     // K row sums
    long* offsets;           // K + 1
    const double* scene;
    double* packed;          // the refit batch
};
// runs after the candidates' hypotheses were recomputed from their keys (k_sample_indices with `keys`, the *_sampled pose kernels).  A candidate
// whose recomputed hypothesis is not a success cannot exist -- it was selected among the successes -- the test of its status is a guard
__global__ void __launch_bounds__(64) k_robust_seed(const RobustState s) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;              // (one workgroup for K <= 64; S * K candidates: robust_scenes_kernel.h)
    if (r >= s.K) return;
    const unsigned long long key = s.sel[r];
    const bool valid = key != 0 && s.status[r] == 0;
    s.cnt[r] = valid ? robust_key_count(key) : -1;
    s.seed_idx[r] = valid ? (int)robust_key_index(key) : -1;
    s.nref[r] = 0;
}
// offsets[r + 1] = offsets[r] + (inliers of candidate r, 0 where there is no candidate): K <= 64, one thread
__global__ void __launch_bounds__(64) k_robust_offsets(const RobustState s) {
    if (threadIdx.x != 0) return;
    long o = 0;
    s.offsets[0] = 0;
    for (int r = 0; r < s.K; ++r) {
        o += (s.cnt[r] >= 0) ? s.mask_cnt[r] : 0;
        s.offsets[r + 1] = o;
    }
}
// one workgroup per candidate walks the scene in tiles of 256: ballot + prefix over the four wavefronts keep the inliers in scene order
constexpr int ROBUST_COMPACT_THREADS = 256;
__global__ void __launch_bounds__(ROBUST_COMPACT_THREADS) k_robust_compact(const RobustState s) {
    __shared__ int wsum[ROBUST_COMPACT_THREADS / 64];
    const int r = (int)blockIdx.x;
    if (s.cnt[r] < 0) return;
    const unsigned char* m = s.mask + (long)r * s.Ns;
    const long end = s.offsets[r + 1];
    long base = s.offsets[r];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    for (int i0 = 0; i0 < s.Ns; i0 += ROBUST_COMPACT_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        const bool in = i < s.Ns && m[i] != 0;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ULL << lane) - 1ULL)), total = 0;
#pragma unroll
        for (int k = 0; k < ROBUST_COMPACT_THREADS / 64; ++k) { before += (k < w) ? wsum[k] : 0; total += wsum[k]; }
        const long slot = base + before;
        if (in && slot < end) {                                              // (slot < end always holds: the offsets are this mask's row sums)
            const double* q = s.scene + 6 * (long)i;
            double* d = s.packed + 6 * slot;
#pragma unroll
            for (int e = 0; e < 6; ++e) d[e] = q[e];
        }
        base += total;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(64) k_robust_adopt(const RobustState s) {
    const long r = (long)blockIdx.x;                                        // (long: S * K candidates index these arrays too, robust_scenes_kernel.h)
    const int lane = (int)threadIdx.x;
    if (s.cnt[r] < 0 || s.ref_status[r] != 0 || s.ref_cnt[r] < s.cnt[r]) return;
    const long K = s.K;
    if (lane < 12) { s.pose[r * 12 + lane] = s.ref_pose[r * 12 + lane]; s.pose[(K + r) * 12 + lane] = s.ref_pose[(K + r) * 12 + lane]; }
    if (lane < 27) s.pose[K * 24 + r * 27 + lane] = s.ref_pose[K * 24 + r * 27 + lane];
    __syncthreads();                                                         // (the count is read above by every lane before lane 0 replaces it)
    if (lane == 0) { s.cnt[r] = s.ref_cnt[r]; s.nref[r] += 1; }
}
struct RobustFinishArgs {
    RobustState s;
    double* Rt2; double* Rt3; double* T;     // 12, 12, 27
    int* info;               // 4
    int* status;             // 1
};
__global__ void __launch_bounds__(64) k_robust_finish(const RobustFinishArgs a) {
    const int lane = (int)threadIdx.x, K = (int)a.s.K;
    int win = -1, best = -1, ncand = 0;
    for (int r = 0; r < K; ++r) {
        const int c = a.s.cnt[r];
        if (c >= 0) ++ncand;
        if (c > best) { best = c; win = r; }
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (lane < 12) {
        a.Rt2[lane] = win >= 0 ? a.s.pose[win * 12 + lane] : qnan;
        a.Rt3[lane] = win >= 0 ? a.s.pose[(K + win) * 12 + lane] : qnan;
    }
    if (lane < 27) a.T[lane] = win >= 0 ? a.s.pose[K * 24 + win * 27 + lane] : qnan;
    if (lane == 0) {
        a.info[0] = win >= 0 ? best : 0;
        a.info[1] = win >= 0 ? a.s.seed_idx[win] : -1;
        a.info[2] = win >= 0 ? a.s.nref[win] : 0;
        a.info[3] = ncand;
        a.status[0] = win >= 0 ? ST_OK : ST_NO_POSE;
    }
}

}  // namespace tff
