// Robust three-view pose estimation, the pieces that know nothing of scenes (tff_sample_indices_dev, tff_inlier_mask_batch_dev and the selection of
// tff_robust_pose_*): RANSAC over minimal samples with local optimisation of the K best hypotheses.  The estimator itself is ONE chain of launches for
// S scenes (robust_scenes_kernel.h); tff_robust_pose_* is its S = 1 form.  The hypotheses, their inlier counts and the refits come from the existing
// kernels (the *_sampled route of the pose kernels, k_inlier_count_scenes -- for the hypotheses of tff_robust_pose_dev the one-scene count kernels of
// blocks_kernel.h, same integers -- and the ragged chain); this file holds:
//
//   k_sample_indices   n distinct indices per hypothesis, a function of (seed, hypothesis index, n, Ns) alone (counter-based): tff_sample_indices_dev
//   k_inlier_mask      the inlier rule of k_repr_error per correspondence, written out as 0 / 1 flags (+ the row sums): tff_inlier_mask_batch_dev
//   k_robust_mark      a failed hypothesis (status != 0) gets the count -1: it is never a candidate
//   k_robust_topk      one round of the top-K selection: the largest packed key (count, index) below the previous round's
//   k_robust_seed      the K keys -> candidate counts, hypothesis indices, validity
//   k_robust_adopt     a candidate takes its refit iff that succeeded and has at least as many inliers
//
// The two public kernels are the definition the estimator is pinned against (tests/test_gpu_robust.py): sample_draw and count_if_inlier are what the
// chain's own k_scenes_sample and k_scenes_mask call.
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
    long first;                              // row b is hypothesis first + b
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
    sample_draw(a.seed, (unsigned long long)(a.first + b), a.n, a.Ns, 0, a.out + b * a.n);
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
};
// One wavefront per hypothesis, the cameras composed and pinned as in k_repr_error, the rule per correspondence that of the count kernels
// (count_if_inlier): the row sums are their counts.
__global__ void __launch_bounds__(64, 4) k_inlier_mask(const InlierMaskArgs a) {
    __shared__ double cam[3][12];
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
// blockIdx.y is the scene: its counts at counts + y * n_hyp, its keys at sel + y * K, the keys built from h within the scene.
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

// The state of the K candidates (K per scene x S scenes, robust_scenes_kernel.h::ScenesState), all device-resident
struct RobustState {
    const unsigned long long* sel;   // K selection keys
    long K;
    int* cnt;                // K current inlier counts, -1 = no such candidate
    int* seed_idx;           // K hypothesis indices
    int* nref;               // K refits adopted
    double* pose;            // K x 51: Rt2 (K x 12) | Rt3 (K x 12) | T (K x 27), the current poses
    int* status;             // K status of the candidates' hypotheses (recomputed with their poses)
    double* ref_pose;        // K x 51, the refits, same layout
    int* ref_status;         // K
    int* ref_cnt;            // K
    const unsigned char* mask;   // the candidates' inlier flags, packed per scene (ScenesMaskArgs)
    const int* mask_cnt;     // K row sums
    long* offsets;           // K + 1
    double* packed;          // the refit batch
};
// runs after the candidates' hypotheses were recomputed from their keys (k_scenes_sample with `keys`, the *_sampled pose kernels).  A candidate
// whose recomputed hypothesis is not a success cannot exist -- it was selected among the successes -- the test of its status is a guard
__global__ void __launch_bounds__(64) k_robust_seed(const RobustState s) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= s.K) return;
    const unsigned long long key = s.sel[r];
    const bool valid = key != 0 && s.status[r] == 0;
    s.cnt[r] = valid ? robust_key_count(key) : -1;
    s.seed_idx[r] = valid ? (int)robust_key_index(key) : -1;
    s.nref[r] = 0;
}
__global__ void __launch_bounds__(64) k_robust_adopt(const RobustState s) {
    const long r = (long)blockIdx.x;                                        // (long: S * K candidates index these arrays)
    const int lane = (int)threadIdx.x;
    if (s.cnt[r] < 0 || s.ref_status[r] != 0 || s.ref_cnt[r] < s.cnt[r]) return;
    const long K = s.K;
    if (lane < 12) { s.pose[r * 12 + lane] = s.ref_pose[r * 12 + lane]; s.pose[(K + r) * 12 + lane] = s.ref_pose[(K + r) * 12 + lane]; }
    if (lane < 27) s.pose[K * 24 + r * 27 + lane] = s.ref_pose[K * 24 + r * 27 + lane];
    __syncthreads();                                                         // (the count is read above by every lane before lane 0 replaces it)
    if (lane == 0) { s.cnt[r] = s.ref_cnt[r]; s.nref[r] += 1; }
}

}  // namespace tff
