// Quality-guided (PROSAC, Chum & Matas 2005) sampling for the robust estimators (tff_robust_pose_scenes_guided_*, tff_sample_indices_guided_dev;
// the definition is in include/tftfund_guided.h, the numpy twins are api.guided_pool_ends and api.sample_indices_guided_reference).  Hypothesis h of a
// scene draws from the n best-ranked correspondences, n growing with h alone, so the sampler stays counter-based: a sample is a function of
// (seed, h, m, N, growth, the scene's ranking) and every bitwise contract of the robust calls holds as it does for the uniform sampler.
//
//   k_guided_ends            per scene the table ends[m .. N]: hypothesis t = h + 1 draws from the smallest pool n with ends[n] >= t
//   k_scenes_sample_guided   scenes_sample_row, k_scenes_sample's body, with the guided draw: rows of a chunk or round, or the re-draw of the candidates from their keys
//   k_sample_indices_guided  the one-scene building block
//
// The table is packed like the scenes: slot offsets[s] + n - 1 holds ends[n] of scene s (slots below m - 1 hold 0), n_total int32 in all.
#pragma once
#include "robust_scenes_kernel.h"

namespace tff {

constexpr long GUIDED_MAX_GROWTH = (1L << 31) - (1L << 25);   // ends[N] <= growth + N stays an int32 for N <= 2^24 (api.GUIDED_MAX_GROWTH)
constexpr int GUIDED_ENDS_THREADS = 256;

// T(n) = growth * C(n, m) / C(N, m), each n on its own: multiply, then divide, m times -- nothing here can be contracted into an FMA
__device__ __forceinline__ double guided_T(const long growth, const int n, const int N, const int m) {
    double T = (double)growth;
    for (int i = 0; i < m; ++i) {
        T = T * (double)(n - i);
        T = T / (double)(N - i);
    }
    return T;
}
// ends[n] - ends[n - 1] for n = 1 .. N, with ends[n] = 0 below m and ends[m] = 1
__device__ __forceinline__ int guided_step(const long growth, const int n, const int N, const int m) {
    if (n < m) return 0;
    if (n == m) return 1;
    return (int)ceil(guided_T(growth, n, N, m) - guided_T(growth, n - 1, N, m));
}

struct GuidedEndsArgs {
    SceneSet q;              // n_min = m: a scene with fewer correspondences has no table (nothing is written for an invalid scene)
    long growth;             // 1 .. GUIDED_MAX_GROWTH
    int m;                   // the sample size
    int* ends;               // n_total
};
// one workgroup per scene, tile by tile: the steps elementwise, an inclusive scan of each wavefront's 64 steps by shuffles, the four wavefronts' sums
// through LDS (two barriers per tile), the running sum carried to the next tile
__global__ void __launch_bounds__(GUIDED_ENDS_THREADS) k_guided_ends(const GuidedEndsArgs a) {
    __shared__ int wsum[GUIDED_ENDS_THREADS / 64];
    const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
    for (long s = blockIdx.x; s < a.q.S; s += gridDim.x) {
        long o; int N;
        if (scene_range(a.q, s, &o, &N) != ST_OK) continue;                  // (the same decision in every thread of the workgroup)
        int carry = 0;
        for (int j0 = 0; j0 < N; j0 += GUIDED_ENDS_THREADS) {
            const int j = j0 + t;                                            // slot j holds ends[j + 1]
            const int step = j < N ? guided_step(a.growth, j + 1, N, a.m) : 0;
            int v = step;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {                               // inclusive scan within the wavefront
                const int u = __shfl_up(v, (unsigned)d, 64);
                v += lane >= d ? u : 0;
            }
            __syncthreads();                                                 // (the previous tile's readers of wsum are done)
            if (lane == 63) wsum[w] = v;
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int k = 0; k < GUIDED_ENDS_THREADS / 64; ++k) { before += k < w ? wsum[k] : 0; total += wsum[k]; }
            if (j < N) a.ends[o + j] = carry + before + v;
            carry += total;
        }
    }
}

// The m indices of hypothesis h of a scene of N correspondences whose table is `ends` and whose ranking is `order` (both the scene's own N entries),
// each plus `base`; a row of -1 when a drawn entry of `order` lies outside [0, N).  With a pool n: the m - 1 ranks of sample_draw(seed, h, m - 1, n - 1),
// then rank n - 1; beyond ends[N]: sample_draw(seed, h, m, N), the uniform sampler's ranks.  The ranks live in registers (both loops are unrolled).
__device__ __forceinline__ void guided_draw(const unsigned long long seed, const unsigned long long h, const int m, const int N, const int* ends,
                                            const int* order, const int base, int* out) {
    const unsigned long long t = h + 1ULL;
    int rk[ROBUST_MAX_SAMPLE];
    if (t > (unsigned long long)ends[N - 1]) {
        sample_draw(seed, h, m, N, 0, rk);
    } else {
        int lo = m, hi = N;                                                  // ends[hi] >= t; the smallest such n in [m, N]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned long long)ends[mid - 1] >= t) hi = mid;
            else lo = mid + 1;
        }
        sample_draw(seed, h, m - 1, lo - 1, 0, rk);
#pragma unroll
        for (int i = 0; i < ROBUST_MAX_SAMPLE; ++i) {
            if (i == m - 1) rk[i] = lo - 1;
        }
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < ROBUST_MAX_SAMPLE; ++i) {
        if (i < m) {
            const int v = order[rk[i]];                                      // (a rank lies in [0, N): an address inside the scene's ranking)
            ok = ok && v >= 0 && v < N;
            rk[i] = v;
        }
    }
#pragma unroll
    for (int i = 0; i < ROBUST_MAX_SAMPLE; ++i) {
        if (i < m) out[i] = ok ? base + rk[i] : -1;
    }
}

struct ScenesSampleGuidedArgs {
    ScenesSampleArgs a;      // what k_scenes_sample is given
    const int* ends;         // n_total: k_guided_ends's table
    const int* order;        // n_total: per scene its ranking, best first, as local indices
};
__global__ void __launch_bounds__(256) k_scenes_sample_guided(const ScenesSampleGuidedArgs ga) {
    scenes_sample_row(ga.a, [&](unsigned long long seed, unsigned long long h, int ns, long o, int* out) {
        guided_draw(seed, h, ga.a.n, ns, ga.ends + o, ga.order + o, (int)o, out);
    });
}

struct SampleGuidedArgs {
    SampleArgs a;            // what k_sample_indices is given
    const int* ends;         // Ns: the one scene's table
    const int* order;        // Ns
};
__global__ void __launch_bounds__(256) k_sample_indices_guided(const SampleGuidedArgs ga) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= ga.a.B) return;
    guided_draw(ga.a.seed, (unsigned long long)(ga.a.first + b), ga.a.n, ga.a.Ns, ga.ends, ga.order, 0, ga.a.out + b * ga.a.n);
}

}  // namespace tff
