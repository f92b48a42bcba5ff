// The `weight` output of tff_bundle_adjust_loss_*: what surrounds k_bundle_adjust_loss<LOSS> (ba_kernel.h), which writes w_i at the final parameters of
// every item it solves -- to the caller's array, or, under a mask, to a compact workspace next to the compact correspondences.
//
//   k_ba_weight_ones       fixed N, TFF_LOSS_NONE: the plain kernel ran and knows no weights; 1 everywhere, NaN over an item whose status is not 0
//   k_ba_ragged_weight     ragged: NaN over an item that failed and at the positions a mask deselects; the compact weights back to their
//                          positions (mask), or 1 at the selected positions (TFF_LOSS_NONE)
//
// Like k_ba_ragged_scatter, neither uses an offset as an address before checking it against n_total.
#pragma once
#include "ba_ragged_kernel.h"

namespace tff {

struct BaOnesArgs { double* weight; const int* status; long B; int N; };   // status may be null
__global__ void __launch_bounds__(256) k_ba_weight_ones(const BaOnesArgs a) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const long total = a.B * (long)a.N;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
        a.weight[e] = (a.status && a.status[e / a.N] != ST_OK) ? qnan : 1.0;
}

struct BaRaggedWeights {
    BaRaggedPlan plan;
    const double* w_ws;           // (mask only) k_bundle_adjust_loss's weights in compact order, n_total
    double* weight;               // packed n_total
    int ones;                     // TFF_LOSS_NONE: no kernel wrote a weight
};

// one workgroup per item
__global__ void __launch_bounds__(BA_RAGGED_TILE) k_ba_ragged_weight(const BaRaggedWeights q) {
    const BaRaggedPlan& a = q.plan;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        long o0, o1;
        if (!ba_ragged_range(a, b, &o0, &o1)) continue;                      // ST_BAD_OFFSETS: the item's range is not defined
        const int m = a.m[b];
        if (m <= 0) {                                                        // the item failed: NaN over its range, unless the scan found it overlapping
            if (a.status[b] == ST_BAD_OFFSETS) continue;
            for (long i = o0 + (long)threadIdx.x; i < o1; i += BA_RAGGED_TILE) q.weight[i] = qnan;
            continue;
        }
        const double one = (a.status[b] == ST_OK) ? 1.0 : qnan;
        if (!a.mask) {                                                       // with a loss, k_bundle_adjust_loss wrote the caller's array itself
            if (q.ones) for (long i = o0 + (long)threadIdx.x; i < o1; i += BA_RAGGED_TILE) q.weight[i] = one;
            continue;
        }
        for (long i = o0 + (long)threadIdx.x; i < o1; i += BA_RAGGED_TILE)
            if (a.mask[i] == 0) q.weight[i] = qnan;
        const long c0 = a.coff[b];
        for (long k = (long)threadIdx.x; k < m; k += BA_RAGGED_TILE) q.weight[o0 + a.src[c0 + k]] = q.ones ? one : q.w_ws[c0 + k];
    }
}

// the arguments of k_bundle_adjust_loss for class c of a plan: those of k_bundle_adjust, the scale, and where the weights go
inline BaLossArgs ba_ragged_class_loss_args(const BaRaggedPlan& p, const double* calm, long calm_stride, const double* Rt2_in, const double* Rt3_in, double* rec_ws, int c,
                                            double scale, double* w_ws, double* weight) {
    BaLossArgs a;
    static_cast<BaArgs&>(a) = ba_ragged_class_args(p, calm, calm_stride, Rt2_in, Rt3_in, rec_ws, c);
    a.scale = scale;
    a.weight = weight ? (p.mask ? w_ws : weight) : nullptr;
    return a;
}

}  // namespace tff
