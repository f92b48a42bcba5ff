// Ragged, masked BundleAdjustment (tff_bundle_adjust_ragged_*): the plan that hands the items of a packed batch -- each with its own number of
// correspondences, optionally thinned by an inlier mask -- to k_bundle_adjust (ba_kernel.h), whose per-item body is not touched.
//
// k_bundle_adjust needs ba_lds_bytes(0) + 48 N bytes of LDS and runs one wavefront per SIMD (256 VGPRs + 202 AGPRs), four per CU.  Up to 40 KiB
// of LDS per item therefore cost no occupancy, up to 80 KiB leave two wavefronts per CU, up to 160 KiB one.  A launch sized for the largest item
// would make every item pay for it, so the items go to three CLASSES by their count m, class c = the smallest with m <= bound[c], and each class
// gets a launch with its own LDS size.  The chain, all on one stream, nothing read by the host:
//
//   k_ba_ragged_count      per item: validate the offsets, m = popcount of its mask range (or n), `used`, the failure statuses with their NaN outputs
//   k_ba_ragged_scan       (mask only) compact offsets of the selected correspondences: a one-workgroup scan, as k_ragged_scan / k_scenes_offsets
//   k_ba_ragged_classes    append every valid item to the list of its class (one atomic per item; the order within a list is free: no output depends on it)
//   k_ba_ragged_compact    (mask only) the selected correspondences, their reconst0 triples and their source indices, in scene order (ballot + prefix)
//   k_bundle_adjust x 3    one launch per class; a block whose slot lies beyond the class's device-side count exits before touching anything
//   k_ba_ragged_scatter    reconst back to the original positions, NaN at the unselected ones and over the range of an item that failed
//
// The bounds are kernel arguments (the emulator test passes tiny ones).  No kernel uses an offset as an address before checking it against n_total.
#pragma once
#include "ba_kernel.h"
#include "ragged_kernel.h"

namespace tff {

constexpr int ST_TOO_LARGE = 7;              // include/tftfund.h TFF_ST_TOO_LARGE
constexpr int BA_CLASSES = 3;
constexpr int BA_RAGGED_SCAN_THREADS = 1024;
constexpr int BA_RAGGED_TILE = 256;          // threads of the compaction and scatter workgroups

// largest N whose ba_lds_bytes(N) fits `bytes` (0 if none does)
constexpr int ba_max_n_for(size_t bytes) { return bytes < ba_lds_bytes(0) ? 0 : (int)((bytes - ba_lds_bytes(0)) / (6 * sizeof(double))); }
constexpr int BA_CLASS_BOUND_0 = ba_max_n_for(40 * 1024), BA_CLASS_BOUND_1 = ba_max_n_for(80 * 1024), BA_CLASS_BOUND_2 = ba_max_n_for(160 * 1024);

struct BaRaggedPlan {
    const long* offsets;          // B + 1, on the device; item b owns [offsets[b], offsets[b + 1]) of the packed arrays
    long B;
    long n_total;                 // every offset must lie in [0, n_total]
    const unsigned char* mask;    // n_total flags or null (every correspondence is selected)
    int bound[BA_CLASSES];        // largest m of each class; bound[2] is the largest m at all
    int* m;                       // B: selected correspondences of a valid item, 0 for an item that failed
    long* coff;                   // B: first compact slot of the item (mask only)
    int* cls_count;               // BA_CLASSES counters, zero on entry
    int* cls_list;                // BA_CLASSES x B item indices
    const double* corresp;        // packed 6 x n_total
    const double* reconst0;       // packed 3 x n_total or null
    double* packed;               // (mask only) compact copies: 6 x n_total, ...
    double* rec0;                 //   ... 3 x n_total (when reconst0), ...
    int* src;                     //   ... and the index within its item of each compact slot
    const double* rec_ws;         // (mask only) k_bundle_adjust's points in compact order, 3 x n_total
    double* Rt2; double* Rt3;     // outputs, as tff_bundle_adjust_batch_dev
    double* reconst;              // packed 3 x n_total or null
    int* iter; double* repr_err;  // may be null
    int* used;                    // may be null
    int* status;                  // never null here (the launcher borrows the context's scratch array)
};

__device__ __forceinline__ bool ba_ragged_range(const BaRaggedPlan& a, const long b, long* o0, long* o1) {
    *o0 = a.offsets[b]; *o1 = a.offsets[b + 1];
    return *o0 >= 0 && *o1 >= *o0 && *o1 <= a.n_total;
}
// one thread: the outputs of an item that does not reach the solver
__device__ inline void ba_ragged_fail(const BaRaggedPlan& a, const long b, const int st) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int e = 0; e < 12; ++e) { a.Rt2[b * 12 + e] = qnan; a.Rt3[b * 12 + e] = qnan; }
    if (a.repr_err) a.repr_err[b] = qnan;
    if (a.iter) a.iter[b] = 0;
    if (a.used) a.used[b] = 0;
    a.m[b] = 0;
    a.status[b] = st;
}

// one wavefront per item
__global__ void __launch_bounds__(64) k_ba_ragged_count(const BaRaggedPlan a) {
    const int lane = lane_id();
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        long o0, o1;
        int st = ST_OK, m = 0;
        if (!ba_ragged_range(a, b, &o0, &o1)) {
            st = ST_BAD_OFFSETS;
        } else {
            if (a.mask) {
                int c = 0;
                for (long i = o0 + lane; i < o1; i += WAVE) c += a.mask[i] != 0;
                m = wave_sum_i(c);
            } else {
                m = (int)(o1 - o0);                                          // (n_total < 2^31)
            }
            if (m == 0) st = ST_TOO_FEW;
            else if (m > a.bound[BA_CLASSES - 1]) st = ST_TOO_LARGE;
        }
        if (lane == 0) {
            if (st != ST_OK) ba_ragged_fail(a, b, st);
            else { a.m[b] = m; if (a.used) a.used[b] = m; }
        }
    }
}

// coff[b] = the selected correspondences of the valid items before b: one workgroup, thread t owns a run of items, the runs' sums scanned in LDS.
// Ranges that overlap -- only malformed offsets make them -- can select more than n_total correspondences in all: an item whose compact range
// would end beyond n_total is ST_BAD_OFFSETS, so that the compact arrays are never overrun.
__global__ void __launch_bounds__(BA_RAGGED_SCAN_THREADS) k_ba_ragged_scan(const BaRaggedPlan a) {
    __shared__ long part[BA_RAGGED_SCAN_THREADS];
    const int t = (int)threadIdx.x;
    const long run = (a.B + BA_RAGGED_SCAN_THREADS - 1) / BA_RAGGED_SCAN_THREADS;
    const long lo = t * run < a.B ? t * run : a.B, hi = lo + run < a.B ? lo + run : a.B;
    long sum = 0;
    for (long r = lo; r < hi; ++r) sum += a.m[r];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < BA_RAGGED_SCAN_THREADS; d <<= 1) {                   // Hillis-Steele inclusive scan
        const long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long o = part[t] - sum;                                                  // exclusive prefix of this thread's run
    for (long r = lo; r < hi; ++r) {
        const int m = a.m[r];
        a.coff[r] = o;
        o += m;
        if (m > 0 && o > a.n_total) ba_ragged_fail(a, r, ST_BAD_OFFSETS);
    }
}

__global__ void __launch_bounds__(256) k_ba_ragged_classes(const BaRaggedPlan a) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const int m = a.m[b];
    if (m <= 0) return;
    const int c = m <= a.bound[0] ? 0 : (m <= a.bound[1] ? 1 : 2);
    a.cls_list[c * a.B + atomicAdd(a.cls_count + c, 1)] = (int)b;
}

// one workgroup per item walks its range in tiles of BA_RAGGED_TILE, as k_scenes_compact
__global__ void __launch_bounds__(BA_RAGGED_TILE) k_ba_ragged_compact(const BaRaggedPlan a) {
    __shared__ int wsum[BA_RAGGED_TILE / 64];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const int m = a.m[b];
        long o0, o1;
        if (m <= 0 || !ba_ragged_range(a, b, &o0, &o1)) continue;            // (a valid item has a valid range: a guard)
        long base = a.coff[b];
        const long end = base + m;
        for (long i0 = 0; i0 < o1 - o0; i0 += BA_RAGGED_TILE) {
            const long i = i0 + (long)threadIdx.x;
            const bool in = i < o1 - o0 && a.mask[o0 + i] != 0;
            const unsigned long long bal = __ballot(in);
            if (lane == 0) wsum[w] = __popcll(bal);
            __syncthreads();
            int before = __popcll(bal & ((1ULL << lane) - 1ULL)), total = 0;
#pragma unroll
            for (int k = 0; k < BA_RAGGED_TILE / 64; ++k) { before += (k < w) ? wsum[k] : 0; total += wsum[k]; }
            const long slot = base + before;
            if (in && slot < end) {                                          // (slot < end always holds: m is this range's popcount)
                const double* q = a.corresp + 6 * (o0 + i);
                double* d = a.packed + 6 * slot;
#pragma unroll
                for (int e = 0; e < 6; ++e) d[e] = q[e];
                if (a.reconst0) for (int e = 0; e < 3; ++e) a.rec0[3 * slot + e] = a.reconst0[3 * (o0 + i) + e];
                a.src[slot] = (int)i;
            }
            base += total;
            __syncthreads();
        }
    }
}

// one workgroup per item; launched only when the call has a `reconst`
__global__ void __launch_bounds__(BA_RAGGED_TILE) k_ba_ragged_scatter(const BaRaggedPlan a) {
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        long o0, o1;
        if (!ba_ragged_range(a, b, &o0, &o1)) continue;                      // ST_BAD_OFFSETS: the item's range is not defined
        const int m = a.m[b];
        if (m <= 0) {                                                        // the item failed: NaN over its range, unless the scan found it overlapping
            if (a.status[b] == ST_BAD_OFFSETS) continue;
            for (long e = 3 * o0 + (long)threadIdx.x; e < 3 * o1; e += BA_RAGGED_TILE) a.reconst[e] = qnan;
            continue;
        }
        if (!a.mask) continue;                                               // k_bundle_adjust wrote the caller's array itself
        for (long i = o0 + (long)threadIdx.x; i < o1; i += BA_RAGGED_TILE)
            if (a.mask[i] == 0) { a.reconst[3 * i] = qnan; a.reconst[3 * i + 1] = qnan; a.reconst[3 * i + 2] = qnan; }
        const long c0 = a.coff[b];
        for (long k = (long)threadIdx.x; k < m; k += BA_RAGGED_TILE) {
            const long i = o0 + a.src[c0 + k];
#pragma unroll
            for (int e = 0; e < 3; ++e) a.reconst[3 * i + e] = a.rec_ws[3 * (c0 + k) + e];
        }
    }
}

// the arguments of k_bundle_adjust for class c of a plan
inline BaArgs ba_ragged_class_args(const BaRaggedPlan& p, const double* calm, long calm_stride, const double* Rt2_in, const double* Rt3_in, double* rec_ws, int c) {
    BaArgs a{calm, calm_stride, Rt2_in, Rt3_in, p.mask ? p.packed : p.corresp, p.B, 0, p.mask ? (p.reconst0 ? p.rec0 : nullptr) : p.reconst0,
             p.Rt2, p.Rt3, p.reconst ? (p.mask ? rec_ws : p.reconst) : nullptr, p.iter, p.repr_err, p.status};
    a.items = p.cls_list + (long)c * p.B;
    a.count = p.cls_count + c;
    a.item_n = p.m;
    a.item_off = p.mask ? p.coff : p.offsets;
    return a;
}

}  // namespace tff
