// Ragged batches: the plan that hands a packed batch of triplets with different correspondence counts to the row kernels.
//
// The row kernels run four triplets per wavefront with one wave-uniform N (loop trip counts, the N < 7 branch, the exact tiers' ladders).
// The plan therefore buckets the items by their exact n, a counting sort on the device: k_ragged_count validates each item and counts the
// buckets, k_ragged_scan lays the buckets out in ascending n with every bucket padded to a multiple of four slots, k_ragged_scatter
// writes the item indices.  A wavefront's four slots then hold triplets of one n, so every row of it does exactly what the fixed-N kernel
// does for that n: the same instructions, the same bits (a padding slot, -1, repeats the slot's first triplet and stores nothing, as the tail
// row of a fixed-N batch repeats the last one).  The cost is at most three idle rows per distinct n.
//
// Routes: items with n < split go to the exact tiers (the fixed-N launcher's `N < exact_below || TFF_OPT_SOLVER = 1`), the others to the
// fast tiers; both are contiguous ranges of the slot list because it is sorted by n: route[0 .. 1] = [0, mid), route[2 .. 3] = [mid, total).
// Everything stays on the device: the counts are never read by the host, the kernels that consume the list stop at the end of their range.
//
// OptimFPoseEstimation (optimf_rows_kernel.h) has two additions.  Its refinement runs in up to three launch classes by n (observations staged in
// LDS | xi in LDS | xi in global slices): with cut[0] <= cut[1] set the scan also writes the three ranges [mid, c0), [c0, c1), [c1, total) to
// route[4 .. 9], c_i being the first slot of bucket cut[i].  And its exact tiers have no row kernel: with retry_count set the scatter marks every
// item with n < split ST_RETRY and appends it to the retry list (where the call has one), which the one-triplet exact kernel walks at the end of the chain.
#pragma once
#include "tft_kernel.h"

namespace tff {

constexpr int ST_BAD_OFFSETS = 6;            // include/tftfund.h TFF_ST_BAD_OFFSETS
constexpr int RAGGED_SCAN_THREADS = 1024;

struct RaggedPlanArgs {
    const long* offsets;  // B + 1
    long B;
    int n_max;            // every valid n_b is <= n_max; buckets 0 .. n_max
    int split;            // n < split: route 0 (exact tiers)
    int* hist;            // n_max + 1 bucket counts (zero on entry)
    int* fill;            // n_max + 1 fill cursors (zero on entry)
    int* start;           // n_max + 1 first slot of each bucket
    int* route;           // 4: [0, mid), [mid, total)
    int* list;            // total slots (<= B + 3 min(B, n_max + 1))
    double* Rt2;          // outputs of a malformed item: NaN, status ST_BAD_OFFSETS
    double* Rt3;
    double* T;
    int* iter;
    int* status;
    int cut[2];           // cut[1] > 0: the refinement classes of OptimF, split <= cut[0] <= cut[1]; route then has RAGGED_ROUTE_INTS entries
    int* retry_list;      // retry_count non-null: items with n < split get status ST_RETRY and, where the call has a list, an entry of it
    int* retry_count;
};
constexpr int RAGGED_ROUTE_INTS = 10;        // route: [0, mid) | [mid, total) | with cut: [mid, c0) | [c0, c1) | [c1, total)

// the slot count the plan can need: every bucket adds at most three padding slots
inline long ragged_slots(long B, int n_max) { const long k = (long)n_max + 1; return B + 3 * (B < k ? B : k); }

__device__ __forceinline__ bool ragged_item(const RaggedPlanArgs& a, const long b, int* n) {
    const long o0 = a.offsets[b], o1 = a.offsets[b + 1];
    *n = (int)(o1 - o0);
    return o0 >= 0 && o1 >= o0 && o1 - o0 <= (long)a.n_max;
}

__global__ void __launch_bounds__(256) k_ragged_count(const RaggedPlanArgs a) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int n;
    if (ragged_item(a, b, &n)) {
        atomicAdd(a.hist + n, 1);
        return;
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);   // only this item's pose outputs (its Reconst range is not defined)
    for (int e = 0; e < 12; ++e) { a.Rt2[b * 12 + e] = qnan; a.Rt3[b * 12 + e] = qnan; }
    for (int e = 0; e < 27; ++e) a.T[b * 27 + e] = qnan;
    if (a.iter) a.iter[b] = 0;
    a.status[b] = ST_BAD_OFFSETS;
}

// one workgroup: thread t owns the buckets [t * chunk, (t + 1) * chunk); exclusive scan of the padded counts over the threads in LDS
__global__ void __launch_bounds__(RAGGED_SCAN_THREADS) k_ragged_scan(const RaggedPlanArgs a) {
    __shared__ int part[RAGGED_SCAN_THREADS];
    const int t = (int)threadIdx.x;
    const int nb = a.n_max + 1;
    const int chunk = (nb + RAGGED_SCAN_THREADS - 1) / RAGGED_SCAN_THREADS;
    const int lo = t * chunk < nb ? t * chunk : nb, hi = lo + chunk < nb ? lo + chunk : nb;
    int sum = 0;
    for (int k = lo; k < hi; ++k) sum += (a.hist[k] + 3) & ~3;
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < RAGGED_SCAN_THREADS; d <<= 1) {          // Hillis-Steele inclusive scan
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int s = part[t] - sum;                                        // exclusive prefix of this thread's buckets
    for (int k = lo; k < hi; ++k) {
        const int c = a.hist[k], padded = (c + 3) & ~3;
        if (k == a.split) { a.route[1] = s; a.route[2] = s; if (a.cut[1] > 0) a.route[4] = s; }
        if (a.cut[1] > 0) {
            if (k == a.cut[0]) { a.route[5] = s; a.route[6] = s; }
            if (k == a.cut[1]) { a.route[7] = s; a.route[8] = s; }
        }
        a.start[k] = s;
        for (int q = c; q < padded; ++q) a.list[s + q] = -1;       // padding slots
        s += padded;
    }
    if (t == RAGGED_SCAN_THREADS - 1) {
        const int total = part[t];
        a.route[0] = 0;
        a.route[3] = total;
        if (a.split > a.n_max) { a.route[1] = total; a.route[2] = total; }
        if (a.split <= 0) { a.route[1] = 0; a.route[2] = 0; }
        if (a.cut[1] > 0) {                                       // (0 <= split <= cut[0] <= cut[1]: a cut of 0 is bucket 0, written above)
            if (a.split > a.n_max) a.route[4] = total;
            if (a.cut[0] > a.n_max) { a.route[5] = total; a.route[6] = total; }
            if (a.cut[1] > a.n_max) { a.route[7] = total; a.route[8] = total; }
            a.route[9] = total;
        }
    }
}

__global__ void __launch_bounds__(256) k_ragged_scatter(const RaggedPlanArgs a) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    int n;
    if (!ragged_item(a, b, &n)) return;
    a.list[a.start[n] + atomicAdd(a.fill + n, 1)] = (int)b;
    if (a.retry_count && n < a.split) {                           // the first write of this item's status: no staged kernel walks its slot
        a.status[b] = ST_RETRY;
        if (a.retry_list) a.retry_list[atomicAdd(a.retry_count, 1)] = (int)b;   // (no list from B = 2^28 on: the exact kernel scans the statuses)
    }
}

}  // namespace tff
