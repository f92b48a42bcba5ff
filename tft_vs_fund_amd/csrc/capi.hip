// C ABI of libtftfund.so (see include/tftfund.h).  gfx950 only; there is no
// CPU path behind these entry points: without a HIP device they fail loudly.
//
// Layout of the host layer: an entry point checks its arguments, takes the context's lock ONCE (TFF_ENTER) and runs the shared prologue
// (run_batch); the launchers below it assume the lock is held, read the options under it and never call an entry point.  A pose call travels
// as one PoseCall record; METHODS maps a TFF_METHOD_* id to its launcher; pose_dev / pose_host are the entry of the stamped-out pose wrappers
// and of the multi-GPU shards.
#include <hip/hip_runtime.h>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include <cstdio>
#include <climits>
#include <cstring>
#include <cmath>
#include "../../include/tftfund.h"
#include "launch.h"
#include "ragged_kernel.h"
#include "robust_kernel.h"
#include "robust_scenes_kernel.h"
#include "robust_guided_kernel.h"
#include "robust_layout.h"
#include "ba_ragged_kernel.h"
#include "ba_loss_kernel.h"
#include "ba_cov_kernel.h"
#include "ba_tracks_kernel.h"
#include "ba_tracks_loss_kernel.h"
#include "ba_tracks_cov_kernel.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* what) {
    g_err = what;
    return code;
}
int hip_fail(hipError_t e, const char* where) {
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return -(int)e;
}
// first statement of every entry point that takes a context: the lock is held until the entry point returns
#define TFF_ENTER(c)                                             \
    if (!(c)) return fail(TFF_E_INVALID, "null context");        \
    std::lock_guard<std::mutex> lk__((c)->mu)
#define TFF_HIP(call)                                    \
    do {                                                 \
        hipError_t e__ = (call);                         \
        if (e__ != hipSuccess) return hip_fail(e__, #call); \
    } while (0)
#define TFF_TRY(call)                                    \
    do {                                                 \
        if (int r__ = (call)) return r__;                \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(workspace)");
        cap = bytes;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

struct tff_ctx {
    std::mutex mu;                         // serialises the entry points of one context (its workspaces and options are shared state); taken once per call
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t handover = nullptr;         // orders work across a change of stream (tff_ctx_set_stream)
    int solver = 0;
    int exact_below = tff::EXACT_BELOW_N;   // TFF_OPT_EXACT_BELOW
    int stage = -1;
    DevBuf in, calm, out, idx, scratch_status, gh_rec, gh_topt, gh_init, spill, pre_rec, retry;
    DevBuf ragged, ragged_off;             // ragged batches: the plan (buckets, slot list), the offsets of a _host call
    DevBuf robust_hyp, robust_counts, robust_cand;   // the robust estimators, one scene or many: one chunk of hypotheses, the counts of all of them, the candidates' state (launch_robust_scenes)
    DevBuf guided_ends, guided_order;      // guided sampling: the pool tables (4 n_total bytes), the ranking of a _host call (4 n_total bytes)
    DevBuf ba_weight;                      // tff_bundle_adjust_loss_*_host: the staged weights
    DevBuf ba_plan, ba_pack, ba_host;      // tff_bundle_adjust_ragged_*: the plan (O(B)), the compact copies of a masked call (100 bytes x n_total), mask + used of a _host call
    DevBuf cov_plan, cov_pack, cov_rec, cov_io;   // tff_ba_covariance_* / tff_bundle_adjust_cov_*: the plan (O(B)), the compact copies of a masked call (124 bytes x n_total), the points of a call without `reconst`, the staging of a _host call
    DevBuf tracks_used;                    // tff_bundle_adjust_tracks_batch_host: the staged `used` (4 B bytes)
    DevBuf tracks_cov_x, tracks_cov_rec, tracks_cov_io;   // tff_ba_tracks_covariance_* / tff_bundle_adjust_tracks_cov_*: the points in the frame of camera 1 (24 B N bytes), the points of a call without `reconst`, the staging of a _host call
    DevBuf tracks_weight, tracks_status;   // tff_bundle_adjust_tracks_loss_batch_*: the staged weights of a _host call (8 B N M bytes); the statuses of a TFF_LOSS_NONE call with weights and no status output (4 B bytes)
    int kernel_variant = 0;                // TFF_OPT_KERNEL
    int gh_exact = 0;                      // TFF_OPT_GH_EXACT
    int spill_only_if_needed = 0;          // TFF_OPT_SPILL
    int rows = 2;                          // TFF_OPT_ROWS: 0 the one-triplet kernels, 1 and 2 (default) the row kernels (use_rows)
    int retry_parity = 0;                  // which of the two retry counters this call uses (retry_list_begin)
    int pre = 0;                           // TFF_OPT_PRE: 0 never (default: measured slower, see pre_for), 1 always, 2 from N >= 48
    int dbg_fp_handover = 0;               // TFF_OPT_DEBUG_FP_HANDOVER
    int dbg_adaptive = 0;                  // TFF_OPT_DEBUG_ADAPTIVE
    int count_rows = 1;                    // TFF_OPT_COUNT_ROWS: inlier counts four hypotheses per wavefront (default) or one
    int score = 0;                         // TFF_OPT_SCORE: what tff_inlier_count_* write and the robust estimators rank by, 0 the inlier count, 1 the MSAC score (blocks_kernel.h::inlier_weight)
    int ba_classes = 0;                    // TFF_OPT_BA_CLASSES: ragged bundle adjustment, 0 the plan by batch size (launch_ba_ragged), 1 one launch class, 2 three
};

namespace {

// One pose call: what the extern "C" signatures spell out, plus what only some entry points carry.  Host or device pointers, as the function says.
struct PoseCall {
    const double* corresp; const double* calm; int64_t calm_stride; int64_t B; int32_t N;
    double* Rt2; double* Rt3; double* T; double* reconst; int32_t* iter; int32_t* status; double* dbg;
    const int32_t* sample_idx = nullptr;   // *_sampled_dev: B x N indices into ONE shared scene at `corresp` ...
    int32_t sample_ns = 0;                 //   ... of sample_ns correspondences
    double* init_p = nullptr; double* init_x = nullptr;   // tff_pi_pose_batch_debug_dev
    const int64_t* offsets = nullptr;      // ragged batches: B + 1 offsets into the packed `corresp`; N is n_max
};
typedef int (*pose_launcher)(tff_ctx*, const PoseCall&);
typedef void (*pose_kernel)(const tff::LinearTftArgs);
typedef size_t (*lds_fn)(int N, int flags, bool jacobi);

int check_common(const void* corresp, const void* calm, int64_t calm_stride, int64_t B, int32_t N) {
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative batch or correspondence count");
    if (B > 0 && (!corresp || !calm)) return fail(TFF_E_INVALID, "null input pointer");
    if (calm_stride != 0 && calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
    return 0;
}

// The prologue of every batched call, after the entry point's own argument checks: an empty batch is done before the output pointers are
// looked at; the context's device becomes current; a null *status borrows the context's scratch array (the kernels hand ST_RETRY over
// through the status array; status == nullptr: the call has none).  Then body().
template <class Body>
int run_batch(tff_ctx* c, int64_t B, bool outputs, const char* null_msg, int32_t** status, Body body) {
    if (B == 0) return 0;
    if (!outputs) return fail(TFF_E_INVALID, null_msg);
    TFF_HIP(hipSetDevice(c->device));
    if (status && !*status) {
        TFF_TRY(c->scratch_status.reserve((size_t)B * sizeof(int32_t)));
        *status = (int32_t*)c->scratch_status.p;
    }
    return body();
}

constexpr size_t LDS_LIMIT = 160 * 1024;
// Every kernel launch of the library: on the context's stream, the dynamic-LDS limit raised where the request exceeds the 64 KiB a kernel gets
// unasked.  (The row kernels, k_tft_moments, k_gh_finish, k_rt_from_tft, k_linear_tft, k_linear_f<., 0> and the staged inlier count ask for an
// amount that does not grow with N and lies below that, see the static_asserts; for them the check is a no-op.)
template <class A>
int launch(tff_ctx* c, void (*kernel)(A), dim3 grid, unsigned block, size_t lds, const A& a) {
    if (lds > LDS_LIMIT) return fail(TFF_E_INVALID, "N too large for the 160 KiB LDS workspace of this method");
    if (lds > 64 * 1024) TFF_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, dim3(block), lds, c->stream, a);
    TFF_HIP(hipGetLastError());
    return 0;
}
template <class A>
int launch(tff_ctx* c, void (*kernel)(A), unsigned grid, unsigned block, size_t lds, const A& a) { return launch(c, kernel, dim3(grid), block, lds, a); }
static_assert((((tff::POSE_LDS_DOUBLES + 1) & ~1) + ((tff::JACOBI_LDS_DOUBLES + 1) & ~1)) * sizeof(double) <= 64 * 1024, "pose_lds_bytes(N, 0, .)");
static_assert((((tff::POSE_LDS_DOUBLES + 1) & ~1) + ((tff::JACOBI_F_LDS_DOUBLES + 1) & ~1)) * sizeof(double) <= 64 * 1024, "f_pose_lds_bytes(N, 0, .)");
static_assert(tff::ROW_TRIPLETS * sizeof(tff::RowLds) <= 64 * 1024 && 48 * tff::PRE_STAGE_MAX_N + 16 <= 64 * 1024, "rows_lds_bytes, moments_lds_bytes");

// Four triplets per wavefront (the row kernels) or one?  The row kernels issue ~2.5x fewer instructions per triplet, but a wavefront of theirs
// lives ~1.3x (N = 200) to 1.7x (N = 500) as long as a one-triplet wavefront, so a batch that fits the device's 2048 wavefront slots in one go
// is ~16 microseconds faster on the one-triplet kernels (tools/ab_rows_sweep.py, ms per batch, rows / one-triplet: N = 200: B = 256
// 0.075 / 0.059, 1024 0.077 / 0.079, 3072 0.085 / 0.125).  The two routes agree to 1e-14 but not bit for bit, and the iterative methods amplify
// a last-bit difference of their start, so the route must not depend on the batch: the row kernels at ANY batch size, for every method (same
// triplet, same bits, same `iter` in a batch of one or of a million, sampled or not, sharded or not) unless TFF_OPT_ROWS = 0 forces the
// one-triplet kernels.
bool use_rows(const tff_ctx* c) { return c->rows != 0; }

// The normalisations and moment sums of the trifocal row kernels as a kernel of their own (tft_moments_kernel.h: one triplet per wavefront,
// correspondences read from HBM once, three wavefronts per SIMD)?  Built and measured in round 5 (profiles/r5_ab_pre.txt, tools/ab_pre.py,
// 10 000 triplets): N = 200 one batch at a time 0.179 -> 0.173 ms, two batches in flight 0.1225 -> 0.1284 ms; slower at every other N
// (N = 100: 0.136 -> 0.139 / 0.092 -> 0.103; N = 500: 0.312 -> 0.322 / 0.204 -> 0.252).  The two passes it removes from the row kernel were
// 31 % of a wavefront's CYCLES but memory waits that the SIMD's other wavefront filled with its compute-bound middle: the path is bound by fp64
// issue, and the pre-kernel only moves ~900 instructions per triplet to a launch of its own.  Hence OFF by default (TFF_OPT_PRE = 1 enables it,
// 2 = from N >= 48); sampled hypotheses (config 4) never take it.
bool pre_for(const tff_ctx* c, const PoseCall& p) {
    if (p.sample_idx || p.N < 7) return false;
    if (c->pre != 2) return c->pre != 0;
    return p.N >= 48;
}
// launches k_tft_moments; *pre_out = the B x PRE_DOUBLES records the row kernels' <true> variants read
int launch_moments(tff_ctx* c, const PoseCall& p, const double** pre_out) {
    TFF_TRY(c->pre_rec.reserve((size_t)p.B * tff::PRE_DOUBLES * sizeof(double)));
    tff::MomentArgs m{p.corresp, (long)p.B, p.N, (double*)c->pre_rec.p};
    const bool stage = p.N <= tff::PRE_STAGE_MAX_N;
    const size_t lds = tff::moments_lds_bytes(p.N, stage);
    if (stage) TFF_TRY(launch(c, tff::k_tft_moments<true>, tff::moments_grid(p.B), 64, lds, m));
    else TFF_TRY(launch(c, tff::k_tft_moments<false>, tff::moments_grid(p.B), 64, lds, m));
    *pre_out = (const double*)c->pre_rec.p;
    return 0;
}
// a row kernel over the whole batch: krows_pre (may be null), the variant that starts from k_tft_moments' records, when pre_for() says so, else krows
template <class A>
int launch_rows(tff_ctx* c, const PoseCall& p, void (*krows_pre)(A), void (*krows)(A), A* a) {
    if (krows_pre && pre_for(c, p)) {
        TFF_TRY(launch_moments(c, p, &a->pre));
        krows = krows_pre;
    }
    const int r = launch(c, krows, tff::rows_grid(p.B), 64, tff::rows_lds_bytes(), *a);
    a->pre = nullptr;
    return r;
}

int base_flags(const tff_ctx* c, bool reconst) {
    return (reconst ? tff::FLAG_RECONST : 0) | (c->gh_exact ? tff::FLAG_GH_EXACT : 0) | (c->dbg_fp_handover ? tff::FLAG_DBG_FP_HANDOVER : 0) |
           (c->dbg_adaptive ? tff::FLAG_DBG_ADAPTIVE : 0);
}
tff::LinearTftArgs pose_args(const tff_ctx* c, const PoseCall& p) {
    return tff::LinearTftArgs{p.corresp, p.calm, (long)p.calm_stride, (long)p.B, p.N, base_flags(c, p.reconst != nullptr),
                              p.Rt2, p.Rt3, p.T, p.reconst, p.iter, p.status, p.dbg, p.sample_idx, p.init_p, p.init_x, nullptr, 0, p.sample_ns};
}

// The staging decision: `flags` with FLAG_STAGE_LDS where the kernel keeps the correspondences in LDS (TFF_OPT_STAGE_LDS; max_n: largest N the
// automatic rule stages, 0: the kernel never stages), without it where they would not fit and are re-read through L2 instead.
int staged_flags(const tff_ctx* c, int N, int flags, bool jacobi, int max_n = tff::STAGE_MAX_N_TFT) {
    if (c->stage < 0) return tff::pose_auto_flags(N, flags, jacobi, max_n);
    if (c->stage > 0) return flags | tff::FLAG_STAGE_LDS;
    return flags;
}
int staged_if_fits(const tff_ctx* c, int N, int flags, bool jacobi, lds_fn ldsfn, int max_n) {
    if (max_n) flags = staged_flags(c, N, flags, jacobi, max_n);
    if ((flags & tff::FLAG_STAGE_LDS) && ldsfn(N, flags, jacobi) > LDS_LIMIT) flags &= ~tff::FLAG_STAGE_LDS;
    return flags;
}
// ... for a pose call: gathered samples always live in LDS
int decide_staging(const tff_ctx* c, const PoseCall& p, bool jacobi, lds_fn ldsfn, int max_n, int* flags) {
    if (!p.sample_idx) { *flags = staged_if_fits(c, p.N, *flags, jacobi, ldsfn, max_n); return 0; }
    *flags |= tff::FLAG_STAGE_LDS;
    if (ldsfn(p.N, *flags, jacobi) > LDS_LIMIT) return fail(TFF_E_INVALID, "sample too large for the LDS (sampled hypotheses are gathered into LDS)");
    return 0;
}

// grid of a fix-up pass: it redoes the few triplets the pass before flagged ST_RETRY (almost always none), so it is sized to be resident in one go
constexpr long FIXUP_GRID = 1024;
unsigned fixup_grid(int64_t B, long resident = FIXUP_GRID) { return (unsigned)(B < resident ? B : resident); }

// Iterative methods at large N: when the per-correspondence state does not fit the 160 KB of LDS it goes to a global
// workspace, one slice per resident block (the kernels loop over the batch with a grid stride).  lds_full / lds_fixed: the
// kernel's LDS request with and without the per-correspondence part.  Returns the LDS bytes to launch with.
// occupancy_cap > 0 (the workgroup kernels; the cap is what their registers allow): spill also when that lets more workgroups share
// the CU's LDS -- their wave-serial steps (KKT solve, pseudo-inverse) make workgroups per CU what counts.  Measured
// (tools/bench_n_sweep.py): Ressl 2.14 -> 3.26 M/s at N = 500, Pi 1.18 -> 1.79 M/s at N = 300, never slower.
// the decision alone (no context: tff_optim_f_ragged_bounds evaluates it too)
bool spill_wanted(bool only_if_needed, size_t lds_full, size_t lds_fixed, int occupancy_cap) {
    auto per_cu = [&](size_t bytes) { const size_t k = LDS_LIMIT / (bytes + 512); return (int)(k < (size_t)occupancy_cap ? k : (size_t)occupancy_cap); };
    const bool for_occupancy = !only_if_needed && occupancy_cap > 0 && lds_fixed < lds_full && per_cu(lds_fixed) > per_cu(lds_full);
    return lds_full > LDS_LIMIT || for_occupancy;
}
// the slices: state_bytes per block + 16 doubles -- the kernels carve their per-correspondence arrays with small alignment pads (e.g. OptimF's
// v = xi + 4N + 2), so a slice of exactly state_bytes would let the tail of one block's arrays overlap the head of its neighbour's.  The grid is
// capped at the number of slices.
int spill_slices(tff_ctx* c, size_t state_bytes, unsigned* grid, double** spill, long* stride) {
    const size_t per_block = state_bytes + 16 * sizeof(double);
    size_t blocks = ((size_t)512 << 20) / per_block;
    if (blocks < 256) blocks = 256;
    if (*grid > blocks) *grid = (unsigned)blocks;
    TFF_TRY(c->spill.reserve((size_t)*grid * per_block));
    *spill = (double*)c->spill.p; *stride = (long)(per_block / sizeof(double));
    return 0;
}
int plan_spill(tff_ctx* c, size_t lds_full, size_t lds_fixed, unsigned* grid, double** spill, long* stride, size_t* lds, int occupancy_cap = 0) {
    *spill = nullptr; *stride = 0; *lds = lds_full;
    if (!spill_wanted(c->spill_only_if_needed != 0, lds_full, lds_fixed, occupancy_cap)) return 0;
    if (lds_fixed > LDS_LIMIT) return fail(TFF_E_INVALID, "LDS workspace of this method exceeds 160 KiB");
    TFF_TRY(spill_slices(c, lds_full - lds_fixed, grid, spill, stride));
    *lds = lds_fixed;
    return 0;
}

// The pair every one-triplet route is made of: the fast kernel (inverse iteration) for the whole batch, then the exact kernel (Jacobi) over
// the (rare) triplets it marked ST_RETRY.  fast = false: the exact kernel alone -- for every triplet (minimal samples, TFF_OPT_SOLVER = 1), or,
// where `a` says FLAG_ONLY_RETRY already, as the fix-up of a stage the caller has run.  plan(exact, &args, &grid, &lds) completes the arguments
// of one launch (staging, spill slices) and gives its LDS bytes; the exact kernel's is planned once the fast kernel is on the stream, the
// spill workspace being shared.
template <class A, class Plan>
int launch_fast_exact(tff_ctx* c, void (*kfast)(A), void (*kexact)(A), bool fast, A a, Plan plan) {
    size_t lds;
    if (fast) {
        A m = a;
        unsigned grid = tff::pose_grid(a.B);
        TFF_TRY(plan(false, &m, &grid, &lds));
        TFF_TRY(launch(c, kfast, grid, 64, lds, m));
        a.flags |= tff::FLAG_ONLY_RETRY;
    }
    unsigned grid = (a.flags & tff::FLAG_ONLY_RETRY) ? fixup_grid(a.B) : tff::pose_grid(a.B);
    TFF_TRY(plan(true, &a, &grid, &lds));
    return launch(c, kexact, grid, 64, lds, a);
}
bool fast_tiers(const tff_ctx* c, int32_t N) { return c->solver == 0 && N >= c->exact_below; }

// One triplet per wavefront.  stage_max_n: see staged_flags; occupancy_cap: wavefronts per CU the fast kernel's registers allow (0: the
// kernel has no per-correspondence LDS state to spill), see plan_spill.  main_done: the caller has run the fast stages (launch_optim_f).
int launch_pose(tff_ctx* c, const PoseCall& p, pose_kernel kmain, pose_kernel kjac, lds_fn ldsfn, int stage_max_n, int occupancy_cap, bool main_done = false) {
    if (p.sample_idx && !stage_max_n) return fail(TFF_E_INVALID, "sampled hypotheses are not supported by this method");
    tff::LinearTftArgs a = pose_args(c, p);
    if (main_done) a.flags |= tff::FLAG_ONLY_RETRY;
    return launch_fast_exact(c, kmain, kjac, !main_done && fast_tiers(c, p.N), a, [&](bool exact, tff::LinearTftArgs* k, unsigned* grid, size_t* lds) {
        TFF_TRY(decide_staging(c, p, exact, ldsfn, stage_max_n, &k->flags));
        return plan_spill(c, ldsfn(p.N, k->flags, exact), ldsfn(0, k->flags, exact), grid, &k->spill, &k->spill_stride, lds, exact ? 0 : occupancy_cap);
    });
}

// The triplets a row kernel flags go to the exact kernel as a compact list: [count 0 | count 1 | B indices].  The row kernel appends to the
// list itself (one atomic per flagged triplet) and zeroes the OTHER counter for the context's next call; this call's counter was zeroed
// during the previous call (both at allocation).  No scan of the status array, no launch in between.
int retry_list_reserve(tff_ctx* c, int64_t rows) {                           // (a call of many launches sizes the list once: launch_robust_scenes)
    void* before = c->retry.p;
    TFF_TRY(c->retry.reserve(((size_t)rows + 2) * sizeof(int32_t)));
    if (c->retry.p != before) { TFF_HIP(hipMemsetAsync(c->retry.p, 0, 2 * sizeof(int32_t), c->stream)); c->retry_parity = 0; }
    return 0;
}
int retry_list_begin(tff_ctx* c, tff::LinearTftArgs* a) {
    TFF_TRY(retry_list_reserve(c, a->B));
    a->retry_count = (int*)c->retry.p + c->retry_parity;
    a->retry_zero = (int*)c->retry.p + (1 - c->retry_parity);
    a->retry_list = (a->B < (1L << tff::RETRY_HINT_SHIFT)) ? (int*)c->retry.p + 2 : nullptr;   // (an entry is index | hints << 28; beyond, the exact kernel scans the status array)
    return 0;
}
// ... and the fix-up after the row kernels: one resident round of wavefronts walks the list (almost always empty; ~0.3 % of a million
// seven-point samples of an outlier-ridden scene, config 4), one triplet per wavefront and round
int launch_retry_fixup(tff_ctx* c, pose_kernel kexact, size_t lds, const tff::LinearTftArgs& a) {
    return launch(c, kexact, fixup_grid(a.B, 2 * FIXUP_GRID), 64, lds, a);
}

// LinearTFTPoseEstimation / LinearFPoseEstimation, default route: four triplets per wavefront (tft_rows_kernel.h / f_rows_kernel.h, fast
// tiers; tft_rows_exact_kernel.h: whole batches for the exact tiers), then the exact kernel (one wavefront per triplet) over what they could
// not finish or certify.
int launch_pose_rows(tff_ctx* c, const PoseCall& p, pose_kernel krows, pose_kernel kexact, lds_fn exact_lds, int stage_max_n, pose_kernel krows_pre = nullptr) {
    tff::LinearTftArgs a = pose_args(c, p);
    TFF_TRY(retry_list_begin(c, &a));
    TFF_TRY(launch_rows(c, p, krows_pre, krows, &a));
    c->retry_parity ^= 1;                  // (only now: the row kernel that zeroes the next call's counter is on the stream)
    a.flags |= tff::FLAG_ONLY_RETRY;
    TFF_TRY(decide_staging(c, p, true, exact_lds, stage_max_n, &a.flags));
    return launch_retry_fixup(c, kexact, exact_lds(p.N, a.flags, true), a);
}

// LinearTFTPoseEstimation; TFF_OPT_ROWS = 0: one wavefront per triplet (fast tiers) + the exact kernel over what they could not finish.
int launch_linear_tft(tff_ctx* c, const PoseCall& p) {
    if (use_rows(c) && fast_tiers(c, p.N))
        return launch_pose_rows(c, p, tff::k_linear_tft_pose_rows<false>, tff::k_linear_tft_pose<true>, tff::pose_lds_bytes, tff::STAGE_MAX_N_TFT,
                                tff::k_linear_tft_pose_rows<true>);
    if (use_rows(c))
        return launch_pose_rows(c, p, tff::k_linear_tft_pose_rows_exact, tff::k_linear_tft_pose<true>, tff::pose_lds_bytes, tff::STAGE_MAX_N_TFT);
    return launch_pose(c, p, tff::k_linear_tft_pose<false>, tff::k_linear_tft_pose<true>, tff::pose_lds_bytes, tff::STAGE_MAX_N_TFT, 0);
}
int launch_linear_f(tff_ctx* c, const PoseCall& p) {
    if (use_rows(c))
        return fast_tiers(c, p.N)
            ? launch_pose_rows(c, p, tff::k_linear_f_pose_rows, tff::k_f_pose<true, 0>, tff::f_pose_lds_bytes, tff::STAGE_MAX_N_F)
            : launch_pose_rows(c, p, tff::k_linear_f_pose_rows_exact, tff::k_f_pose<true, 0>, tff::f_pose_lds_bytes, tff::STAGE_MAX_N_F);
    return launch_pose(c, p, tff::k_f_pose<false, 0>, tff::k_f_pose<true, 0>, tff::f_pose_lds_bytes, tff::STAGE_MAX_N_F, 0);
}
// OptimFPoseEstimation.  Three stages (optimf_rows_kernel.h) -- linear stage and pose tail four triplets per wavefront, the Gauss-Helmert
// refinement one wavefront per triplet -- then the exact kernel over what they could not finish.  Minimal samples, TFF_OPT_ROWS = 0,
// TFF_OPT_SOLVER = 1, TFF_OPT_KERNEL = 1, debug records: the fused one-triplet kernel.
// k_optimf_refine's storage of N correspondences, as the fixed-N launcher picks it (the ragged launcher's classes and tff_optim_f_ragged_bounds
// follow the same two rules).  The normalised observations go to LDS with xi while eight wavefronts still fit a CU (N <= ~220); beyond, the passes
// read the correspondences through L2 as the fused kernel does, and xi follows plan_spill's occupancy rule.
bool optimf_stage_x(int N) { return tff::optimf_refine_lds_bytes(N, true) + 512 <= LDS_LIMIT / (4 * tff::OPTIMF_REFINE_WAVES); }
bool optimf_xi_in_lds(bool spill_only_if_needed, int N) {
    return !spill_wanted(spill_only_if_needed, tff::optimf_refine_lds_bytes(N, false), tff::optimf_refine_lds_bytes(0, false), 4 * tff::OPTIMF_REFINE_WAVES);
}
int launch_optim_f(tff_ctx* c, const PoseCall& p) {
    const bool staged_route = use_rows(c) && fast_tiers(c, p.N) && p.N >= 8 && !p.dbg && !p.sample_idx && c->kernel_variant != 1;
    if (staged_route) {
        const int32_t N = p.N;
        TFF_TRY(c->gh_rec.reserve((size_t)p.B * tff::OPTIMF_REC_DOUBLES * sizeof(double)));
        tff::OptimFStageArgs sa{};
        sa.la = pose_args(c, p);
        sa.rec = (double*)c->gh_rec.p;
        TFF_TRY(launch(c, tff::k_optimf_linear_rows, tff::rows_grid(p.B), 64, tff::rows_lds_bytes(), sa));
        {
            tff::OptimFStageArgs m = sa;
            unsigned grid = tff::pose_grid(p.B);
            size_t lds;
            if (optimf_stage_x(N)) {
                TFF_TRY(launch(c, tff::k_optimf_refine<tff::OPTIMF_REFINE_WAVES, true>, grid, 64, tff::optimf_refine_lds_bytes(N, true), m));
            } else {
                TFF_TRY(plan_spill(c, tff::optimf_refine_lds_bytes(N, false), tff::optimf_refine_lds_bytes(0, false), &grid, &m.spill, &m.spill_stride, &lds, 4 * tff::OPTIMF_REFINE_WAVES));
                TFF_TRY(launch(c, tff::k_optimf_refine<tff::OPTIMF_REFINE_WAVES, false>, grid, 64, lds, m));
            }
        }
        TFF_TRY(launch(c, tff::k_optimf_finish_rows, tff::rows_grid(p.B), 64, tff::rows_lds_bytes(), sa));
    }
    return launch_pose(c, p, tff::k_f_pose<false, 1>, tff::k_f_pose<true, 1>, tff::optimf_lds_bytes, 0, 12, staged_route);
}

// Iterative TFT methods: a workgroup per triplet for the iteration (gh_wg_kernel.h, pi_wg_kernel.h) between a linear stage (k_gh_linear_rows,
// or k_gh_linear + its exact fix-up) and the pose tail (k_gh_finish_rows / k_gh_finish).  What differs between the methods:
struct WgRoute {
    int occupancy_cap;                     // workgroups per CU the block kernel's registers allow (plan_spill)
    int block_threads;
    bool rows_linear = true;               // linear stage four triplets per wavefront (where TFF_OPT_ROWS allows)
    bool nordberg_pre = false;             // k_nordberg_init before the block kernel
    bool fp_first = false;                 // FaugPapa's own block kernel first, the generic one over what it hands back
    size_t xi_bytes_per_n = 0;             // > 0: when the state is spilled for occupancy, xi alone may stay in LDS (FLAG_XI_IN_LDS)
};
// wg_lds(n): LDS bytes of the block kernel for n correspondences held in LDS.
template <class KBlock, class LdsFn>
int launch_wg(tff_ctx* c, const PoseCall& p, KBlock kblock, LdsFn wg_lds, const WgRoute& route) {
    const int64_t B = p.B;
    const int32_t N = p.N;
    TFF_TRY(c->gh_rec.reserve((size_t)B * tff::GH_REC_DOUBLES * sizeof(double)));
    TFF_TRY(c->gh_topt.reserve((size_t)B * 27 * sizeof(double)));
    tff::GhWgArgs a{p.corresp, p.calm, (long)p.calm_stride, (long)B, N, base_flags(c, p.reconst != nullptr), (double*)c->gh_rec.p, (double*)c->gh_topt.p,
                    p.Rt2, p.Rt3, p.T, p.reconst, p.iter, p.status, p.dbg, nullptr, 0};
    {   // linear stage: fast tiers, then the exact kernel over the triplets they marked ST_RETRY (minimal samples, TFF_OPT_SOLVER = 1: exact kernel for all)
        tff::GhWgArgs m = a;
        bool fast = fast_tiers(c, N);
        if (fast && route.rows_linear && use_rows(c)) {                                // four triplets per wavefront (gh_rows_kernel.h), whatever the batch size
            TFF_TRY(launch_rows(c, p, tff::k_gh_linear_rows<true>, tff::k_gh_linear_rows<false>, &m));
            m.flags |= tff::FLAG_ONLY_RETRY;
            fast = false;
        }
        TFF_TRY(launch_fast_exact(c, tff::k_gh_linear<false>, tff::k_gh_linear<true>, fast, m, [&](bool exact, tff::GhWgArgs* k, unsigned*, size_t* lds) {
            k->flags = staged_flags(c, N, k->flags, exact);
            *lds = tff::pose_lds_bytes(N, k->flags, exact);
            return 0;
        }));
    }
    if (route.nordberg_pre) {   // the serial part of Nordberg's initial parameters, one triplet per lane (gh_wg_kernel.h::k_nordberg_init)
        TFF_TRY(c->gh_init.reserve((size_t)B * tff::NordbergModel::PRE_DOUBLES * sizeof(double)));
        a.init_rec = (double*)c->gh_init.p;
        TFF_TRY(launch(c, tff::k_nordberg_init, (unsigned)((B + 63) / 64), 64, 0, a));
    }
    if (route.fp_first) {   // FaugPapa's own block kernel (gh_fp_kernel.h); the generic one below then redoes what it handed back (ST_RETRY: almost always nothing)
        tff::GhWgArgs m = a;
        unsigned grid = tff::pose_grid(B);
        size_t lds;
        TFF_TRY(plan_spill(c, tff::fp_lds_bytes(N), tff::fp_lds_bytes(0), &grid, &m.spill, &m.spill_stride, &lds, tff::FP_WG_PER_CU));
        if (m.spill) TFF_TRY(launch(c, tff::k_fp_block<false>, grid, tff::FP_THREADS, lds, m));
        else TFF_TRY(launch(c, tff::k_fp_block<true>, grid, tff::FP_THREADS, lds, m));
    }
    {
        tff::GhWgArgs m = a;
        unsigned grid = route.fp_first ? fixup_grid(B) : tff::pose_grid(B);
        if (route.fp_first) m.flags |= tff::FLAG_ONLY_RETRY;
        size_t lds;
        TFF_TRY(plan_spill(c, wg_lds(N), wg_lds(0), &grid, &m.spill, &m.spill_stride, &lds, route.occupancy_cap));
        if (m.spill && route.xi_bytes_per_n) {                               // the state went to global slices for occupancy: does xi alone still fit in LDS?
            const size_t partial = wg_lds(0) + route.xi_bytes_per_n * (size_t)N;
            if (partial <= LDS_LIMIT && LDS_LIMIT / (partial + 512) >= (size_t)route.occupancy_cap) { lds = partial; m.flags |= tff::FLAG_XI_IN_LDS; }
        }
        TFF_TRY(launch(c, kblock, grid, route.block_threads, lds, m));
    }
    if (N >= 12 && use_rows(c))                                              // four triplets per wavefront (gh_rows_kernel.h); minimal samples: the one-triplet kernel's ladder
        return launch(c, tff::k_gh_finish_rows, tff::rows_grid(B), 64, tff::rows_lds_bytes(), a);
    return launch(c, tff::k_gh_finish, tff::pose_grid(B), 64, tff::pose_lds_bytes(N, 0, false), a);
}
// TFF_OPT_KERNEL = 1 selects the fused single-wavefront kernels (gh_kernel.h; for the Pi methods also TFF_OPT_SOLVER = 1, pi_kernel.h).
template <class Model>
int launch_gh(tff_ctx* c, const PoseCall& p, pose_kernel kfused, pose_kernel kfused_jac) {
    // Both kernels evaluate the weights in the factored form that reproduces the 50-digit iteration (tests/test_gpu_gh_noise.py runs
    // each of them on every fixture).  With TWO wavefronts per workgroup and four workgroups per CU (gh_wg_kernel.h::gh_wg_waves) the
    // workgroup path wins at every N -- tools/ab_wg_fused.py, 10 k triplets, workgroup / fused: Ressl 1.62 / 2.33 ms at N = 12, 1.58 / 2.34 at 60,
    // 1.77 / 2.85 at 100; Nordberg 2.00 / 2.96, 1.94 / 2.92, 2.10 / 3.74 -- so the fused kernels remain as TFF_OPT_KERNEL = 1 only.
    if (c->kernel_variant == 1)                                              // TFF_OPT_SOLVER = 1 is honoured by launch_wg's linear stage
        return launch_pose(c, p, kfused, kfused_jac, tff::gh_lds_bytes<Model>, 0, std::is_same<Model, tff::ResslModel>::value ? 8 : 4);
    auto wg_lds = [](int n) { return (size_t)(((tff::POSE_LDS_DOUBLES + 1) & ~1) + tff::gh_wg_lds_doubles(Model::U, Model::C, n, Model::REDUNDANT_CONSTRAINTS)) * sizeof(double); };
    // occupancy policy of the per-correspondence state (plan_spill): Nordberg runs as fast with it in LDS at two workgroups per CU as with it in global
    // slices at three (3.89 vs 3.87 ms per 10 k x 200) -- without the state's HBM round trips (what is left of its 52x algorithmic traffic is scratch:
    // the 168-register build spills 368 registers, and is still faster than the 256-register one, 3.69 vs 3.90 ms)
    WgRoute route{tff::gh_wg_per_cu<Model>::value, tff::gh_wg_waves<Model>::value * tff::WAVE};
    route.nordberg_pre = std::is_same<Model, tff::NordbergModel>::value;
    // FaugPapa: the factored iteration of gh_fp_kernel.h (the threads stride over the correspondences: any N) unless an A/B switch asks for the generic kernel
    route.fp_first = std::is_same<Model, tff::FaugPapaModel>::value && c->kernel_variant == 0 && !c->gh_exact;
    route.xi_bytes_per_n = tff::GH_XI * sizeof(double);
    return launch_wg(c, p, tff::k_gh_block<Model>, wg_lds, route);
}
template <class Model>
int launch_pi_model(tff_ctx* c, const PoseCall& p) {
    // both kernels carry the factored weights; the two-wavefront workgroups of pi_wg_kernel.h win at every N -- Pi 2.12 / 2.42 ms at N = 12,
    // 2.09 / 2.35 at 60, 2.28 / 3.04 at 100, workgroup / fused, tools/ab_wg_fused.py
    if (c->kernel_variant == 1 || c->solver != 0 || p.init_p)                // the debug outputs (init_p, init_x) come from the fused kernel
        return launch_pose(c, p, tff::k_pi_tft_pose<Model, false>, tff::k_pi_tft_pose<Model, true>, tff::pi_lds_bytes<Model>, 0, 4);
    auto wg_lds = [](int n) { return (size_t)(((tff::POSE_LDS_DOUBLES + 1) & ~1) + tff::pi_wg_lds_doubles(Model::E, Model::C, n)) * sizeof(double); };
    // PiCol keeps the one-triplet-per-wavefront LINEAR stage: its scenes that take seven Gauss-Helmert iterations amplify a last-bit difference
    // of the start a million times (tools/diag_gh_noise_picol.py: 3.3e-10 from the 50-digit iteration with this start, 2.5e-9 with the rows
    // kernel's on the same N = 60 scene -- both draws of the same rounding noise, one of them over the 1e-9 gate of tests/test_gpu_gh_noise.py).
    // Its POSE TAIL (transform_TFT, R_t_from_TFT of the optimised tensor) is a fixed, well-conditioned function of that tensor and nothing
    // amplifies its rounding: it runs four triplets per wavefront like everyone else's since round 5 (k_gh_finish was 0.56 of PiCol's 5.4 ms).
    WgRoute route{4, tff::pi_wg_waves<Model>::value * tff::WAVE};
    route.rows_linear = !Model::PINV_KKT;
    return launch_wg(c, p, tff::k_pi_block<Model>, wg_lds, route);
}
int launch_ressl_tft(tff_ctx* c, const PoseCall& p) {
    return launch_gh<tff::ResslModel>(c, p, tff::k_gh_tft_pose<tff::ResslModel, false>, tff::k_gh_tft_pose<tff::ResslModel, true>);
}
int launch_nordberg_tft(tff_ctx* c, const PoseCall& p) {
    return launch_gh<tff::NordbergModel>(c, p, tff::k_gh_tft_pose<tff::NordbergModel, false>, tff::k_gh_tft_pose<tff::NordbergModel, true>);
}
int launch_faugpapa_tft(tff_ctx* c, const PoseCall& p) {
    return launch_gh<tff::FaugPapaModel>(c, p, tff::k_gh_tft_pose<tff::FaugPapaModel, false>, tff::k_gh_tft_pose<tff::FaugPapaModel, true>);
}
int launch_pi(tff_ctx* c, const PoseCall& p) { return launch_pi_model<tff::PiModel>(c, p); }
int launch_picol(tff_ctx* c, const PoseCall& p) { return launch_pi_model<tff::PiColModel>(c, p); }

// ---- the methods ----------------------------------------------------------------------------------------------------------------------------
struct RaggedRoute {                       // the kernels of one method's ragged chain (row kernel of the fast tiers, of the exact tiers, fix-up), or, for a
    pose_kernel fast, exact, fixup;        // chain of more stages, a launcher of its own (both null: the method has none)
    lds_fn fix_lds;
    int stage_max_n;
    pose_launcher chain = nullptr;
};
int launch_ragged_optim_f(tff_ctx* c, const PoseCall& p);
struct Method {
    pose_launcher launch;
    RaggedRoute ragged;
};
const Method METHODS[] = {                 // indexed by TFF_METHOD_*
    {launch_linear_tft, {tff::k_linear_tft_pose_rows<false, true>, tff::k_linear_tft_pose_rows_exact_ragged, tff::k_linear_tft_pose<true, true>,
                         tff::pose_lds_bytes, tff::STAGE_MAX_N_TFT}},
    {launch_ressl_tft, {}},
    {launch_nordberg_tft, {}},
    {launch_faugpapa_tft, {}},
    {launch_pi, {}},
    {launch_picol, {}},
    {launch_linear_f, {tff::k_linear_f_pose_rows_ragged, tff::k_linear_f_pose_rows_exact_ragged, tff::k_f_pose<true, 0, true>,
                       tff::f_pose_lds_bytes, tff::STAGE_MAX_N_F}},
    {launch_optim_f, {nullptr, nullptr, nullptr, nullptr, 0, launch_ragged_optim_f}},
};
static_assert(TFF_METHOD_LINEAR_TFT == 0 && TFF_METHOD_RESSL_TFT == 1 && TFF_METHOD_NORDBERG_TFT == 2 && TFF_METHOD_FAUGPAPA_TFT == 3 && TFF_METHOD_PI == 4 &&
              TFF_METHOD_PICOL == 5 && TFF_METHOD_LINEAR_F == 6 && TFF_METHOD_OPTIM_F == 7 && sizeof(METHODS) / sizeof(METHODS[0]) == 8, "METHODS follows the ids");
const Method* method_of(int32_t id) { return (id >= TFF_METHOD_LINEAR_TFT && id <= TFF_METHOD_OPTIM_F) ? &METHODS[id] : nullptr; }

// ---- a pose call, under the lock ---------------------------------------------------------------------------------------------------------------
template <class Body>
int run_pose(tff_ctx* c, PoseCall* p, bool borrow_status, Body body) {
    return run_batch(c, p->B, p->Rt2 && p->Rt3 && p->T, "null output pointer", borrow_status ? &p->status : nullptr, body);
}
int pose_dev_locked(tff_ctx* c, const Method* m, PoseCall p) {
    TFF_TRY(check_common(p.corresp, p.calm, p.calm_stride, p.B, p.N));
    return run_pose(c, &p, true, [&] { return m->launch(c, p); });
}
// Host-pointer variant of any pose call, fixed-N or ragged: H2D, launch(the same call on device pointers), six D2H copies, synchronise.
// [first, total): the correspondences of `h.corresp` (and 3-vectors of h.reconst) in use.
template <class Launch>
int pose_via_staging(tff_ctx* c, const PoseCall& h, size_t first, size_t total, Launch launch) {
    const size_t B = (size_t)h.B;
    const size_t ncal = (h.calm_stride ? B : 1) * 27 * sizeof(double);
    TFF_TRY(c->in.reserve(total ? total * 6 * sizeof(double) : 8));
    TFF_TRY(c->calm.reserve(ncal));
    TFF_TRY(c->out.reserve((B * (12 + 12 + 27) + (h.reconst ? 3 * total : 0)) * sizeof(double)));
    TFF_TRY(c->idx.reserve(B * 2 * sizeof(int32_t)));
    if (h.offsets) TFF_TRY(c->ragged_off.reserve((B + 1) * sizeof(int64_t)));
    PoseCall d = h;
    double* d_in = (double*)c->in.p;
    d.corresp = d_in;
    d.calm = (double*)c->calm.p;
    d.Rt2 = (double*)c->out.p;
    d.Rt3 = d.Rt2 + B * 12;
    d.T = d.Rt3 + B * 12;
    d.reconst = h.reconst ? d.T + B * 27 : nullptr;
    d.iter = (int32_t*)c->idx.p;
    d.status = d.iter + B;
    if (total > first) TFF_HIP(hipMemcpyAsync(d_in + 6 * first, h.corresp + 6 * first, (total - first) * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    TFF_HIP(hipMemcpyAsync((void*)d.calm, h.calm, ncal, hipMemcpyHostToDevice, c->stream));
    if (h.offsets) {
        TFF_HIP(hipMemcpyAsync(c->ragged_off.p, h.offsets, (B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        d.offsets = (const int64_t*)c->ragged_off.p;
    }
    TFF_TRY(launch(d));
    TFF_HIP(hipMemcpyAsync(h.Rt2, d.Rt2, B * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipMemcpyAsync(h.Rt3, d.Rt3, B * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipMemcpyAsync(h.T, d.T, B * 27 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h.reconst && total > first)
        TFF_HIP(hipMemcpyAsync(h.reconst + 3 * first, d.reconst + 3 * first, (total - first) * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (h.iter) TFF_HIP(hipMemcpyAsync(h.iter, d.iter, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (h.status) TFF_HIP(hipMemcpyAsync(h.status, d.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
// the two forms of a fixed-N pose call; they take the lock (the multi-GPU calls come through here too, one context per thread)
int pose_dev(tff_ctx* c, int32_t method, const PoseCall& p) {
    TFF_ENTER(c);
    return pose_dev_locked(c, &METHODS[method], p);
}
int pose_host(tff_ctx* c, int32_t method, PoseCall h) {
    TFF_ENTER(c);
    TFF_TRY(check_common(h.corresp, h.calm, h.calm_stride, h.B, h.N));
    return run_pose(c, &h, false, [&] {
        return pose_via_staging(c, h, 0, (size_t)h.B * (size_t)h.N, [&](const PoseCall& d) { return METHODS[method].launch(c, d); });
    });
}

// ---- ragged batches (tff_pose_batch_ragged_*; plan in ragged_kernel.h) ------------------------------------------------------------------------
// Triplet b of a ragged batch takes the kernel chain the fixed-N launcher takes for its own n_b: the row kernel of its tier (exact tiers for
// n < exact_below or TFF_OPT_SOLVER = 1, fast tiers otherwise), then the one-triplet exact kernel over the retry list.  The plan buckets the items
// by n, so each wavefront of a row kernel carries one n and runs exactly the fixed-N instructions for it; the fix-up kernel reads n and the
// LDS staging decision per triplet.  No host synchronisation: the plan's counts stay on the device.
constexpr int32_t RAGGED_MAX_N = 1 << 24;   // bounds the plan's buckets (n_max + 1 of them)

// the ragged chain of a known method under the context's options, or the refusal (the robust estimator's refits come through here too)
int ragged_route(const tff_ctx* c, int32_t method, const RaggedRoute** route) {
    if (!use_rows(c)) return fail(TFF_E_INVALID, "ragged batches run on the row kernels: TFF_OPT_ROWS = 0 is not supported");
    if (c->kernel_variant == 1) return fail(TFF_E_INVALID, "ragged batches: TFF_OPT_KERNEL = 1 (fused single-wavefront kernels) is not supported");
    *route = &method_of(method)->ragged;
    if (!(*route)->fast && !(*route)->chain)
        return fail(TFF_E_INVALID, "ragged batches are implemented for LinearTFT, LinearF and OptimF only; group this method's triplets by N");
    return 0;
}
int check_ragged(const tff_ctx* c, int32_t method, const PoseCall& p, const RaggedRoute** route) {
    if (!method_of(method)) return fail(TFF_E_INVALID, "unknown method");
    if (p.B < 0 || p.N < 0) return fail(TFF_E_INVALID, "negative batch size or n_max");
    if (p.N > RAGGED_MAX_N) return fail(TFF_E_INVALID, "ragged batches: n_max above 2^24");
    if (p.B >= (1L << tff::RETRY_HINT_SHIFT)) return fail(TFF_E_INVALID, "ragged batches: at most 2^28 - 1 triplets per call");
    if (!p.offsets) return fail(TFF_E_INVALID, "null offsets");
    if (p.B > 0 && (!p.corresp || !p.calm)) return fail(TFF_E_INVALID, "null input pointer");
    if (p.calm_stride != 0 && p.calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
    return ragged_route(c, method, route);
}

// largest n <= n_max whose fixed-N call stages the correspondences of the fix-up kernel in LDS (launch_pose_rows), -1 if none: the rule holds
// for every n up to some bound, so a bisection finds it
int ragged_stage_upto(const tff_ctx* c, const RaggedRoute& r, int flags, int32_t n_max) {
    auto staged = [&](int n) { return (staged_if_fits(c, n, flags, true, r.fix_lds, r.stage_max_n) & tff::FLAG_STAGE_LDS) != 0; };
    if (!staged(0)) return -1;
    int lo = 0, hi = n_max;                // staged(lo) holds
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (staged(mid)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the plan on the stream: hist | fill | start (n_max + 1 each) | route (RAGGED_ROUTE_INTS) | slot list.  *pa: offsets, B, n_max, split, cut and the retry
// list are the caller's; the workspace pointers and outputs are filled in here.
int launch_ragged_plan(tff_ctx* c, const PoseCall& p, tff::RaggedPlanArgs* pa, long* slots) {
    const size_t nb = (size_t)p.N + 1;
    *slots = tff::ragged_slots((long)p.B, p.N);
    TFF_TRY(c->ragged.reserve((3 * nb + tff::RAGGED_ROUTE_INTS + (size_t)*slots) * sizeof(int32_t)));
    int* ws = (int*)c->ragged.p;
    pa->offsets = (const long*)p.offsets; pa->B = (long)p.B; pa->n_max = p.N;
    pa->hist = ws; pa->fill = ws + nb; pa->start = ws + 2 * nb; pa->route = ws + 3 * nb; pa->list = ws + 3 * nb + tff::RAGGED_ROUTE_INTS;
    pa->Rt2 = p.Rt2; pa->Rt3 = p.Rt3; pa->T = p.T; pa->iter = p.iter; pa->status = p.status;
    TFF_HIP(hipMemsetAsync(ws, 0, 2 * nb * sizeof(int32_t), c->stream));
    const unsigned items = (unsigned)((p.B + 255) / 256);
    TFF_TRY(launch(c, tff::k_ragged_count, items, 256, 0, *pa));
    TFF_TRY(launch(c, tff::k_ragged_scan, 1, tff::RAGGED_SCAN_THREADS, 0, *pa));
    return launch(c, tff::k_ragged_scatter, items, 256, 0, *pa);
}
int ragged_split(const tff_ctx* c, int32_t n_max, int least) {
    const int at = c->exact_below > least ? c->exact_below : least;
    return (c->solver != 0 || at > n_max) ? n_max + 1 : at;
}

int launch_ragged(tff_ctx* c, const RaggedRoute& r, const PoseCall& p) {
    if (r.chain) return r.chain(c, p);
    const int64_t B = p.B;
    const int32_t n_max = p.N;
    tff::RaggedPlanArgs pa{};
    pa.split = ragged_split(c, n_max, 0);
    long slots;
    TFF_TRY(launch_ragged_plan(c, p, &pa, &slots));
    tff::LinearTftArgs a{p.corresp, p.calm, (long)p.calm_stride, (long)B, 0, base_flags(c, p.reconst != nullptr), p.Rt2, p.Rt3, p.T, p.reconst, p.iter, p.status};
    TFF_TRY(retry_list_begin(c, &a));
    a.offsets = (const long*)p.offsets;
    a.rlist = pa.list;
    a.stage_upto = -1;
    const unsigned grid = tff::rows_grid(slots);
    if (pa.split > 0) {                    // some n may be below the split: the exact tiers' row kernel over [0, mid)
        a.rrange = pa.route;
        TFF_TRY(launch(c, r.exact, grid, 64, tff::rows_lds_bytes(), a));
    }
    if (pa.split <= n_max) {               // ... and the fast tiers' over [mid, total)
        a.rrange = pa.route + 2;
        TFF_TRY(launch(c, r.fast, grid, 64, tff::rows_lds_bytes(), a));
    }
    c->retry_parity ^= 1;
    a.rrange = nullptr;
    a.flags |= tff::FLAG_ONLY_RETRY;
    a.stage_upto = ragged_stage_upto(c, r, a.flags, n_max);
    const size_t lds = a.stage_upto >= 0 ? r.fix_lds(a.stage_upto, a.flags | tff::FLAG_STAGE_LDS, true) : r.fix_lds(0, a.flags, true);
    return launch_retry_fixup(c, r.fixup, lds, a);
}

// largest n <= n_max with pred(n), pred holding for every n up to some bound; -1 if not even pred(0)
template <class Pred>
int largest_n(int n_max, Pred pred) {
    if (!pred(0)) return -1;
    int lo = 0, hi = n_max;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (pred(mid)) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// the two bounds of k_optimf_refine's storage routes (launch_optim_f): observations staged in LDS up to [0], xi in LDS up to [1]
void optimf_ragged_bounds(bool spill_only_if_needed, int32_t bounds[2]) {
    bounds[0] = largest_n(RAGGED_MAX_N, optimf_stage_x);
    bounds[1] = largest_n(RAGGED_MAX_N, [&](int n) { return optimf_xi_in_lds(spill_only_if_needed, n); });
    if (bounds[1] < bounds[0]) bounds[1] = bounds[0];
}

// OptimFPoseEstimation, ragged.  Item b takes launch_optim_f's chain for N = n_b:
//   n_b < max(8, exact_below) or TFF_OPT_SOLVER = 1   the plan marks it ST_RETRY and lists it: k_f_pose<true, 1, true> does it whole (n_b < 8: ST_TOO_FEW)
//   otherwise                                         k_optimf_linear_rows_ragged -> k_optimf_refine<., ., true> -> k_optimf_finish_rows_ragged over the
//                                                     slots [mid, total), then k_f_pose<true, 1, true> over what they marked ST_RETRY
// The refinement runs as up to three launches over contiguous ranges of the slot list (it is sorted by n), each with the storage route and so the
// kernel instance the fixed-N launcher picks for every n of its range: STAGE_X up to bounds[0], xi in LDS up to bounds[1], xi in global slices
// beyond (slices sized for n_max).  An LDS request is sized for the largest n its range can hold, so the small items keep their eight wavefronts
// per CU whatever n_max is.  A range the host knows to be empty is not launched; one that is empty on the device costs an empty launch.
// Workspaces (grown on demand): gh_rec B x OPTIMF_REC_DOUBLES (indexed by item), spill (slices x (4 n_max + 16) doubles, only when n_max is beyond
// the LDS bounds), ragged (the plan), retry.
int launch_ragged_optim_f(tff_ctx* c, const PoseCall& p) {
    const int64_t B = p.B;
    const int32_t n_max = p.N;
    int32_t bounds[2];
    optimf_ragged_bounds(c->spill_only_if_needed != 0, bounds);
    tff::OptimFStageArgs sa{};
    sa.la = tff::LinearTftArgs{p.corresp, p.calm, (long)p.calm_stride, (long)B, 0, base_flags(c, p.reconst != nullptr), p.Rt2, p.Rt3, p.T, p.reconst, p.iter, p.status};
    tff::LinearTftArgs& a = sa.la;
    TFF_TRY(retry_list_begin(c, &a));
    tff::RaggedPlanArgs pa{};
    pa.split = ragged_split(c, n_max, 8);
    const auto cut_at = [&](int upto, int least) { const long k = (long)upto + 1 > least ? (long)upto + 1 : least; return (int)(k > n_max ? (long)n_max + 1 : k); };
    pa.cut[0] = cut_at(bounds[0], pa.split);
    pa.cut[1] = cut_at(bounds[1], pa.cut[0]);
    pa.retry_list = a.retry_list; pa.retry_count = a.retry_count;
    // Every workspace is reserved before the plan goes on the stream: its scatter already appends to this call's retry counter, and only the linear
    // stage below zeroes the other one, so nothing that can fail may come between the two.  Both users of the spill slices are sized together (the
    // workspace is shared and must not move under the first of them).  All of it needs B, n_max and the slot count's upper bound only.
    long slots = tff::ragged_slots((long)B, n_max);
    const bool refine_spills = pa.cut[1] <= n_max;
    const size_t fix_full = tff::optimf_lds_bytes(n_max, a.flags, true), fix_fixed = tff::optimf_lds_bytes(0, a.flags, true);
    const bool fix_spills = fix_full > LDS_LIMIT;
    unsigned grid_c = tff::pose_grid(slots), grid_fix = fixup_grid(B, 2 * FIXUP_GRID);
    double* slices = nullptr; long stride = 0;
    if (refine_spills || fix_spills) {     // one slice per block of the larger of the two grids, stride sized for n_max; the grids are capped at the slice count
        unsigned need = 1;
        if (refine_spills) need = grid_c;
        if (fix_spills && grid_fix > need) need = grid_fix;
        TFF_TRY(spill_slices(c, 4 * (size_t)n_max * sizeof(double), &need, &slices, &stride));
        if (grid_c > need) grid_c = need;
        if (grid_fix > need) grid_fix = need;
    }
    TFF_TRY(c->gh_rec.reserve((size_t)B * tff::OPTIMF_REC_DOUBLES * sizeof(double)));
    sa.rec = (double*)c->gh_rec.p;
    TFF_TRY(launch_ragged_plan(c, p, &pa, &slots));
    a.offsets = (const long*)p.offsets;
    a.rlist = pa.list;
    a.stage_upto = -1;
    const unsigned rows = tff::rows_grid(slots);
    a.rrange = pa.route + 2;
    TFF_TRY(launch(c, tff::k_optimf_linear_rows_ragged, rows, 64, tff::rows_lds_bytes(), sa));   // (always: it zeroes the next call's retry counter)
    c->retry_parity ^= 1;
    if (pa.split <= n_max) {
        constexpr int W = tff::OPTIMF_REFINE_WAVES;
        tff::OptimFStageArgs m = sa;
        if (pa.split < pa.cut[0]) {
            m.la.rrange = pa.route + 4;
            m.lds_n = pa.cut[0] - 1;
            TFF_TRY(launch(c, tff::k_optimf_refine<W, true, true>, tff::pose_grid(slots), 64, tff::optimf_refine_lds_bytes(m.lds_n, true), m));
        }
        if (pa.cut[0] < pa.cut[1]) {
            m.la.rrange = pa.route + 6;
            m.lds_n = pa.cut[1] - 1;
            TFF_TRY(launch(c, tff::k_optimf_refine<W, false, true>, tff::pose_grid(slots), 64, tff::optimf_refine_lds_bytes(m.lds_n, false), m));
        }
        if (refine_spills) {
            m.la.rrange = pa.route + 8;
            m.lds_n = 0;
            m.spill = slices; m.spill_stride = stride;
            TFF_TRY(launch(c, tff::k_optimf_refine<W, false, true>, grid_c, 64, tff::optimf_refine_lds_bytes(0, false), m));
        }
        TFF_TRY(launch(c, tff::k_optimf_finish_rows_ragged, rows, 64, tff::rows_lds_bytes(), sa));
    }
    a.rrange = nullptr;
    a.flags |= tff::FLAG_ONLY_RETRY;
    if (fix_spills) { a.spill = slices; a.spill_stride = stride; }
    return launch(c, tff::k_f_pose<true, 1, true>, grid_fix, 64, fix_spills ? fix_fixed : fix_full, a);
}

// ---- inlier counts and flags of pose hypotheses against one shared scene ------------------------------------------------------------------------
// the c of blocks_kernel.h::inlier_weight: 1 / (6 thr^2) in double, once per call, so that no kernel divides
double score_scale(double threshold) { return 1.0 / (6.0 * threshold * threshold); }
int launch_inlier_count(tff_ctx* c, const double* scene, int32_t Ns, const double* calm, const double* Rt2, const double* Rt3, int64_t B, double threshold,
                        int32_t* counts, double* err) {
    tff::ReprErrorArgs a{nullptr, 0, calm, Rt2, Rt3, scene, 0, nullptr, (long)B, Ns, threshold, err, counts};
    const bool msac = c->score == 1;                                         // every route has its *_msac twin: the same launch, scores instead of counts
    if (msac) a.score_c = score_scale(threshold);
    const size_t staged = ((size_t)6 * Ns + 36 * tff::INLIER_WG_WAVES) * sizeof(double);
    if (err || staged > 48 * 1024 || B < 4096) return launch(c, msac ? tff::k_repr_error_msac : tff::k_repr_error, tff::pose_grid(B), 64, 0, a);
    // counts only, many hypotheses, a scene that fits the LDS a few times over: stage it once per workgroup (blocks_kernel.h)
    if (c->count_rows) {                                                 // four hypotheses per wavefront (blocks_kernel.h::k_inlier_count_rows): two workgroups per CU
        const size_t staged_rows = ((size_t)6 * Ns + 36 * 4 * tff::INLIER_WG_WAVES) * sizeof(double);
        long grid_rows = 256L * 2;
        const long per_wg = 4L * tff::INLIER_WG_WAVES;
        if (grid_rows * per_wg > B) grid_rows = (B + per_wg - 1) / per_wg;
        return launch(c, msac ? tff::k_inlier_count_rows_msac : tff::k_inlier_count_rows, (unsigned)grid_rows, 64 * tff::INLIER_WG_WAVES, staged_rows, a);
    }
    const int per_cu = (int)((LDS_LIMIT / (staged + 512) < 4) ? LDS_LIMIT / (staged + 512) : 4);
    long grid = 256L * per_cu;
    if (grid * tff::INLIER_WG_WAVES > B) grid = (B + tff::INLIER_WG_WAVES - 1) / tff::INLIER_WG_WAVES;
    return launch(c, msac ? tff::k_inlier_count_staged_msac : tff::k_inlier_count_staged, (unsigned)grid, 64 * tff::INLIER_WG_WAVES, staged, a);
}

// ---- robust estimation (tff_robust_pose_*, tff_robust_pose_scenes_*; kernels and the chunking in robust_kernel.h, robust_scenes_kernel.h) ------------------
// Every entry point fills one ScenesCall and hands it to robust_dev or robust_host (below, with the entry points); both go through check_scenes and end
// in launch_robust_scenes, whose workspaces reserve_robust lays out (robust_layout.h).

// The rounds of the adaptive call (include/tftfund.h): round r ends at ends[r - 1] = min(n_hyp, first_round << (r - 1)) hypotheses per scene, and a scene
// stops there once w^n_sample >= qmin[r - 1] = -expm1(log1p(-confidence) / ends[r - 1]) for the inlier ratio w of its best hypothesis
constexpr int MAX_ROUNDS = 32;
struct RoundPlan { int rounds; int64_t ends[MAX_ROUNDS]; double qmin[MAX_ROUNDS]; };
// one call of the chain, in any form: S scenes, host or device pointers as the function says
struct ScenesCall {
    int32_t method; const double* scenes; const int64_t* offsets; int64_t n_total; int32_t ns_max; int64_t S; const double* calm; int64_t calm_stride;
    uint64_t seed; int64_t n_hyp; int32_t n_sample; double threshold; int32_t n_cand; int32_t lo_rounds;
    double* Rt2; double* Rt3; double* T; uint8_t* mask; int32_t* info; int32_t* status;
    bool one_scene = false;                  // tff_robust_pose_*: S = 1, a shared CalM and n_total = ns_max = Ns, judged as the scene's size (check_scenes)
    bool rounds = false;                     // the early stop: confidence and first_round make ...
    double confidence = 0.0; int32_t first_round = 0;
    const RoundPlan* plan = nullptr;         // ... the rounds (check_scenes), and ...
    int32_t* used = nullptr;                 // ... S: the hypotheses each scene drew
    bool guided = false;                     // tff_robust_pose_scenes_guided_*: the two arguments below are judged (first) ...
    const int32_t* order = nullptr;          // ... n_total ranks, packed like the scenes (null: the uniform sampler), and ...
    int64_t growth = 0;                      // ... the number of draws after which the guided sampler is the uniform one
};
int make_round_plan(double confidence, int64_t n_hyp, int32_t first_round, RoundPlan* p) {
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(TFF_E_INVALID, "robust estimation: the confidence must lie strictly between 0 and 1");
    if (first_round < 4 || first_round % 4 != 0) return fail(TFF_E_INVALID, "robust estimation: first_round must be a multiple of 4 and at least 4");
    if (n_hyp < 1) return fail(TFF_E_INVALID, "robust estimation: n_hyp must be at least 1");
    const double lg = std::log1p(-confidence);
    for (int r = 0; r < MAX_ROUNDS; ++r) {
        const int64_t grown = (int64_t)first_round << r;                     // (at most 2^31 << 31)
        const int64_t e = grown < n_hyp ? grown : n_hyp;
        p->ends[r] = e;
        p->qmin[r] = -std::expm1(lg / (double)e);
        if (e == n_hyp) { p->rounds = r + 1; return 0; }
    }
    return fail(TFF_E_INVALID, "robust estimation: more than 32 rounds between first_round and n_hyp");
}
// the two arguments every guided entry point adds, refused first
int check_guided(const int32_t* order, int64_t growth) {
    if (!order) return fail(TFF_E_INVALID, "guided sampling: null order");
    if (growth < 1 || growth > (int64_t)tff::GUIDED_MAX_GROWTH) return fail(TFF_E_INVALID, "guided sampling: growth must be between 1 and 2^31 - 2^25");
    return 0;
}
// The argument checks of every form, in the order the forms have always refused in; n_sample = 0 becomes the method's minimum; *route: the method's ragged
// chain (the refit); with a confidence *plan becomes the call's rounds.  A list's scene with too few correspondences is a per-scene status, not a refusal.
// ONE-SCENE VARIANT (q->one_scene): no list to judge, and the two scene-size tests see the real Ns = n_total (TFF_E_INVALID, not a status).
int check_scenes(const tff_ctx* c, ScenesCall* q, bool host, RoundPlan* plan, const RaggedRoute** route) {
    if (q->guided) TFF_TRY(check_guided(q->order, q->growth));
    // a _host list: the offsets are readable, so they are judged here (a _dev list's are a per-scene status), and n_total and ns_max come from them
    if (host && !q->one_scene) {
        if (q->S < 0) return fail(TFF_E_INVALID, "robust estimation: negative number of scenes");
        if (!q->offsets) return fail(TFF_E_INVALID, "null offsets");
        if (q->offsets[0] < 0) return fail(TFF_E_INVALID, "robust estimation: negative offset");
        int64_t ns_max = 0;
        for (int64_t s = 0; s < q->S; ++s) {
            const int64_t ns = q->offsets[s + 1] - q->offsets[s];
            if (ns < 0) return fail(TFF_E_INVALID, "robust estimation: decreasing offsets");
            if (ns > ns_max) ns_max = ns;
        }
        if (ns_max > RAGGED_MAX_N) return fail(TFF_E_INVALID, "robust estimation: a scene of more than 2^24 correspondences");
        q->n_total = q->offsets[q->S]; q->ns_max = (int32_t)ns_max;
    }
    if (!q->one_scene) {
        if (q->S < 0) return fail(TFF_E_INVALID, "robust estimation: negative number of scenes");
        if (q->n_total < 0 || q->n_total > (int64_t)INT32_MAX) return fail(TFF_E_INVALID, "robust estimation: n_total must be between 0 and 2^31 - 1");
        if (q->ns_max < 0 || q->ns_max > RAGGED_MAX_N) return fail(TFF_E_INVALID, "robust estimation: ns_max must be between 0 and 2^24");
        if (q->calm_stride != 0 && q->calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
        if (!q->offsets) return fail(TFF_E_INVALID, "null offsets");
    }
    if (q->method != TFF_METHOD_LINEAR_TFT && q->method != TFF_METHOD_LINEAR_F)
        return fail(TFF_E_INVALID, "robust estimation: the method must be TFF_METHOD_LINEAR_TFT or TFF_METHOD_LINEAR_F");
    const int32_t least = q->method == TFF_METHOD_LINEAR_F ? 8 : 7;
    if (q->n_sample == 0) q->n_sample = least;
    if (q->n_sample < least || q->n_sample > tff::ROBUST_MAX_SAMPLE) return fail(TFF_E_INVALID, "robust estimation: n_sample must be 0 or between the method's minimum (7 / 8) and 16");
    if (q->one_scene && q->n_total < q->n_sample) return fail(TFF_E_INVALID, "robust estimation: fewer correspondences than one sample");   // one-scene variant
    if (q->n_hyp < 1 || q->n_hyp > (int64_t)INT32_MAX) return fail(TFF_E_INVALID, "robust estimation: n_hyp must be between 1 and 2^31 - 1");
    if (q->n_cand < 1 || q->n_cand > tff::ROBUST_MAX_CAND) return fail(TFF_E_INVALID, "robust estimation: n_cand must be between 1 and 64");
    if (q->lo_rounds < 0 || q->lo_rounds > 8) return fail(TFF_E_INVALID, "robust estimation: lo_rounds must be between 0 and 8");
    if (!(q->threshold > 0.0) || !(q->threshold <= 1.79769313486231570e308)) return fail(TFF_E_INVALID, "robust estimation: the threshold must be a positive finite number");
    const bool packed = q->n_total != 0;                                     // (nothing packed, no flags: scenes and mask may be null)
    if ((packed && (!q->scenes || !q->mask)) || !q->calm || !q->Rt2 || !q->Rt3 || !q->T || !q->info || !q->status) return fail(TFF_E_INVALID, "null pointer");
    if (q->one_scene && q->n_total > RAGGED_MAX_N) return fail(TFF_E_INVALID, "robust estimation: more than 2^24 correspondences");   // one-scene variant
    TFF_TRY(ragged_route(c, q->method, route));                              // the refit's refusals: TFF_OPT_ROWS = 0, TFF_OPT_KERNEL = 1
    if (q->S > (int64_t)INT32_MAX / q->n_hyp) return fail(TFF_E_INVALID, "robust estimation: S * n_hyp above 2^31 - 1");
    if (q->S * q->n_cand >= (1L << tff::RETRY_HINT_SHIFT)) return fail(TFF_E_INVALID, "robust estimation: S * n_cand above the ragged call's 2^28 - 1 items");
    if (!q->rounds) return 0;
    TFF_TRY(make_round_plan(q->confidence, q->n_hyp, q->first_round, plan));   // its refusals: confidence, first_round, more than 32 rounds
    if (!q->used) return fail(TFF_E_INVALID, "null pointer");
    q->plan = plan;
    return 0;
}
// the inlier counts of B hypotheses, hypothesis b being g = first + b of the call and belonging to scene g / per
int launch_count_scenes(tff_ctx* c, const tff::SceneSet& set, const double* Rt2, const double* Rt3, int64_t first, int64_t B, int64_t per, double threshold,
                        int32_t* counts, const int32_t* live = nullptr) {
    const long rows = tff::SCENES_COUNT_ROWS;
    long grid = (B + rows - 1) / rows;
    if (grid > 256L * 2) grid = 256L * 2;                                    // two workgroups per CU
    const long slab = ((B + grid - 1) / grid + rows - 1) / rows * rows;
    grid = (B + slab - 1) / slab;
    const long want = 6L * set.ns_max;
    const int stage = (int)(want < tff::SCENES_STAGE_MAX_DOUBLES ? want : tff::SCENES_STAGE_MAX_DOUBLES);
    tff::ScenesCountArgs a{set, Rt2, Rt3, (long)first, (long)B, (long)per, slab, threshold, counts, stage};
    const bool msac = c->score == 1;
    if (msac) a.score_c = score_scale(threshold);
    a.live = live;
    return launch(c, msac ? tff::k_inlier_count_scenes_msac : tff::k_inlier_count_scenes, (unsigned)grid, 64 * tff::INLIER_WG_WAVES, ((size_t)36 * rows + (size_t)stage) * sizeof(double), a);
}
// The workspaces of one call, carved by the layouts of robust_layout.h: one chunk of hypotheses, the counts of all of them, the candidates' state
struct RobustSpace {
    int64_t G, C, chunk;                     // hypotheses (S * n_hyp) and candidates (S * n_cand) of the call; rows of a chunk
    double* h_pose; double* h_calm; int32_t* h_status; int32_t* h_idx;       // the chunk (h_calm: null with a shared CalM) ...
    int32_t* dense; unsigned long long* best; int32_t* live;                 // ... and the rounds' state (the adaptive call)
    int32_t* counts;                         // G
    tff::ScenesState st;                     // the candidates; what the host clears or hands to a kernel as an output, writable: ...
    unsigned long long* sel; uint8_t* masks; int32_t* mask_cnt;              // ... the keys, the K flags per correspondence, their row sums; and ...
    int32_t* c_idx; double* c_calm;          // ... their sample indices and CalM copies (null with a shared CalM)
    int32_t* g_ends;                         // the pool tables of a guided call
};
// Every reservation of the call, before anything of it is on the stream (DevBuf::reserve frees and allocates, which synchronises the device: none may
// happen between two launches), and the pointers.  The refit's own workspaces stay with launch_ragged.
int reserve_robust(tff_ctx* c, const ScenesCall& q, const tff::SceneSet& set, RobustSpace* w) {
    const int K = q.n_cand, n = q.n_sample;
    const int64_t S = q.S, G = q.n_total ? S * q.n_hyp : 0, C = S * K;       // (without a correspondence nothing is drawn: no chunk, no counts)
    // one chunk of hypotheses: the fixed call cuts g = s * n_hyp + h, the adaptive call the rows of a round (its longest round sizes the chunk)
    int64_t rows_max = G;
    if (q.plan && G) {
        rows_max = 0;
        for (int r = 0; r < q.plan->rounds; ++r) {
            const int64_t len = q.plan->ends[r] - (r ? q.plan->ends[r - 1] : 0);
            if (S * len > rows_max) rows_max = S * len;
        }
    }
    const int64_t chunk = rows_max < tff::ROBUST_CHUNK ? rows_max : tff::ROBUST_CHUNK;
    // one CalM per scene: every row gets a copy of its scene's for the pose kernels (stride 27).  A shared CalM goes to them as it is (stride 0): no copy is carved or written
    const size_t copies = q.calm_stride ? 27 * sizeof(double) : 0;
    const tff::ChunkLayout h = tff::chunk_layout(chunk, S, n, copies, q.plan != nullptr);
    const tff::CandLayout k = tff::cand_layout(C, K, n, q.n_total, copies);
    TFF_TRY(c->robust_hyp.reserve(h.total));
    TFF_TRY(c->robust_counts.reserve((size_t)G * sizeof(int32_t)));
    TFF_TRY(c->robust_cand.reserve(k.total));
    if (q.order) TFF_TRY(c->guided_ends.reserve((size_t)(q.n_total ? q.n_total : 1) * sizeof(int32_t)));
    TFF_TRY(retry_list_reserve(c, chunk > C ? chunk : C));                   // the largest sampled pose launch: a chunk, or the candidates' re-draw
    w->G = G; w->C = C; w->chunk = chunk;
    char* hp = (char*)c->robust_hyp.p;
    w->h_pose = (double*)(hp + h.pose); w->h_calm = copies ? (double*)(hp + h.calm) : nullptr;
    w->h_status = (int32_t*)(hp + h.status); w->h_idx = (int32_t*)(hp + h.idx);
    w->dense = (int32_t*)(hp + h.dense); w->best = (unsigned long long*)(hp + h.best); w->live = (int32_t*)(hp + h.live);
    w->counts = (int32_t*)c->robust_counts.p;
    w->g_ends = (int32_t*)c->guided_ends.p;
    char* cp = (char*)c->robust_cand.p;
    int32_t* ints = (int32_t*)(cp + k.ints);
    tff::RobustState& s = w->st.s;
    w->st.q = set; w->st.K = K; w->st.cap = (long)K * q.n_total;
    w->sel = (unsigned long long*)(cp + k.sel); w->masks = (uint8_t*)(cp + k.mask); w->mask_cnt = ints + 6 * C;
    s.sel = w->sel; s.K = C;
    s.cnt = ints; s.seed_idx = ints + C; s.nref = ints + 2 * C; s.status = ints + 3 * C; s.ref_status = ints + 4 * C; s.ref_cnt = ints + 5 * C;
    s.mask_cnt = w->mask_cnt;
    s.pose = (double*)(cp + k.pose); s.ref_pose = (double*)(cp + k.ref);
    s.offsets = (long*)(cp + k.off);
    s.mask = w->masks;
    s.packed = (double*)(cp + k.pack);
    w->c_idx = (int32_t*)(cp + k.idx);
    w->c_calm = copies ? (double*)(cp + k.calm) : nullptr;
    return 0;
}
// device pointers; the lock is held and the context's device current
int launch_robust_scenes(tff_ctx* c, const RaggedRoute& route, const ScenesCall& q) {
    const Method& m = METHODS[q.method];
    const int K = q.n_cand, n = q.n_sample;
    const int64_t S = q.S;
    const tff::SceneSet set{q.scenes, (const long*)q.offsets, (long)S, (long)q.n_total, q.ns_max, n, q.calm, (long)q.calm_stride};
    RobustSpace w{};
    TFF_TRY(reserve_robust(c, q, set, &w));
    const int64_t G = w.G, C = w.C, chunk = w.chunk;
    tff::RobustState& s = w.st.s;
    // the sampler of the call: k_scenes_sample, or its guided variant over the pool tables (robust_guided_kernel.h)
    auto sample = [&](const tff::ScenesSampleArgs& a) {
        const unsigned grid = (unsigned)((a.B + 255) / 256);
        if (!q.order) return launch(c, tff::k_scenes_sample, grid, 256, 0, a);
        return launch(c, tff::k_scenes_sample_guided, grid, 256, 0, tff::ScenesSampleGuidedArgs{a, w.g_ends, q.order});
    };
    // the method's *_pose_sampled_dev on the packed array: global indices, one CalM per row (`calm`) or the shared one
    auto sampled = [&](const int32_t* idx, const double* calm, int64_t B, double* pose, int32_t* status) {
        PoseCall p{q.scenes, calm ? calm : q.calm, q.calm_stride, B, n, pose, pose + B * 12, pose + B * 24, nullptr, nullptr, status, nullptr};
        p.sample_idx = idx; p.sample_ns = (int32_t)q.n_total;
        return m.launch(c, p);
    };
    const tff::ScenesFinishArgs fin{w.st, q.Rt2, q.Rt3, q.T, q.info, q.status};
    if (q.order && !q.plan && q.used) TFF_HIP(hipMemsetD32Async((hipDeviceptr_t)q.used, (int)q.n_hyp, (size_t)S, c->stream));   // guided, a fixed n_hyp: used[s] = n_hyp
    if (q.n_total == 0) {                                                    // no scene can be valid, and the pose kernels must not gather from an empty array
        if (q.plan) TFF_HIP(hipMemsetAsync(q.used, 0, (size_t)S * sizeof(int32_t), c->stream));
        return launch(c, tff::k_scenes_finish, (unsigned)S, 64, 0, fin);
    }
    TFF_HIP(hipMemsetAsync(q.mask, 0, (size_t)q.n_total, c->stream));
    // 0. guided sampling only: every scene's pool table, one workgroup per scene
    if (q.order)
        TFF_TRY(launch(c, tff::k_guided_ends, (unsigned)(S < 65536 ? S : 65536), tff::GUIDED_ENDS_THREADS, 0, tff::GuidedEndsArgs{set, (long)q.growth, n, w.g_ends}));
    // 1a. the adaptive call: round r draws the hypotheses [e_prev, e_end) of the scenes that are still live, chunk by chunk over the round's rows
    //     g' = s * len + i; the counts land where the fixed call puts them (stride n_hyp, -1 where nothing was drawn), the rule closes the round
    if (q.plan) {
        const tff::RoundState rs{set, w.live, w.best, q.used};
        const unsigned sgrid = (unsigned)((S + 255) / 256);
        TFF_HIP(hipMemsetAsync(w.counts, 0xFF, (size_t)G * sizeof(int32_t), c->stream));
        TFF_TRY(launch(c, tff::k_round_init, sgrid, 256, 0, rs));
        int64_t e_prev = 0;
        for (int r = 0; r < q.plan->rounds; ++r) {
            const int64_t e_end = q.plan->ends[r], len = e_end - e_prev, Gr = S * len;
            for (int64_t first = 0; first < Gr; first += chunk) {
                const int64_t B = Gr - first < chunk ? Gr - first : chunk;
                TFF_TRY(sample(tff::ScenesSampleArgs{set, (unsigned long long)q.seed, (long)first, nullptr, (long)B, (long)len, n, w.h_idx, w.h_calm, (long)e_prev, w.live}));
                TFF_TRY(sampled(w.h_idx, w.h_calm, B, w.h_pose, w.h_status));
                TFF_TRY(launch_count_scenes(c, set, w.h_pose, w.h_pose + B * 12, first, B, len, q.threshold, w.dense, w.live));
                TFF_TRY(launch(c, tff::k_round_scatter, (unsigned)((B + 255) / 256), 256, 0,
                               tff::RoundScatterArgs{w.dense, w.h_status, (long)first, (long)B, (long)len, (long)e_prev, (long)q.n_hyp, w.live, w.best, w.counts}));
            }
            TFF_TRY(launch(c, tff::k_round_close, sgrid, 256, 0,
                           tff::RoundCloseArgs{rs, (long)e_end, q.plan->qmin[r], n, c->score == 1 ? TFF_SCORE_UNITS : 1}));
            e_prev = e_end;
        }
    }
    // 1. hypotheses and their counts, chunk by chunk over g = s * n_hyp + h
    for (int64_t first = 0; !q.plan && first < G; first += chunk) {
        const int64_t B = G - first < chunk ? G - first : chunk;
        TFF_TRY(sample(tff::ScenesSampleArgs{set, (unsigned long long)q.seed, (long)first, nullptr, (long)B, (long)q.n_hyp, n, w.h_idx, w.h_calm}));
        TFF_TRY(sampled(w.h_idx, w.h_calm, B, w.h_pose, w.h_status));
        // The one branch on the form of the call: without offsets (tff_robust_pose_dev: one valid scene [0, n_total), shared CalM) the hypotheses are counted
        // by the one-scene launcher, whose one-wavefront-per-hypothesis route serves a few thousand hypotheses better than sixteen per workgroup.  Measured
        // (DESIGN.md 3.4): 0.05 ms per 1 000-hypothesis call, and the 1 M-hypothesis LinearF call back under the bar it missed by 0.16 % without it.  The
        // integers are those of k_inlier_count_scenes (count_if_inlier / score_if_inlier in both; tests/test_gpu_robust.py, test_gpu_score.py).
        // tff_robust_pose_host arrives with the offsets {0, Ns} and takes the other route, on purpose: it is keyed on what the kernels are given, the call
        // is dominated by its copies and its synchronisation, and a second key would be a second special case.  The refit counts always go the scenes route.
        if (!q.offsets) TFF_TRY(launch_inlier_count(c, q.scenes, (int32_t)q.n_total, q.calm, w.h_pose, w.h_pose + B * 12, B, q.threshold, w.counts + first, nullptr));
        else TFF_TRY(launch_count_scenes(c, set, w.h_pose, w.h_pose + B * 12, first, B, q.n_hyp, q.threshold, w.counts + first));
        TFF_TRY(launch(c, tff::k_robust_mark, (unsigned)((B + 255) / 256), 256, 0, tff::RobustMarkArgs{w.counts + first, w.h_status, (long)B}));
    }
    // 2. per scene the K best successes, then their poses again from their indices
    TFF_HIP(hipMemsetAsync(w.sel, 0, (size_t)C * 8, c->stream));
    long topk_blocks = (q.n_hyp + tff::ROBUST_TOPK_THREADS - 1) / tff::ROBUST_TOPK_THREADS;
    if (topk_blocks > 1024) topk_blocks = 1024;
    for (int64_t s0 = 0; s0 < S; s0 += 65535) {                              // (gridDim.y)
        const unsigned sy = (unsigned)(S - s0 < 65535 ? S - s0 : 65535);
        for (int r = 0; r < K; ++r)
            TFF_TRY(launch(c, tff::k_robust_topk, dim3((unsigned)topk_blocks, sy), tff::ROBUST_TOPK_THREADS, 0,
                           tff::RobustTopkArgs{w.counts + s0 * q.n_hyp, (long)q.n_hyp, w.sel + s0 * K, r, K}));
    }
    TFF_TRY(sample(tff::ScenesSampleArgs{set, (unsigned long long)q.seed, 0, w.sel, (long)C, (long)K, n, w.c_idx, w.c_calm}));
    TFF_TRY(sampled(w.c_idx, w.c_calm, C, s.pose, s.status));
    TFF_TRY(launch(c, tff::k_robust_seed, (unsigned)((C + 63) / 64), 64, 0, s));
    // 3. local optimisation, the candidates of all scenes at once: flags -> packed inliers -> one ragged refit -> counts -> adopt
    for (int round = 0; round < q.lo_rounds; ++round) {
        TFF_TRY(launch(c, tff::k_scenes_mask, tff::pose_grid(C), 64, 0,
                       tff::ScenesMaskArgs{set, s.pose, s.pose + C * 12, (long)C, (long)K, q.threshold, w.masks, w.mask_cnt, s.cnt, nullptr}));
        TFF_TRY(launch(c, tff::k_scenes_offsets, 1, tff::SCENES_SCAN_THREADS, 0, w.st));
        TFF_TRY(launch(c, tff::k_scenes_compact, (unsigned)C, tff::ROBUST_COMPACT_THREADS, 0, w.st));
        PoseCall p{s.packed, w.c_calm ? w.c_calm : q.calm, q.calm_stride, C, q.ns_max, s.ref_pose, s.ref_pose + C * 12, s.ref_pose + C * 24, nullptr, nullptr, s.ref_status, nullptr};
        p.offsets = (const int64_t*)s.offsets;
        TFF_TRY(launch_ragged(c, route, p));
        TFF_TRY(launch_count_scenes(c, set, s.ref_pose, s.ref_pose + C * 12, 0, C, K, q.threshold, s.ref_cnt));
        TFF_TRY(launch(c, tff::k_robust_adopt, (unsigned)C, 64, 0, s));
    }
    // 4. per scene the winner, and the flags of its pose in the scene's range of the packed mask (skipped where there is none)
    TFF_TRY(launch(c, tff::k_scenes_finish, (unsigned)S, 64, 0, fin));
    if (c->score != 1)
        return launch(c, tff::k_scenes_mask, tff::pose_grid(S), 64, 0,
                      tff::ScenesMaskArgs{set, q.Rt2, q.Rt3, (long)S, 1, q.threshold, q.mask, nullptr, nullptr, q.status});
    // MSAC: info[0] holds the winner's score; the row sums of the returned flags replace it (mask_cnt is free again: C >= S ints)
    TFF_TRY(launch(c, tff::k_scenes_mask, tff::pose_grid(S), 64, 0,
                   tff::ScenesMaskArgs{set, q.Rt2, q.Rt3, (long)S, 1, q.threshold, q.mask, w.mask_cnt, nullptr, q.status}));
    return launch(c, tff::k_scenes_info, (unsigned)((S + 255) / 256), 256, 0, tff::ScenesInfoArgs{w.mask_cnt, q.status, q.info, (long)S});
}

}  // namespace

extern "C" {

int tff_version(void) { return 110; }
const char* tff_last_error(void) { return g_err.c_str(); }

int tff_ctx_create(tff_ctx** out, int device) {
    if (!out) return fail(TFF_E_INVALID, "null out pointer");
    *out = nullptr;
    int n = 0;
    TFF_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(TFF_E_INVALID, "no such HIP device (libtftfund has no CPU path)");
    TFF_HIP(hipSetDevice(device));
    tff_ctx* c = new (std::nothrow) tff_ctx();
    if (!c) return fail(TFF_E_NOMEM, "out of host memory");
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return hip_fail(e, "hipStreamCreate"); }
    c->stream = c->own;
    *out = c;
    return 0;
}

void tff_ctx_destroy(tff_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->own) { (void)hipStreamSynchronize(c->own); (void)hipStreamDestroy(c->own); }
    if (c->handover) (void)hipEventDestroy(c->handover);
    for (DevBuf* b : {&c->in, &c->calm, &c->out, &c->idx, &c->scratch_status, &c->gh_rec, &c->gh_topt, &c->gh_init, &c->spill, &c->pre_rec, &c->retry, &c->ragged, &c->ragged_off, &c->robust_hyp, &c->robust_counts,
                      &c->robust_cand, &c->guided_ends, &c->guided_order, &c->ba_plan, &c->ba_pack, &c->ba_host, &c->ba_weight, &c->cov_plan, &c->cov_pack, &c->cov_rec, &c->cov_io, &c->tracks_used, &c->tracks_weight, &c->tracks_status, &c->tracks_cov_x, &c->tracks_cov_rec, &c->tracks_cov_io})
        b->release();
    delete c;
}

// The workspaces of a context (status scratch, Gauss-Helmert records, spill slices, host-path staging) are reused by every
// call, so work enqueued on the previous stream must finish before work on the new one touches them: an event recorded on the
// old stream, waited for by the new one (no host synchronisation).
static int switch_stream(tff_ctx* c, hipStream_t s) {
    if (s == c->stream) return 0;
    // the hand-over touches the context's device; the calling thread's current device is the caller's business and is put back
    int caller_device = -1;
    (void)hipGetDevice(&caller_device);
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore{caller_device};
    TFF_HIP(hipSetDevice(c->device));
    if (!c->handover) TFF_HIP(hipEventCreateWithFlags(&c->handover, hipEventDisableTiming));
    // The previous stream must still be alive here (a caller that destroys its stream first hands the context a dangling handle).  If
    // recording on it fails all the same -- a destroyed user stream -- the new stream is adopted anyway, after draining the context's
    // own stream and the device: refusing would leave the context stuck on the dead stream for every later call.
    if (hipEventRecord(c->handover, c->stream) == hipSuccess) {
        TFF_HIP(hipStreamWaitEvent(s, c->handover, 0));
    } else {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->own);
        (void)hipDeviceSynchronize();
    }
    c->stream = s;
    return 0;
}
int tff_ctx_set_stream(tff_ctx* c, void* s) {
    TFF_ENTER(c);
    return switch_stream(c, (hipStream_t)s);
}
int tff_ctx_use_own_stream(tff_ctx* c) {
    TFF_ENTER(c);
    return switch_stream(c, c->own);
}
void* tff_ctx_get_stream(tff_ctx* c) { return c ? (void*)c->stream : nullptr; }

int tff_ctx_set_option(tff_ctx* c, int option, long value) {
    TFF_ENTER(c);
    switch (option) {
        case TFF_OPT_SOLVER: if (value != 0 && value != 1) return fail(TFF_E_INVALID, "solver must be 0 or 1"); c->solver = (int)value; return 0;
        case TFF_OPT_EXACT_BELOW: if (value < 0 || value > (1L << 30)) return fail(TFF_E_INVALID, "exact_below must be >= 0"); c->exact_below = (int)value; return 0;
        case TFF_OPT_STAGE_LDS: if (value < -1 || value > 1) return fail(TFF_E_INVALID, "stage_lds must be -1, 0 or 1"); c->stage = (int)value; return 0;
        case TFF_OPT_GH_EXACT: c->gh_exact = value != 0; return 0;
        case TFF_OPT_SPILL: c->spill_only_if_needed = value != 0; return 0;
        case TFF_OPT_ROWS: if (value < 0 || value > 2) return fail(TFF_E_INVALID, "rows must be 0, 1 or 2"); c->rows = (int)value; return 0;
        case TFF_OPT_PRE: if (value < 0 || value > 2) return fail(TFF_E_INVALID, "pre must be 0, 1 or 2"); c->pre = (int)value; return 0;
        case TFF_OPT_COUNT_ROWS: c->count_rows = value != 0; return 0;
        case TFF_OPT_SCORE: if (value != 0 && value != 1) return fail(TFF_E_INVALID, "score must be 0 (count) or 1 (MSAC)"); c->score = (int)value; return 0;
        case TFF_OPT_BA_CLASSES: if (value < 0 || value > 2) return fail(TFF_E_INVALID, "ba_classes must be 0, 1 or 2"); c->ba_classes = (int)value; return 0;
        case TFF_OPT_DEBUG_FP_HANDOVER: c->dbg_fp_handover = value != 0; return 0;
        case TFF_OPT_DEBUG_ADAPTIVE: c->dbg_adaptive = value != 0; return 0;
        case TFF_OPT_KERNEL: if (value < 0 || value > 2) return fail(TFF_E_INVALID, "kernel must be 0, 1 or 2"); c->kernel_variant = (int)value; return 0;
        default: return fail(TFF_E_INVALID, "unknown option");
    }
}

int tff_ctx_synchronize(tff_ctx* c) {
    TFF_ENTER(c);
    TFF_HIP(hipSetDevice(c->device));
    TFF_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- the pose methods: _dev, _host and, where the header declares it, _debug_dev (need_dbg: a null debug buffer is refused) ------------------
#define TFF_POSE_PARAMS                                                                                                                     \
    const double *corresp, const double *calm, int64_t calm_stride, int64_t B, int32_t N, double *Rt2, double *Rt3, double *T, double *reconst, \
        int32_t *iter, int32_t *status
#define TFF_POSE_CALL(dbg) PoseCall{corresp, calm, calm_stride, B, N, Rt2, Rt3, T, reconst, iter, status, dbg}
#define TFF_POSE_METHOD(name, id)                                                                                               \
    int tff_##name##_pose_batch_dev(tff_ctx* c, TFF_POSE_PARAMS) { return pose_dev(c, id, TFF_POSE_CALL(nullptr)); }            \
    int tff_##name##_pose_batch_host(tff_ctx* c, TFF_POSE_PARAMS) { return pose_host(c, id, TFF_POSE_CALL(nullptr)); }
#define TFF_POSE_DEBUG(name, id, need_dbg)                                                       \
    int tff_##name##_pose_batch_debug_dev(tff_ctx* c, TFF_POSE_PARAMS, double* dbg) {            \
        if (need_dbg && !dbg) return fail(TFF_E_INVALID, "null debug buffer");                   \
        return pose_dev(c, id, TFF_POSE_CALL(dbg));                                              \
    }
TFF_POSE_METHOD(linear_tft, TFF_METHOD_LINEAR_TFT)
TFF_POSE_METHOD(ressl_tft, TFF_METHOD_RESSL_TFT)
TFF_POSE_METHOD(nordberg_tft, TFF_METHOD_NORDBERG_TFT)
TFF_POSE_METHOD(faugpapa_tft, TFF_METHOD_FAUGPAPA_TFT)
TFF_POSE_METHOD(pi, TFF_METHOD_PI)
TFF_POSE_METHOD(picol, TFF_METHOD_PICOL)
TFF_POSE_METHOD(linear_f, TFF_METHOD_LINEAR_F)
TFF_POSE_METHOD(optim_f, TFF_METHOD_OPTIM_F)
TFF_POSE_DEBUG(linear_tft, TFF_METHOD_LINEAR_TFT, true)
TFF_POSE_DEBUG(linear_f, TFF_METHOD_LINEAR_F, true)
TFF_POSE_DEBUG(ressl_tft, TFF_METHOD_RESSL_TFT, true)
TFF_POSE_DEBUG(nordberg_tft, TFF_METHOD_NORDBERG_TFT, false)
TFF_POSE_DEBUG(faugpapa_tft, TFF_METHOD_FAUGPAPA_TFT, false)

int tff_pi_pose_batch_debug_dev(tff_ctx* c, int32_t collinear, TFF_POSE_PARAMS, double* init_p, double* init_x) {
    TFF_ENTER(c);
    if ((init_p == nullptr) != (init_x == nullptr)) return fail(TFF_E_INVALID, "init_p and init_x come together");
    PoseCall p = TFF_POSE_CALL(nullptr);
    p.init_p = init_p; p.init_x = init_x;
    return pose_dev_locked(c, &METHODS[collinear ? TFF_METHOD_PICOL : TFF_METHOD_PI], p);
}

// Minimal-sample hypotheses (config 4): hypothesis b uses correspondences sample_idx[b*n .. b*n+n) of ONE shared scene.
static int pose_sampled_dev(tff_ctx* c, int32_t method, const double* scene, int32_t Ns, const double* calm, const int32_t* sample_idx, int64_t B, int32_t n,
                            double* Rt2, double* Rt3, double* T, int32_t* status) {
    TFF_ENTER(c);
    if (!sample_idx || Ns <= 0) return fail(TFF_E_INVALID, "null sample indices / empty scene");
    PoseCall p{scene, calm, 0, B, n, Rt2, Rt3, T, nullptr, nullptr, status, nullptr};
    p.sample_idx = sample_idx; p.sample_ns = Ns;
    return pose_dev_locked(c, &METHODS[method], p);
}
int tff_linear_tft_pose_sampled_dev(tff_ctx* c, const double* scene, int32_t Ns, const double* calm, const int32_t* sample_idx, int64_t B,
                                    int32_t n, double* Rt2, double* Rt3, double* T, int32_t* status) {
    return pose_sampled_dev(c, TFF_METHOD_LINEAR_TFT, scene, Ns, calm, sample_idx, B, n, Rt2, Rt3, T, status);
}
int tff_linear_f_pose_sampled_dev(tff_ctx* c, const double* scene, int32_t Ns, const double* calm, const int32_t* sample_idx, int64_t B,
                                  int32_t n, double* Rt2, double* Rt3, double* T, int32_t* status) {
    return pose_sampled_dev(c, TFF_METHOD_LINEAR_F, scene, Ns, calm, sample_idx, B, n, Rt2, Rt3, T, status);
}

int tff_pose_batch_ragged_dev(tff_ctx* c, int32_t method, const double* corresp, const int64_t* offsets, int32_t n_max, const double* calm,
                              int64_t calm_stride, int64_t B, double* Rt2, double* Rt3, double* T, double* reconst, int32_t* iter, int32_t* status) {
    TFF_ENTER(c);
    PoseCall p{corresp, calm, calm_stride, B, n_max, Rt2, Rt3, T, reconst, iter, status, nullptr};
    p.offsets = offsets;
    const RaggedRoute* route;
    TFF_TRY(check_ragged(c, method, p, &route));
    return run_pose(c, &p, true, [&] { return launch_ragged(c, *route, p); });
}

// host pointers: the offsets are checked here (TFF_E_INVALID before any work), the packed range offsets[0] .. offsets[B] goes over as one copy
int tff_pose_batch_ragged_host(tff_ctx* c, int32_t method, const double* corresp, const int64_t* offsets, const double* calm, int64_t calm_stride,
                               int64_t B, double* Rt2, double* Rt3, double* T, double* reconst, int32_t* iter, int32_t* status) {
    if (!offsets) return fail(TFF_E_INVALID, "null offsets");
    if (B < 0) return fail(TFF_E_INVALID, "negative batch size");
    int64_t n_max = 0;
    if (offsets[0] < 0) return fail(TFF_E_INVALID, "offsets[0] < 0");
    for (int64_t b = 0; b < B; ++b) {
        const int64_t n = offsets[b + 1] - offsets[b];
        if (n < 0) return fail(TFF_E_INVALID, "offsets must not decrease");
        if (n > n_max) n_max = n;
    }
    if (n_max > RAGGED_MAX_N) return fail(TFF_E_INVALID, "ragged batches: a triplet with more than 2^24 correspondences");
    TFF_ENTER(c);
    PoseCall h{corresp, calm, calm_stride, B, (int32_t)n_max, Rt2, Rt3, T, reconst, iter, status, nullptr};
    h.offsets = offsets;
    const RaggedRoute* route;
    TFF_TRY(check_ragged(c, method, h, &route));
    return run_pose(c, &h, false, [&] {
        return pose_via_staging(c, h, (size_t)offsets[0], (size_t)offsets[B], [&](const PoseCall& d) { return launch_ragged(c, *route, d); });
    });
}

// ---- matches with outliers: sampler, inlier flags, the robust estimator ------------------------------------------------------------------------
int tff_sample_indices_dev(tff_ctx* c, uint64_t seed, int64_t first, int64_t B, int32_t n, int32_t Ns, int32_t* sample_idx) {
    TFF_ENTER(c);
    if (n < 1 || n > tff::ROBUST_MAX_SAMPLE || Ns < n || B < 0 || first < 0) return fail(TFF_E_INVALID, "sample_indices: need 1 <= n <= 16, Ns >= n, B >= 0, first >= 0");
    return run_batch(c, B, sample_idx != nullptr, "null pointer", nullptr, [&] {
        return launch(c, tff::k_sample_indices, (unsigned)((B + 255) / 256), 256, 0, tff::SampleArgs{(unsigned long long)seed, (long)first, (long)B, n, Ns, sample_idx});
    });
}

int tff_inlier_mask_batch_dev(tff_ctx* c, const double* scene, int32_t Ns, const double* calm, const double* Rt2, const double* Rt3, int64_t B,
                              double threshold, uint8_t* mask, int32_t* counts) {
    TFF_ENTER(c);
    if (B < 0 || Ns < 0) return fail(TFF_E_INVALID, "negative size");
    return run_batch(c, B, scene && calm && Rt2 && Rt3 && mask, "null pointer", nullptr,
                     [&] {                                                   // one wavefront per hypothesis
                         return launch(c, tff::k_inlier_mask, tff::pose_grid(B), 64, 0, tff::InlierMaskArgs{scene, calm, Rt2, Rt3, (long)B, Ns, threshold, mask, counts});
                     });
}

// The two drivers of every robust entry point.  Device pointers: the checks, the rounds, an empty list (only now: S == 0 is no licence for bad arguments),
// the chain.  No synchronisation.
static int robust_dev(tff_ctx* c, ScenesCall q) {
    const RaggedRoute* route;
    RoundPlan plan;
    TFF_TRY(check_scenes(c, &q, false, &plan, &route));
    if (q.S == 0) return 0;
    TFF_HIP(hipSetDevice(c->device));
    return launch_robust_scenes(c, *route, q);
}
// Host pointers: the checks of robust_dev, a list's offsets among them (n_total and ns_max come from them); H2D, its chain, D2H, one synchronisation
static int robust_host(tff_ctx* c, ScenesCall h) {
    const int64_t S = h.S;
    const RaggedRoute* route;
    RoundPlan plan;
    TFF_TRY(check_scenes(c, &h, true, &plan, &route));
    if (S == 0) return 0;
    TFF_HIP(hipSetDevice(c->device));
    const int64_t n_total = h.n_total;
    const size_t nscene = (size_t)n_total * 6 * sizeof(double), ncal = (size_t)(h.calm_stride ? S : 1) * 27 * sizeof(double), nS = (size_t)S;
    TFF_TRY(c->in.reserve(nscene ? nscene : 8));
    TFF_TRY(c->calm.reserve(ncal));
    TFF_TRY(c->ragged_off.reserve((nS + 1) * sizeof(int64_t)));
    TFF_TRY(c->out.reserve(nS * 51 * sizeof(double) + (size_t)n_total + 8));
    TFF_TRY(c->idx.reserve(nS * 6 * sizeof(int32_t)));
    if (h.order) TFF_TRY(c->guided_order.reserve((size_t)(n_total ? n_total : 1) * sizeof(int32_t)));   // the guided form: the ranking's copy
    ScenesCall d = h;
    d.scenes = (const double*)c->in.p; d.calm = (const double*)c->calm.p; d.offsets = (const int64_t*)c->ragged_off.p;
    d.Rt2 = (double*)c->out.p; d.Rt3 = d.Rt2 + nS * 12; d.T = d.Rt3 + nS * 12; d.mask = (uint8_t*)(d.T + nS * 27);
    d.info = (int32_t*)c->idx.p; d.status = d.info + nS * 4; d.used = d.status + nS;
    if (nscene) TFF_HIP(hipMemcpyAsync(c->in.p, h.scenes, nscene, hipMemcpyHostToDevice, c->stream));
    TFF_HIP(hipMemcpyAsync(c->calm.p, h.calm, ncal, hipMemcpyHostToDevice, c->stream));
    TFF_HIP(hipMemcpyAsync(c->ragged_off.p, h.offsets, (nS + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (h.order) {                                                           // the guided form: the ranking travels like the scenes
        if (n_total) TFF_HIP(hipMemcpyAsync(c->guided_order.p, h.order, (size_t)n_total * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        d.order = (const int32_t*)c->guided_order.p;
        if (!h.plan) d.used = nullptr;                                       // (a fixed n_hyp: the caller's used, if any, is filled on the host, below)
    }
    TFF_TRY(launch_robust_scenes(c, *route, d));
    TFF_HIP(hipMemcpyAsync(h.Rt2, d.Rt2, nS * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipMemcpyAsync(h.Rt3, d.Rt3, nS * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipMemcpyAsync(h.T, d.T, nS * 27 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_total) TFF_HIP(hipMemcpyAsync(h.mask, d.mask, (size_t)n_total, hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipMemcpyAsync(h.info, d.info, nS * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipMemcpyAsync(h.status, d.status, nS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (h.plan) TFF_HIP(hipMemcpyAsync(h.used, d.used, nS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
// the one-scene forms: S = 1 with a shared CalM; offsets: none (_dev) or {0, Ns} on the host (_host)
int tff_robust_pose_dev(tff_ctx* c, int32_t method, const double* scene, int32_t Ns, const double* calm, uint64_t seed, int64_t n_hyp, int32_t n_sample,
                        double threshold, int32_t n_cand, int32_t lo_rounds, double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info,
                        int32_t* status) {
    TFF_ENTER(c);
    ScenesCall q{method, scene, nullptr, Ns, Ns, 1, calm, 0, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds, Rt2, Rt3, T, mask, info, status};
    q.one_scene = true;
    return robust_dev(c, q);
}
int tff_robust_pose_host(tff_ctx* c, int32_t method, const double* scene, int32_t Ns, const double* calm, uint64_t seed, int64_t n_hyp, int32_t n_sample,
                         double threshold, int32_t n_cand, int32_t lo_rounds, double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info,
                         int32_t* status) {
    TFF_ENTER(c);
    const int64_t offsets[2] = {0, Ns};
    ScenesCall q{method, scene, offsets, Ns, Ns, 1, calm, 0, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds, Rt2, Rt3, T, mask, info, status};
    q.one_scene = true;
    return robust_host(c, q);
}

int tff_robust_pose_scenes_dev(tff_ctx* c, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int32_t ns_max, int64_t S,
                               const double* calm, int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand,
                               int32_t lo_rounds, double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* status) {
    TFF_ENTER(c);
    return robust_dev(c, ScenesCall{method, scenes, scene_offsets, n_total, ns_max, S, calm, calm_stride, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds,
                                    Rt2, Rt3, T, mask, info, status});
}
int tff_robust_pose_scenes_host(tff_ctx* c, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t S, const double* calm,
                                int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand, int32_t lo_rounds,
                                double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* status) {
    TFF_ENTER(c);
    return robust_host(c, ScenesCall{method, scenes, scene_offsets, 0, 0, S, calm, calm_stride, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds,
                                     Rt2, Rt3, T, mask, info, status});
}

int tff_robust_round_plan(double confidence, int64_t n_hyp, int32_t first_round, int64_t* ends, double* qmin, int32_t* rounds) {
    if (!ends || !qmin || !rounds) return fail(TFF_E_INVALID, "null pointer");
    RoundPlan p;
    TFF_TRY(make_round_plan(confidence, n_hyp, first_round, &p));
    for (int r = 0; r < p.rounds; ++r) { ends[r] = p.ends[r]; qmin[r] = p.qmin[r]; }
    *rounds = p.rounds;
    return 0;
}

// the adaptive and the guided forms (include/tftfund_adaptive.h, include/tftfund_guided.h; kernels in robust_guided_kernel.h): the list's record plus the
// early stop (the guided forms: with a confidence other than 0; 0 is a fixed n_hyp, no rounds) and the ranking
int tff_robust_pose_scenes_adaptive_dev(tff_ctx* c, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int32_t ns_max,
                                        int64_t S, const double* calm, int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold,
                                        int32_t n_cand, int32_t lo_rounds, double confidence, int32_t first_round, double* Rt2, double* Rt3, double* T,
                                        uint8_t* mask, int32_t* info, int32_t* used, int32_t* status) {
    TFF_ENTER(c);
    ScenesCall q{method, scenes, scene_offsets, n_total, ns_max, S, calm, calm_stride, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds,
                 Rt2, Rt3, T, mask, info, status};
    q.rounds = true; q.confidence = confidence; q.first_round = first_round; q.used = used;
    return robust_dev(c, q);
}
int tff_robust_pose_scenes_adaptive_host(tff_ctx* c, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t S, const double* calm,
                                         int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand,
                                         int32_t lo_rounds, double confidence, int32_t first_round, double* Rt2, double* Rt3, double* T, uint8_t* mask,
                                         int32_t* info, int32_t* used, int32_t* status) {
    TFF_ENTER(c);
    ScenesCall q{method, scenes, scene_offsets, 0, 0, S, calm, calm_stride, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds,
                 Rt2, Rt3, T, mask, info, status};
    q.rounds = true; q.confidence = confidence; q.first_round = first_round; q.used = used;
    return robust_host(c, q);
}
int tff_robust_pose_scenes_guided_dev(tff_ctx* c, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int32_t ns_max,
                                      int64_t S, const double* calm, int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold,
                                      int32_t n_cand, int32_t lo_rounds, double confidence, int32_t first_round, const int32_t* order, int64_t growth,
                                      double* Rt2, double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* used, int32_t* status) {
    TFF_ENTER(c);
    ScenesCall q{method, scenes, scene_offsets, n_total, ns_max, S, calm, calm_stride, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds,
                 Rt2, Rt3, T, mask, info, status};
    q.rounds = confidence != 0.0; q.confidence = confidence; q.first_round = first_round;
    q.used = used;                                                           // (without rounds: null, or filled with n_hyp by launch_robust_scenes)
    q.guided = true; q.order = order; q.growth = growth;
    return robust_dev(c, q);
}
int tff_robust_pose_scenes_guided_host(tff_ctx* c, int32_t method, const double* scenes, const int64_t* scene_offsets, int64_t S, const double* calm,
                                       int64_t calm_stride, uint64_t seed, int64_t n_hyp, int32_t n_sample, double threshold, int32_t n_cand,
                                       int32_t lo_rounds, double confidence, int32_t first_round, const int32_t* order, int64_t growth, double* Rt2,
                                       double* Rt3, double* T, uint8_t* mask, int32_t* info, int32_t* used, int32_t* status) {
    TFF_ENTER(c);
    ScenesCall q{method, scenes, scene_offsets, 0, 0, S, calm, calm_stride, seed, n_hyp, n_sample, threshold, n_cand, lo_rounds,
                 Rt2, Rt3, T, mask, info, status};
    q.rounds = confidence != 0.0; q.confidence = confidence; q.first_round = first_round; q.used = used;
    q.guided = true; q.order = order; q.growth = growth;
    TFF_TRY(robust_host(c, q));
    if (confidence == 0.0 && used)                                           // a fixed n_hyp: documented as used[s] = n_hyp, and the call had no device copy of it
        for (int64_t s = 0; s < S; ++s) used[s] = (int32_t)n_hyp;
    return 0;
}
// the guided one-scene building block (include/tftfund_guided.h)
int tff_sample_indices_guided_dev(tff_ctx* c, uint64_t seed, int64_t first, int64_t B, int32_t n, int32_t Ns, const int32_t* order, int64_t growth,
                                  int32_t* sample_idx) {
    TFF_ENTER(c);
    TFF_TRY(check_guided(order, growth));
    if (n < 1 || n > tff::ROBUST_MAX_SAMPLE || Ns < n || Ns > RAGGED_MAX_N || B < 0 || first < 0)
        return fail(TFF_E_INVALID, "sample_indices_guided: need 1 <= n <= 16, n <= Ns <= 2^24, B >= 0, first >= 0");
    return run_batch(c, B, sample_idx != nullptr, "null pointer", nullptr, [&] {
        TFF_TRY(c->guided_ends.reserve((size_t)Ns * sizeof(int32_t)));      // (before the table's launch: nothing of this call is on the stream yet)
        int32_t* ends = (int32_t*)c->guided_ends.p;
        const tff::SceneSet one{nullptr, nullptr, 1, (long)Ns, Ns, n, nullptr, 0};
        TFF_TRY(launch(c, tff::k_guided_ends, 1, tff::GUIDED_ENDS_THREADS, 0, tff::GuidedEndsArgs{one, (long)growth, n, ends}));
        return launch(c, tff::k_sample_indices_guided, (unsigned)((B + 255) / 256), 256, 0,
                      tff::SampleGuidedArgs{tff::SampleArgs{(unsigned long long)seed, (long)first, (long)B, n, Ns, sample_idx}, ends, order});
    });
}

int tff_inlier_count_scenes_dev(tff_ctx* c, const double* scenes, const int64_t* scene_offsets, int64_t n_total, int64_t S, const double* calm,
                                int64_t calm_stride, const double* Rt2, const double* Rt3, int64_t per_scene, double threshold, int32_t* counts) {
    TFF_ENTER(c);
    if (S < 0 || per_scene < 0) return fail(TFF_E_INVALID, "negative size");
    if (n_total < 0 || n_total > (int64_t)INT32_MAX) return fail(TFF_E_INVALID, "inlier_count_scenes: n_total must be between 0 and 2^31 - 1");
    if (calm_stride != 0 && calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
    if (per_scene > 0 && S > (int64_t)INT32_MAX / per_scene) return fail(TFF_E_INVALID, "inlier_count_scenes: S * per_scene above 2^31 - 1");
    const int64_t B = S * per_scene;
    return run_batch(c, B, (scenes || n_total == 0) && scene_offsets && calm && Rt2 && Rt3 && counts, "null pointer", nullptr, [&] {
        const tff::SceneSet set{scenes, (const long*)scene_offsets, (long)S, (long)n_total, INT32_MAX, 0, calm, (long)calm_stride};
        return launch_count_scenes(c, set, Rt2, Rt3, 0, B, per_scene, threshold, counts);
    });
}


// ---------------------------------------------------------------------------------------------
// Building blocks (device pointers only)
// ---------------------------------------------------------------------------------------------
int tff_triangulate_batch_dev(tff_ctx* c, const double* cams, int64_t cam_stride, const double* pts, int64_t B, int32_t M,
                              int32_t N, double* X) {
    TFF_ENTER(c);
    if (B < 0 || N < 0 || (M != 2 && M != 3)) return fail(TFF_E_INVALID, "triangulate: M must be 2 or 3");    // triangulation3D.m:33,46
    if (cam_stride != 0 && cam_stride != 12 * M) return fail(TFF_E_INVALID, "cam_stride must be 0 or 12*M");
    return run_batch(c, N == 0 ? 0 : B, cams && pts && X, "null pointer", nullptr, [&] {
        tff::TriangulateArgs a{cams, (long)cam_stride, pts, (long)B, M, N, X};
        return launch(c, tff::k_triangulate, tff::pose_grid(B), 64, 0, a);
    });
}

int tff_repr_error_batch_dev(tff_ctx* c, const double* cams, int64_t cam_stride, const double* corresp, int64_t corresp_stride,
                             const double* pts3d, int64_t B, int32_t N, double* err) {
    TFF_ENTER(c);
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative size");
    if (cam_stride != 0 && cam_stride != 36) return fail(TFF_E_INVALID, "cam_stride must be 0 or 36");
    if (corresp_stride != 0 && corresp_stride != 6 * (int64_t)N) return fail(TFF_E_INVALID, "corresp_stride must be 0 or 6*N");
    return run_batch(c, B, cams && corresp && err, "null pointer", nullptr, [&] {
        tff::ReprErrorArgs a{cams, (long)cam_stride, nullptr, nullptr, nullptr, corresp, (long)corresp_stride, pts3d, (long)B, N, 0.0, err, nullptr};
        return launch(c, tff::k_repr_error, tff::pose_grid(B), 64, 0, a);
    });
}

int tff_inlier_count_batch_dev(tff_ctx* c, const double* scene, int32_t Ns, const double* calm, const double* Rt2, const double* Rt3,
                               int64_t B, double threshold, int32_t* counts, double* err) {
    TFF_ENTER(c);
    if (B < 0 || Ns < 0) return fail(TFF_E_INVALID, "negative size");
    return run_batch(c, B, scene && calm && Rt2 && Rt3 && counts, "null pointer", nullptr,
                     [&] { return launch_inlier_count(c, scene, Ns, calm, Rt2, Rt3, B, threshold, counts, err); });
}

int tff_transform_tft_batch_dev(tff_ctx* c, const double* T, const double* M1, const double* M2, const double* M3, int64_t m_stride,
                                int64_t B, int32_t inverse, double* Tout) {
    TFF_ENTER(c);
    if (B < 0 || (m_stride != 0 && m_stride != 9) || (inverse != 0 && inverse != 1)) return fail(TFF_E_INVALID, "bad argument");
    return run_batch(c, B, T && M1 && M2 && M3 && Tout, "null pointer", nullptr, [&] {
        tff::TransformArgs a{T, M1, M2, M3, (long)m_stride, (long)B, inverse, Tout};
        return launch(c, tff::k_transform_tft, tff::pose_grid(B), 64, 0, a);
    });
}

int tff_rt_from_tft_batch_dev(tff_ctx* c, const double* T, const double* calm, int64_t calm_stride, const double* corresp, int64_t B,
                              int32_t N, double* Rt2, double* Rt3, int32_t* status) {
    TFF_ENTER(c);
    TFF_TRY(check_common(corresp, calm, calm_stride, B, N));
    return run_batch(c, B, T && Rt2 && Rt3, "null pointer", nullptr, [&] {
        tff::RtFromTftArgs a{T, calm, (long)calm_stride, corresp, (long)B, N, Rt2, Rt3, status};
        return launch(c, tff::k_rt_from_tft, tff::pose_grid(B), 64, tff::pose_lds_bytes(N, 0, false), a);
    });
}

int tff_linear_tft_batch_dev(tff_ctx* c, const double* corresp, int64_t B, int32_t N, double* T, double* P2, double* P3,
                             int32_t* status) {
    TFF_ENTER(c);
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative size");
    return run_batch(c, B, corresp && T && (P2 == nullptr) == (P3 == nullptr), "null pointer (P2 and P3 come together)", &status, [&] {
        tff::LinearTftOnlyArgs a{corresp, (long)B, N, 0, T, P2, P3, status};
        return launch_fast_exact(c, tff::k_linear_tft<false>, tff::k_linear_tft<true>, fast_tiers(c, N), a,
                                 [&](bool exact, tff::LinearTftOnlyArgs*, unsigned*, size_t* lds) { *lds = tff::pose_lds_bytes(N, 0, exact); return 0; });
    });
}

}  // extern "C"

namespace {

// ---- bundle adjustment ------------------------------------------------------------------------------------------------------------------------
static_assert(TFF_LOSS_NONE == tff::BA_LOSS_NONE && TFF_LOSS_HUBER == tff::BA_LOSS_HUBER && TFF_LOSS_CAUCHY == tff::BA_LOSS_CAUCHY, "loss codes");
int check_loss(int32_t loss, double scale) {
    if (loss != TFF_LOSS_NONE && loss != TFF_LOSS_HUBER && loss != TFF_LOSS_CAUCHY) return fail(TFF_E_INVALID, "loss must be TFF_LOSS_NONE, TFF_LOSS_HUBER or TFF_LOSS_CAUCHY");
    if (loss != TFF_LOSS_NONE && !(scale > 0.0 && std::isfinite(scale))) return fail(TFF_E_INVALID, "the scale of a loss must be a positive finite number");
    return 0;
}
// the instance of k_bundle_adjust_loss for a loss other than TFF_LOSS_NONE (that one is k_bundle_adjust itself)
int launch_ba_loss(tff_ctx* c, int32_t loss, unsigned grid, size_t lds, const tff::BaLossArgs& a) {
    return loss == TFF_LOSS_HUBER ? launch(c, tff::k_bundle_adjust_loss<tff::BA_LOSS_HUBER>, grid, 64, lds, a)
                                  : launch(c, tff::k_bundle_adjust_loss<tff::BA_LOSS_CAUCHY>, grid, 64, lds, a);
}
int launch_bundle_adjust(tff_ctx* c, const tff::BaArgs& a, int32_t loss = TFF_LOSS_NONE, double scale = 0.0, double* weight = nullptr) {
    if (a.N < 1) return fail(TFF_E_INVALID, "bundle adjustment needs at least one correspondence");
    if (loss == TFF_LOSS_NONE) {
        TFF_TRY(launch(c, tff::k_bundle_adjust, tff::pose_grid(a.B), 64, tff::ba_lds_bytes(a.N), a));
        if (!weight) return 0;
        const long blocks = (a.B * (long)a.N + 255) / 256;
        return launch(c, tff::k_ba_weight_ones, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, tff::BaOnesArgs{weight, a.status, a.B, a.N});
    }
    tff::BaLossArgs la;
    static_cast<tff::BaArgs&>(la) = a;
    la.scale = scale; la.weight = weight;
    return launch_ba_loss(c, loss, tff::pose_grid(a.B), tff::ba_lds_bytes(a.N), la);
}
// ---- ragged, masked bundle adjustment (tff_bundle_adjust_ragged_*; the chain is described in ba_ragged_kernel.h) -------------------------------
static_assert(TFF_BA_MAX_N == tff::BA_CLASS_BOUND_2 && tff::ba_lds_bytes(TFF_BA_MAX_N) <= LDS_LIMIT && tff::ba_lds_bytes(TFF_BA_MAX_N + 1) > LDS_LIMIT,
              "TFF_BA_MAX_N is the largest N whose ba_lds_bytes(N) fits the 160 KiB of LDS");
static_assert(0 < tff::BA_CLASS_BOUND_0 && tff::BA_CLASS_BOUND_0 < tff::BA_CLASS_BOUND_1 && tff::BA_CLASS_BOUND_1 < tff::BA_CLASS_BOUND_2, "three classes");
static_assert(TFF_ST_TOO_LARGE == tff::ST_TOO_LARGE && TFF_ST_BAD_OFFSETS == tff::ST_BAD_OFFSETS, "status codes");
// the upper classes hold one or two wavefronts per CU: a grid of this many blocks walks their lists with a stride
constexpr long BA_UPPER_CLASS_GRID = 8192;
constexpr long BA_ONE_CLASS_MAX_B = 256;   // the CUs of an MI355X

struct BaRaggedCall {                      // device pointers
    const double* corresp; const int64_t* offsets; int64_t n_total; const uint8_t* mask; const double* calm; int64_t calm_stride;
    const double* Rt2_in; const double* Rt3_in; const double* reconst0; int64_t B;
    double* Rt2; double* Rt3; double* reconst; int32_t* iter; double* repr_err; int32_t* used; int32_t* status;
    int32_t loss = TFF_LOSS_NONE; double scale = 0.0; double* weight = nullptr;      // tff_bundle_adjust_loss_ragged_*
};
int check_ba_ragged(const void* corresp, const void* offsets, int64_t n_total, const void* calm, int64_t calm_stride, const void* Rt2_in, const void* Rt3_in,
                    int64_t B, const void* Rt2, const void* Rt3) {
    if (B < 0) return fail(TFF_E_INVALID, "negative batch size");
    if (n_total < 0 || n_total > (int64_t)INT32_MAX) return fail(TFF_E_INVALID, "n_total must lie in [0, 2^31 - 1]");
    if (calm_stride != 0 && calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
    if (B > 0 && (!offsets || !calm || !Rt2_in || !Rt3_in || !Rt2 || !Rt3 || (n_total > 0 && !corresp))) return fail(TFF_E_INVALID, "null pointer");
    return 0;
}
int launch_ba_ragged(tff_ctx* c, const BaRaggedCall& q) {
    const size_t B = (size_t)q.B, nt = (size_t)q.n_total;
    // the plan: coff (B int64) | m (B) | class lists (3 B) | class counts (3);  a masked call: packed (6) | rec0 (3) | rec_ws (3 doubles) | src (int32) per correspondence
    TFF_TRY(c->ba_plan.reserve(B * sizeof(int64_t) + (4 * B + tff::BA_CLASSES) * sizeof(int32_t)));
    // ... and, with a loss and a weight output, the compact weights (1 double)
    const bool compact_w = q.mask && q.weight && q.loss != TFF_LOSS_NONE;
    if (q.mask) TFF_TRY(c->ba_pack.reserve(nt * ((compact_w ? 13 : 12) * sizeof(double) + sizeof(int32_t)) + 8));
    tff::BaRaggedPlan p{};
    p.offsets = (const long*)q.offsets; p.B = (long)q.B; p.n_total = (long)q.n_total; p.mask = q.mask;
    // A launch lasts as long as its slowest item and the class launches follow one another on the stream, so classes pay only where a single launch
    // would leave items waiting for a CU.  Up to BA_ONE_CLASS_MAX_B items are all resident at once even at one wavefront per CU: one launch, sized for
    // TFF_BA_MAX_N (measured on the fountain and Herz-Jesu lists: 1.5 times faster than three).  B is a host value: no synchronisation.
    const bool one_class = c->ba_classes == 1 || (c->ba_classes == 0 && q.B <= BA_ONE_CLASS_MAX_B);
    p.bound[0] = one_class ? TFF_BA_MAX_N : tff::BA_CLASS_BOUND_0;
    p.bound[1] = one_class ? TFF_BA_MAX_N : tff::BA_CLASS_BOUND_1;
    p.bound[2] = TFF_BA_MAX_N;
    p.coff = (long*)c->ba_plan.p;
    p.m = (int*)(p.coff + B);
    p.cls_list = p.m + B;
    p.cls_count = p.cls_list + tff::BA_CLASSES * B;
    p.corresp = q.corresp; p.reconst0 = q.reconst0;
    double* rec_ws = nullptr;
    double* w_ws = nullptr;
    if (q.mask) {
        p.packed = (double*)c->ba_pack.p;
        p.rec0 = p.packed + 6 * nt;
        rec_ws = p.rec0 + 3 * nt;
        if (compact_w) w_ws = rec_ws + 3 * nt;
        p.src = (int*)(rec_ws + (compact_w ? 4 : 3) * nt);
    }
    p.rec_ws = rec_ws;
    p.Rt2 = q.Rt2; p.Rt3 = q.Rt3; p.reconst = q.reconst; p.iter = q.iter; p.repr_err = q.repr_err; p.used = q.used; p.status = q.status;
    TFF_HIP(hipMemsetAsync(p.cls_count, 0, tff::BA_CLASSES * sizeof(int32_t), c->stream));
    const unsigned per_item = (unsigned)(q.B < (1L << 20) ? q.B : (1L << 20)), per_thread = (unsigned)((q.B + 255) / 256);
    TFF_TRY(launch(c, tff::k_ba_ragged_count, per_item, 64, 0, p));
    if (q.mask) TFF_TRY(launch(c, tff::k_ba_ragged_scan, 1, tff::BA_RAGGED_SCAN_THREADS, 0, p));
    TFF_TRY(launch(c, tff::k_ba_ragged_classes, per_thread, 256, 0, p));
    if (q.mask) TFF_TRY(launch(c, tff::k_ba_ragged_compact, per_item, tff::BA_RAGGED_TILE, 0, p));
    for (int k = 0; k < tff::BA_CLASSES; ++k) {
        if (k > 0 && p.bound[k] == p.bound[k - 1]) continue;                 // (an empty class: the one-class plan)
        const tff::BaArgs a = tff::ba_ragged_class_args(p, q.calm, (long)q.calm_stride, q.Rt2_in, q.Rt3_in, rec_ws, k);
        const long grid = (k == 0 || q.B < BA_UPPER_CLASS_GRID) ? (long)tff::pose_grid(q.B) : BA_UPPER_CLASS_GRID;
        if (q.loss == TFF_LOSS_NONE) TFF_TRY(launch(c, tff::k_bundle_adjust, (unsigned)grid, 64, tff::ba_lds_bytes(p.bound[k]), a));
        else TFF_TRY(launch_ba_loss(c, q.loss, (unsigned)grid, tff::ba_lds_bytes(p.bound[k]),
                                    tff::ba_ragged_class_loss_args(p, q.calm, (long)q.calm_stride, q.Rt2_in, q.Rt3_in, rec_ws, k, q.scale, w_ws, q.weight)));
    }
    if (q.reconst) TFF_TRY(launch(c, tff::k_ba_ragged_scatter, per_item, tff::BA_RAGGED_TILE, 0, p));
    if (q.weight) TFF_TRY(launch(c, tff::k_ba_ragged_weight, per_item, tff::BA_RAGGED_TILE, 0, tff::BaRaggedWeights{p, w_ws, q.weight, q.loss == TFF_LOSS_NONE}));
    return 0;
}

// ---- covariance of the bundle adjustment (tff_ba_covariance_*, tff_bundle_adjust_cov_*; include/tftfund_cov.h, csrc/ba_cov_kernel.h) ----------------
static_assert(tff::ba_cov_lds_bytes() <= 64 * 1024, "k_ba_cov's LDS does not grow with N");
int launch_ba_cov_kernel(tff_ctx* c, int32_t loss, unsigned grid, const tff::BaCovArgs& a) {
    constexpr size_t lds = tff::ba_cov_lds_bytes();
    if (loss == TFF_LOSS_NONE) return launch(c, tff::k_ba_cov<tff::BA_LOSS_NONE>, grid, 64, lds, a);
    return loss == TFF_LOSS_HUBER ? launch(c, tff::k_ba_cov<tff::BA_LOSS_HUBER>, grid, 64, lds, a) : launch(c, tff::k_ba_cov<tff::BA_LOSS_CAUCHY>, grid, 64, lds, a);
}
int check_ba_cov(const void* reconst, const void* cov, const void* sigma0, int64_t B) {
    if (B > 0 && (!reconst || !cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs reconst, cov and sigma0");
    return 0;
}
int launch_ba_cov(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2, const double* Rt3, const double* corresp, int64_t B, int32_t N,
                  const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov) {
    return launch_ba_cov_kernel(c, loss, tff::pose_grid(B), tff::BaCovArgs{calm, (long)calm_stride, Rt2, Rt3, corresp, (long)B, N, reconst, scale, cov, sigma0, point_cov});
}
struct BaCovRaggedCall {                   // device pointers
    const double* corresp; const int64_t* offsets; int64_t n_total; const uint8_t* mask; const double* calm; int64_t calm_stride;
    const double* Rt2; const double* Rt3; const double* reconst; int64_t B; int32_t loss; double scale;
    double* cov; double* sigma0; double* point_cov;
};
// The selection is that of launch_ba_ragged -- its count, scan and compact kernels on a plan of this call's own --; there are no classes (one launch, one
// LDS size) and no largest m.  What those kernels write for an item that fails (poses, status) goes to the plan's workspace.
int launch_ba_cov_ragged(tff_ctx* c, const BaCovRaggedCall& q) {
    const size_t B = (size_t)q.B, nt = (size_t)q.n_total;
    // the plan: coff (B int64) | the poses of a failed item (24 B doubles) | m (B) | status (B);  a masked call: packed (6) | points (3) | point_cov (6 doubles) | src (int32) per correspondence
    TFF_TRY(c->cov_plan.reserve(B * (sizeof(int64_t) + 24 * sizeof(double) + 2 * sizeof(int32_t)) + 8));
    if (q.mask) TFF_TRY(c->cov_pack.reserve(nt * ((q.point_cov ? 15 : 9) * sizeof(double) + sizeof(int32_t)) + 8));
    tff::BaRaggedPlan p{};
    p.offsets = (const long*)q.offsets; p.B = (long)q.B; p.n_total = (long)q.n_total; p.mask = q.mask;
    p.bound[0] = p.bound[1] = p.bound[2] = INT32_MAX;
    p.coff = (long*)c->cov_plan.p;
    p.Rt2 = (double*)(p.coff + B); p.Rt3 = p.Rt2 + 12 * B;
    p.m = (int*)(p.Rt3 + 12 * B);
    p.status = p.m + B;
    p.corresp = q.corresp; p.reconst0 = q.reconst;
    double* pc_ws = nullptr;
    if (q.mask) {
        p.packed = (double*)c->cov_pack.p;
        p.rec0 = p.packed + 6 * nt;
        if (q.point_cov) pc_ws = p.rec0 + 3 * nt;
        p.src = (int*)(p.rec0 + (q.point_cov ? 9 : 3) * nt);
    }
    const unsigned per_item = (unsigned)(q.B < (1L << 20) ? q.B : (1L << 20));
    TFF_HIP(hipMemsetAsync(p.status, 0, B * sizeof(int32_t), c->stream));
    TFF_TRY(launch(c, tff::k_ba_ragged_count, per_item, 64, 0, p));
    if (q.mask) {
        TFF_TRY(launch(c, tff::k_ba_ragged_scan, 1, tff::BA_RAGGED_SCAN_THREADS, 0, p));
        TFF_TRY(launch(c, tff::k_ba_ragged_compact, per_item, tff::BA_RAGGED_TILE, 0, p));
    }
    TFF_TRY(launch_ba_cov_kernel(c, q.loss, tff::pose_grid(q.B), tff::ba_cov_ragged_args(p, q.calm, (long)q.calm_stride, q.Rt2, q.Rt3, q.scale, q.cov, q.sigma0, pc_ws, q.point_cov)));
    if (q.point_cov) TFF_TRY(launch(c, tff::k_ba_cov_scatter, per_item, tff::BA_RAGGED_TILE, 0, tff::BaCovScatter{p, pc_ws, q.point_cov}));
    return 0;
}
// the offsets of a ragged _host call, as tff_bundle_adjust_loss_ragged_host checks them
int check_host_offsets(const int64_t* offsets, int64_t B) {
    if (B < 0) return fail(TFF_E_INVALID, "negative batch size");
    if (B > 0 && !offsets) return fail(TFF_E_INVALID, "null pointer");
    if (B > 0 && offsets[0] < 0) return fail(TFF_E_INVALID, "offsets[0] must be >= 0");
    for (int64_t b = 0; b < B; ++b) if (offsets[b + 1] < offsets[b]) return fail(TFF_E_INVALID, "offsets must not decrease");
    return 0;
}

// BundleAdjustment as the reference writes it, M = 2 .. 6 views, MATLAB's own array layouts (csrc/ba_views_kernel.h)
template <int M>
int launch_bundle_adjust_views(tff_ctx* c, const tff::BavArgs& a) {
    return launch(c, tff::k_bundle_adjust_views<M>, tff::pose_grid(a.B), 64, tff::bav_lds_bytes<M>(a.N), a);
}
int launch_bundle_adjust_views(tff_ctx* c, int32_t M, const tff::BavArgs& a) {
    switch (M) {
        case 2: return launch_bundle_adjust_views<2>(c, a);
        case 3: return launch_bundle_adjust_views<3>(c, a);
        case 4: return launch_bundle_adjust_views<4>(c, a);
        case 5: return launch_bundle_adjust_views<5>(c, a);
        default: return launch_bundle_adjust_views<6>(c, a);
    }
}
// ... over tracks: a non-finite observation is a point not seen in that view (csrc/ba_tracks_kernel.h, include/tftfund_tracks.h)
template <int M>
int launch_bundle_adjust_tracks(tff_ctx* c, const tff::BatArgs& a) {
    return launch(c, tff::k_bundle_adjust_tracks<M>, tff::pose_grid(a.v.B), 64, tff::bav_lds_bytes<M>(a.v.N), a);
}
int launch_bundle_adjust_tracks(tff_ctx* c, int32_t M, const tff::BatArgs& a) {
    switch (M) {
        case 2: return launch_bundle_adjust_tracks<2>(c, a);
        case 3: return launch_bundle_adjust_tracks<3>(c, a);
        case 4: return launch_bundle_adjust_tracks<4>(c, a);
        case 5: return launch_bundle_adjust_tracks<5>(c, a);
        default: return launch_bundle_adjust_tracks<6>(c, a);
    }
}
// ... with a robust loss per observation (csrc/ba_tracks_loss_kernel.h, include/tftfund_tracks_loss.h).  TFF_LOSS_NONE is the plain call, the same kernel
// instance, and a small kernel of its own for the weights.
template <int M>
int launch_bundle_adjust_tracks_loss(tff_ctx* c, int32_t loss, const tff::BatLossArgs& a) {
    const unsigned grid = tff::pose_grid(a.t.v.B);
    const size_t lds = tff::bav_lds_bytes<M>(a.t.v.N);
    return loss == TFF_LOSS_HUBER ? launch(c, tff::k_bundle_adjust_tracks_loss<M, tff::BA_LOSS_HUBER>, grid, 64, lds, a)
                                  : launch(c, tff::k_bundle_adjust_tracks_loss<M, tff::BA_LOSS_CAUCHY>, grid, 64, lds, a);
}
int launch_bundle_adjust_tracks_loss(tff_ctx* c, int32_t M, tff::BatArgs a, int32_t loss, double scale, double* weight) {
    if (loss == TFF_LOSS_NONE) {
        if (weight && !a.v.status) {                                         // the weights of an item that failed are NaN: its status is needed
            TFF_TRY(c->tracks_status.reserve((size_t)a.v.B * sizeof(int32_t) + 8));
            a.v.status = (int*)c->tracks_status.p;
        }
        TFF_TRY(launch_bundle_adjust_tracks(c, M, a));
        if (!weight) return 0;
        const long blocks = (a.v.B * (long)a.v.N + 255) / 256;
        return launch(c, tff::k_bat_weight_ones, (unsigned)(blocks < 4096 ? blocks : 4096), 256, 0, tff::BatOnesArgs{weight, a.v.corresp, a.v.status, a.v.B, a.v.N, M});
    }
    const tff::BatLossArgs la{a, scale, weight};
    switch (M) {
        case 2: return launch_bundle_adjust_tracks_loss<2>(c, loss, la);
        case 3: return launch_bundle_adjust_tracks_loss<3>(c, loss, la);
        case 4: return launch_bundle_adjust_tracks_loss<4>(c, loss, la);
        case 5: return launch_bundle_adjust_tracks_loss<5>(c, loss, la);
        default: return launch_bundle_adjust_tracks_loss<6>(c, loss, la);
    }
}
// ... and its covariance at given poses and points (csrc/ba_tracks_cov_kernel.h, include/tftfund_tracks_cov.h): fifteen instances, M x loss; the LDS does not
// grow with N, so there are no launch classes
static_assert(tff::batc_lds_bytes<tff::BAV_MAX_VIEWS>() <= 64 * 1024, "k_ba_tracks_cov's LDS does not grow with N");
template <int M>
int launch_ba_tracks_cov(tff_ctx* c, int32_t loss, const tff::BatCovArgs& a) {
    const unsigned grid = tff::pose_grid(a.B);
    constexpr size_t lds = tff::batc_lds_bytes<M>();
    if (loss == TFF_LOSS_NONE) return launch(c, tff::k_ba_tracks_cov<M, tff::BA_LOSS_NONE>, grid, 64, lds, a);
    return loss == TFF_LOSS_HUBER ? launch(c, tff::k_ba_tracks_cov<M, tff::BA_LOSS_HUBER>, grid, 64, lds, a)
                                  : launch(c, tff::k_ba_tracks_cov<M, tff::BA_LOSS_CAUCHY>, grid, 64, lds, a);
}
int launch_ba_tracks_cov(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt, const double* corresp, int64_t B, int32_t N,
                         const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov) {
    TFF_TRY(c->tracks_cov_x.reserve((size_t)B * 3 * (size_t)N * sizeof(double) + 8));
    const tff::BatCovArgs a{calm, (long)calm_stride, Rt, corresp, (long)B, N, reconst, scale, (double*)c->tracks_cov_x.p, cov, sigma0, point_cov};
    switch (M) {
        case 2: return launch_ba_tracks_cov<2>(c, loss, a);
        case 3: return launch_ba_tracks_cov<3>(c, loss, a);
        case 4: return launch_ba_tracks_cov<4>(c, loss, a);
        case 5: return launch_ba_tracks_cov<5>(c, loss, a);
        default: return launch_ba_tracks_cov<6>(c, loss, a);
    }
}
int check_views(int32_t M, const void* calm, int64_t calm_stride, const void* Rt_in, const void* corresp, int64_t B, int32_t N, const void* Rt) {
    if (M < tff::BAV_MIN_VIEWS || M > tff::BAV_MAX_VIEWS) return fail(TFF_E_INVALID, "bundle adjustment takes 2 .. 6 views");
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative batch or correspondence count");
    if (B > 0 && (!corresp || !calm || !Rt_in || !Rt)) return fail(TFF_E_INVALID, "null pointer");
    if (calm_stride != 0 && calm_stride != 9 * (int64_t)M) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 9 M");
    if (B > 0 && N < 1) return fail(TFF_E_INVALID, "bundle adjustment needs at least one correspondence");
    return 0;
}
// what the two bundle-adjustment host calls share: the context's staging buffers cut into the inputs (corresp | reconst0 | npose bytes of
// poses; calm apart), the outputs (npose bytes of poses | reconst | repr_err) and iter | status, with the copies both calls make
struct BaStaging {
    double *corresp, *reconst0, *poses_in, *calm, *poses_out, *reconst, *repr_err;
    int32_t *iter, *status;
};
int ba_stage_in(tff_ctx* c, size_t B, size_t nin, size_t npt, size_t npose, size_t ncal, const double* corresp, const double* reconst0, BaStaging* s) {
    TFF_TRY(c->in.reserve(nin + npt + npose));
    TFF_TRY(c->calm.reserve(ncal));
    TFF_TRY(c->out.reserve(npose + npt + B * sizeof(double)));
    TFF_TRY(c->idx.reserve(B * 2 * sizeof(int32_t)));
    char* din = (char*)c->in.p;
    char* dout = (char*)c->out.p;
    *s = BaStaging{(double*)din, (double*)(din + nin), (double*)(din + nin + npt), (double*)c->calm.p,
                   (double*)dout, (double*)(dout + npose), (double*)(dout + npose + npt), (int32_t*)c->idx.p, (int32_t*)c->idx.p + B};
    TFF_HIP(hipMemcpyAsync(s->corresp, corresp, nin, hipMemcpyHostToDevice, c->stream));
    if (reconst0) TFF_HIP(hipMemcpyAsync(s->reconst0, reconst0, npt, hipMemcpyHostToDevice, c->stream));
    else s->reconst0 = nullptr;
    return 0;
}
int ba_stage_out(tff_ctx* c, size_t B, size_t npt, const BaStaging& s, double* reconst, int32_t* iter, double* repr_err, int32_t* status) {
    if (reconst) TFF_HIP(hipMemcpyAsync(reconst, s.reconst, npt, hipMemcpyDeviceToHost, c->stream));
    if (iter) TFF_HIP(hipMemcpyAsync(iter, s.iter, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (repr_err) TFF_HIP(hipMemcpyAsync(repr_err, s.repr_err, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status) TFF_HIP(hipMemcpyAsync(status, s.status, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    TFF_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

extern "C" {

// BundleAdjustment for three views: refines (R_t_2, R_t_3) and the points
int tff_bundle_adjust_batch_dev(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3,
                                double* reconst, int32_t* iter, double* repr_err, int32_t* status) {
    return tff_bundle_adjust_loss_batch_dev(c, calm, calm_stride, Rt2_in, Rt3_in, corresp, B, N, reconst0, Rt2, Rt3, reconst, iter, repr_err, status, TFF_LOSS_NONE, 0.0,
                                            nullptr);
}
// ... with a robust loss and the weights (include/tftfund_loss.h); TFF_LOSS_NONE is the call above
int tff_bundle_adjust_loss_batch_dev(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                     const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3,
                                     double* reconst, int32_t* iter, double* repr_err, int32_t* status, int32_t loss, double scale, double* weight) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_common(corresp, calm, calm_stride, B, N));
    return run_batch(c, B, Rt2_in && Rt3_in && Rt2 && Rt3, "null pose pointer", nullptr, [&] {
        return launch_bundle_adjust(c, tff::BaArgs{calm, (long)calm_stride, Rt2_in, Rt3_in, corresp, (long)B, N, reconst0, Rt2, Rt3, reconst, iter, repr_err, status},
                                    loss, scale, weight);
    });
}

// host-pointer variant: H2D, launch, D2H, synchronise (what the MEX shim calls)
int tff_bundle_adjust_batch_host(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                 const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3,
                                 double* reconst, int32_t* iter, double* repr_err, int32_t* status) {
    return tff_bundle_adjust_loss_batch_host(c, calm, calm_stride, Rt2_in, Rt3_in, corresp, B, N, reconst0, Rt2, Rt3, reconst, iter, repr_err, status, TFF_LOSS_NONE, 0.0,
                                             nullptr);
}
int tff_bundle_adjust_loss_batch_host(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in,
                                      const double* corresp, int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3,
                                      double* reconst, int32_t* iter, double* repr_err, int32_t* status, int32_t loss, double scale, double* weight) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_common(corresp, calm, calm_stride, B, N));
    return run_batch(c, B, Rt2_in && Rt3_in && Rt2 && Rt3, "null pose pointer", nullptr, [&] {
        const size_t nin = (size_t)B * 6 * (size_t)N * sizeof(double), npt = (size_t)B * 3 * (size_t)N * sizeof(double);
        const size_t ncal = (calm_stride ? (size_t)B : 1) * 27 * sizeof(double), npose = (size_t)B * 12 * sizeof(double);
        BaStaging s;
        TFF_TRY(ba_stage_in(c, (size_t)B, nin, npt, 2 * npose, ncal, corresp, reconst0, &s));
        double* d_r3 = s.poses_in + (size_t)B * 12;
        double* d_o3 = s.poses_out + (size_t)B * 12;
        TFF_HIP(hipMemcpyAsync(s.poses_in, Rt2_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r3, Rt3_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(s.calm, calm, ncal, hipMemcpyHostToDevice, c->stream));
        const size_t nw = (size_t)B * (size_t)N * sizeof(double);
        if (weight) TFF_TRY(c->ba_weight.reserve(nw));
        TFF_TRY(launch_bundle_adjust(c, tff::BaArgs{s.calm, (long)calm_stride, s.poses_in, d_r3, s.corresp, (long)B, N, s.reconst0, s.poses_out, d_o3, s.reconst,
                                                    s.iter, s.repr_err, s.status}, loss, scale, weight ? (double*)c->ba_weight.p : nullptr));
        if (weight) TFF_HIP(hipMemcpyAsync(weight, c->ba_weight.p, nw, hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(Rt2, s.poses_out, npose, hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(Rt3, d_o3, npose, hipMemcpyDeviceToHost, c->stream));
        return ba_stage_out(c, (size_t)B, npt, s, reconst, iter, repr_err, status);
    });
}

// BundleAdjustment for a packed batch of items with different correspondence counts, optionally thinned by a mask (launch_ba_ragged above)
int tff_bundle_adjust_ragged_dev(tff_ctx* c, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                 int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2, double* Rt3,
                                 double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status) {
    return tff_bundle_adjust_loss_ragged_dev(c, corresp, offsets, n_total, mask, calm, calm_stride, Rt2_in, Rt3_in, reconst0, B, Rt2, Rt3, reconst, iter, repr_err, used,
                                             status, TFF_LOSS_NONE, 0.0, nullptr);
}
int tff_bundle_adjust_loss_ragged_dev(tff_ctx* c, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                      int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2, double* Rt3,
                                      double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss, double scale,
                                      double* weight) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_ba_ragged(corresp, offsets, n_total, calm, calm_stride, Rt2_in, Rt3_in, B, Rt2, Rt3));
    return run_batch(c, B, true, nullptr, &status, [&] {
        return launch_ba_ragged(c, BaRaggedCall{corresp, offsets, n_total, mask, calm, calm_stride, Rt2_in, Rt3_in, reconst0, B, Rt2, Rt3, reconst, iter, repr_err,
                                                used, status, loss, scale, weight});
    });
}
int tff_bundle_adjust_ragged_host(tff_ctx* c, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm, int64_t calm_stride,
                                  const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2, double* Rt3, double* reconst,
                                  int32_t* iter, double* repr_err, int32_t* used, int32_t* status) {
    return tff_bundle_adjust_loss_ragged_host(c, corresp, offsets, mask, calm, calm_stride, Rt2_in, Rt3_in, reconst0, B, Rt2, Rt3, reconst, iter, repr_err, used, status,
                                              TFF_LOSS_NONE, 0.0, nullptr);
}
int tff_bundle_adjust_loss_ragged_host(tff_ctx* c, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm, int64_t calm_stride,
                                       const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2, double* Rt3, double* reconst,
                                       int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss, double scale, double* weight) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    if (B < 0) return fail(TFF_E_INVALID, "negative batch size");
    if (B > 0 && !offsets) return fail(TFF_E_INVALID, "null pointer");
    if (B > 0 && offsets[0] < 0) return fail(TFF_E_INVALID, "offsets[0] must be >= 0");
    for (int64_t b = 0; b < B; ++b) if (offsets[b + 1] < offsets[b]) return fail(TFF_E_INVALID, "offsets must not decrease");
    const int64_t first = B > 0 ? offsets[0] : 0, n_total = B > 0 ? offsets[B] : 0;
    TFF_TRY(check_ba_ragged(corresp, offsets, n_total, calm, calm_stride, Rt2_in, Rt3_in, B, Rt2, Rt3));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        const size_t nb = (size_t)B, nt = (size_t)n_total, f = (size_t)first, cnt = nt - f;
        const size_t nin = nt * 6 * sizeof(double), npt = nt * 3 * sizeof(double), npose = nb * 12 * sizeof(double);
        const size_t ncal = (calm_stride ? nb : 1) * 27 * sizeof(double);
        TFF_TRY(c->in.reserve(nin + npt + 2 * npose + 8));
        TFF_TRY(c->calm.reserve(ncal));
        TFF_TRY(c->out.reserve(2 * npose + npt + nb * sizeof(double) + 8));
        TFF_TRY(c->idx.reserve(nb * 2 * sizeof(int32_t)));
        TFF_TRY(c->ragged_off.reserve((nb + 1) * sizeof(int64_t)));
        TFF_TRY(c->ba_host.reserve(nb * sizeof(int32_t) + nt + 8));
        if (weight) TFF_TRY(c->ba_weight.reserve(nt * sizeof(double) + 8));
        double* d_w = weight ? (double*)c->ba_weight.p : nullptr;
        double* d_in = (double*)c->in.p;
        double* d_x0 = d_in + 6 * nt;
        double* d_r2 = d_x0 + 3 * nt;
        double* d_r3 = d_r2 + 12 * nb;
        double* d_o2 = (double*)c->out.p;
        double* d_o3 = d_o2 + 12 * nb;
        double* d_rec = d_o3 + 12 * nb;
        double* d_err = d_rec + 3 * nt;
        int32_t* d_iter = (int32_t*)c->idx.p;
        int32_t* d_used = (int32_t*)c->ba_host.p;
        uint8_t* d_mask = (uint8_t*)(d_used + nb);
        if (cnt) TFF_HIP(hipMemcpyAsync(d_in + 6 * f, corresp + 6 * f, cnt * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (reconst0 && cnt) TFF_HIP(hipMemcpyAsync(d_x0 + 3 * f, reconst0 + 3 * f, cnt * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (mask && cnt) TFF_HIP(hipMemcpyAsync(d_mask + f, mask + f, cnt, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r2, Rt2_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r3, Rt3_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(c->calm.p, calm, ncal, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(c->ragged_off.p, offsets, (nb + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_ba_ragged(c, BaRaggedCall{d_in, (const int64_t*)c->ragged_off.p, n_total, mask ? d_mask : nullptr, (const double*)c->calm.p, calm_stride, d_r2, d_r3,
                                                 reconst0 ? d_x0 : nullptr, B, d_o2, d_o3, reconst ? d_rec : nullptr, d_iter, d_err, d_used, d_iter + nb,
                                                 loss, scale, d_w}));
        if (weight && cnt) TFF_HIP(hipMemcpyAsync(weight + f, d_w + f, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(Rt2, d_o2, npose, hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(Rt3, d_o3, npose, hipMemcpyDeviceToHost, c->stream));
        if (reconst && cnt) TFF_HIP(hipMemcpyAsync(reconst + 3 * f, d_rec + 3 * f, cnt * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (iter) TFF_HIP(hipMemcpyAsync(iter, d_iter, nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (repr_err) TFF_HIP(hipMemcpyAsync(repr_err, d_err, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (used) TFF_HIP(hipMemcpyAsync(used, d_used, nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (status) TFF_HIP(hipMemcpyAsync(status, d_iter + nb, nb * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipStreamSynchronize(c->stream));
        return 0;
    });
}
int tff_bundle_adjust_ragged_class_bounds(int32_t bounds[3]) {
    if (!bounds) return fail(TFF_E_INVALID, "null pointer");
    bounds[0] = tff::BA_CLASS_BOUND_0; bounds[1] = tff::BA_CLASS_BOUND_1; bounds[2] = tff::BA_CLASS_BOUND_2;
    return 0;
}

// ---- the covariance of the adjusted poses and points (include/tftfund_cov.h) ------------------------------------------------------------------------
int tff_ba_covariance_batch_dev(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2, const double* Rt3, const double* corresp, int64_t B,
                                int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_common(corresp, calm, calm_stride, B, N));
    TFF_TRY(check_ba_cov(reconst, cov, sigma0, B));
    return run_batch(c, B, Rt2 && Rt3, "null pose pointer", nullptr, [&] {
        if (N < 1) return fail(TFF_E_INVALID, "bundle adjustment needs at least one correspondence");
        return launch_ba_cov(c, calm, calm_stride, Rt2, Rt3, corresp, B, N, reconst, loss, scale, cov, sigma0, point_cov);
    });
}
int tff_ba_covariance_batch_host(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2, const double* Rt3, const double* corresp, int64_t B,
                                 int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_common(corresp, calm, calm_stride, B, N));
    TFF_TRY(check_ba_cov(reconst, cov, sigma0, B));
    return run_batch(c, B, Rt2 && Rt3, "null pose pointer", nullptr, [&] {
        if (N < 1) return fail(TFF_E_INVALID, "bundle adjustment needs at least one correspondence");
        const size_t nb = (size_t)B, nn = nb * (size_t)N, ncal = (calm_stride ? nb : 1) * 27;
        // corresp (6) | reconst (3) | point_cov (6) per correspondence, Rt2 | Rt3 | cov | sigma0 per item, calm
        TFF_TRY(c->cov_io.reserve((15 * nn + (24 + 145) * nb + ncal) * sizeof(double)));
        double* d_in = (double*)c->cov_io.p;
        double* d_x = d_in + 6 * nn;
        double* d_pc = d_x + 3 * nn;
        double* d_r2 = d_pc + 6 * nn;
        double* d_r3 = d_r2 + 12 * nb;
        double* d_cov = d_r3 + 12 * nb;
        double* d_s0 = d_cov + 144 * nb;
        double* d_cal = d_s0 + nb;
        TFF_HIP(hipMemcpyAsync(d_in, corresp, 6 * nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_x, reconst, 3 * nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r2, Rt2, 12 * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r3, Rt3, 12 * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_cal, calm, ncal * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_ba_cov(c, d_cal, calm_stride, d_r2, d_r3, d_in, B, N, d_x, loss, scale, d_cov, d_s0, point_cov ? d_pc : nullptr));
        TFF_HIP(hipMemcpyAsync(cov, d_cov, 144 * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(sigma0, d_s0, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (point_cov) TFF_HIP(hipMemcpyAsync(point_cov, d_pc, 6 * nn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipStreamSynchronize(c->stream));
        return 0;
    });
}
int tff_ba_covariance_ragged_dev(tff_ctx* c, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                 int64_t calm_stride, const double* Rt2, const double* Rt3, const double* reconst, int64_t B, int32_t loss, double scale,
                                 double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_ba_ragged(corresp, offsets, n_total, calm, calm_stride, Rt2, Rt3, B, cov, sigma0));
    if (B > 0 && n_total > 0 && !reconst) return fail(TFF_E_INVALID, "the covariance needs reconst, cov and sigma0");
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        return launch_ba_cov_ragged(c, BaCovRaggedCall{corresp, offsets, n_total, mask, calm, calm_stride, Rt2, Rt3, reconst, B, loss, scale, cov, sigma0, point_cov});
    });
}
int tff_ba_covariance_ragged_host(tff_ctx* c, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm, int64_t calm_stride,
                                  const double* Rt2, const double* Rt3, const double* reconst, int64_t B, int32_t loss, double scale, double* cov, double* sigma0,
                                  double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_host_offsets(offsets, B));
    const int64_t n_total = B > 0 ? offsets[B] : 0;
    TFF_TRY(check_ba_ragged(corresp, offsets, n_total, calm, calm_stride, Rt2, Rt3, B, cov, sigma0));
    if (B > 0 && n_total > 0 && !reconst) return fail(TFF_E_INVALID, "the covariance needs reconst, cov and sigma0");
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        const size_t nb = (size_t)B, nt = (size_t)n_total, f = (size_t)offsets[0], cnt = nt - f, ncal = (calm_stride ? nb : 1) * 27;
        // corresp (6) | reconst (3) | point_cov (6) per correspondence, Rt2 | Rt3 | cov | sigma0 per item, calm, offsets, mask
        TFF_TRY(c->cov_io.reserve((15 * nt + (24 + 145) * nb + ncal) * sizeof(double) + (nb + 1) * sizeof(int64_t) + nt + 8));
        double* d_in = (double*)c->cov_io.p;
        double* d_x = d_in + 6 * nt;
        double* d_pc = d_x + 3 * nt;
        double* d_r2 = d_pc + 6 * nt;
        double* d_r3 = d_r2 + 12 * nb;
        double* d_cov = d_r3 + 12 * nb;
        double* d_s0 = d_cov + 144 * nb;
        double* d_cal = d_s0 + nb;
        int64_t* d_off = (int64_t*)(d_cal + ncal);
        uint8_t* d_mask = (uint8_t*)(d_off + nb + 1);
        if (cnt) TFF_HIP(hipMemcpyAsync(d_in + 6 * f, corresp + 6 * f, cnt * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (cnt) TFF_HIP(hipMemcpyAsync(d_x + 3 * f, reconst + 3 * f, cnt * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (mask && cnt) TFF_HIP(hipMemcpyAsync(d_mask + f, mask + f, cnt, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r2, Rt2, 12 * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_r3, Rt3, 12 * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_cal, calm, ncal * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_off, offsets, (nb + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_ba_cov_ragged(c, BaCovRaggedCall{d_in, d_off, n_total, mask ? d_mask : nullptr, d_cal, calm_stride, d_r2, d_r3, d_x, B, loss, scale, d_cov, d_s0,
                                                        point_cov ? d_pc : nullptr}));
        TFF_HIP(hipMemcpyAsync(cov, d_cov, 144 * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(sigma0, d_s0, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (point_cov && cnt) TFF_HIP(hipMemcpyAsync(point_cov + 6 * f, d_pc + 6 * f, cnt * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipStreamSynchronize(c->stream));
        return 0;
    });
}

// the adjustment followed by the covariance at its outputs, on one stream
int tff_bundle_adjust_cov_batch_dev(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* corresp,
                                    int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3, double* reconst, int32_t* iter, double* repr_err,
                                    int32_t* status, int32_t loss, double scale, double* weight, double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_common(corresp, calm, calm_stride, B, N));
    if (B > 0 && (!cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs cov and sigma0");
    return run_batch(c, B, Rt2_in && Rt3_in && Rt2 && Rt3, "null pose pointer", nullptr, [&] {
        double* rec = reconst;
        if (!rec) {
            TFF_TRY(c->cov_rec.reserve((size_t)B * 3 * (size_t)(N > 0 ? N : 0) * sizeof(double) + 8));
            rec = (double*)c->cov_rec.p;
        }
        TFF_TRY(launch_bundle_adjust(c, tff::BaArgs{calm, (long)calm_stride, Rt2_in, Rt3_in, corresp, (long)B, N, reconst0, Rt2, Rt3, rec, iter, repr_err, status},
                                     loss, scale, weight));
        return launch_ba_cov(c, calm, calm_stride, Rt2, Rt3, corresp, B, N, rec, loss, scale, cov, sigma0, point_cov);
    });
}
int tff_bundle_adjust_cov_ragged_dev(tff_ctx* c, const double* corresp, const int64_t* offsets, int64_t n_total, const uint8_t* mask, const double* calm,
                                     int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2, double* Rt3,
                                     double* reconst, int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss, double scale, double* weight,
                                     double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_ba_ragged(corresp, offsets, n_total, calm, calm_stride, Rt2_in, Rt3_in, B, Rt2, Rt3));
    if (B > 0 && (!cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs cov and sigma0");
    return run_batch(c, B, true, nullptr, &status, [&] {
        double* rec = reconst;
        if (!rec) {
            TFF_TRY(c->cov_rec.reserve((size_t)n_total * 3 * sizeof(double) + 8));
            rec = (double*)c->cov_rec.p;
        }
        TFF_TRY(launch_ba_ragged(c, BaRaggedCall{corresp, offsets, n_total, mask, calm, calm_stride, Rt2_in, Rt3_in, reconst0, B, Rt2, Rt3, rec, iter, repr_err,
                                                 used, status, loss, scale, weight}));
        return launch_ba_cov_ragged(c, BaCovRaggedCall{corresp, offsets, n_total, mask, calm, calm_stride, Rt2, Rt3, rec, B, loss, scale, cov, sigma0, point_cov});
    });
}
// host-pointer forms: the two host calls one after the other (each stages, runs and synchronises), the points in between kept by the caller or here
int tff_bundle_adjust_cov_batch_host(tff_ctx* c, const double* calm, int64_t calm_stride, const double* Rt2_in, const double* Rt3_in, const double* corresp,
                                     int64_t B, int32_t N, const double* reconst0, double* Rt2, double* Rt3, double* reconst, int32_t* iter, double* repr_err,
                                     int32_t* status, int32_t loss, double scale, double* weight, double* cov, double* sigma0, double* point_cov) {
    if (!c) return fail(TFF_E_INVALID, "null context");
    if (B > 0 && (!cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs cov and sigma0");
    std::vector<double> own;
    double* rec = reconst;
    if (!rec && B > 0 && N > 0) { own.resize((size_t)B * 3 * (size_t)N); rec = own.data(); }
    TFF_TRY(tff_bundle_adjust_loss_batch_host(c, calm, calm_stride, Rt2_in, Rt3_in, corresp, B, N, reconst0, Rt2, Rt3, rec, iter, repr_err, status, loss, scale, weight));
    return tff_ba_covariance_batch_host(c, calm, calm_stride, Rt2, Rt3, corresp, B, N, rec, loss, scale, cov, sigma0, point_cov);
}
int tff_bundle_adjust_cov_ragged_host(tff_ctx* c, const double* corresp, const int64_t* offsets, const uint8_t* mask, const double* calm, int64_t calm_stride,
                                      const double* Rt2_in, const double* Rt3_in, const double* reconst0, int64_t B, double* Rt2, double* Rt3, double* reconst,
                                      int32_t* iter, double* repr_err, int32_t* used, int32_t* status, int32_t loss, double scale, double* weight, double* cov,
                                      double* sigma0, double* point_cov) {
    if (!c) return fail(TFF_E_INVALID, "null context");
    TFF_TRY(check_host_offsets(offsets, B));
    if (B > 0 && (!cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs cov and sigma0");
    std::vector<double> own;
    double* rec = reconst;
    if (!rec && B > 0 && offsets[B] > 0) { own.resize((size_t)offsets[B] * 3); rec = own.data(); }
    TFF_TRY(tff_bundle_adjust_loss_ragged_host(c, corresp, offsets, mask, calm, calm_stride, Rt2_in, Rt3_in, reconst0, B, Rt2, Rt3, rec, iter, repr_err, used, status,
                                               loss, scale, weight));
    return tff_ba_covariance_ragged_host(c, corresp, offsets, mask, calm, calm_stride, Rt2, Rt3, rec, B, loss, scale, cov, sigma0, point_cov);
}

int tff_optim_f_ragged_bounds(int32_t bounds[2]) {
    if (!bounds) return fail(TFF_E_INVALID, "null pointer");
    optimf_ragged_bounds(false, bounds);
    return 0;
}

// BundleAdjustment as the reference writes it, M = 2 .. 6 views (launch_bundle_adjust_views above)
int tff_bundle_adjust_views_batch_dev(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                      int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                      int32_t* status) {
    TFF_ENTER(c);
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        return launch_bundle_adjust_views(c, M, tff::BavArgs{calm, (long)calm_stride, Rt_in, corresp, (long)B, N, reconst0, Rt, reconst, iter, repr_err, status});
    });
}
int tff_bundle_adjust_views_batch_host(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                       int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                       int32_t* status) {
    TFF_ENTER(c);
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        const size_t nin = (size_t)B * 2 * M * (size_t)N * sizeof(double), npt = (size_t)B * 3 * (size_t)N * sizeof(double);
        const size_t ncal = (calm_stride ? (size_t)B : 1) * 9 * M * sizeof(double), npose = (size_t)B * 12 * M * sizeof(double);
        BaStaging s;
        TFF_TRY(ba_stage_in(c, (size_t)B, nin, npt, npose, ncal, corresp, reconst0, &s));
        TFF_HIP(hipMemcpyAsync(s.poses_in, Rt_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(s.calm, calm, ncal, hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_bundle_adjust_views(c, M, tff::BavArgs{s.calm, (long)calm_stride, s.poses_in, s.corresp, (long)B, N, s.reconst0, s.poses_out, s.reconst,
                                                              s.iter, s.repr_err, s.status}));
        TFF_HIP(hipMemcpyAsync(Rt, s.poses_out, npose, hipMemcpyDeviceToHost, c->stream));
        return ba_stage_out(c, (size_t)B, npt, s, reconst, iter, repr_err, status);
    });
}

// BundleAdjustment as the reference documents it: per-point visibility (launch_bundle_adjust_tracks above; include/tftfund_tracks.h)
int tff_bundle_adjust_tracks_batch_dev(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                       int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                       int32_t* used, int32_t* status) {
    TFF_ENTER(c);
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        return launch_bundle_adjust_tracks(c, M, tff::BatArgs{tff::BavArgs{calm, (long)calm_stride, Rt_in, corresp, (long)B, N, reconst0, Rt, reconst, iter, repr_err,
                                                                           status}, used});
    });
}
int tff_bundle_adjust_tracks_batch_host(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                        int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                        int32_t* used, int32_t* status) {
    TFF_ENTER(c);
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        const size_t nin = (size_t)B * 2 * M * (size_t)N * sizeof(double), npt = (size_t)B * 3 * (size_t)N * sizeof(double);
        const size_t ncal = (calm_stride ? (size_t)B : 1) * 9 * M * sizeof(double), npose = (size_t)B * 12 * M * sizeof(double);
        BaStaging s;
        TFF_TRY(ba_stage_in(c, (size_t)B, nin, npt, npose, ncal, corresp, reconst0, &s));
        TFF_TRY(c->tracks_used.reserve((size_t)B * sizeof(int32_t)));
        int32_t* d_used = (int32_t*)c->tracks_used.p;
        TFF_HIP(hipMemcpyAsync(s.poses_in, Rt_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(s.calm, calm, ncal, hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_bundle_adjust_tracks(c, M, tff::BatArgs{tff::BavArgs{s.calm, (long)calm_stride, s.poses_in, s.corresp, (long)B, N, s.reconst0, s.poses_out,
                                                                            s.reconst, s.iter, s.repr_err, s.status}, d_used}));
        TFF_HIP(hipMemcpyAsync(Rt, s.poses_out, npose, hipMemcpyDeviceToHost, c->stream));
        if (used) TFF_HIP(hipMemcpyAsync(used, d_used, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        return ba_stage_out(c, (size_t)B, npt, s, reconst, iter, repr_err, status);
    });
}

// ... with a robust loss per observation and the weights (launch_bundle_adjust_tracks_loss above; include/tftfund_tracks_loss.h)
int tff_bundle_adjust_tracks_loss_batch_dev(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                            int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                            int32_t* used, int32_t* status, int32_t loss, double scale, double* weight) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        return launch_bundle_adjust_tracks_loss(c, M, tff::BatArgs{tff::BavArgs{calm, (long)calm_stride, Rt_in, corresp, (long)B, N, reconst0, Rt, reconst, iter,
                                                                                repr_err, status}, used}, loss, scale, weight);
    });
}
int tff_bundle_adjust_tracks_loss_batch_host(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                             int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                             int32_t* used, int32_t* status, int32_t loss, double scale, double* weight) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        const size_t nin = (size_t)B * 2 * M * (size_t)N * sizeof(double), npt = (size_t)B * 3 * (size_t)N * sizeof(double);
        const size_t ncal = (calm_stride ? (size_t)B : 1) * 9 * M * sizeof(double), npose = (size_t)B * 12 * M * sizeof(double);
        const size_t nw = (size_t)B * (size_t)N * M * sizeof(double);
        BaStaging s;
        TFF_TRY(ba_stage_in(c, (size_t)B, nin, npt, npose, ncal, corresp, reconst0, &s));
        TFF_TRY(c->tracks_used.reserve((size_t)B * sizeof(int32_t)));
        int32_t* d_used = (int32_t*)c->tracks_used.p;
        if (weight) TFF_TRY(c->tracks_weight.reserve(nw));
        double* d_w = weight ? (double*)c->tracks_weight.p : nullptr;
        TFF_HIP(hipMemcpyAsync(s.poses_in, Rt_in, npose, hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(s.calm, calm, ncal, hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_bundle_adjust_tracks_loss(c, M, tff::BatArgs{tff::BavArgs{s.calm, (long)calm_stride, s.poses_in, s.corresp, (long)B, N, s.reconst0, s.poses_out,
                                                                                 s.reconst, s.iter, s.repr_err, s.status}, d_used}, loss, scale, d_w));
        TFF_HIP(hipMemcpyAsync(Rt, s.poses_out, npose, hipMemcpyDeviceToHost, c->stream));
        if (used) TFF_HIP(hipMemcpyAsync(used, d_used, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (weight) TFF_HIP(hipMemcpyAsync(weight, d_w, nw, hipMemcpyDeviceToHost, c->stream));
        return ba_stage_out(c, (size_t)B, npt, s, reconst, iter, repr_err, status);
    });
}

// ... and the covariance of its poses and points (launch_ba_tracks_cov above; include/tftfund_tracks_cov.h)
int tff_ba_tracks_covariance_batch_dev(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt, const double* corresp, int64_t B,
                                       int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_views(M, calm, calm_stride, Rt, corresp, B, N, cov));
    TFF_TRY(check_ba_cov(reconst, cov, sigma0, B));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        return launch_ba_tracks_cov(c, M, calm, calm_stride, Rt, corresp, B, N, reconst, loss, scale, cov, sigma0, point_cov);
    });
}
int tff_ba_tracks_covariance_batch_host(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt, const double* corresp, int64_t B,
                                        int32_t N, const double* reconst, int32_t loss, double scale, double* cov, double* sigma0, double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_views(M, calm, calm_stride, Rt, corresp, B, N, cov));
    TFF_TRY(check_ba_cov(reconst, cov, sigma0, B));
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        const size_t nb = (size_t)B, nn = nb * (size_t)N, ncal = (calm_stride ? nb : 1) * 9 * (size_t)M, pp = (size_t)(36 * (M - 1) * (M - 1));
        // corresp (2M) | reconst (3) | point_cov (6) per point, Rt | cov | sigma0 per item, calm
        TFF_TRY(c->tracks_cov_io.reserve(((2 * (size_t)M + 9) * nn + (12 * (size_t)M + pp + 1) * nb + ncal) * sizeof(double)));
        double* d_in = (double*)c->tracks_cov_io.p;
        double* d_x = d_in + 2 * (size_t)M * nn;
        double* d_pc = d_x + 3 * nn;
        double* d_rt = d_pc + 6 * nn;
        double* d_cov = d_rt + 12 * (size_t)M * nb;
        double* d_s0 = d_cov + pp * nb;
        double* d_cal = d_s0 + nb;
        TFF_HIP(hipMemcpyAsync(d_in, corresp, 2 * (size_t)M * nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_x, reconst, 3 * nn * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_rt, Rt, 12 * (size_t)M * nb * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_HIP(hipMemcpyAsync(d_cal, calm, ncal * sizeof(double), hipMemcpyHostToDevice, c->stream));
        TFF_TRY(launch_ba_tracks_cov(c, M, d_cal, calm_stride, d_rt, d_in, B, N, d_x, loss, scale, d_cov, d_s0, point_cov ? d_pc : nullptr));
        TFF_HIP(hipMemcpyAsync(cov, d_cov, pp * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipMemcpyAsync(sigma0, d_s0, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (point_cov) TFF_HIP(hipMemcpyAsync(point_cov, d_pc, 6 * nn * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        TFF_HIP(hipStreamSynchronize(c->stream));
        return 0;
    });
}
// the adjustment followed by the covariance at its outputs, on one stream
int tff_bundle_adjust_tracks_cov_batch_dev(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                           int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                           int32_t* used, int32_t* status, int32_t loss, double scale, double* weight, double* cov, double* sigma0,
                                           double* point_cov) {
    TFF_ENTER(c);
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    if (B > 0 && (!cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs cov and sigma0");
    return run_batch(c, B, true, nullptr, nullptr, [&] {
        double* rec = reconst;
        if (!rec) {
            TFF_TRY(c->tracks_cov_rec.reserve((size_t)B * 3 * (size_t)N * sizeof(double) + 8));
            rec = (double*)c->tracks_cov_rec.p;
        }
        TFF_TRY(launch_bundle_adjust_tracks_loss(c, M, tff::BatArgs{tff::BavArgs{calm, (long)calm_stride, Rt_in, corresp, (long)B, N, reconst0, Rt, rec, iter,
                                                                                 repr_err, status}, used}, loss, scale, weight));
        return launch_ba_tracks_cov(c, M, calm, calm_stride, Rt, corresp, B, N, rec, loss, scale, cov, sigma0, point_cov);
    });
}
// host-pointer form: the two host calls one after the other (each stages, runs and synchronises), the points in between kept by the caller or here
int tff_bundle_adjust_tracks_cov_batch_host(tff_ctx* c, int32_t M, const double* calm, int64_t calm_stride, const double* Rt_in, const double* corresp,
                                            int64_t B, int32_t N, const double* reconst0, double* Rt, double* reconst, int32_t* iter, double* repr_err,
                                            int32_t* used, int32_t* status, int32_t loss, double scale, double* weight, double* cov, double* sigma0,
                                            double* point_cov) {
    if (!c) return fail(TFF_E_INVALID, "null context");
    TFF_TRY(check_loss(loss, scale));
    TFF_TRY(check_views(M, calm, calm_stride, Rt_in, corresp, B, N, Rt));
    if (B > 0 && (!cov || !sigma0)) return fail(TFF_E_INVALID, "the covariance needs cov and sigma0");
    std::vector<double> own;
    double* rec = reconst;
    if (!rec && B > 0 && N > 0) { own.resize((size_t)B * 3 * (size_t)N); rec = own.data(); }
    TFF_TRY(tff_bundle_adjust_tracks_loss_batch_host(c, M, calm, calm_stride, Rt_in, corresp, B, N, reconst0, Rt, rec, iter, repr_err, used, status, loss, scale, weight));
    return tff_ba_tracks_covariance_batch_host(c, M, calm, calm_stride, Rt, corresp, B, N, rec, loss, scale, cov, sigma0, point_cov);
}

// linearF (refine = 0) / optimF (refine = 1) for the view pairs (1,2) and (1,3)
int tff_linear_f_batch_dev(tff_ctx* c, const double* corresp, int64_t B, int32_t N, int32_t refine, double* F21, double* F31,
                           int32_t* iter, int32_t* status) {
    TFF_ENTER(c);
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative size");
    return run_batch(c, B, corresp && F21 && F31, "null pointer", &status, [&] {
        tff::LinearFOnlyArgs a{corresp, (long)B, N, 0, F21, F31, iter, status};
        const lds_fn ldsfn = refine ? tff::optimf_lds_bytes : tff::f_pose_lds_bytes;
        auto plan = [&](bool exact, tff::LinearFOnlyArgs*, unsigned*, size_t* lds) { *lds = ldsfn(N, 0, exact); return 0; };
        if (refine) return launch_fast_exact(c, tff::k_linear_f<false, 1>, tff::k_linear_f<true, 1>, fast_tiers(c, N), a, plan);
        return launch_fast_exact(c, tff::k_linear_f<false, 0>, tff::k_linear_f<true, 0>, fast_tiers(c, N), a, plan);
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Multi-GPU behind the C ABI: ONE process, one context + one host thread + one stream per
// device; the batch is cut into contiguous shards of ceil(B / G) triplets; independent triplets need no
// collective on the data path.  The _host variant lands every shard directly in the caller's host
// arrays.  The _dev variant leaves shard g on device g and then gathers the fixed-size result records
// of all shards onto every device with ONE ncclAllGather over xGMI (RCCL, single-process communicators
// from ncclCommInitAll; librccl.so is opened on first use, libtftfund.so itself does not depend on it).
// ---------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <thread>

struct tff_multi {
    std::vector<tff_ctx*> ctx;
    std::vector<int> devices;
    // RCCL (lazily): communicators of the single-process clique, one per device
    void* rccl = nullptr;
    std::mutex rccl_mu;
    std::vector<void*> comms;
    int (*p_init_all)(void**, int, const int*) = nullptr;
    int (*p_allgather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*p_group_start)() = nullptr;
    int (*p_group_end)() = nullptr;
    int (*p_comm_destroy)(void*) = nullptr;
    const char* (*p_err)(int) = nullptr;
};

namespace {

int multi_load_rccl(tff_multi* m) {
    std::lock_guard<std::mutex> guard(m->rccl_mu);                             // concurrent first calls: one of them initialises the communicators
    if (m->rccl) return 0;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(TFF_E_INVALID, "librccl.so not found (needed only by tff_pose_batch_dev_multi)");
    m->p_init_all = (int (*)(void**, int, const int*))dlsym(h, "ncclCommInitAll");
    m->p_allgather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    m->p_group_start = (int (*)())dlsym(h, "ncclGroupStart");
    m->p_group_end = (int (*)())dlsym(h, "ncclGroupEnd");
    m->p_comm_destroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    m->p_err = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!m->p_init_all || !m->p_allgather || !m->p_group_start || !m->p_group_end || !m->p_comm_destroy) {
        dlclose(h);
        return fail(TFF_E_INVALID, "librccl.so lacks the expected symbols");
    }
    m->comms.assign(m->ctx.size(), nullptr);
    const int rc = m->p_init_all(m->comms.data(), (int)m->devices.size(), m->devices.data());
    if (rc != 0) {
        g_err = std::string("ncclCommInitAll: ") + (m->p_err ? m->p_err(rc) : "error");
        dlclose(h);
        m->comms.clear();
        return TFF_E_INVALID;
    }
    m->rccl = h;
    return 0;
}

}  // namespace

extern "C" {

int tff_multi_create(tff_multi** out, const int32_t* devices, int32_t n_devices) {
    if (!out) return fail(TFF_E_INVALID, "null out pointer");
    *out = nullptr;
    int have = 0;
    TFF_HIP(hipGetDeviceCount(&have));
    if (n_devices <= 0) n_devices = have;                                    // all visible devices
    if (n_devices <= 0 || n_devices > have) return fail(TFF_E_INVALID, "no such set of HIP devices");
    tff_multi* m = new (std::nothrow) tff_multi();
    if (!m) return fail(TFF_E_NOMEM, "out of host memory");
    for (int g = 0; g < n_devices; ++g) {
        const int dev = devices ? devices[g] : g;
        for (int d : m->devices) if (d == dev) { tff_multi_destroy(m); return fail(TFF_E_INVALID, "duplicate device"); }
        tff_ctx* c = nullptr;
        const int rc = tff_ctx_create(&c, dev);
        if (rc != 0) { tff_multi_destroy(m); return rc; }
        m->ctx.push_back(c);
        m->devices.push_back(dev);
    }
    *out = m;
    return 0;
}

void tff_multi_destroy(tff_multi* m) {
    if (!m) return;
    if (m->rccl) {
        for (void* cm : m->comms) if (cm) (void)m->p_comm_destroy(cm);
        dlclose(m->rccl);
    }
    for (tff_ctx* c : m->ctx) tff_ctx_destroy(c);
    delete m;
}

int32_t tff_multi_size(const tff_multi* m) { return m ? (int32_t)m->ctx.size() : 0; }
tff_ctx* tff_multi_ctx(tff_multi* m, int32_t rank) { return (m && rank >= 0 && rank < (int32_t)m->ctx.size()) ? m->ctx[rank] : nullptr; }

void tff_multi_shard(const tff_multi* m, int64_t B, int32_t rank, int64_t* begin, int64_t* end) {
    const int64_t G = m ? (int64_t)m->ctx.size() : 1;
    const int64_t chunk = (B + G - 1) / G;
    int64_t b0 = chunk * rank, b1 = b0 + chunk;
    if (b0 > B) b0 = B;
    if (b1 > B) b1 = B;
    if (begin) *begin = b0;
    if (end) *end = b1;
}

int tff_pose_batch_host_multi(tff_multi* m, int32_t method, const double* corresp, const double* calm, int64_t calm_stride,
                              int64_t B, int32_t N, double* Rt2, double* Rt3, double* T, double* reconst, int32_t* iter,
                              int32_t* status) {
    if (!m) return fail(TFF_E_INVALID, "null multi-GPU handle");
    if (!method_of(method)) return fail(TFF_E_INVALID, "unknown method id");
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative batch or correspondence count");
    if (calm_stride != 0 && calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
    const int G = (int)m->ctx.size();
    std::vector<int> rc(G, 0);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g) {
        th.emplace_back([&, g]() {
            int64_t b0, b1;
            tff_multi_shard(m, B, g, &b0, &b1);
            if (b1 <= b0) return;
            rc[g] = pose_host(m->ctx[g], method, PoseCall{corresp + b0 * 6 * (int64_t)N, calm + b0 * calm_stride, calm_stride, b1 - b0, N,
                                                          Rt2 + b0 * 12, Rt3 + b0 * 12, T + b0 * 27, reconst ? reconst + b0 * 3 * (int64_t)N : nullptr,
                                                          iter ? iter + b0 : nullptr, status ? status + b0 : nullptr, nullptr});
            if (rc[g] != 0) msg[g] = g_err;                                  // tff_last_error() is thread-local: carry it over
        });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < G; ++g) if (rc[g] != 0) { g_err = "device " + std::to_string(m->devices[g]) + ": " + msg[g]; return rc[g]; }
    return 0;
}

// Device-resident variant.  corresp[g], calm[g]: device pointers ON DEVICE g holding shard g of the batch (shard bounds:
// tff_multi_shard).  records[g]: device buffer on device g of G * chunk * 51 doubles, chunk = ceil(B / G); after the call
// EVERY device holds all shards: block r (chunk * 51 doubles) = [Rt2 (chunk x 12) | Rt3 (chunk x 12) | T (chunk x 27)] of
// shard r.  status[g] (optional): G * chunk int32 per device, gathered the same way.  Work is enqueued on each context's
// stream; tff_ctx_synchronize(tff_multi_ctx(m, g)) to wait.
int tff_pose_batch_dev_multi(tff_multi* m, int32_t method, const double* const* corresp, const double* const* calm,
                             int64_t calm_stride, int64_t B, int32_t N, double* const* records, int32_t* const* status) {
    if (!m) return fail(TFF_E_INVALID, "null multi-GPU handle");
    if (!method_of(method)) return fail(TFF_E_INVALID, "unknown method id");
    if (!corresp || !calm || !records) return fail(TFF_E_INVALID, "null pointer array");
    if (B < 0 || N < 0) return fail(TFF_E_INVALID, "negative batch or correspondence count");
    if (calm_stride != 0 && calm_stride != 27) return fail(TFF_E_INVALID, "calm_stride must be 0 (shared CalM) or 27");
    if (B == 0) return 0;
    if (int r = multi_load_rccl(m)) return r;
    const int G = (int)m->ctx.size();
    const int64_t chunk = (B + G - 1) / G;
    int caller_device = 0;
    TFF_HIP(hipGetDevice(&caller_device));
    std::vector<int> rc(G, 0);
    std::vector<std::string> msg(G);
    std::vector<std::thread> th;
    for (int g = 0; g < G; ++g) {
        th.emplace_back([&, g]() {
            int64_t b0, b1;
            tff_multi_shard(m, B, g, &b0, &b1);
            double* blk = records[g] + (int64_t)g * chunk * 51;
            int32_t* sblk = status ? status[g] + (int64_t)g * chunk : nullptr;
            // The all-gather below sends the WHOLE block of every device: the part of it no triplet fills (an uneven last shard, or an
            // empty one when B < G) is defined first -- quiet NaN records with status TFF_ST_TOO_FEW -- on the stream the kernels use.
            if (b1 - b0 < chunk) {
                hipError_t e = hipSetDevice(m->devices[g]);
                if (e == hipSuccess) e = hipMemsetAsync(blk, 0xff, (size_t)chunk * 51 * sizeof(double), m->ctx[g]->stream);
                if (e == hipSuccess && sblk) e = hipMemsetD32Async((hipDeviceptr_t)sblk, TFF_ST_TOO_FEW, (size_t)chunk, m->ctx[g]->stream);
                if (e != hipSuccess) { rc[g] = hip_fail(e, "hipMemsetAsync(record block)"); msg[g] = g_err; return; }
            }
            if (b1 <= b0) return;
            rc[g] = pose_dev(m->ctx[g], method, PoseCall{corresp[g], calm[g], calm_stride, b1 - b0, N, blk, blk + chunk * 12, blk + chunk * 24, nullptr, nullptr,
                                                         sblk, nullptr});
            if (rc[g] != 0) msg[g] = g_err;
        });
    }
    for (auto& t : th) t.join();
    for (int g = 0; g < G; ++g) if (rc[g] != 0) { g_err = "device " + std::to_string(m->devices[g]) + ": " + msg[g]; return rc[g]; }
    // one collective per result kind, all devices in one group (single-process clique)
    int nrc = m->p_group_start();
    hipError_t herr = hipSuccess;
    for (int g = 0; g < G && nrc == 0 && herr == hipSuccess; ++g) {
        herr = hipSetDevice(m->devices[g]);                                  // (no early return inside the group: it must be closed)
        if (herr != hipSuccess) break;
        nrc = m->p_allgather(records[g] + (int64_t)g * chunk * 51, records[g], (size_t)(chunk * 51), 8 /* ncclFloat64 */, m->comms[g], m->ctx[g]->stream);
        if (nrc == 0 && status) nrc = m->p_allgather(status[g] + (int64_t)g * chunk, status[g], (size_t)chunk, 2 /* ncclInt32 */, m->comms[g], m->ctx[g]->stream);
    }
    const int erc = m->p_group_end();
    (void)hipSetDevice(caller_device);                                       // the caller's current device is not ours to change
    if (herr != hipSuccess) return hip_fail(herr, "hipSetDevice");
    if (nrc == 0) nrc = erc;
    if (nrc != 0) { g_err = std::string("ncclAllGather: ") + (m->p_err ? m->p_err(nrc) : "error"); return TFF_E_INVALID; }
    return 0;
}

}  // extern "C"
