// The robust pose estimator (tff_robust_pose_*, tff_robust_pose_scenes_*, tff_inlier_count_scenes_dev): the hypotheses of S scenes share ONE chain of
// launches, and the one-scene call is that chain with S = 1.  Scene s owns the correspondences offsets[s] .. offsets[s + 1] - 1 of a packed array;
// hypothesis g = s * n_hyp + h is hypothesis h of scene s, drawn with seed + s, and nothing it computes depends on the other scenes: the sampler is
// counter-based (robust_kernel.h::sample_draw), the unchanged *_sampled pose kernels gather GLOBAL indices from the packed array, the per-match inlier
// rule is count_if_inlier, the refit is the ragged chain over the S * K candidates.  This file holds the glue:
//
//   k_scenes_sample        sample_draw per scene: global indices (-1 for an invalid scene) + with one CalM per scene the hypothesis's own copy of it
//   k_inlier_count_scenes  the hot kernel: four hypotheses per wavefront, a workgroup serves one scene at a time (staged in LDS when it fits)
//   k_scenes_mask          the inlier flags of one pose per item, rows of different lengths, packed; the row sums are k_inlier_count_scenes's counts
//   k_scenes_offsets       offsets of the S * K + 1 packed refit items: a one-workgroup scan
//   k_scenes_compact       a candidate's inliers, in scene order, into its range of the packed refit batch
//   k_scenes_finish        per scene the winner (largest count, ties to the earlier candidate) -> the caller's outputs; the outputs of an invalid scene
//   k_round_init / k_round_scatter / k_round_close   the adaptive call (tff_robust_pose_scenes_adaptive_*): rounds of hypotheses and the stop rule
//
// k_robust_mark, k_robust_topk (gridDim.y = S), k_robust_seed and k_robust_adopt (robust_kernel.h) do the selection.  A chunk of ROBUST_CHUNK
// hypotheses may cut a scene anywhere: every kernel derives (s, h) from g.
#pragma once
#include "robust_kernel.h"
#include "ragged_kernel.h"

namespace tff {

struct SceneSet {
    const double* scenes;    // packed 6 x n_total
    const long* offsets;     // S + 1, on the device; null (tff_robust_pose_dev, which is given none): S = 1 and the scene is [0, n_total)
    long S;
    long n_total;            // every offset lies in [0, n_total]
    int ns_max;              // a scene with more correspondences is ST_BAD_OFFSETS
    int n_min;               // ... with fewer ST_TOO_FEW (the sample size; 0 for tff_inlier_count_scenes_dev)
    const double* calm;      // 27 doubles shared (calm_stride 0) or one per scene (27)
    long calm_stride;
};
// the status of scene s and, when it is ST_OK, its range [*o, *o + *n) of the packed arrays: nothing else is ever used as an address
__device__ __forceinline__ int scene_range(const SceneSet& q, const long s, long* o, int* n) {
    const long o0 = q.offsets ? q.offsets[s] : 0, o1 = q.offsets ? q.offsets[s + 1] : q.n_total;
    *o = 0; *n = 0;
    if (o0 < 0 || o1 < o0 || o1 > q.n_total || o1 - o0 > (long)q.ns_max) return ST_BAD_OFFSETS;
    if (o1 - o0 < (long)q.n_min) return ST_TOO_FEW;
    *o = o0; *n = (int)(o1 - o0);
    return ST_OK;
}

// ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
struct ScenesSampleArgs {
    SceneSet q;
    unsigned long long seed; // scene s draws with seed + s (wrapping)
    long first;              // row b is hypothesis g = first + b: scene g / per, index g % per ...
    const unsigned long long* keys;   // ... or, when non-null, scene b / per and the hypothesis of selection key keys[b]
    long B;
    long per;                // n_hyp, or K with `keys`
    int n;
    int* out;                // B x n indices into the packed array, -1 for an invalid scene
    double* calm_out;        // B x 27: the row's CalM, for the pose kernels (calm_stride 27); null with a shared CalM, which they read themselves
    long hyp_base;           // a round of the adaptive call (per = the round's length): the row's hypothesis is hyp_base + g % per; 0 otherwise
    const int* live;         // null, or S: a scene with live[s] == 0 gets indices -1, like an invalid one
};
// One row of a scene sampler (k_scenes_sample; k_scenes_sample_guided in robust_guided_kernel.h): the row's (s, h), its scene's validity and liveness,
// the n indices by draw(seed + s, h, ns, o, out) or a row of -1, the CalM copy
template <class Draw>
__device__ __forceinline__ void scenes_sample_row(const ScenesSampleArgs& a, const Draw draw) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const long g = a.first + b;
    const long s = g / a.per;
    const unsigned long long h = a.keys ? (unsigned long long)robust_key_index(a.keys[b]) : (unsigned long long)(a.hyp_base + (g - s * a.per));
    long o; int ns;
    const bool ok = scene_range(a.q, s, &o, &ns) == ST_OK && !(a.live && a.live[s] == 0);
    int* out = a.out + b * a.n;
    if (ok) draw(a.seed + (unsigned long long)s, h, ns, o, out);
    else for (int i = 0; i < a.n; ++i) out[i] = -1;
    if (!a.calm_out) return;
    const double* calm = a.q.calm + s * a.q.calm_stride;
    for (int e = 0; e < 27; ++e) a.calm_out[b * 27 + e] = calm[e];
}
__global__ void __launch_bounds__(256) k_scenes_sample(const ScenesSampleArgs a) {
    scenes_sample_row(a, [&](unsigned long long seed, unsigned long long h, int ns, long o, int* out) { sample_draw(seed, h, a.n, ns, (int)o, out); });
}

// ---- inlier counts: hypotheses of many scenes -------------------------------------------------------------------------------------------------
// Hypothesis b of the launch is g = first + b of the call and belongs to scene g / per.  A workgroup owns the slab [blockIdx.x * slab, + slab) of
// hypotheses and cuts it where the scene changes: within a segment all sixteen rows of the workgroup (four wavefronts x four rows of 16 lanes, the
// layout of k_inlier_count_rows) work on one scene, which is staged in LDS first when its 6 n doubles fit stage_doubles and the segment is long
// enough to repay the copy, and read through L2 otherwise.  Per correspondence: count_if_inlier, so the integers are those of the one-scene kernels.
struct ScenesCountArgs {
    SceneSet q;
    const double* Rt2; const double* Rt3;    // B x 12 column-major poses (rows of THIS launch)
    long first, B, per, slab;
    double thr;
    int* counts;             // B; -1 for a hypothesis of an invalid scene
    int stage_doubles;       // LDS doubles behind the cameras
    double score_c;          // k_inlier_count_scenes_msac only: 1 / (6 thr^2) from the host (blocks_kernel.h::inlier_weight); 0 for the count kernel
    const int* live;         // null, or S: the segment of a scene with live[s] == 0 is skipped like an invalid scene's (-1)
};
constexpr int SCENES_COUNT_ROWS = 4 * INLIER_WG_WAVES;       // hypotheses a workgroup serves at a time
constexpr int SCENES_STAGE_MIN = 8;                          // shorter segments read their scene through L2
constexpr int SCENES_STAGE_MAX_DOUBLES = 48 * 1024 / 8 - 36 * SCENES_COUNT_ROWS;   // scene + cameras within the 48 KB of the one-scene launcher

template <bool MSAC>
__device__ __forceinline__ void scenes_count_segment(const ScenesCountArgs& a, const double* scene, const int n, const double* calm, double* camw,
                                                     const long seg_begin, const long seg_end) {
    const int p = lane_id() & 15, row = lane_id() >> 4;
    for (long b0 = seg_begin + 4 * wave_in_block(); b0 < seg_end; b0 += SCENES_COUNT_ROWS) {
        const bool valid = b0 + row < seg_end;
        const long b = valid ? b0 + row : seg_end - 1;                       // (a tail row repeats the segment's last hypothesis and does not store)
        wave_sync();
        if (p < 3) {
            const Mat3 K = load_K(calm, p);
            double Rt[12];                                                   // row-major pose of view p
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                const int r = e >> 2, c = e & 3;
                Rt[e] = (p == 0) ? ((r == c) ? 1.0 : 0.0) : ((p == 1) ? a.Rt2[b * 12 + r + 3 * c] : a.Rt3[b * 12 + r + 3 * c]);
            }
            compose_camera_from_pose(K, Rt, camw + 12 * p);
        }
        wave_sync();
        double P[3][12];
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int c = 0; c < 12; ++c) P[v][c] = camw[12 * v + c];
        double Zt[4][4];
        inlier_threshold_form(P, a.thr, Zt);
        int cnt = 0;
#pragma unroll 1
        for (int i = p; i < n; i += 16) {
            score_if_inlier<MSAC>(P, Zt, camw, camw + 12, camw + 24, load_pt(scene, i), a.thr, a.score_c, cnt);
        }
        const double tot = row_sum16((double)cnt);
        if (p == 0 && valid) a.counts[b] = (int)tot;
    }
}
template <bool MSAC>
__global__ void __launch_bounds__(64 * INLIER_WG_WAVES, 2) k_inlier_count_scenes_t(const ScenesCountArgs a) {
    TFF_DYNAMIC_LDS(double, smem);
    double* camw = smem + 36 * (4 * wave_in_block() + (lane_id() >> 4));     // the row's three cameras (row-major 3 x 4)
    double* staged = smem + 36 * SCENES_COUNT_ROWS;                          // up to stage_doubles of one scene
    long b = (long)blockIdx.x * a.slab;
    const long slab_end = b + a.slab < a.B ? b + a.slab : a.B;
    while (b < slab_end) {                                                   // (b, the segment and the staging decision are the workgroup's)
        const long s = (a.first + b) / a.per;
        long seg_end = (s + 1) * a.per - a.first;
        if (seg_end > slab_end) seg_end = slab_end;
        long o; int n;
        if (scene_range(a.q, s, &o, &n) != ST_OK || (a.live && a.live[s] == 0)) {
            for (long i = b + thread_in_block(); i < seg_end; i += 64 * INLIER_WG_WAVES) a.counts[i] = -1;
        } else {
            const double* src = a.q.scenes + 6 * o;
            const double* calm = a.q.calm + s * a.q.calm_stride;
            if (6L * n <= (long)a.stage_doubles && seg_end - b >= SCENES_STAGE_MIN) {
                __syncthreads();                                             // (the previous segment's readers are done)
                const double2* s2 = reinterpret_cast<const double2*>(src);   // (6 o doubles: 16-byte aligned)
                double2* d2 = reinterpret_cast<double2*>(staged);
                for (int i = thread_in_block(); i < 3 * n; i += 64 * INLIER_WG_WAVES) d2[i] = s2[i];
                __syncthreads();
                scenes_count_segment<MSAC>(a, staged, n, calm, camw, b, seg_end);
            } else {
                scenes_count_segment<MSAC>(a, src, n, calm, camw, b, seg_end);
            }
        }
        b = seg_end;
    }
}
constexpr auto k_inlier_count_scenes = k_inlier_count_scenes_t<false>;   // (the pattern of blocks_kernel.h::k_repr_error_t)
constexpr auto k_inlier_count_scenes_msac = k_inlier_count_scenes_t<true>;

// ---- the adaptive call: hypotheses in rounds, a scene stops once its best hypothesis makes another all-inlier sample unnecessary ----------------------
// Round r draws the hypotheses [e_prev, e_end) of every scene that is still live; the round's rows are g' = s * len + i (len = e_end - e_prev), cut
// into chunks like the fixed call's.  k_round_scatter moves a chunk's dense counts to the scene-major array of the fixed call (stride n_hyp; the whole
// array is -1 before round 1, so a hypothesis never drawn is never selected) and keeps the scene's best; k_round_close applies the rule once the round's
// last chunk is in.  The rule has no log and no pow: q = w^n_sample by repeated multiplication against a threshold the host computed (include/tftfund.h).
struct RoundState {
    SceneSet q;
    int* live;               // S: 1 while the scene draws
    unsigned long long* best;   // S: the largest count so far + 1, 0 = no success yet (64 bits: the atomic maximum of k_robust_topk)
    int* used;               // S: hypotheses drawn (the caller's array)
};
__global__ void __launch_bounds__(256) k_round_init(const RoundState a) {
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.q.S) return;
    long o; int n;
    a.live[s] = scene_range(a.q, s, &o, &n) == ST_OK ? 1 : 0;
    a.best[s] = 0ULL;
    a.used[s] = 0;
}
struct RoundScatterArgs {
    const int* dense;        // B counts of this chunk (k_inlier_count_scenes_t: -1 for a scene that is not live)
    const int* status;       // B pose statuses
    long first, B;           // row b of the chunk is g' = first + b of the round
    long len;                // the round's hypotheses per scene
    long e_prev;             // ... the first of them
    long n_hyp;              // stride of `counts`
    const int* live;
    unsigned long long* best;
    int* counts;             // S x n_hyp
};
__global__ void __launch_bounds__(256) k_round_scatter(const RoundScatterArgs a) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const long g = a.first + b;
    const long s = g / a.len;
    if (a.live[s] == 0) return;                                              // (its range of `counts` keeps what it holds: -1 beyond used[s])
    const int c = a.status[b] != 0 ? -1 : a.dense[b];                        // k_robust_mark's rule
    a.counts[s * a.n_hyp + a.e_prev + (g - s * a.len)] = c;
    if (c >= 0) atomicMax(a.best + s, (unsigned long long)c + 1ULL);
}
struct RoundCloseArgs {
    RoundState r;
    long e_end;              // hypotheses per scene drawn after this round
    double qmin;             // -expm1(log1p(-confidence) / e_end), from the host
    int n_sample;
    int units;               // 1, or TFF_SCORE_UNITS when the counts are MSAC scores: best / units is a lower bound on the inliers
};
// does a scene of n correspondences whose best hypothesis has I inliers stop at the threshold qmin?  (the numpy twin: api.adaptive_stop)
__device__ __forceinline__ bool round_stops(const int I, const int n, const int n_sample, const double qmin) {
    if (I < 1) return false;
    const double w = (double)I / (double)n;
    double q = w;
    for (int k = 1; k < n_sample; ++k) q = q * w;
    return q >= qmin;
}
__global__ void __launch_bounds__(256) k_round_close(const RoundCloseArgs a) {
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.r.q.S || a.r.live[s] == 0) return;
    long o; int n;
    if (scene_range(a.r.q, s, &o, &n) != ST_OK) return;                      // (such a scene was never live: a guard)
    a.r.used[s] = (int)a.e_end;
    const int best = (int)a.r.best[s] - 1;
    if (round_stops(best >= 0 ? best / a.units : -1, n, a.n_sample, a.qmin)) a.r.live[s] = 0;
}

// ---- per-correspondence inlier flags with a scene lookup ---------------------------------------------------------------------------------------
struct ScenesMaskArgs {
    SceneSet q;
    const double* Rt2; const double* Rt3;    // B x 12
    long B;
    long per;                // item r belongs to scene r / per; its flags are the n_s bytes at mask + per * offsets[s] + (r % per) * n_s
    double thr;
    unsigned char* mask;
    int* counts;             // B or null: the row sums
    const int* alive;        // null, or B: nothing is done for an item with alive[r] < 0 (no such candidate)
    const int* gate;         // null, or S: nothing is done for a scene with gate[s] != 0 (the estimator's status)
};
// robust_kernel.h::k_inlier_mask per item: one wavefront per hypothesis, the cameras composed and pinned the same way
__global__ void __launch_bounds__(64, 4) k_scenes_mask(const ScenesMaskArgs a) {
    __shared__ double cam[3][12];
    const int lane = lane_id();
    for (long b = blockIdx.x; b < a.B; b += gridDim.x) {
        const long s = b / a.per;
        long o; int n;
        if (scene_range(a.q, s, &o, &n) != ST_OK) continue;
        if (a.gate && a.gate[s] != 0) continue;
        if (a.alive && a.alive[b] < 0) continue;
        const double* calm = a.q.calm + s * a.q.calm_stride;
        const double* scene = a.q.scenes + 6 * o;
        wave_sync();
        if (lane < 3) {
            const Mat3 K = load_K(calm, lane);
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
        unsigned char* row = a.mask + a.per * o + (b - s * a.per) * (long)n;
        int cnt = 0;
#pragma unroll 1
        for (int i = lane; i < n; i += WAVE) {
            int in = 0;
            count_if_inlier(P, Zt, cam[0], cam[1], cam[2], load_pt(scene, i), a.thr, in);
            row[i] = (unsigned char)in;
            cnt += in;
        }
        cnt = wave_sum_i(cnt);
        if (lane == 0 && a.counts) a.counts[b] = cnt;
    }
}

// ---- the candidates of all scenes: C = S * K of them, candidate r = scene r / K ------------------------------------------------------------------
// The state is RobustState's with K = C (poses, refits and the int arrays are C long); these two fields say how the C candidates map to scenes.
struct ScenesState {
    RobustState s;           // s.K = C; s.mask: the packed flags (K x n_s per scene, at K * offsets[s])
    SceneSet q;
    int K;                   // candidates per scene
    long cap;                // correspondences the packed refit batch holds (K * n_total: enough unless scenes overlap, which only malformed offsets do)
};
constexpr int SCENES_SCAN_THREADS = 1024;
// offsets[r + 1] = offsets[r] + (inliers of candidate r, 0 where there is no candidate): one workgroup, thread t owns a run of candidates, the
// runs' sums scanned in LDS (as k_ragged_scan).  The offsets stop at cap, so that no refit item reaches beyond the packed batch whatever the scenes' offsets hold
__global__ void __launch_bounds__(SCENES_SCAN_THREADS) k_scenes_offsets(const ScenesState a) {
    __shared__ long part[SCENES_SCAN_THREADS];
    const int t = (int)threadIdx.x;
    const long C = a.s.K;
    const long run = (C + SCENES_SCAN_THREADS - 1) / SCENES_SCAN_THREADS;
    const long lo = t * run < C ? t * run : C, hi = lo + run < C ? lo + run : C;
    long sum = 0;
    for (long r = lo; r < hi; ++r) sum += (a.s.cnt[r] >= 0) ? a.s.mask_cnt[r] : 0;
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < SCENES_SCAN_THREADS; d <<= 1) {                      // Hillis-Steele inclusive scan
        const long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long o = part[t] - sum;                                                  // exclusive prefix of this thread's run
    if (t == 0) a.s.offsets[0] = 0;
    for (long r = lo; r < hi; ++r) {
        o += (a.s.cnt[r] >= 0) ? a.s.mask_cnt[r] : 0;
        a.s.offsets[r + 1] = o < a.cap ? o : a.cap;
    }
}
// one workgroup per candidate walks its scene in tiles of 256: ballot + prefix over the four wavefronts keep the inliers in scene order
constexpr int ROBUST_COMPACT_THREADS = 256;
__global__ void __launch_bounds__(ROBUST_COMPACT_THREADS) k_scenes_compact(const ScenesState a) {
    __shared__ int wsum[ROBUST_COMPACT_THREADS / 64];
    const long r = (long)blockIdx.x;
    if (a.s.cnt[r] < 0) return;
    const long sc = r / a.K;
    long o; int n;
    if (scene_range(a.q, sc, &o, &n) != ST_OK) return;                       // (such a scene has no candidate: a guard)
    const unsigned char* m = a.s.mask + (long)a.K * o + (r - sc * a.K) * (long)n;
    const double* scene = a.q.scenes + 6 * o;
    const long end = a.s.offsets[r + 1];
    long base = a.s.offsets[r];
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
    for (int i0 = 0; i0 < n; i0 += ROBUST_COMPACT_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        const bool in = i < n && m[i] != 0;
        const unsigned long long bal = __ballot(in);
        if (lane == 0) wsum[w] = __popcll(bal);
        __syncthreads();
        int before = __popcll(bal & ((1ULL << lane) - 1ULL)), total = 0;
#pragma unroll
        for (int k = 0; k < ROBUST_COMPACT_THREADS / 64; ++k) { before += (k < w) ? wsum[k] : 0; total += wsum[k]; }
        const long slot = base + before;
        if (in && slot < end) {                                              // (slot < end always holds: the offsets are this mask's row sums)
            const double* q = scene + 6 * (long)i;
            double* d = a.s.packed + 6 * slot;
#pragma unroll
            for (int e = 0; e < 6; ++e) d[e] = q[e];
        }
        base += total;
        __syncthreads();
    }
}
struct ScenesFinishArgs {
    ScenesState a;
    double* Rt2; double* Rt3; double* T;     // S x 12, S x 12, S x 27
    int* info;               // S x 4
    int* status;             // S
};
// one wavefront per scene: the winner among the scene's K candidates; an invalid scene reports its status and reads no candidate
__global__ void __launch_bounds__(64) k_scenes_finish(const ScenesFinishArgs f) {
    const int lane = (int)threadIdx.x, K = f.a.K;
    const long sc = (long)blockIdx.x, C = f.a.s.K;
    long o; int n;
    const int st = scene_range(f.a.q, sc, &o, &n);
    int win = -1, best = -1, ncand = 0;
    if (st == ST_OK) {
        for (int r = 0; r < K; ++r) {
            const int c = f.a.s.cnt[sc * K + r];
            if (c >= 0) ++ncand;
            if (c > best) { best = c; win = r; }
        }
    }
    const long w = sc * K + win;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    if (lane < 12) {
        f.Rt2[sc * 12 + lane] = win >= 0 ? f.a.s.pose[w * 12 + lane] : qnan;
        f.Rt3[sc * 12 + lane] = win >= 0 ? f.a.s.pose[(C + w) * 12 + lane] : qnan;
    }
    if (lane < 27) f.T[sc * 27 + lane] = win >= 0 ? f.a.s.pose[C * 24 + w * 27 + lane] : qnan;
    if (lane == 0) {
        f.info[sc * 4 + 0] = win >= 0 ? best : 0;
        f.info[sc * 4 + 1] = win >= 0 ? f.a.s.seed_idx[w] : -1;
        f.info[sc * 4 + 2] = win >= 0 ? f.a.s.nref[w] : 0;
        f.info[sc * 4 + 3] = ncand;
        f.status[sc] = st != ST_OK ? st : (win >= 0 ? ST_OK : ST_NO_POSE);
    }
}

// TFF_OPT_SCORE = 1 only: k_scenes_finish put the winner's SCORE into info[0]; the row sums of the final k_scenes_mask launch (the number of set flags of
// each returned mask, written for the scenes with status 0) take its place
struct ScenesInfoArgs { const int* flags; const int* status; int* info; long S; };
__global__ void __launch_bounds__(256) k_scenes_info(const ScenesInfoArgs a) {
    const long sc = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (sc < a.S && a.status[sc] == 0) a.info[sc * 4] = a.flags[sc];
}

}  // namespace tff
