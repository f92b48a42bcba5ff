// TEST INFRASTRUCTURE ONLY: the kernels of csrc/robust_scenes_kernel.h (and k_robust_topk, k_repr_error as their references) compiled by g++ against the
// lane emulator (hip_emu.h), for tests/test_emulated_scenes.py.  emu_primitives.h: what robust_kernel.h uses beyond wave.h.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "robust_scenes_kernel.h"
using namespace tff;
static SceneSet mk(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs) {
    return SceneSet{scenes, off, S, n_total, ns_max, n_min, calm, cs};
}
extern "C" {
void e_sample(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
              unsigned long long seed, long first, const unsigned long long* keys, long B, long per, int n, int* out, double* calm_out) {
    ScenesSampleArgs a{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), seed, first, keys, B, per, n, out, calm_out};
    emu::launch(k_scenes_sample, (unsigned)((B + 255) / 256), 256, 0, a);
}
void e_count(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
             const double* Rt2, const double* Rt3, long first, long B, long per, long slab, double thr, int* counts, int stage) {
    ScenesCountArgs a{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), Rt2, Rt3, first, B, per, slab, thr, counts, stage};
    emu::launch(k_inlier_count_scenes, (unsigned)((B + slab - 1) / slab), 256, (576 + (size_t)stage) * 8, a);
}
void e_count_one(const double* scene, int Ns, const double* calm, const double* Rt2, const double* Rt3, long B, double thr, int* counts) {
    ReprErrorArgs a{nullptr, 0, calm, Rt2, Rt3, scene, 0, nullptr, B, Ns, thr, nullptr, counts};
    emu::launch(k_repr_error, (unsigned)B, 64, 0, a);
}
void e_mask(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
            const double* Rt2, const double* Rt3, long B, long per, double thr, unsigned char* mask, int* counts, const int* alive, const int* gate) {
    ScenesMaskArgs a{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), Rt2, Rt3, B, per, thr, mask, counts, alive, gate};
    emu::launch(k_scenes_mask, (unsigned)B, 64, 0, a);
}
// offsets + compact + finish on given candidate state
void e_cand(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs, int K,
            int* cnt, int* seed_idx, int* nref, double* pose, const unsigned char* mask, const int* mask_cnt, long* offsets, double* packed, long cap,
            double* Rt2, double* Rt3, double* T, int* info, int* status) {
    ScenesState st{};
    st.q = mk(scenes, off, S, n_total, ns_max, n_min, calm, cs); st.K = K; st.cap = cap;
    st.s.K = S * K; st.s.cnt = cnt; st.s.seed_idx = seed_idx; st.s.nref = nref; st.s.pose = pose; st.s.mask = mask; st.s.mask_cnt = mask_cnt;
    st.s.offsets = offsets; st.s.packed = packed;
    emu::launch(k_scenes_offsets, 1, SCENES_SCAN_THREADS, 0, st);
    emu::launch(k_scenes_compact, (unsigned)(S * K), ROBUST_COMPACT_THREADS, 0, st);
    emu::launch(k_scenes_finish, (unsigned)S, 64, 0, ScenesFinishArgs{st, Rt2, Rt3, T, info, status});
}
void e_topk(const int* counts, long n_hyp, unsigned long long* sel, int K, int rounds, unsigned grid) {
    for (int r = 0; r < rounds; ++r) emu::launch(k_robust_topk, grid, ROBUST_TOPK_THREADS, 0, RobustTopkArgs{counts, n_hyp, sel, r, K});
}
}
