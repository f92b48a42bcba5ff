// TEST INFRASTRUCTURE ONLY: what the adaptive robust call adds -- the sampler's hypothesis base and liveness, the kernels that close a round
// (csrc/robust_scenes_kernel.h) and the early exit of the exact-tier row kernels for a wavefront of dead rows -- compiled by g++ against the lane
// emulator (hip_emu.h), for tests/test_emulated_adaptive.py.  emu_primitives.h: what robust_kernel.h uses beyond wave.h.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "robust_scenes_kernel.h"
using namespace tff;
static SceneSet mk(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs) {
    return SceneSet{scenes, off, S, n_total, ns_max, n_min, calm, cs};
}
extern "C" {
// k_scenes_sample over the rows [first, first + B) of a round of `len` hypotheses per scene starting at hypothesis `base`
void a_sample(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
              unsigned long long seed, long first, long B, long len, int n, int* out, double* calm_out, long base, const int* live) {
    ScenesSampleArgs a{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), seed, first, nullptr, B, len, n, out, calm_out, base, live};
    emu::launch(k_scenes_sample, (unsigned)((B + 255) / 256), 256, 0, a);
}
// the count kernel with liveness
void a_count(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
             const double* Rt2, const double* Rt3, long first, long B, long per, long slab, double thr, int* counts, int stage, const int* live) {
    ScenesCountArgs a{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), Rt2, Rt3, first, B, per, slab, thr, counts, stage, 0.0, live};
    emu::launch(k_inlier_count_scenes, (unsigned)((B + slab - 1) / slab), 256, (576 + (size_t)stage) * 8, a);
}
void a_round_init(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
                  int* live, unsigned long long* best, int* used) {
    emu::launch(k_round_init, (unsigned)((S + 255) / 256), 256, 0, RoundState{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), live, best, used});
}
void a_round_scatter(const int* dense, const int* status, long first, long B, long len, long e_prev, long n_hyp, const int* live,
                     unsigned long long* best, int* counts) {
    emu::launch(k_round_scatter, (unsigned)((B + 255) / 256), 256, 0, RoundScatterArgs{dense, status, first, B, len, e_prev, n_hyp, live, best, counts});
}
void a_round_close(const double* scenes, const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs,
                   int* live, unsigned long long* best, int* used, long e_end, double qmin, int n_sample, int units) {
    const RoundState r{mk(scenes, off, S, n_total, ns_max, n_min, calm, cs), live, best, used};
    emu::launch(k_round_close, (unsigned)((S + 255) / 256), 256, 0, RoundCloseArgs{r, e_end, qmin, n_sample, units});
}
// the exact-tier row kernel of a method alone (no fix-up) on sampled hypotheses of a packed array: row b gathers idx[b * n ..], CalM per row
void a_rows_exact(int linear_f, const double* scenes, int n_total, const double* calm, const int* idx, long B, int n, double* Rt2, double* Rt3, double* T,
                  int* status) {
    LinearTftArgs a{scenes, calm, 27, B, n, 0, Rt2, Rt3, T, nullptr, nullptr, status, nullptr, idx, nullptr, nullptr, nullptr, 0, n_total};
    if (linear_f) emu::launch(k_linear_f_pose_rows_exact, rows_grid(B), 64, rows_lds_bytes(), a);
    else emu::launch(k_linear_tft_pose_rows_exact, rows_grid(B), 64, rows_lds_bytes(), a);
}
}
