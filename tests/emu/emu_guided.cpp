// TEST INFRASTRUCTURE ONLY: the kernels of the guided (PROSAC) sampler (csrc/robust_guided_kernel.h) compiled by g++ against the lane emulator
// (hip_emu.h), for tests/test_emulated_guided.py.  emu_primitives.h: what robust_kernel.h uses beyond wave.h.
#include <vector>
#include "emu_primitives.h"
inline int __shfl_up(int v, unsigned d, int) {                               // (every lane exchanges; the lanes below d keep their own value)
    const unsigned lane = emu::tl_threadIdx.x & 63u;
    const int u = (int)(unsigned)emu::exchange((uint64_t)(unsigned)v, (int)((lane - d) & 63u));
    return lane >= d ? u : v;
}
#include "launch.h"
#include "robust_guided_kernel.h"
using namespace tff;
static SceneSet mk(const long* off, long S, long n_total, int ns_max, int n_min, const double* calm, long cs) {
    return SceneSet{nullptr, off, S, n_total, ns_max, n_min, calm, cs};
}
extern "C" {
// k_guided_ends over S scenes with `blocks` workgroups (fewer than S: a workgroup serves several scenes)
void g_ends(const long* off, long S, long n_total, int ns_max, int m, long growth, int* ends, int blocks) {
    emu::launch(k_guided_ends, (unsigned)blocks, GUIDED_ENDS_THREADS, 0, GuidedEndsArgs{mk(off, S, n_total, ns_max, m, nullptr, 0), growth, m, ends});
}
// k_scenes_sample_guided: the rows [first, first + B) of `len` hypotheses per scene starting at hypothesis `base`, or (keys non-null) the re-draw of
// len candidates per scene from their selection keys
void g_sample(const long* off, long S, long n_total, int ns_max, int m, const double* calm, long cs, unsigned long long seed, long first,
              const unsigned long long* keys, long B, long len, int* out, double* calm_out, long base, const int* live, const int* ends, const int* order) {
    ScenesSampleArgs a{mk(off, S, n_total, ns_max, m, calm, cs), seed, first, keys, B, len, m, out, calm_out, base, live};
    emu::launch(k_scenes_sample_guided, (unsigned)((B + 255) / 256), 256, 0, ScenesSampleGuidedArgs{a, ends, order});
}
// k_scenes_sample, the uniform sampler, over the same rows
void g_sample_uniform(const long* off, long S, long n_total, int ns_max, int m, const double* calm, long cs, unsigned long long seed, long first,
                      const unsigned long long* keys, long B, long len, int* out, double* calm_out, long base, const int* live) {
    ScenesSampleArgs a{mk(off, S, n_total, ns_max, m, calm, cs), seed, first, keys, B, len, m, out, calm_out, base, live};
    emu::launch(k_scenes_sample, (unsigned)((B + 255) / 256), 256, 0, a);
}
// k_sample_indices_guided for one scene whose table is `ends`
void g_sample_one(unsigned long long seed, long first, long B, int m, int Ns, int* out, const int* ends, const int* order) {
    emu::launch(k_sample_indices_guided, (unsigned)((B + 255) / 256), 256, 0, SampleGuidedArgs{SampleArgs{seed, first, B, m, Ns, out}, ends, order});
}
}
