// TEST INFRASTRUCTURE ONLY: the count kernels of csrc/blocks_kernel.h and csrc/robust_scenes_kernel.h in their count and MSAC forms (TFF_OPT_SCORE), and
// k_triangulate as the source of the reference's points, compiled by g++ against the lane emulator (hip_emu.h), for tests/test_emulated_score.py.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "robust_scenes_kernel.h"
using namespace tff;
static ReprErrorArgs one(const double* scene, int Ns, const double* calm, const double* Rt2, const double* Rt3, long B, double thr, double c, int* counts,
                         double* err) {
    ReprErrorArgs a{nullptr, 0, calm, Rt2, Rt3, scene, 0, nullptr, B, Ns, thr, err, counts};
    a.score_c = c;
    return a;
}
extern "C" {
// cams: B x 3 cameras, 3 x 4 column-major each; the scene (N x 6) is every item's points
void s_triangulate(const double* cams, const double* scene, long B, int N, double* X) {
    std::vector<double> pts((size_t)B * 6 * N);
    for (long b = 0; b < B; ++b) std::memcpy(pts.data() + (size_t)b * 6 * N, scene, sizeof(double) * 6 * N);
    emu::launch(k_triangulate, (unsigned)B, 64, 0, TriangulateArgs{cams, 36, pts.data(), B, 3, N, X});
}
// one wavefront per hypothesis; err may be null
void s_repr(const double* scene, int Ns, const double* calm, const double* Rt2, const double* Rt3, long B, double thr, double c, int* counts, double* err,
            int msac) {
    emu::launch(msac ? k_repr_error_msac : k_repr_error, (unsigned)B, 64, 0, one(scene, Ns, calm, Rt2, Rt3, B, thr, c, counts, err));
}
void s_staged(const double* scene, int Ns, const double* calm, const double* Rt2, const double* Rt3, long B, double thr, double c, int* counts, int msac) {
    emu::launch(msac ? k_inlier_count_staged_msac : k_inlier_count_staged, (unsigned)((B + INLIER_WG_WAVES - 1) / INLIER_WG_WAVES), 64 * INLIER_WG_WAVES,
                ((size_t)6 * Ns + 36 * INLIER_WG_WAVES) * 8, one(scene, Ns, calm, Rt2, Rt3, B, thr, c, counts, nullptr));
}
// four hypotheses per wavefront: one workgroup serves 16
void s_rows(const double* scene, int Ns, const double* calm, const double* Rt2, const double* Rt3, long B, double thr, double c, int* counts, int msac) {
    const long per_wg = 4L * INLIER_WG_WAVES;
    emu::launch(msac ? k_inlier_count_rows_msac : k_inlier_count_rows, (unsigned)((B + per_wg - 1) / per_wg), 64 * INLIER_WG_WAVES,
                ((size_t)6 * Ns + 36 * 4 * INLIER_WG_WAVES) * 8, one(scene, Ns, calm, Rt2, Rt3, B, thr, c, counts, nullptr));
}
void s_scenes(const double* scenes, const long* off, long S, long n_total, int ns_max, const double* calm, const double* Rt2, const double* Rt3, long B,
              long per, long slab, double thr, double c, int* counts, int stage, int msac) {
    ScenesCountArgs a{SceneSet{scenes, off, S, n_total, ns_max, 0, calm, 27}, Rt2, Rt3, 0, B, per, slab, thr, counts, stage};
    a.score_c = c;
    emu::launch(msac ? k_inlier_count_scenes_msac : k_inlier_count_scenes, (unsigned)((B + slab - 1) / slab), 64 * INLIER_WG_WAVES,
                ((size_t)36 * SCENES_COUNT_ROWS + (size_t)stage) * 8, a);
}
}
