// TEST INFRASTRUCTURE ONLY: the fifteen instances of the covariance kernel of the bundle adjustment over tracks (csrc/ba_tracks_cov_kernel.h:
// k_ba_tracks_cov<2 .. 6, none | Huber | Cauchy>), compiled by g++ against the lane emulator (hip_emu.h), for tests/test_emulated_ba_tracks_cov.py.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "ba_tracks_cov_kernel.h"
using namespace tff;
namespace {
template <int M> void emu_batc(int loss, const BatCovArgs& a) {
    const unsigned B = (unsigned)a.B;
    if (loss == BA_LOSS_NONE) emu::launch(k_ba_tracks_cov<M, BA_LOSS_NONE>, B, 64, batc_lds_bytes<M>(), a);
    else if (loss == BA_LOSS_HUBER) emu::launch(k_ba_tracks_cov<M, BA_LOSS_HUBER>, B, 64, batc_lds_bytes<M>(), a);
    else emu::launch(k_ba_tracks_cov<M, BA_LOSS_CAUCHY>, B, 64, batc_lds_bytes<M>(), a);
}
}
extern "C" {
// the call as launch_ba_tracks_cov (capi.hip) makes it; the workspace of the moved points is the function's own.  Returns -1 for a number of views or a
// loss it has no instance for.
int e_ba_tracks_cov(int M, const double* calm, long calm_stride, const double* Rt, const double* corresp, long B, int N, const double* reconst, int loss,
                    double scale, double* cov, double* sigma0, double* point_cov) {
    if (M < 2 || M > 6 || loss < BA_LOSS_NONE || loss > BA_LOSS_CAUCHY) return -1;
    std::vector<double> xwork((size_t)B * 3 * (size_t)N + 1);
    const BatCovArgs a{calm, calm_stride, Rt, corresp, B, N, reconst, scale, xwork.data(), cov, sigma0, point_cov};
    switch (M) {
        case 2: emu_batc<2>(loss, a); break;
        case 3: emu_batc<3>(loss, a); break;
        case 4: emu_batc<4>(loss, a); break;
        case 5: emu_batc<5>(loss, a); break;
        default: emu_batc<6>(loss, a); break;
    }
    return 0;
}
}
