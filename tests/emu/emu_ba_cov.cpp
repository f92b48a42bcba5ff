// TEST INFRASTRUCTURE ONLY: the three instances of the covariance kernel of the bundle adjustment (csrc/ba_cov_kernel.h: k_ba_cov<0 | 1 | 2>) and the
// kernels around its ragged form, compiled by g++ against the lane emulator (hip_emu.h), for tests/test_emulated_ba_cov.py.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "ba_cov_kernel.h"
using namespace tff;
namespace {
int launch_cov(int loss, unsigned grid, const BaCovArgs& a) {
    if (loss == BA_LOSS_NONE) emu::launch(k_ba_cov<BA_LOSS_NONE>, grid, 64, ba_cov_lds_bytes(), a);
    else if (loss == BA_LOSS_HUBER) emu::launch(k_ba_cov<BA_LOSS_HUBER>, grid, 64, ba_cov_lds_bytes(), a);
    else if (loss == BA_LOSS_CAUCHY) emu::launch(k_ba_cov<BA_LOSS_CAUCHY>, grid, 64, ba_cov_lds_bytes(), a);
    else return -1;
    return 0;
}
}
extern "C" {
// the fixed-N call as launch_ba_cov (capi.hip) makes it.  Returns -1 for an unknown loss.
int e_ba_cov_fixed(const double* calm, long calm_stride, const double* Rt2, const double* Rt3, const double* corresp, long B, int N, const double* reconst,
                   int loss, double scale, double* cov, double* sigma0, double* point_cov) {
    return launch_cov(loss, (unsigned)B, BaCovArgs{calm, calm_stride, Rt2, Rt3, corresp, B, N, reconst, scale, cov, sigma0, point_cov});
}
// the chain of launch_ba_cov_ragged (capi.hip); the workspaces are the function's own.  bounds: the class bounds of the plan, which this chain has no use
// for (the library passes INT32_MAX three times); `status` receives the plan's statuses.
int e_ba_cov_ragged(const double* corresp, const long* offsets, long B, long n_total, const unsigned char* mask, const double* calm, long calm_stride,
                    const double* Rt2, const double* Rt3, const double* reconst, const int* bounds, int loss, double scale, double* cov, double* sigma0,
                    double* point_cov, int* status) {
    const size_t nt = (size_t)n_total + 1, nb = (size_t)B + 1;
    std::vector<int> m(nb), src(nt);
    std::vector<long> coff(nb);
    std::vector<double> packed(6 * nt), rec0(3 * nt), pc_ws(6 * nt), f2(12 * nb), f3(12 * nb);
    BaRaggedPlan p{};
    p.offsets = offsets; p.B = B; p.n_total = n_total; p.mask = mask;
    for (int k = 0; k < BA_CLASSES; ++k) p.bound[k] = bounds[k];
    p.m = m.data(); p.coff = coff.data();
    p.corresp = corresp; p.reconst0 = reconst; p.packed = packed.data(); p.rec0 = rec0.data(); p.src = src.data();
    p.Rt2 = f2.data(); p.Rt3 = f3.data(); p.status = status;
    emu::launch(k_ba_ragged_count, (unsigned)B, 64, 0, p);
    if (mask) {
        emu::launch(k_ba_ragged_scan, 1, BA_RAGGED_SCAN_THREADS, 0, p);
        emu::launch(k_ba_ragged_compact, (unsigned)B, BA_RAGGED_TILE, 0, p);
    }
    if (launch_cov(loss, (unsigned)B, ba_cov_ragged_args(p, calm, calm_stride, Rt2, Rt3, scale, cov, sigma0, pc_ws.data(), point_cov))) return -1;
    if (point_cov) emu::launch(k_ba_cov_scatter, (unsigned)B, BA_RAGGED_TILE, 0, BaCovScatter{p, pc_ws.data(), point_cov});
    return 0;
}
}
