// TEST INFRASTRUCTURE ONLY: the three instances of the bundle-adjustment kernel (csrc/ba_kernel.h: k_bundle_adjust, k_bundle_adjust_loss<1 | 2>) and the
// weight kernels around them (csrc/ba_loss_kernel.h), compiled by g++ against the lane emulator (hip_emu.h), for tests/test_emulated_ba_loss.py.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "ba_loss_kernel.h"
using namespace tff;
extern "C" {
// the fixed-N call as launch_bundle_adjust (capi.hip) makes it; loss 0 launches k_bundle_adjust itself.  Returns -1 for an unknown loss.
int e_ba_loss_fixed(const double* calm, long calm_stride, const double* Rt2_in, const double* Rt3_in, const double* corresp, long B, int N, const double* reconst0,
                    double* Rt2, double* Rt3, double* reconst, int* iter, double* repr_err, int* status, int loss, double scale, double* weight) {
    BaArgs a{calm, calm_stride, Rt2_in, Rt3_in, corresp, B, N, reconst0, Rt2, Rt3, reconst, iter, repr_err, status};
    if (loss == BA_LOSS_NONE) {
        emu::launch(k_bundle_adjust, (unsigned)B, 64, ba_lds_bytes(N), a);
        if (weight) emu::launch(k_ba_weight_ones, 2u, 256, 0, BaOnesArgs{weight, status, B, N});
        return 0;
    }
    BaLossArgs la;
    static_cast<BaArgs&>(la) = a;
    la.scale = scale; la.weight = weight;
    if (loss == BA_LOSS_HUBER) emu::launch(k_bundle_adjust_loss<BA_LOSS_HUBER>, (unsigned)B, 64, ba_lds_bytes(N), la);
    else if (loss == BA_LOSS_CAUCHY) emu::launch(k_bundle_adjust_loss<BA_LOSS_CAUCHY>, (unsigned)B, 64, ba_lds_bytes(N), la);
    else return -1;
    return 0;
}
// the chain of launch_ba_ragged (capi.hip) with a loss and the class bounds of the caller; the workspaces are the function's own
int e_ba_loss_ragged(const double* corresp, const long* offsets, long B, long n_total, const unsigned char* mask, const double* calm, long calm_stride,
                     const double* Rt2_in, const double* Rt3_in, const double* reconst0, const int* bounds, double* Rt2, double* Rt3, double* reconst, int* iter,
                     double* repr_err, int* used, int* status, int loss, double scale, double* weight) {
    const size_t nt = (size_t)n_total + 1, nb = (size_t)B + 1;
    std::vector<int> m(nb), cls_count(BA_CLASSES, 0), cls_list(BA_CLASSES * nb), src(nt);
    std::vector<long> coff(nb);
    std::vector<double> packed(6 * nt), rec0(3 * nt), rec_ws(3 * nt), w_ws(nt);
    BaRaggedPlan p{};
    p.offsets = offsets; p.B = B; p.n_total = n_total; p.mask = mask;
    for (int k = 0; k < BA_CLASSES; ++k) p.bound[k] = bounds[k];
    p.m = m.data(); p.coff = coff.data(); p.cls_count = cls_count.data(); p.cls_list = cls_list.data();
    p.corresp = corresp; p.reconst0 = reconst0; p.packed = packed.data(); p.rec0 = rec0.data(); p.src = src.data(); p.rec_ws = rec_ws.data();
    p.Rt2 = Rt2; p.Rt3 = Rt3; p.reconst = reconst; p.iter = iter; p.repr_err = repr_err; p.used = used; p.status = status;
    emu::launch(k_ba_ragged_count, (unsigned)B, 64, 0, p);
    if (mask) emu::launch(k_ba_ragged_scan, 1, BA_RAGGED_SCAN_THREADS, 0, p);
    emu::launch(k_ba_ragged_classes, (unsigned)((B + 255) / 256), 256, 0, p);
    if (mask) emu::launch(k_ba_ragged_compact, (unsigned)B, BA_RAGGED_TILE, 0, p);
    for (int k = 0; k < BA_CLASSES; ++k) {
        const BaLossArgs la = ba_ragged_class_loss_args(p, calm, calm_stride, Rt2_in, Rt3_in, rec_ws.data(), k, scale, w_ws.data(), weight);
        if (loss == BA_LOSS_NONE) emu::launch(k_bundle_adjust, (unsigned)B, 64, ba_lds_bytes(bounds[k]), static_cast<const BaArgs&>(la));
        else if (loss == BA_LOSS_HUBER) emu::launch(k_bundle_adjust_loss<BA_LOSS_HUBER>, (unsigned)B, 64, ba_lds_bytes(bounds[k]), la);
        else if (loss == BA_LOSS_CAUCHY) emu::launch(k_bundle_adjust_loss<BA_LOSS_CAUCHY>, (unsigned)B, 64, ba_lds_bytes(bounds[k]), la);
        else return -1;
    }
    if (reconst) emu::launch(k_ba_ragged_scatter, (unsigned)B, BA_RAGGED_TILE, 0, p);
    if (weight) emu::launch(k_ba_ragged_weight, (unsigned)B, BA_RAGGED_TILE, 0, BaRaggedWeights{p, w_ws.data(), weight, loss == BA_LOSS_NONE});
    return 0;
}
// the kernel as it was launched before there were losses (what tests/emu/emu_ba_ragged.cpp calls e_ba_fixed)
void e_ba_plain(const double* calm, long calm_stride, const double* Rt2_in, const double* Rt3_in, const double* corresp, long B, int N, const double* reconst0,
                double* Rt2, double* Rt3, double* reconst, int* iter, double* repr_err, int* status) {
    BaArgs a{calm, calm_stride, Rt2_in, Rt3_in, corresp, B, N, reconst0, Rt2, Rt3, reconst, iter, repr_err, status};
    emu::launch(k_bundle_adjust, (unsigned)B, 64, ba_lds_bytes(N), a);
}
}
