// TEST INFRASTRUCTURE ONLY: the chain of csrc/ba_ragged_kernel.h around k_bundle_adjust, compiled by g++ against the lane emulator (hip_emu.h), for
// tests/test_emulated_ba_ragged.py.  The caller owns every workspace, so the test can look at the plan.
#include <vector>
#include "emu_primitives.h"
#include "launch.h"
#include "ba_ragged_kernel.h"
using namespace tff;
extern "C" {
// the chain of launch_ba_ragged (capi.hip) with the class bounds of the caller; status must not be null
void e_ba_ragged(const double* corresp, const long* offsets, long B, long n_total, const unsigned char* mask, const double* calm, long calm_stride,
                 const double* Rt2_in, const double* Rt3_in, const double* reconst0, const int* bounds,
                 int* m, long* coff, int* cls_count, int* cls_list, double* packed, double* rec0, int* src, double* rec_ws,
                 double* Rt2, double* Rt3, double* reconst, int* iter, double* repr_err, int* used, int* status) {
    BaRaggedPlan p{};
    p.offsets = offsets; p.B = B; p.n_total = n_total; p.mask = mask;
    for (int k = 0; k < BA_CLASSES; ++k) { p.bound[k] = bounds[k]; cls_count[k] = 0; }
    p.m = m; p.coff = coff; p.cls_count = cls_count; p.cls_list = cls_list;
    p.corresp = corresp; p.reconst0 = reconst0; p.packed = packed; p.rec0 = rec0; p.src = src; p.rec_ws = rec_ws;
    p.Rt2 = Rt2; p.Rt3 = Rt3; p.reconst = reconst; p.iter = iter; p.repr_err = repr_err; p.used = used; p.status = status;
    emu::launch(k_ba_ragged_count, (unsigned)B, 64, 0, p);
    if (mask) emu::launch(k_ba_ragged_scan, 1, BA_RAGGED_SCAN_THREADS, 0, p);
    emu::launch(k_ba_ragged_classes, (unsigned)((B + 255) / 256), 256, 0, p);
    if (mask) emu::launch(k_ba_ragged_compact, (unsigned)B, BA_RAGGED_TILE, 0, p);
    for (int k = 0; k < BA_CLASSES; ++k)
        emu::launch(k_bundle_adjust, (unsigned)B, 64, ba_lds_bytes(bounds[k]), ba_ragged_class_args(p, calm, calm_stride, Rt2_in, Rt3_in, rec_ws, k));
    if (reconst) emu::launch(k_ba_ragged_scatter, (unsigned)B, BA_RAGGED_TILE, 0, p);
}
// the fixed-N call (what tff_bundle_adjust_batch_dev launches)
void e_ba_fixed(const double* calm, long calm_stride, const double* Rt2_in, const double* Rt3_in, const double* corresp, long B, int N, const double* reconst0,
                double* Rt2, double* Rt3, double* reconst, int* iter, double* repr_err, int* status) {
    BaArgs a{calm, calm_stride, Rt2_in, Rt3_in, corresp, B, N, reconst0, Rt2, Rt3, reconst, iter, repr_err, status};
    emu::launch(k_bundle_adjust, (unsigned)B, 64, ba_lds_bytes(N), a);
}
}
