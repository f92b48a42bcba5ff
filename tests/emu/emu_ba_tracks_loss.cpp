// TEST INFRASTRUCTURE ONLY: the ten instances of the bundle adjustment over tracks with a robust loss (csrc/ba_tracks_loss_kernel.h:
// k_bundle_adjust_tracks_loss<2 .. 6, Huber | Cauchy>) and the weight kernel of the TFF_LOSS_NONE route, compiled by g++ against the lane emulator
// (hip_emu.h), for tests/test_emulated_ba_tracks_loss.py.
#include "emu_primitives.h"
#include "launch.h"
#include "ba_tracks_loss_kernel.h"
using namespace tff;
namespace {
template <int M> void emu_batl(int loss, const BatLossArgs& a) {
    const unsigned B = (unsigned)a.t.v.B;
    if (loss == BA_LOSS_HUBER) emu::launch(k_bundle_adjust_tracks_loss<M, BA_LOSS_HUBER>, B, 64, bav_lds_bytes<M>(a.t.v.N), a);
    else emu::launch(k_bundle_adjust_tracks_loss<M, BA_LOSS_CAUCHY>, B, 64, bav_lds_bytes<M>(a.t.v.N), a);
}
template <int M> void emu_bat(const BatArgs& a) { emu::launch(k_bundle_adjust_tracks<M>, (unsigned)a.v.B, 64, bav_lds_bytes<M>(a.v.N), a); }
}
extern "C" {
// the call as launch_bundle_adjust_tracks_loss (capi.hip) makes it; loss 0 launches k_bundle_adjust_tracks itself and the weight kernel.  Returns -1 for
// a number of views or a loss it has no instance for.
int e_ba_tracks_loss(int M, const double* calm, long calm_stride, const double* Rt_in, const double* corresp, long B, int N, const double* reconst0, double* Rt,
                     double* reconst, int* iter, double* repr_err, int* used, int* status, int loss, double scale, double* weight) {
    if (M < 2 || M > 6 || loss < BA_LOSS_NONE || loss > BA_LOSS_CAUCHY) return -1;
    const BatArgs t{BavArgs{calm, calm_stride, Rt_in, corresp, B, N, reconst0, Rt, reconst, iter, repr_err, status}, used};
    if (loss == BA_LOSS_NONE) {
        switch (M) {
            case 2: emu_bat<2>(t); break;
            case 3: emu_bat<3>(t); break;
            case 4: emu_bat<4>(t); break;
            case 5: emu_bat<5>(t); break;
            default: emu_bat<6>(t); break;
        }
        if (weight) emu::launch(k_bat_weight_ones, 2u, 256, 0, BatOnesArgs{weight, corresp, status, B, N, M});
        return 0;
    }
    const BatLossArgs a{t, scale, weight};
    switch (M) {
        case 2: emu_batl<2>(loss, a); break;
        case 3: emu_batl<3>(loss, a); break;
        case 4: emu_batl<4>(loss, a); break;
        case 5: emu_batl<5>(loss, a); break;
        default: emu_batl<6>(loss, a); break;
    }
    return 0;
}
}
