// TEST INFRASTRUCTURE ONLY: the five instances of the bundle adjustment over tracks (csrc/ba_tracks_kernel.h: k_bundle_adjust_tracks<2 .. 6>), compiled by
// g++ against the lane emulator (hip_emu.h), for tests/test_emulated_ba_tracks.py.
#include "emu_primitives.h"
#include "launch.h"
#include "ba_tracks_kernel.h"
using namespace tff;
namespace {
template <int M> void emu_bat(const BatArgs& a) { emu::launch(k_bundle_adjust_tracks<M>, (unsigned)a.v.B, 64, bav_lds_bytes<M>(a.v.N), a); }
}
extern "C" {
// the call as launch_bundle_adjust_tracks (capi.hip) makes it.  Returns -1 for a number of views it has no instance for.
int e_ba_tracks(int M, const double* calm, long calm_stride, const double* Rt_in, const double* corresp, long B, int N, const double* reconst0, double* Rt,
                double* reconst, int* iter, double* repr_err, int* used, int* status) {
    const BatArgs a{BavArgs{calm, calm_stride, Rt_in, corresp, B, N, reconst0, Rt, reconst, iter, repr_err, status}, used};
    switch (M) {
        case 2: emu_bat<2>(a); break;
        case 3: emu_bat<3>(a); break;
        case 4: emu_bat<4>(a); break;
        case 5: emu_bat<5>(a); break;
        case 6: emu_bat<6>(a); break;
        default: return -1;
    }
    return 0;
}
}
