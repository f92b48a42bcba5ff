// TEST INFRASTRUCTURE ONLY: the ragged chain of OptimFPoseEstimation (capi.hip::launch_ragged_optim_f) and the fixed-N chain (launch_optim_f) on the
// lane emulator of tests/emu/hip_emu.h, with the two storage bounds of the refinement passed in so that small items reach all three launch classes.
// Never linked into libtftfund.so.
#include <vector>
#include "../../tft_vs_fund_amd/csrc/launch.h"
#include "../../tft_vs_fund_amd/csrc/ragged_kernel.h"

namespace {
constexpr int W = tff::OPTIMF_REFINE_WAVES;
int cut_at(int upto, int least, int n_max) { const long k = (long)upto + 1 > least ? (long)upto + 1 : least; return (int)(k > n_max ? (long)n_max + 1 : k); }
}

// split: items below it go to the exact kernel whole; stage_upto / xi_upto: the bounds tff_optim_f_ragged_bounds reports for the library.
// route_out: the plan's RAGGED_ROUTE_INTS entries; list_out: `slots` entries (ragged_slots(B, n_max)), filled up to route_out[3].
extern "C" int e_optimf_ragged(const double* corresp, const long* offsets, long B, int n_max, const double* calm, long calm_stride, int split, int stage_upto,
                               int xi_upto, double* Rt2, double* Rt3, double* T, double* reconst, int* iter, int* status, int* route_out, int* list_out) {
    const size_t nb = (size_t)n_max + 1;
    const long slots = tff::ragged_slots(B, n_max);
    std::vector<int> ws(3 * nb + tff::RAGGED_ROUTE_INTS + (size_t)slots, -9);
    for (size_t k = 0; k < 2 * nb; ++k) ws[k] = 0;
    std::vector<int> retry((size_t)B + 2, 0);
    tff::RaggedPlanArgs pa{};
    pa.offsets = offsets; pa.B = B; pa.n_max = n_max;
    pa.split = split > n_max ? n_max + 1 : split;
    pa.hist = ws.data(); pa.fill = ws.data() + nb; pa.start = ws.data() + 2 * nb; pa.route = ws.data() + 3 * nb; pa.list = pa.route + tff::RAGGED_ROUTE_INTS;
    pa.Rt2 = Rt2; pa.Rt3 = Rt3; pa.T = T; pa.iter = iter; pa.status = status;
    pa.cut[0] = cut_at(stage_upto, pa.split, n_max);
    pa.cut[1] = cut_at(xi_upto, pa.cut[0], n_max);
    pa.retry_list = retry.data() + 2; pa.retry_count = retry.data();
    const unsigned items = (unsigned)((B + 255) / 256);
    emu::launch(tff::k_ragged_count, items, 256, 0, pa);
    emu::launch(tff::k_ragged_scan, 1, tff::RAGGED_SCAN_THREADS, 0, pa);
    emu::launch(tff::k_ragged_scatter, items, 256, 0, pa);
    for (int k = 0; k < tff::RAGGED_ROUTE_INTS; ++k) route_out[k] = pa.route[k];
    for (long k = 0; k < slots; ++k) list_out[k] = pa.list[k];

    std::vector<double> rec((size_t)B * tff::OPTIMF_REC_DOUBLES, 0.0);
    tff::OptimFStageArgs sa{};
    sa.la = tff::LinearTftArgs{corresp, calm, calm_stride, B, 0, reconst ? tff::FLAG_RECONST : 0, Rt2, Rt3, T, reconst, iter, status};
    sa.la.retry_count = retry.data(); sa.la.retry_zero = retry.data() + 1; sa.la.retry_list = retry.data() + 2;
    sa.la.offsets = offsets; sa.la.rlist = pa.list; sa.la.stage_upto = -1;
    sa.rec = rec.data();
    const unsigned rows = tff::rows_grid(slots), waves = 3;                      // (three blocks: the refinement's grid-stride loop takes several items through one LDS)
    const long stride = 4 * (long)n_max + 16;
    std::vector<double> slices((size_t)waves * stride, 0.0);
    sa.la.rrange = pa.route + 2;
    emu::launch(tff::k_optimf_linear_rows_ragged, rows, 64, tff::rows_lds_bytes(), sa);
    if (pa.split <= n_max) {
        tff::OptimFStageArgs m = sa;
        if (pa.split < pa.cut[0]) {
            m.la.rrange = pa.route + 4; m.lds_n = pa.cut[0] - 1;
            emu::launch(tff::k_optimf_refine<W, true, true>, waves, 64, tff::optimf_refine_lds_bytes(m.lds_n, true), m);
        }
        if (pa.cut[0] < pa.cut[1]) {
            m.la.rrange = pa.route + 6; m.lds_n = pa.cut[1] - 1;
            emu::launch(tff::k_optimf_refine<W, false, true>, waves, 64, tff::optimf_refine_lds_bytes(m.lds_n, false), m);
        }
        if (pa.cut[1] <= n_max) {
            m.la.rrange = pa.route + 8; m.lds_n = 0; m.spill = slices.data(); m.spill_stride = stride;
            emu::launch(tff::k_optimf_refine<W, false, true>, waves, 64, tff::optimf_refine_lds_bytes(0, false), m);
        }
        emu::launch(tff::k_optimf_finish_rows_ragged, rows, 64, tff::rows_lds_bytes(), sa);
    }
    tff::LinearTftArgs a = sa.la;
    a.rrange = nullptr;
    a.flags |= tff::FLAG_ONLY_RETRY;
    const int listed = retry[0];
    if (listed) emu::launch(tff::k_f_pose<true, 1, true>, (unsigned)(listed < 4 ? listed : 4), 64, tff::optimf_lds_bytes(n_max, a.flags, true), a);
    return listed;
}

// the fixed-N chain for B items of N correspondences: the exact kernel for all (exact != 0: N below the split), else the three stages with the storage
// route the launcher picks for N (stage_x; spill: xi in a global slice) and the exact kernel over what they flag
extern "C" int e_optimf_fixed(const double* corresp, const double* calm, long calm_stride, long B, int N, int exact, int stage_x, int spill, double* Rt2,
                              double* Rt3, double* T, double* reconst, int* iter, int* status) {
    tff::OptimFStageArgs sa{};
    sa.la = tff::LinearTftArgs{corresp, calm, calm_stride, B, N, reconst ? tff::FLAG_RECONST : 0, Rt2, Rt3, T, reconst, iter, status};
    tff::LinearTftArgs a = sa.la;
    if (!exact && N >= 8) {
        std::vector<double> rec((size_t)B * tff::OPTIMF_REC_DOUBLES, 0.0);
        sa.rec = rec.data();
        const long stride = 4 * (long)N + 16;
        std::vector<double> slices((size_t)B * stride, 0.0);
        emu::launch(tff::k_optimf_linear_rows, tff::rows_grid(B), 64, tff::rows_lds_bytes(), sa);
        tff::OptimFStageArgs m = sa;
        if (stage_x) {
            emu::launch(tff::k_optimf_refine<W, true>, (unsigned)B, 64, tff::optimf_refine_lds_bytes(N, true), m);
        } else {
            if (spill) { m.spill = slices.data(); m.spill_stride = stride; }
            emu::launch(tff::k_optimf_refine<W, false>, (unsigned)B, 64, tff::optimf_refine_lds_bytes(spill ? 0 : N, false), m);
        }
        emu::launch(tff::k_optimf_finish_rows, tff::rows_grid(B), 64, tff::rows_lds_bytes(), sa);
        bool any = false;
        for (long b = 0; b < B; ++b) any = any || status[b] == tff::ST_RETRY;
        if (!any) return 0;
        a.flags |= tff::FLAG_ONLY_RETRY;
    }
    emu::launch(tff::k_f_pose<true, 1>, (unsigned)B, 64, tff::optimf_lds_bytes(N, a.flags, true), a);
    return 1;
}
