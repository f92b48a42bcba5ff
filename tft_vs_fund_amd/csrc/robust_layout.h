// The two workspaces of a robust call (capi.hip::launch_robust_scenes), each described once: the byte offset of every region and the total, used both
// to reserve the buffer and to carve its pointers.  Every region starts on a 256-byte boundary; a region the call does not have (the CalM copies with a
// shared CalM, the rounds' state of a fixed call, flags and refit batch with n_total = 0) has zero bytes.  Plain C++, no HIP: a host compiler builds it
// alone (tests/test_robust_layout_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>

namespace tff {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Carver { size_t off = 0; size_t operator()(size_t bytes) { const size_t o = off; off += align256(bytes); return o; } };

// one chunk of hypotheses (tff_ctx::robust_hyp): poses (51 doubles a row) | CalM per row (`copies` = 216 bytes with one CalM per scene, 0 with a shared
// one) | status | sample indices (n a row), and behind them for the adaptive call: the round's dense counts | best (S x 8) | live (S x 4)
struct ChunkLayout { size_t pose, calm, status, idx, dense, best, live, total; };
inline ChunkLayout chunk_layout(int64_t chunk, int64_t S, int n, size_t copies, bool adaptive) {
    Carver carve;                            // (a braced list is evaluated left to right)
    const size_t rows = (size_t)chunk, r = adaptive ? 1 : 0;
    ChunkLayout l{carve(rows * 51 * 8), carve(rows * copies), carve(rows * 4), carve(rows * n * 4), carve(r * rows * 4), carve(r * S * 8), carve(r * S * 4), 0};
    l.total = carve.off;
    return l;
}

// the C = S * K candidates (tff_ctx::robust_cand): keys | poses | refits | offsets (C + 1) | seven int arrays of C | sample indices | CalM per candidate
// (`copies` as above) | K flags per packed correspondence | the packed refit batch
struct CandLayout { size_t sel, pose, ref, off, ints, idx, calm, mask, pack, total; };
inline CandLayout cand_layout(int64_t C, int K, int n, int64_t n_total, size_t copies) {
    Carver carve;
    const size_t rows = (size_t)C, flags = (size_t)K * n_total;
    CandLayout l{carve(rows * 8), carve(rows * 51 * 8), carve(rows * 51 * 8), carve((rows + 1) * 8), carve(rows * 7 * 4), carve(rows * n * 4),
                 carve(rows * copies), carve(flags), carve(flags * 6 * 8), 0};
    l.total = carve.off;
    return l;
}

}  // namespace tff
