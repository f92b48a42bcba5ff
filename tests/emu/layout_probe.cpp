// TEST INFRASTRUCTURE ONLY: csrc/robust_layout.h built by g++ alone (no HIP), for tests/test_robust_layout_cpu.py.
// layout_probe chunk S C K n n_total copies adaptive -> the chunk layout's seven offsets and total, then the candidates layout's nine and total
#include <cstdio>
#include <cstdlib>
#include "robust_layout.h"
int main(int argc, char** argv) {
    if (argc != 9) return 2;
    long v[8];
    for (int i = 0; i < 8; ++i) v[i] = std::atol(argv[i + 1]);
    const tff::ChunkLayout h = tff::chunk_layout(v[0], v[1], (int)v[4], (size_t)v[6], v[7] != 0);
    const tff::CandLayout k = tff::cand_layout(v[2], (int)v[3], (int)v[4], v[5], (size_t)v[6]);
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", h.pose, h.calm, h.status, h.idx, h.dense, h.best, h.live, h.total);
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", k.sel, k.pose, k.ref, k.off, k.ints, k.idx, k.calm, k.mask, k.pack, k.total);
    return 0;
}
