// TEST INFRASTRUCTURE ONLY: the four primitives robust_kernel.h and ba_ragged_kernel.h use beyond wave.h, on the lane emulator.  Include after hip_emu.h.
#pragma once
#include "hip_emu.h"
inline unsigned long long __shfl_xor(unsigned long long v, int d, int) { return emu::exchange(v, (int)((emu::tl_threadIdx.x & 63u) ^ (unsigned)d)); }
inline unsigned long long __ballot(bool p) {
    uint64_t c = p ? (1ull << (emu::tl_threadIdx.x & 63u)) : 0ull;
    for (int m = 32; m >= 1; m >>= 1) c |= emu::exchange(c, (int)((emu::tl_threadIdx.x & 63u) ^ (unsigned)m));
    return c;
}
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) {
    unsigned long long o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
