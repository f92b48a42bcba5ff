// gfx950 implementation of a register-level primitive of the row kernels; the GPU-less unit tests find tests/emu/regs_target.h first on their
// include path (as with wave_target.h and rows_target.h).
#pragma once
#include <hip/hip_runtime.h>

namespace tff {

// +0.0 in ONE instruction: the compiler materialises a double constant as two 32-bit moves, one per half of the register pair, and copies a
// pair the same way.  For register files full of accumulators that start at zero (48 of them in the trifocal moment pass).
__device__ __forceinline__ double zero_f64() {
    double r;
    asm volatile("v_mov_b64 %0, 0" : "=v"(r));                                  // (volatile: not merged into one value that is then copied by halves)
    return r;
}

}  // namespace tff
