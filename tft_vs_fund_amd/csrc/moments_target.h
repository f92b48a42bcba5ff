// gfx950 implementation of two primitives of the trifocal row kernel's moment pass (tft_rows_kernel.h::rows_distances_moments); the GPU-less unit
// tests find tests/emu/moments_target.h first on their include path (as with wave_target.h, rows_target.h and regs_target.h).
#pragma once
#include <hip/hip_runtime.h>

namespace tff {

// x * x + y * y in the fused form the compiler has always picked for the moment loop's squared distances: the square of y fused into the rounded
// square of x.  Written out, the form no longer depends on the shape of the loop around it.  (The lane emulator, built without fused
// multiply-add, keeps the plain sum it always computed: tests/emu/moments_target.h.)
__device__ __forceinline__ double sum_sq_yx(double x, double y) { return fma(y, y, x * x); }

// The values are IN their registers from here on: an empty statement that reads them, so the compiler waits for the loads that produce them at
// this point and not at their first arithmetic use.  For a loop that issues the next trip's loads under a lane mask before it consumes this
// trip's: behind the masked region the number of loads in flight is not known statically, and the wait the compiler has to place there is
// for ALL of them -- the new ones included, which then never overlap the arithmetic.  No instruction of its own.
template <int N>
__device__ __forceinline__ void loads_landed(const double (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("" ::"v"(v[k]));
}

}  // namespace tff
