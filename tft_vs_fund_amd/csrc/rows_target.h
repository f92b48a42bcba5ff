// gfx950 implementation of two primitives of the four-triplet row kernels; the GPU-less unit tests find tests/emu/rows_target.h first on their
// include path (as with wave_target.h).
#pragma once
#include <hip/hip_runtime.h>
#include <wave_target.h>

namespace tff {

// The running kernel's argument record, read AGAIN from the kernarg segment (scalar loads through the constant cache).  For a kernel whose single
// by-value parameter is `a` (explicit arguments start at offset 0 of the segment): fields that are needed only at the far end of a long kernel --
// output pointers at the stores -- are fetched there instead of staying live in scalar registers, or in the lanes of a spill register, from the
// first instruction on.  The pointer is opaque to the optimiser, so the loads stay where they are written.
#define TFF_KERNARG_SPACE __attribute__((address_space(4)))
template <class Args>
__device__ __forceinline__ const TFF_KERNARG_SPACE Args* kernarg_again(const Args&) {
    const TFF_KERNARG_SPACE Args* p = (const TFF_KERNARG_SPACE Args*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

// sqrt_nonneg (wave_target.h) with its x == 0 select off the common path: x * rsqrt_pos(x) is NaN for x == 0, and the select that mends it runs
// only when some lane of the wavefront has such an x -- one compare and a scalar branch where there were a compare and two selects.  Same value
// for every x.  The rare branch ends the caller's basic block, and sums of products are fused within a block only: a caller whose fused forms
// straddle the call gets other last bits (the trifocal moment loop does not; LinearF's does and keeps sqrt_nonneg).
__device__ __forceinline__ double sqrt_nonneg_uniform(double x) {
#pragma clang fp contract(off)                                               // (the product is not to be fused into the caller's sum: the select used to stand between the two)
    double s = x * rsqrt_pos(x);
    if (__ballot(x == 0.0) != 0ull) {
        s = (x == 0.0) ? 0.0 : s;
        asm volatile("" : "+v"(s));                                          // (keeps the branch a branch: without it the select is hoisted back onto the common path)
    }
    return s;
}

}  // namespace tff
