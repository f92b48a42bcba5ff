// TEST INFRASTRUCTURE ONLY: csrc/rows_target.h for the lane emulator.
#pragma once
#include <cmath>

namespace tff {

// the argument record a kernel was called with is the one it has
template <class Args>
inline const Args* kernarg_again(const Args& a) { return &a; }
// (as sqrt_nonneg in wave_target.h)
inline double sqrt_nonneg_uniform(double v) { return std::sqrt(v); }

}  // namespace tff
