// TEST INFRASTRUCTURE ONLY: csrc/moments_target.h for the lane emulator.
#pragma once

namespace tff {

// (the host build has no fused multiply-add: the plain sum, as before the form was written out for the GPU)
inline double sum_sq_yx(double x, double y) { return x * x + y * y; }
// (a lane's loads have landed when they return)
template <int N>
inline void loads_landed(const double (&)[N]) {}

}  // namespace tff
