// TEST INFRASTRUCTURE ONLY: csrc/regs_target.h for the lane emulator.
#pragma once

namespace tff {

inline double zero_f64() { return 0.0; }

}  // namespace tff
