// gar_cubic_seg.hpp -- the CubicStage checkpoint record: written by the host counter arithmetic
// (gar_counters.cpp cntCubic), read by cubic_kernel (gar_kernels.hip).  Plain data, no HIP.
#pragma once
#include <cstdint>

namespace gar {

// CubicStage checkpoint (cubic.go:42-61): before input i (absolute stage-input
// index) the phase is `phase` and the next output index is o.  Checkpoints are
// kCubicSegInputs inputs apart.
struct CubicSeg {
    double phase;
    int64_t o, i;
};
constexpr int64_t kCubicSegInputs = 256;
constexpr int kCubicSegInputsShort = 16;  // segment of short calls (closed-form walks only)

}  // namespace gar
