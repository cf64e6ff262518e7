// gar_counters.hpp -- per-stage streaming counters: the reference's exact integer arithmetic, so every
// call returns exactly the reference's number of samples.  Host only, no HIP (gar_counters.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "gar_cubic_seg.hpp"
#include "gar_design.hpp"

#pragma GCC visibility push(hidden)
namespace gar {

struct Counters {
    bool staged = false;       // DFT+poly engine running stage-by-stage (else fused)
    int64_t x_count = 0;       // samples appended to the stage input stream
    int64_t dft_hist = 0;      // len(DFTStage.history)
    int64_t poly_hist = 0;     // len(PolyphaseStage.history)
    int64_t at = 0;            // PolyphaseStage.at
    int64_t u_base = 0;        // poly-stream index of PolyphaseStage.history[0]
    int64_t u_count = 0;       // samples appended to the poly stream
    int64_t dec_hist = 0;      // len(DFTDecimationStage.history)
    int dec_phase = 0;         // DFTDecimationStage.decimPhase
    int64_t y_count = 0;       // samples emitted
    double cub_phase = 0.0;    // CubicStage.phase (cubic.go:17)
};

// DFTStage.processZeroCopy counts (dft_stage.go:156-207)
int64_t cntDft(Counters& s, const DftBank& b, int64_t n);
// PolyphaseStage.processZeroCopy counts (polyphase_stage.go:186-312)
int64_t cntPoly(Counters& s, const PolyBank& b, int64_t m, bool& quirk);
// DFTDecimationStage.processZeroCopy counts (dft_stage.go:488-554)
int64_t cntDecim(Counters& s, const DecimBank& b, int64_t n);
// CubicStage.Process walk (cubic.go:42-61): the f64 phase recurrence, run once for
// all channels; `segs` (when given) receives the state every segLen inputs (the closed form takes the
// caller's spacing -- short segments for short calls; the sequential walk uses kCubicSegInputs).
int64_t cntCubic(Counters& s, double ratio, int64_t n, std::vector<CubicSeg>* segs, int* segLen = nullptr);

// StageAdapter.GetLatency (internal/engine/stage_adapter.go:43-57)
int stageLatency(const EngineDesign& d);

}  // namespace gar
#pragma GCC visibility pop
