// gar_bg_launch.hpp -- host-only launch planner of the banded-GEMM FIR kernels (bg_kernel, bg_rb_kernel,
// bg_rt_kernel: every GAR_F64 and GAR_F32_EXACT stage).  bgPlanLaunch takes every decision of a launch --
// small or large launch, kernel, instantiation unit, G, parity, the LDS budget, B from global memory, the
// epilogue layout, the grid -- from integers alone (plan fields, strides, the CU count, the knobs): no HIP
// call, no device pointer dereferenced, so it runs and is tested on a machine without a GPU (gar.h
// gar_dev_fir_plan).  launchBg (gar_kernels.hip) fills the pointers and dispatches.
#pragma once
#include <cstddef>
#include <cstdint>

#include "gar_bg_geo.hpp"
#include "gar_kernels.hpp"

namespace gar {

// Every environment knob of a bg launch (names and reading: kBgKnobTable in gar_bg_launch.cpp), all read
// once per process.  Development knobs: the defaults are the tuned values.
struct BgKnobs {
    int g = 0;         // GAR_BG_G: cap on the macro periods per column
    int wgPerCu = 0;   // GAR_BG_WGPERCU: workgroups per CU of a large launch (0: two)
    int dbg = 0;       // GAR_BG_DBG: timing bits (BgGrid::dbg); 8: no small launches
    int rt = -1;       // GAR_BG_RT: 1 / 0 force bg_rt_kernel / bg_rb_kernel for small launches (unset: by row blocks)
    int noVst = 0;     // GAR_BG_NOVST (set at all): scalar f32 epilogue
    int noParity = 0;  // GAR_BG_NOPARITY (set at all): one buffer of partial slots
    int trace = 0;     // GAR_BG_TRACE (set at all): one line per launch on stderr, 64 lines per process
    int prof = 0;      // GAR_BG_PROF (set at all): phase stamps of the small launches (GAR_BG_DEV build)
};
// Every knob read from the environment now / as first read in this process.
BgKnobs bgReadKnobs();
const BgKnobs& bgLaunchKnobs();

enum class BgOutcome { Launch, Nothing, Invalid };  // Invalid: hipErrorInvalidConfiguration
enum class BgKernel { Bg, BgRb, BgRt };
enum class BgUnit { F64, F32a, F32b };  // the instantiation unit (gar_bg_*.hip): f32 plans split at NS = 56

struct BgLaunchPlan {
    BgOutcome outcome = BgOutcome::Nothing;
    BgKernel kernel = BgKernel::Bg;
    BgUnit unit = BgUnit::F64;
    BgGrid g{};              // hdst / ht0 / hn / prof: the launcher's
    int64_t nmac = 0;        // macro periods of the launch
    int threads = 0;
    size_t lds = 0;
    int64_t blocks = 0;
    bool globalB = false;    // bg_kernel reads B from global memory (the tiles do not fit LDS)
    bool histFolded = false; // the history keep runs inside this launch
};

// histKeep / histN: a HistCopy with a destination is requested, and its row count.
BgLaunchPlan bgPlanLaunch(const BgDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const BgKnobs& k,
                          bool histKeep, int64_t histN);
// The GAR_BG_TRACE line of a planned launch (tests parse it); returns the length written.
int bgTraceLine(const BgLaunchPlan& pl, const BgDev& p, const OutDesc& od, char* buf, size_t cap);

}  // namespace gar
