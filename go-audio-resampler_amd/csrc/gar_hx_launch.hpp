// gar_hx_launch.hpp -- host-only launch planner of the split-f16 block kernel (hx_kernel, gar_hx.hpp) and
// the routing of an x == 0 FIR launch among the three kernel families.  hxPlanLaunch takes every decision of
// an hx_kernel launch -- G, the interior chunk range, load / store layout, interior and edge blocks -- and
// firPlanLaunch the choice bg / streaming split-f16 / hx_kernel with its two fallbacks, from integers alone
// (plan fields, strides, addresses as integers, the CU count, the knobs): no HIP call, no device pointer
// dereferenced, so both run and are tested on a machine without a GPU (gar.h gar_dev_fir_plan).
#pragma once
#include <cstddef>
#include <cstdint>

#include "gar_bg_launch.hpp"
#include "gar_hxs_launch.hpp"

namespace gar {

// Every environment knob of an hx_kernel launch and of the routing (names and reading: kHxKnobTable in gar_hx_launch.cpp), all read
// once per process.  Development knobs.
struct HxKnobs {
    int hxs = 1;    // GAR_HXS=0: row-block plans run hx_kernel, not the streaming kernels (A/B runs)
    int g = 0;      // GAR_HX_G: cap on the macro periods per column
    int dbg = 0;    // GAR_HX_DBG bits (HxArgs::dbg): 1 skip staging after the first block, 2 skip the MFMA programs, 16 skip the loop
    int dword = 0;  // GAR_HX_DWORD (set at all): dword loads where a wider raw load format applies
    int trace = 0;  // GAR_HX_TRACE (set at all): one line per launch on stderr
};
HxKnobs hxReadKnobs();
const HxKnobs& hxLaunchKnobs();

enum class HxOutcome { Launch, Invalid, Refused };  // hipErrorInvalidConfiguration; hipErrorNotSupported (PCM output)

// The integer fields of HxArgs a launch computes, under HxArgs's names.
struct HxLaunchPlan {
    HxOutcome outcome = HxOutcome::Invalid;
    int G = 0, W = 0, Ws = 0, ncols = 0, nblocks = 0, parity = 0;
    int k0 = 0, k1 = 0, ib0 = 0, ib1 = 0;  // interior chunks [k0, k1), interior blocks [ib0, ib1)
    int fmt = 0, vst = 0;
    int64_t a_lo = 0, nchunk = 0;
    uintptr_t in = 0, out = 0;  // addresses of chunk 0's first input row / first output (either may lie outside the buffers)
    int64_t in_chunk = 0, out_fs = 0, out_cs = 0, out_chunk = 0;
    int waves = 0;
    size_t lds = 0;
    int64_t blocks = 0, eblocks = 0;  // interior launch, edge launch (+ the fix list's workgroups)
    bool fixReset = false;            // the interior launch appends to the fix list: its counter is zeroed first
};

HxLaunchPlan hxPlanLaunch(const HxDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const HxKnobs& k);
// The GAR_HX_TRACE line of a planned hx_kernel launch (tests parse it); returns the length written.
int hxTraceLine(const HxLaunchPlan& pl, const SrcDesc& src, const OutDesc& od, int C, char* buf, size_t cap);

// ---- routing ----------------------------------------------------------------------------------------
// launchBg's chain: an f32 plan with a split-f16 variant runs that variant; a row-block split-f16 plan
// streams (hxs / hxq / hxt kernels) unless GAR_HXS=0 or the streaming planner declines, then hx_kernel,
// which refuses PCM output (the engine stages it); every other plan runs the bg kernels.
struct FirKnobs {
    BgKnobs bg;
    HxKnobs hx;
    HxsKnobs hxs;
};
FirKnobs firReadKnobs();    // every knob read from the environment now
FirKnobs firLaunchKnobs();  // the knobs of a launch (per-process ones as first read)

enum class FirPath { Nothing, Bg, Hxs, Hx };
struct FirLaunchPlan {
    FirPath path = FirPath::Nothing;
    BgLaunchPlan bg;    // path Bg
    HxsLaunchPlan hxs;  // path Hxs
    HxLaunchPlan hx;    // path Hx
};
FirLaunchPlan firPlanLaunch(const BgDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const FirKnobs& k,
                            bool histKeep, int64_t histN);
// The trace line(s) of the planned launch, or "not supported\n" / "invalid configuration\n", or nothing.
int firTraceLines(const FirLaunchPlan& pl, const BgDev& p, const SrcDesc& src, const OutDesc& od, int C, char* buf, size_t cap);

// ---- dispatch of a planned launch (gar_kernels.hip, gar_hxs.hip, gar_hx.hip) ---------------------------
// Each traces from the plan (its knobs' trace switch), fills the kernel arguments and launches.
hipError_t launchBgPlan(const BgLaunchPlan& pl, const BgKnobs& k, const BgDev& p, const SrcDesc& src, const OutDesc& od,
                        hipStream_t stream, HistCopy* hc);
hipError_t launchHxsPlan(const HxsLaunchPlan& pl, const HxsKnobs& k, const HxDev& p, const SrcDesc& src, const OutDesc& od, int C,
                         hipStream_t stream, HistCopy* hc, uint64_t* meter = nullptr);
hipError_t launchHxPlan(const HxLaunchPlan& pl, const HxKnobs& k, const HxDev& p, const SrcDesc& src, const OutDesc& od, int C,
                        hipStream_t stream);

}  // namespace gar
