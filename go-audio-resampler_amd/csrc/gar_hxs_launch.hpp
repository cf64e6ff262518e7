// gar_hxs_launch.hpp -- host-only launch planner of the streaming split-f16 FIR kernels (hxs_kernel,
// hxs_small_kernel, hxq_kernel, hxt_kernel).  hxsPlanLaunch takes every decision of a launch -- kernel,
// load / store layout, chunking, group size and ring, compute-wave roles, block order -- from integers
// alone (plan fields, strides, address alignments, the CU count, the knobs): no HIP call, no pointer
// dereferenced, so it runs and is tested on a machine without a GPU (gar.h gar_dev_hxs_plan).
// launchHxsPlan (gar_hxs.hip) fills HxsArgs from the result and dispatches.
#pragma once
#include <cstddef>
#include <cstdint>

#include "gar_hxs_geo.hpp"
#include "gar_kernels.hpp"

namespace gar {

// Every environment knob of the streaming launch path (table with names and defaults: kHxsKnobTable
// in gar_hxs_launch.cpp).  Development knobs unless DESIGN.md says otherwise.
struct HxsKnobs {
    // read once per process
    int g = 0;            // GAR_HXS_G: cap on the periods per group
    int wgPerCu = 0;      // GAR_HXS_WGPERCU: target blocks per CU of the chunk length (0: one)
    int trace = 0;        // GAR_HX_TRACE (set at all): one line per launch on stderr
    int dbg = 0;          // GAR_HXS_DBG: attribution bits of the GAR_HXS_DEV build (HxsArgs::dbg)
    int prof = 0;         // GAR_HXS_PROF (set at all): per-phase cycle sums of the GAR_HXS_DEV build
    int small = -1;       // GAR_HXS_SMALL: 0 / 1 force the small-launch rule off / on
    int np = 0;           // GAR_HXS_NP: chunk length in macro periods (streaming launches)
    int hxt = -1;         // GAR_HXT: 0 keeps hxs_kernel where hxt_kernel applies
    int smallK = 1;       // GAR_HXS_SMALLK: 0 runs small launches on hxs_kernel (HxsArgs::bigSmall)
    int nt = 0;           // GAR_HXS_NT: non-temporal output stores (GAR_HXS_DEV build)
    int pair = 1;         // GAR_HXS_PAIR: 0 turns the ROW16 XCD pairing off
    int chunkMajor = 1;   // GAR_HXT_CHUNKMAJOR: 0 turns the ROW32 chunk-major block order off
    int coop = 2;         // GAR_HXT_COOP: cooperative first-window fill, 2 ordered / 1 unordered / 0 loaders
    int hxq = 1;          // GAR_HXQ: 0 keeps hxs_small_kernel where hxq_kernel applies
    int hxqNr = 0;        // GAR_HXQ_NR: row blocks per hxq workgroup (0: by the CU count)
    int hxqOpt = 1;       // GAR_HXQ_OPT: hxq_kernel variant (HxsArgs::qOpt)
    int hxqW = 4;         // GAR_HXQ_W: waves per hxq workgroup (hxsLaunch clamps it to [max(1, qRbs), kHxqMaxWaves])
    // re-read on every launch (tests switch them inside one process)
    int roles = -1;       // GAR_HXT_ROLES: 1 balanced compute roles, 0 one wave per row block, unset: by plan
    int wide = 1;         // GAR_HXT_WIDE: 0 keeps 16-channel blocks where 32-channel blocks apply
    int lean = 1;         // GAR_HXT_LEAN: 0 keeps the generic loaders where the lean ones apply
    int fault = 0;        // GAR_HXT_FAULT=1: unreachable load count, short wait bound (the launch must fail)
};
// Every knob read from the environment now.
HxsKnobs hxsReadKnobs();
// The knobs of a launch: the per-process ones as first read, the per-launch ones read now.
HxsKnobs hxsLaunchKnobs();

enum class HxsKernel { Hxs, HxsSmall, Hxq, Hxt };

struct HxsLaunchPlan {
    bool ok = false;          // false: the plan does not fit these kernels (hipErrorNotSupported)
    HxsKernel kernel = HxsKernel::Hxs;
    int fmt = kFmtGather, vst = kVstAny;
    int small = 0, bigSmall = 0;
    int64_t Np = 0, nchunk = 0, ncols = 0;
    int nblocks = 0, ngroups = 0;
    int G = 0, R = 0, Rt = 0, mirror = 0, Wg = 0;  // ring as staged (small launches: one window, no mirror)
    int groupR = 0, groupRt = 0;                    // ring of G periods before that trim (the trace line's R, Rt)
    int64_t a_lo = 0, a_hi = 0;
    int64_t fastLo = 0, fastHi = 0;                 // input rows raw loads may touch
    int in_esz = 4, out_esz = 4;
    uintptr_t inBase = 0, outBase = 0;              // addresses of input row 0 / output 0 (HxsArgs::in, out)
    int xcdPair = 0;
    int ncomp = 0, role[kHxtMaxComp] = {}, maxStride = 1;
    bool lean = false;
    int loaders = 0;                                // hxt_kernel: 4 or 6
    int qRbs = 0, qGroups = 0, qOpt = 0;
    size_t lds = 0;
    bool histFolded = false;                        // the history keep runs inside this launch
};

// histKeep / histN: a HistCopy with a destination is requested, and its row count.
HxsLaunchPlan hxsPlanLaunch(const HxDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const HxsKnobs& k,
                            bool histKeep, int64_t histN);
// The GAR_HX_TRACE line(s) of a planned launch (tests parse them); returns the length written.
int hxsTraceLines(const HxsLaunchPlan& pl, const OutDesc& od, int C, char* buf, size_t cap);

}  // namespace gar
