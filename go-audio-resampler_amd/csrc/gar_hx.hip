// gar_hx.hip -- dispatch of a planned launch (gar_hx_launch.hpp hxPlanLaunch) of the split-f16 FIR
// kernel (gar_hx.hpp).  Every output of a launch, edges included, runs on hx_kernel.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "gar_hx.hpp"
#include "gar_hx_launch.hpp"

namespace gar {

// hxLaunch instantiations live in gar_hx_i*.hip (compiled in parallel)
#define GAR_HX_EXTERN(NS, RB, V) \
    extern template hipError_t hxLaunch<NS, RB, V>(const HxArgs&, int, size_t, int64_t, int64_t, hipStream_t);
GAR_HX_FOR_ALL(GAR_HX_EXTERN)
#undef GAR_HX_EXTERN

namespace {

// row-block mode: the epilogue store layout (HxArgs::vst) is a template parameter
template <int NS, bool RB>
hipError_t hxDispatch(const HxArgs& x, int waves, size_t lds, int64_t blocks, int64_t eblocks, hipStream_t st) {
    if constexpr (!RB) return hxLaunch<NS, false, 0>(x, waves, lds, blocks, eblocks, st);
    switch (x.vst) {
        case 0: return hxLaunch<NS, RB, 0>(x, waves, lds, blocks, eblocks, st);
        case 1: return hxLaunch<NS, RB, 1>(x, waves, lds, blocks, eblocks, st);
        case 2: return hxLaunch<NS, RB, 2>(x, waves, lds, blocks, eblocks, st);
        default: return hxLaunch<NS, RB, 3>(x, waves, lds, blocks, eblocks, st);
    }
}

}  // namespace

hipError_t launchHxPlan(const HxLaunchPlan& pl, const HxKnobs& k, const HxDev& p, const SrcDesc& src, const OutDesc& od, int C,
                        hipStream_t stream) {
    if (pl.outcome == HxOutcome::Refused) return hipErrorNotSupported;
    if (pl.outcome == HxOutcome::Invalid) return hipErrorInvalidConfiguration;
    if (k.trace) {
        char line[768];
        hxTraceLine(pl, src, od, C, line, sizeof(line));
        fputs(line, stderr);
    }
    HxArgs x{};
    x.A = static_cast<const h8v*>(p.A);
    x.progs = p.progs;
    x.reds = p.reds;
    x.ea = p.ea;
    x.kch = p.kch;
    x.Pc = p.Pc; x.Qc = p.Qc; x.G = pl.G; x.C = C;
    x.W = pl.W;
    x.Ws = pl.Ws;
    x.ncols = pl.ncols;
    x.nblocks = pl.nblocks;
    x.nred = p.nred; x.nslots = p.nslots; x.parity = pl.parity;
    x.dbg = k.dbg;
    x.k0 = pl.k0;
    x.k1 = pl.k1;
    x.a_lo = pl.a_lo;
    x.o_lo = od.o_lo;
    x.o_hi = od.o_hi;
    x.in = reinterpret_cast<const float*>(pl.in);
    x.in_fs = src.in_fs;
    x.in_cs = src.in_cs;
    x.in_chunk = pl.in_chunk;
    x.out_f64 = od.f64;
    x.out = reinterpret_cast<char*>(pl.out);
    x.out_fs = pl.out_fs;
    x.out_cs = pl.out_cs;
    x.out_chunk = pl.out_chunk;
    x.vst = pl.vst;
    x.fmt = pl.fmt;
    x.src = src;
    x.od = od;
    x.ex = p.ex;
    x.ib0 = pl.ib0;
    x.ib1 = pl.ib1;
    x.fix = p.fix;
    x.fixCap = p.fixCap;
    x.nprog = p.nw;
    if (pl.fixReset) {
        const hipError_t e = hipMemsetAsync(p.fix, 0, sizeof(int), stream);
        if (e != hipSuccess) return e;
    }
    if (p.rb) {
        switch (p.NS) {
#define GAR_HX_RB(n) case n: return hxDispatch<n, true>(x, pl.waves, pl.lds, pl.blocks, pl.eblocks, stream);
            GAR_HX_RB(1) GAR_HX_RB(2) GAR_HX_RB(3) GAR_HX_RB(4) GAR_HX_RB(5) GAR_HX_RB(6) GAR_HX_RB(7) GAR_HX_RB(8)
            GAR_HX_RB(9) GAR_HX_RB(10)
#undef GAR_HX_RB
            default: return hipErrorInvalidConfiguration;
        }
    }
    switch (p.NS) {
#define GAR_HX_SEG(n) case n: return hxDispatch<n, false>(x, pl.waves, pl.lds, pl.blocks, pl.eblocks, stream);
        GAR_HX_SEG(2) GAR_HX_SEG(4) GAR_HX_SEG(6) GAR_HX_SEG(8)
#undef GAR_HX_SEG
        default: return hipErrorInvalidConfiguration;
    }
}

}  // namespace gar
