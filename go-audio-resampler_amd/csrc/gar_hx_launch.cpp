// gar_hx_launch.cpp -- host-only launch planner of hx_kernel and the routing of an x == 0 FIR launch
// (gar_hx_launch.hpp).
#include "gar_hx_launch.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gar_knobs.hpp"

namespace gar {

namespace {
// name, field (its default: the member initialiser in HxKnobs), how the value reads, when it is read
constexpr KnobRow<HxKnobs> kHxKnobTable[] = {
    {"GAR_HXS", &HxKnobs::hxs, kNotZero, false},
    {"GAR_HX_G", &HxKnobs::g, kInt, false},
    {"GAR_HX_DBG", &HxKnobs::dbg, kInt, false},
    {"GAR_HX_DWORD", &HxKnobs::dword, kIsSet, false},
    {"GAR_HX_TRACE", &HxKnobs::trace, kIsSet, false},
};

// an instantiated hxLaunch (gar_hx.hpp GAR_HX_FOR_ALL): row-block NS 1..10, segmented NS 2, 4, 6, 8
bool hxNsBuilt(bool rb, int NS) { return rb ? (NS >= 1 && NS <= 10) : (NS >= 2 && NS <= 8 && NS % 2 == 0); }
}  // namespace

HxKnobs hxReadKnobs() {
    HxKnobs k;
    readKnobTable(kHxKnobTable, k, false);
    return k;
}

const HxKnobs& hxLaunchKnobs() {
    static const HxKnobs perProcess = hxReadKnobs();
    return perProcess;
}

HxLaunchPlan hxPlanLaunch(const HxDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const HxKnobs& k) {
    HxLaunchPlan pl;
    if (od.pcm) {  // PCM output is fused into hxs_kernel only (engine stages it otherwise)
        pl.outcome = HxOutcome::Refused;
        return pl;
    }
    const int64_t Pc = p.Pc, Qc = p.Qc;
    const int64_t a_lo = floorDiv(od.o_lo, Pc);
    const int64_t nmac = ceilDiv(od.o_hi, Pc) - a_lo;
    const size_t kLds = 160 * 1024;
    // window rows staged per column (the padded program steps read up to Kread + (G-1)*Qc),
    // whole 64-row item slots
    auto wsFor = [&](int G) { return (p.Kread + (G - 1) * p.Qc + 63) / 64 * 64; };
    const int parity = (p.nred > 0 && hxLdsBytes(wsFor(1), p.nslots, 1) <= kLds) ? 1 : 0;
    auto ldsFor = [&](int G) { return hxLdsBytes(wsFor(G), p.nslots, parity); };
    // G macro periods per column: the largest whose window fits LDS without
    // dropping below one block per CU (small launches: G = 1, the most blocks)
    auto nbFor = [&](int G) { return ((nmac + G - 1) / G * C + 15) / 16; };
    int G = 1;
    for (int cand = 2; cand <= 8; ++cand) {
        if (cand > nmac || wsFor(cand) > kHxMaxRows || ldsFor(cand) > kLds) break;
        if (nbFor(cand) < ncu) break;
        G = cand;
    }
    if (k.g > 0 && k.g < G) G = k.g;
    if (wsFor(G) > kHxMaxRows || ldsFor(G) > kLds) return pl;
    const int64_t W = p.Kc + static_cast<int64_t>(G - 1) * Qc;
    const int64_t nchunk = (nmac + G - 1) / G;
    const int64_t ncols = nchunk * C;
    if (ncols > (int64_t(1) << 30)) return pl;
    if (!hxNsBuilt(p.rb, p.NS) || (p.rb && p.nw > kHxRbMaxWaves)) return pl;

    // interior chunks [k0, k1): outputs inside [o_lo, o_hi), window rows [0, W) inside the f32 input,
    // and 32-bit lane offsets (row * frame stride) inside a buffer resource
    int64_t k0 = 0, k1 = 0;
    const bool fastIn = src.in && !src.in_f64 && !src.in_pcm && src.in_len > 0 &&
                        static_cast<double>(wsFor(G)) * static_cast<double>(std::llabs(src.in_fs)) * 4.0 < 2147483647.0 &&
                        src.in_fs > 0 && src.in_cs >= 0;
    if (fastIn) {
        const int64_t GQ = G * Qc, GP = G * Pc;
        const int64_t inEnd = std::min(src.in_base + src.in_len, src.valid_end);
        k0 = std::max<int64_t>({0, ceilDiv(od.o_lo - a_lo * Pc, GP), ceilDiv(src.in_base - a_lo * Qc, GQ)});
        k1 = std::min<int64_t>({nchunk, floorDiv(od.o_hi - a_lo * Pc, GP), floorDiv(inEnd - W - a_lo * Qc, GQ) + 1});
        // an empty interior range stays inside [0, nchunk]: a short call whose windows all cross the
        // history seam has k0 > nchunk (e.g. 399 frames after 912 history rows), and an interior
        // range placed past the last chunk made ib1 > nblocks below (sweep: 88.2k -> 44.1k High)
        k0 = std::min(k0, nchunk);
        if (k1 < k0) k1 = k0;
    }
    pl.outcome = HxOutcome::Launch;
    pl.G = G;
    pl.W = static_cast<int>(W);
    pl.Ws = wsFor(G);
    pl.ncols = static_cast<int>(ncols);
    pl.nblocks = static_cast<int>((ncols + 15) / 16);
    pl.parity = parity;
    pl.k0 = static_cast<int>(k0);
    pl.k1 = static_cast<int>(k1);
    pl.a_lo = a_lo;
    pl.nchunk = nchunk;
    // pointer arithmetic in integers: chunk 0 may start before the caller's buffers
    const int isz = 4;
    pl.in = reinterpret_cast<uintptr_t>(src.in) + static_cast<intptr_t>((a_lo * Qc - src.in_base) * src.in_fs * isz);
    pl.in_chunk = G * Qc * src.in_fs;
    const int esz = od.f64 ? 8 : 4;
    pl.out = reinterpret_cast<uintptr_t>(od.out) + static_cast<intptr_t>((a_lo * Pc - od.o0) * od.fs * esz);
    pl.out_fs = od.fs * esz;
    pl.out_cs = od.cs * esz;
    pl.out_chunk = G * Pc * od.fs * esz;
    // epilogue layout of interior blocks (16-B stores need every row quad 16-B aligned)
    const bool al = (pl.out & 15) == 0 && ((G * Pc * od.fs * esz) & 15) == 0;
    if (od.f64) pl.vst = 3;
    else if (al && C == 2 && od.fs == 2 && od.cs == 1 && Pc % 2 == 0) pl.vst = 2;
    else if (al && od.fs == 1 && (od.cs * 4) % 16 == 0 && Pc % 4 == 0) pl.vst = 1;
    else pl.vst = 0;
    // raw load format of interior blocks: 8-B stereo frames / 16-B four-channel rows where the layout
    // allows it; per-block buffer resources need every in-block offset below 2^31 (else 64-bit loads)
    const uintptr_t inA = reinterpret_cast<uintptr_t>(src.in);
    pl.fmt = 0;
    if ((inA & 7) == 0 && C == 2 && src.in_fs == 2 && src.in_cs == 1) pl.fmt = 1;
    else if ((inA & 15) == 0 && C % 4 == 0 && src.in_cs == 1 && src.in_fs % 4 == 0) pl.fmt = 2;
    if (k.dword) pl.fmt = 0;
    {
        const double chunksPerBlock = 16.0 / C + 2.0;
        const double maxOff = chunksPerBlock * static_cast<double>(pl.in_chunk) * 4.0 +
                              static_cast<double>(C) * static_cast<double>(src.in_cs) * 4.0 + 16.0;
        if (maxOff >= 2147483647.0) pl.fmt = 3;
    }
    // interior blocks: every column an interior chunk
    pl.ib0 = static_cast<int>(std::min<int64_t>((k0 * C + 15) / 16, pl.nblocks));
    pl.ib1 = static_cast<int>(std::max<int64_t>(pl.ib0, std::min<int64_t>((k1 * C) / 16, pl.nblocks)));
    pl.lds = ldsFor(G);
    const int64_t nInt = pl.ib1 - pl.ib0;
    const int64_t nEdge = pl.nblocks - nInt;
    pl.blocks = std::min<int64_t>(nInt, ncu);
    // edge blocks + workgroups draining the interior kernel's (normally empty) fix list
    pl.eblocks = std::max<int64_t>(nEdge, 1) + (nInt > 0 ? kHxFixWgs : 0);
    pl.fixReset = nInt > 0;
    pl.waves = p.rb ? std::max(p.nw, kHxMinWaves) : kHxWaves;
    return pl;
}

int hxTraceLine(const HxLaunchPlan& pl, const SrcDesc& src, const OutDesc& od, int C, char* buf, size_t cap) {
    return std::snprintf(buf, cap,
                         "hx: o[%lld,%lld) C=%d G=%d W=%d a_lo=%lld nchunk=%lld k0=%d k1=%d in_base=%lld in_len=%lld valid_end=%lld "
                         "hist_len=%lld Ws=%d ncols=%d nblocks=%d parity=%d ib0=%d ib1=%d fmt=%d vst=%d in=%#llx in_chunk=%lld out=%#llx "
                         "out_fs=%lld out_cs=%lld out_chunk=%lld waves=%d lds=%zu blocks=%lld eblocks=%lld fixReset=%d\n",
                         (long long)od.o_lo, (long long)od.o_hi, C, pl.G, pl.W, (long long)pl.a_lo, (long long)pl.nchunk, pl.k0, pl.k1,
                         (long long)src.in_base, (long long)src.in_len, (long long)src.valid_end, (long long)src.hist_len, pl.Ws,
                         pl.ncols, pl.nblocks, pl.parity, pl.ib0, pl.ib1, pl.fmt, pl.vst, (unsigned long long)pl.in,
                         (long long)pl.in_chunk, (unsigned long long)pl.out, (long long)pl.out_fs, (long long)pl.out_cs,
                         (long long)pl.out_chunk, pl.waves, pl.lds, (long long)pl.blocks, (long long)pl.eblocks, pl.fixReset ? 1 : 0);
}

// ---- routing ----------------------------------------------------------------------------------------
FirKnobs firReadKnobs() { return {bgReadKnobs(), hxReadKnobs(), hxsReadKnobs()}; }
FirKnobs firLaunchKnobs() { return {bgLaunchKnobs(), hxLaunchKnobs(), hxsLaunchKnobs()}; }

FirLaunchPlan firPlanLaunch(const BgDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const FirKnobs& k,
                            bool histKeep, int64_t histN) {
    FirLaunchPlan pl;
    if (od.o_hi <= od.o_lo) return pl;
    if (!p.hx || p.f64) {  // f64 / exact-f32 compute
        pl.path = FirPath::Bg;
        pl.bg = bgPlanLaunch(p, src, od, C, ncu, k.bg, histKeep, histN);
        return pl;
    }
    // f32 compute on the split-f16 kernels (every output of the launch, any input dtype): row-block plans
    // stream through the wave-specialised kernels unless their planner declines
    const HxDev& hx = *p.hx;
    if (hx.rb && k.hx.hxs) {
        pl.hxs = hxsPlanLaunch(hx, src, od, C, ncu, k.hxs, histKeep, histN);
        if (pl.hxs.ok) {
            pl.path = FirPath::Hxs;
            return pl;
        }
    }
    pl.path = FirPath::Hx;
    pl.hx = hxPlanLaunch(hx, src, od, C, ncu, k.hx);
    return pl;
}

int firTraceLines(const FirLaunchPlan& pl, const BgDev& p, const SrcDesc& src, const OutDesc& od, int C, char* buf, size_t cap) {
    const bool invalid = (pl.path == FirPath::Bg && pl.bg.outcome == BgOutcome::Invalid) ||
                         (pl.path == FirPath::Hx && pl.hx.outcome == HxOutcome::Invalid);
    if (invalid) return std::snprintf(buf, cap, "invalid configuration\n");
    if (pl.path == FirPath::Hx && pl.hx.outcome == HxOutcome::Refused) return std::snprintf(buf, cap, "not supported\n");
    if (pl.path == FirPath::Hxs) return hxsTraceLines(pl.hxs, od, C, buf, cap);
    if (pl.path == FirPath::Hx) return hxTraceLine(pl.hx, src, od, C, buf, cap);
    if (pl.path == FirPath::Bg && pl.bg.outcome == BgOutcome::Launch) return bgTraceLine(pl.bg, p, od, buf, cap);
    if (cap > 0) buf[0] = 0;
    return 0;
}

}  // namespace gar
