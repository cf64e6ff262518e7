// gar_bg_launch.cpp -- host-only launch planner of the banded-GEMM FIR kernels (gar_bg_launch.hpp).
#include "gar_bg_launch.hpp"

#include <algorithm>
#include <cstdio>

#include "gar_knobs.hpp"

namespace gar {

namespace {
// name, field (its default: the member initialiser in BgKnobs), how the value reads, when it is read
constexpr KnobRow<BgKnobs> kBgKnobTable[] = {
    {"GAR_BG_G", &BgKnobs::g, kInt, false},
    {"GAR_BG_WGPERCU", &BgKnobs::wgPerCu, kInt, false},
    {"GAR_BG_DBG", &BgKnobs::dbg, kInt, false},
    {"GAR_BG_RT", &BgKnobs::rt, kInt, false},
    {"GAR_BG_NOVST", &BgKnobs::noVst, kIsSet, false},
    {"GAR_BG_NOPARITY", &BgKnobs::noParity, kIsSet, false},
    {"GAR_BG_TRACE", &BgKnobs::trace, kIsSet, false},
    {"GAR_BG_PROF", &BgKnobs::prof, kIsSet, false},
};

// Small launch of a row-block-aligned f64 plan (stream chunks): one macro period per column, one (column
// block, row block) per workgroup -- same programs, same sums.
bool isSmall(const BgDev& p, int64_t nmac, int C, int ncu, const BgKnobs& k) {
    return p.f64 && p.rbAligned && p.rbStart && p.hRbStart && p.nrb <= kBgRbKMaxRb && p.nprog <= kBgRbKMaxProg &&
           (nmac * C + 15) / 16 <= 2 * static_cast<int64_t>(ncu) && !(k.dbg & 8);
}

void planSmall(BgLaunchPlan& pl, const BgDev& p, int C, const BgKnobs& k) {
    BgGrid& g = pl.g;
    for (int i = 0; i <= p.nrb; ++i) g.rbStart[i] = p.hRbStart[i];
    for (int i = 0; i < p.nprog; ++i) g.rbK0[i] = p.hRbK0[i];
    g.G = 1;
    g.W = p.Kc;
    g.Wl = p.Kread;
    g.Ws = g.Wl;
    g.nchunk = static_cast<int>(pl.nmac);
    g.ncols = static_cast<int>(pl.nmac * C);
    g.nblocks = (g.ncols + 15) / 16;
    pl.threads = 64 * p.maxPrb;
    // time-major (bg_rt_kernel): workgroups = row blocks x channels x blocks of 16 consecutive macro periods,
    // each window staged once in LDS.  Default: time-major for plans of one or two row blocks (the integer
    // decimator: each window is staged once; 4800-frame cfg5 calls 26.8 -> 18.9 us), bg_rb_kernel otherwise (a
    // plan of ten row blocks would stage every window ten times: the cfg5 composite 21.8 -> 33.6 us).
    const size_t rtLds = bgRtLds(p.Qc, p.Kread, p.maxPrb, 8);
    if ((k.rt == 1 || (k.rt < 0 && p.nrb <= 2)) && rtLds <= 64 * 1024) {
        pl.kernel = BgKernel::BgRt;
        g.rbMode = 2;
        const int64_t nkb = (pl.nmac + 15) / 16;
        pl.blocks = std::min<int64_t>(bgXcdSlots(nkb, static_cast<int64_t>(C) * p.nrb), 65528);  // XCD-grouped slots
        pl.lds = rtLds;
    } else {
        pl.kernel = BgKernel::BgRb;
        g.rbMode = 1;
        pl.blocks = std::min<int64_t>(bgXcdSlots(g.nblocks, p.nrb), 65528);  // XCD-grouped slots
        pl.lds = 0;
    }
    pl.outcome = BgOutcome::Launch;
}

void planLarge(BgLaunchPlan& pl, const BgDev& p, const OutDesc& od, int C, int ncu, const BgKnobs& k) {
    BgGrid& g = pl.g;
    const int64_t nmac = pl.nmac;
    const int sz = p.f64 ? 8 : 4;
    pl.threads = 64 * g.ncg * g.nwt;
    const int tileN = 16 * g.ncg;
    const size_t slotBytes = static_cast<size_t>(g.ncg) * g.nslots * 256 * sz;
    // Two LDS tiles (double buffer) + partial slots (two buffers when they fit
    // beside a tile of >= 4 macro periods, else one + a second barrier).
    const int rowsPerPiece = p.f64 ? 2 : 4;
    auto wsFor = [&](int W) { return (W + rowsPerPiece - 1) / rowsPerPiece * rowsPerPiece; };
    auto tileBytes = [&](int G) { return 2 * static_cast<size_t>(tileN) * wsFor(p.Kread + (G - 1) * p.Qc) * sz; };
    const size_t kLds = 160 * 1024 - kBgStaticLds;  // bg_kernel's static LDS: the non-finite ranges
    g.parity = (g.nred > 0 && !k.noParity && tileBytes(std::min<int64_t>(4, std::max<int64_t>(nmac, 1))) + 2 * slotBytes <= kLds) ? 1 : 0;
    const size_t partBytes = (g.parity ? 2 : 1) * slotBytes;
    int G = 1;
    for (int cand = 2; cand <= 8; ++cand) {
        if (cand > nmac) break;
        if (tileBytes(cand) + partBytes > kLds) break;
        G = cand;
    }
    if (k.g > 0 && k.g < G) G = k.g;
    g.G = G;
    g.W = p.Kc + (G - 1) * p.Qc;
    g.Wl = p.Kread + (G - 1) * p.Qc;
    g.Ws = wsFor(g.Wl);
    const int64_t nchunk = (nmac + G - 1) / G;
    g.nchunk = static_cast<int>(nchunk);
    g.ncols = static_cast<int>(nchunk * C);
    g.nblocks = (g.ncols + tileN - 1) / tileN;
    if (!p.f64 && !od.f64 && !od.pcm && !k.noVst) {
        if (od.fs == 1) g.vst = 1;
        else if (C == 2 && od.fs == 2 && od.cs == 1) g.vst = 2;
    }
    pl.lds = tileBytes(G) + partBytes;
    pl.globalB = pl.lds > kLds;
    if (pl.globalB) pl.lds = partBytes;
    pl.blocks = std::min<int64_t>(g.nblocks, static_cast<int64_t>(ncu) * (k.wgPerCu > 0 ? k.wgPerCu : 2));
    pl.outcome = pl.lds > kLds ? BgOutcome::Invalid : (g.nblocks <= 0 ? BgOutcome::Nothing : BgOutcome::Launch);
}
}  // namespace

BgKnobs bgReadKnobs() {
    BgKnobs k;
    readKnobTable(kBgKnobTable, k, false);
    return k;
}

const BgKnobs& bgLaunchKnobs() {
    static const BgKnobs perProcess = bgReadKnobs();
    return perProcess;
}

BgLaunchPlan bgPlanLaunch(const BgDev& p, const SrcDesc&, const OutDesc& od, int C, int ncu, const BgKnobs& k, bool histKeep,
                          int64_t histN) {
    BgLaunchPlan pl;
    if (od.o_hi <= od.o_lo) return pl;
    pl.unit = p.f64 ? BgUnit::F64 : (p.NS < 56 ? BgUnit::F32a : BgUnit::F32b);
    BgGrid& g = pl.g;
    g.Pc = p.Pc; g.Qc = p.Qc; g.Kc = p.Kc; g.C = C;
    g.nprog = p.nprog;
    g.kch = p.kch;
    g.nwt = p.nw;
    g.ncg = p.ncg;
    g.nred = p.nred;
    g.nslots = p.nslots;
    g.dbg = k.dbg;
    g.a_lo = od.o_lo / p.Pc;
    pl.nmac = (od.o_hi + p.Pc - 1) / p.Pc - g.a_lo;
    if (isSmall(p, pl.nmac, C, ncu, k)) planSmall(pl, p, C, k);
    else planLarge(pl, p, od, C, ncu, k);
    pl.histFolded = pl.outcome == BgOutcome::Launch && histKeep && histN > 0;
    return pl;
}

int bgTraceLine(const BgLaunchPlan& pl, const BgDev& p, const OutDesc& od, char* buf, size_t cap) {
    const BgGrid& g = pl.g;
    static const char* const kernels[] = {"bg", "bg_rb", "bg_rt"};
    static const char* const units[] = {"f64", "f32a", "f32b"};
    return std::snprintf(buf, cap,
                         "bg: f64=%d Pc=%d Qc=%d Kc=%d Kread=%d NS=%d kch=%d nw=%d ncg=%d nprog=%d nred=%d nslots=%d G=%d nmac=%lld C=%d "
                         "nblocks=%d blocks=%lld lds=%zu globalB=%d o[%lld,%lld) kernel=%s unit=%s rbMode=%d parity=%d vst=%d W=%d Wl=%d "
                         "Ws=%d a_lo=%lld nchunk=%d ncols=%d threads=%d dbg=%d hist=%d\n",
                         p.f64, p.Pc, p.Qc, p.Kc, p.Kread, p.NS, g.kch, g.nwt, g.ncg, g.nprog, g.nred, g.nslots, g.G, (long long)pl.nmac,
                         g.C, g.nblocks, (long long)pl.blocks, pl.lds, pl.globalB ? 1 : 0, (long long)od.o_lo, (long long)od.o_hi,
                         kernels[static_cast<int>(pl.kernel)], units[static_cast<int>(pl.unit)], g.rbMode, g.parity, g.vst, g.W, g.Wl,
                         g.Ws, (long long)g.a_lo, g.nchunk, g.ncols, pl.threads, g.dbg, pl.histFolded ? 1 : 0);
}

}  // namespace gar
