// gar_hxs_launch.cpp -- host-only launch planner of the streaming FIR kernels (gar_hxs_launch.hpp).
// A sequence of small functions, each computing its part of the plan once from its inputs; the only
// revisions are the two named fallbacks of the group-size step.
#include "gar_hxs_launch.hpp"

#include <algorithm>
#include <cstdio>

#include "gar_knobs.hpp"

namespace gar {

// ---- knobs ----------------------------------------------------------------------------------------
namespace {
// name, field (its default: the member initialiser in HxsKnobs), how the value reads, when it is read
constexpr KnobRow<HxsKnobs> kHxsKnobTable[] = {
    {"GAR_HXS_G", &HxsKnobs::g, kInt, false},
    {"GAR_HXS_WGPERCU", &HxsKnobs::wgPerCu, kInt, false},
    {"GAR_HX_TRACE", &HxsKnobs::trace, kIsSet, false},
    // attribution bits: 1 no loads, 2 no stores, 4 no MFMA, 16 no conversion, 64 consume without converting, 128 no load issue
    {"GAR_HXS_DBG", &HxsKnobs::dbg, kInt, false},
    {"GAR_HXS_PROF", &HxsKnobs::prof, kIsSet, false},
    {"GAR_HXS_SMALL", &HxsKnobs::small, kInt, false},
    {"GAR_HXS_NP", &HxsKnobs::np, kInt, false},
    {"GAR_HXT", &HxsKnobs::hxt, kInt, false},
    {"GAR_HXS_SMALLK", &HxsKnobs::smallK, kInt, false},
    {"GAR_HXS_NT", &HxsKnobs::nt, kInt, false},
    {"GAR_HXS_PAIR", &HxsKnobs::pair, kInt, false},
    {"GAR_HXT_CHUNKMAJOR", &HxsKnobs::chunkMajor, kInt, false},
    {"GAR_HXT_COOP", &HxsKnobs::coop, kInt, false},
    {"GAR_HXQ", &HxsKnobs::hxq, kInt, false},
    {"GAR_HXQ_NR", &HxsKnobs::hxqNr, kInt, false},
    {"GAR_HXQ_OPT", &HxsKnobs::hxqOpt, kInt, false},
    {"GAR_HXQ_W", &HxsKnobs::hxqW, kInt, false},
    {"GAR_HXT_ROLES", &HxsKnobs::roles, kInt, true},
    {"GAR_HXT_WIDE", &HxsKnobs::wide, kInt, true},
    {"GAR_HXT_LEAN", &HxsKnobs::lean, kInt, true},
    {"GAR_HXT_FAULT", &HxsKnobs::fault, kIsOne, true},
};
}  // namespace

HxsKnobs hxsReadKnobs() {
    HxsKnobs k;
    readKnobTable(kHxsKnobTable, k, false);
    return k;
}

HxsKnobs hxsLaunchKnobs() {
    static const HxsKnobs perProcess = hxsReadKnobs();
    HxsKnobs k = perProcess;
    readKnobTable(kHxsKnobTable, k, true);
    return k;
}

// ---- plan steps -----------------------------------------------------------------------------------
namespace {

int sampleBytes(int pcm, int f64) { return pcm ? pcmBytes(pcm) : (f64 ? 8 : 4); }

// Compute-wave roles of hxt_kernel for nprog row blocks (HxsArgs::role): the first 4*floor(nprog/4)
// row blocks one wave each; one remaining row block shared by 4 waves (every 4th period), two by
// 2 waves each (every 2nd period), so waves w, w+4, w+8 -- one SIMD -- carry equal MFMA work.
struct HxtRoles {
    int ncomp = 0, maxStride = 1;  // compute waves; the largest period stride
    int role[kHxtMaxComp] = {};
};
HxtRoles hxtRoles(int nprog, int NS, bool leanPlan, const HxsKnobs& k) {
    // knob GAR_HXT_ROLES: 1 balanced, 0 one wave per row block; default balanced for NS >= 10, and for the
    // NS = 9 launches that run the lean loaders.
    // r04 (profiles/r04_ab): NS = 9 cfg2 0.125 ms one-per-row-block vs 0.145 balanced -- four generic loaders
    // beside twelve compute waves did not keep the ring ahead; NS = 10 cfg3 was the other way round.
    // r07 (profiles/r07_ab_cfg2_roles.txt): with the lean loaders four are enough -- cfg2 0.112-0.120 ms
    // balanced against 0.121-0.127 one-per-row-block and 0.123-0.129 for the r06 build on the same box.
    // NS = 9 plans on the generic loaders (other geometries, 16- / 32-channel rows) keep one wave per row block.
    const bool balanced = k.roles >= 0 ? k.roles != 0 : (NS >= 10 || leanPlan);
    HxtRoles r;
    int w = 0;
    if (!balanced) {  // one wave per row block (hxs_kernel's mapping), six loaders beside ten compute waves
        for (int i = 0; i < nprog; ++i) r.role[w++] = i | (1 << 16);
        r.ncomp = w;
        return r;
    }
    const int q = nprog / 4 * 4, rem = nprog - q;
    for (int i = 0; i < q; ++i) r.role[w++] = i | (1 << 16);
    if (rem == 2 && q + 4 <= kHxtMaxComp) {
        for (int i = 0; i < 4; ++i) r.role[w++] = (q + (i & 1)) | ((i >> 1) << 8) | (2 << 16);
        r.maxStride = 2;
    } else if (rem == 1 && q + 4 <= kHxtMaxComp) {
        for (int i = 0; i < 4; ++i) r.role[w++] = q | (i << 8) | (4 << 16);
        r.maxStride = 4;
    } else {
        for (int i = q; i < nprog; ++i) r.role[w++] = i | (1 << 16);
    }
    r.ncomp = w;
    return r;
}

// small launches (stream chunks, flush tails): one macro period per column, each block's window
// gathered in one pass -- latency over bandwidth (knob GAR_HXS_SMALL=0/1 forces)
bool isSmall(int64_t nmac, int C, int ncu, const HxsKnobs& k) {
    return k.small >= 0 ? k.small == 1 : nmac * C <= static_cast<int64_t>(16) * 2 * ncu;
}

// 32-channel blocks of f32 rows on hxt_kernel (ROW32, gar_hxt.hpp): whole 128-B lines per load and store
// instruction.  Decided before the chunk count, which is sized for the block width (r06g: cfg3 fell back to
// 16-channel blocks after chunks sized for 32, 512 half-length blocks, traffic / algorithmic 1.06 -> 1.12,
// +7 %): only where the 32-channel ring takes groups of >= 2 periods and the plan runs one compute wave per
// row block (balanced roles, NS = 10 as cfg3, measured slower on 32 channels).  Knob GAR_HXT_WIDE=0: never.
bool wantsWideBlocks(const HxDev& p, const SrcDesc& src, const OutDesc& od, int C, bool small, const HxsKnobs& k) {
    const bool rows32 = !small && src.in && !src.in_pcm && !src.in_f64 && !od.pcm && !od.f64 && C % 32 == 0 && od.cs == 1 &&
                        (reinterpret_cast<uintptr_t>(src.in) & 15) == 0 && src.in_cs == 1 && src.in_fs % 4 == 0;
    if (!rows32 || k.wide == 0) return false;
    const HxtRoles roles = hxtRoles(p.nw, p.NS, false, k);
    const HxsRing r2 = hxsRingFor(p.Qc, p.Kread, 2);
    return roles.maxStride == 1 && hxtLdsWide(r2.Rt) <= kHxsLdsMax &&
           2 * p.Qc <= hxtMaxRowsF(kFmtRow32, hxtLoadersFor(roles.ncomp)) && r2.R / (2 * p.Qc) + 3 <= kHxtSlots;
}

// Columns are (channel, chunk of Np consecutive macro periods), blocks of bw columns: about one block
// per CU.  Raw loads address a chunk's rows with 32-bit offsets from the chunk's first row, so
// (Np*Qc + rows of one group + a piece) rows must span less than 2^31 bytes (rawSpan).
struct HxsChunks {
    int64_t Np, nchunk, ncols;
    bool rawSpan;
};
HxsChunks chunkLaunch(const HxDev& p, const SrcDesc& src, int C, int ncu, int64_t nmac, bool small, int bw, int inEsz,
                      const HxsKnobs& k) {
    const int64_t Qc = p.Qc;
    const int64_t targetBlocks = static_cast<int64_t>(ncu) * (k.wgPerCu > 0 ? k.wgPerCu : 1);
    const int64_t nchunkT = small ? nmac : std::max<int64_t>(1, (targetBlocks * bw + C - 1) / C);
    const int64_t NpT = (k.np > 0 && !small) ? k.np : std::max<int64_t>(1, ceilDiv(nmac, nchunkT));
    const int64_t rowBytes = std::max<int64_t>(4, src.in_fs * inEsz);
    const int64_t chunksPerRsrc = (C <= 16 && 16 % C == 0) ? 16 / C : 1;  // STEREO: one resource spans 8 chunks
    const int64_t npMax = ((int64_t(1) << 31) / rowBytes / chunksPerRsrc - (3 * Qc + p.Kread + 256)) / Qc;
    HxsChunks c;
    c.rawSpan = npMax >= 1;
    c.Np = c.rawSpan ? std::min(NpT, npMax) : NpT;
    const int64_t nchunk = ceilDiv(nmac, c.Np);
    // whole blocks where the channel count divides 16 (empty trailing chunks read zeros, store nothing)
    c.nchunk = (16 % C == 0 && !small) ? ceilDiv(nchunk * C, 16) * 16 / C : nchunk;
    c.ncols = c.nchunk * C;
    return c;
}

// Load layout: stereo frames, 16-channel rows, or gathered at conversion time for any other layout.
// No caller input (a flush: history + zeros): every row comes from the history, [t][C] f32 with row stride
// hist_ld, so the layout is the history's -- instead of per-column element gathers (cfg2's flush launch:
// 13.7 us on the gathers, r05d trace).
int loadLayout(const SrcDesc& src, int C) {
    if (!src.in) {
        const uintptr_t hA = reinterpret_cast<uintptr_t>(src.hist);
        if (C == 2 && src.hist_ld == 2 && (hA & 7) == 0) return kFmtStereo;
        if (C % 16 == 0 && src.hist_ld % 4 == 0 && (hA & 15) == 0) return kFmtRow16;
        return kFmtGather;
    }
    const uintptr_t inA = reinterpret_cast<uintptr_t>(src.in);
    const bool stereoIl = C == 2 && src.in_fs == 2 && src.in_cs == 1;
    const bool rows16 = C % 16 == 0 && src.in_cs == 1 && src.in_fs % 4 == 0;
    if (sampIsHalf(src.in_pcm)) {  // stereo frames (one dword each) or 16-channel rows (32 B)
        if ((inA & 3) == 0 && stereoIl) return kFmtStereoHalf;
        if ((inA & 7) == 0 && rows16) return kFmtRow16Half;
        return kFmtGather;
    }
    if (src.in_pcm == 16) return ((inA & 3) == 0 && stereoIl) ? kFmtStereoPcm16 : kFmtGather;
    if (src.in_pcm) return ((inA & 7) == 0 && stereoIl) ? kFmtStereoPcm32 : kFmtGather;  // other PCM layouts are gathered
    if (src.in_f64) return kFmtGather;
    if ((inA & 7) == 0 && stereoIl) return kFmtStereo;
    if ((inA & 15) == 0 && rows16) return kFmtRow16;
    return kFmtGather;
}

// Store layout of the epilogue (hxsStoreFast VST); outBase: the address of output 0.
int storeLayout(const OutDesc& od, int C, int Pc, uintptr_t outBase) {
    const bool al = (outBase & 15) == 0;
    const bool stereoIl = C == 2 && od.fs == 2 && od.cs == 1 && Pc % 4 == 0;
    if (od.pcm == 16 && al && stereoIl) return kVstStereoPcm16;
    // half stereo frame pairs: 8-B stores at multiples of 8 B from the base, so an 8-B aligned base does (a flush
    // after an odd number of output frame pairs has one)
    if (sampIsHalf(od.pcm) && (outBase & 7) == 0 && stereoIl) return kVstStereoHalf;
    if (od.pcm) return kVstAny;  // other PCM / half stores: the epilogue's checked per-element path
    if (od.f64) return kVstF64;
    if (al && stereoIl) return kVstStereo;
    if (al && od.fs == 1 && (od.cs * 4) % 16 == 0 && Pc % 4 == 0) return kVstRows;
    return kVstAny;
}

// Balanced kernel (hxt_kernel): f32 stereo frames or 16-channel rows in, f32 out (knob GAR_HXT=0: hxs_kernel).
// Default: hxt_kernel wherever its load / store layouts apply -- after its loader spill fixes it beats
// hxs_kernel on every BASELINE plan (profiles/r04_ab: cfg2 0.125 vs 0.130 ms, ns256 1.81 vs 1.84 ms, cfg3 0.33
// vs 0.46 ms); hxs_kernel keeps PCM, f16 / bf16, f64 and other layouts.
bool hxtApplies(const SrcDesc& src, const OutDesc& od, bool small, int fmt, int vst, const HxsKnobs& k) {
    return k.hxt != 0 && !small && !od.pcm && !od.f64 && !src.in_pcm &&
           ((fmt == kFmtStereo && vst == kVstStereo) || (fmt == kFmtRow16 && (vst == kVstAny || vst == kVstRows)));
}

// The launch can run the lean loaders (gar_hxt.hpp: the Q24 44.1k -> 48k plan on stereo f32 frames; knob
// GAR_HXT_LEAN=0: generic loaders and their role default for this plan too) -- confirmed against the ring
// geometry once the group size is known (leanGeoIs).
bool isLeanPlan(const HxDev& p, const SrcDesc& src, bool hxt, int fmt, int vst, int inEsz, int64_t Np, const HxsKnobs& k) {
    using Geo = HxtLeanGeo<4>;
    return hxt && !kHxsDev && p.NS == kHxtLeanNS && p.Pc == kHxtLeanPc && p.Qc == Geo::Qc && p.Kread == Geo::Kread &&
           p.nw == kHxtLeanNw && fmt == kFmtStereo && vst == kVstStereo && src.in_fs == 2 && inEsz == 4 && Np >= Geo::G &&
           k.lean != 0;
}
template <int NL>
bool leanGeoIs(const HxDev& p, int G, const HxsRing& r) {
    using Geo = HxtLeanGeo<NL>;
    return p.Qc == Geo::Qc && G == Geo::G && r.R == Geo::R && r.Rt == Geo::Rt && r.Wg == Geo::Wg &&
           std::max(0, r.Wg - G * p.Qc) == Geo::mirror;
}

// Group size: the largest G <= kHxsMaxG (small launches: 1) that is not above Np or the GAR_HXS_G cap and
// fits the LDS ring and, on hxt_kernel, the loaders' registers and the arrival slots: a producer runs at
// most (ring slots + 2) loads / groups ahead of the slowest one, which the slots must cover (gar_hxt.hpp
// progress counters).  hxt_kernel with shared row blocks: a multiple of the period stride first.  G = 0: none.
struct HxsGroup {
    int G = 0;
    HxsRing ring{0, 0, 0};
};
HxsGroup pickGroup(const HxDev& p, int fmt, bool hxt, const HxtRoles& roles, bool small, int64_t Np, const HxsKnobs& k) {
    for (int pass = hxt && roles.maxStride > 1 ? 0 : 1; pass < 2; ++pass) {
        for (int cand = small ? 1 : kHxsMaxG; cand >= 1; --cand) {
            const HxsRing r = hxsRingFor(p.Qc, p.Kread, cand);
            if (cand > 1 && cand > Np) continue;
            if (k.g > 0 && cand > k.g && cand > 1) continue;
            if (fmt == kFmtRow32 ? hxtLdsWide(r.Rt) > kHxsLdsMax : !hxsRingFits(p.Qc, cand, r.Rt)) continue;
            if (hxt && cand * p.Qc > hxtMaxRowsF(fmt, hxtLoadersFor(roles.ncomp))) continue;
            if (hxt && r.R / (cand * p.Qc) + 3 > kHxtSlots) continue;
            if (pass == 0 && cand % roles.maxStride != 0) continue;
            return {cand, r};
        }
    }
    return {};
}

// Kernel, layout and group size together, with the two fallbacks:
//  * 32-channel blocks -> 16-channel blocks: a 32-channel ring holds half the rows, so it is kept only with
//    groups of >= 2 periods and one compute wave per row block (r06y / r06z: cfg3, NS = 10 on balanced roles
//    at G = 2, lost 4-12 % -- its chunks halve, traffic / algorithmic 1.06 -> 1.12);
//  * hxt_kernel -> hxs_kernel: no group size fits hxt_kernel's limits, so hxs_kernel's apply.
struct HxsChoice {
    bool hxt = false;
    int fmt = kFmtGather;
    HxtRoles roles;
    HxsGroup grp;
};
HxsChoice chooseKernel(const HxDev& p, int fmt, bool hxt, bool wide, const HxtRoles& roles, bool small, int64_t Np,
                       const HxsKnobs& k) {
    if (wide) {
        const HxsGroup g = pickGroup(p, kFmtRow32, true, roles, small, Np, k);
        if (g.G >= 2 && roles.maxStride == 1) return {true, kFmtRow32, roles, g};
    }
    const HxsGroup g = pickGroup(p, fmt, hxt, roles, small, Np, k);
    if (g.G > 0 || !hxt) return {hxt, fmt, hxt ? roles : HxtRoles{}, g};
    return {false, fmt, HxtRoles{}, pickGroup(p, fmt, false, HxtRoles{}, small, Np, k)};
}

// Block order over the 8 XCDs: ROW16 blocks 2m, 2m+1 share every 128-B line, so they run on one XCD (1);
// ROW32 blocks run chunk-major (2).
int xcdOrder(int fmt, int C, int nblocks, const HxsKnobs& k) {
    if (k.chunkMajor && fmt == kFmtRow32 && nblocks % 8 == 0) return 2;
    return k.pair && fmt == kFmtRow16 && (C / 16) % 2 == 0 && nblocks % 16 == 0 ? 1 : 0;
}

// Small float launches: hxq_kernel over (block, row-block group) workgroups, the largest group whose launch
// still has a workgroup per CU (a stereo 4096-frame call: one row block per workgroup, 40 workgroups; 256
// channels: all ten, 448 workgroups -- measured 18 us per call against 30 us with five).  Knobs: GAR_HXQ=0
// (hxs_small_kernel), GAR_HXQ_NR (group size).  Returns the row blocks per workgroup, 0: not hxq_kernel.
int hxqRowBlocks(const HxDev& p, const SrcDesc& src, int C, int ncu, const HxsLaunchPlan& pl, bool rawSpan, int64_t histN,
                 const HxsKnobs& k) {
    const int fmt = pl.fmt, inEsz = pl.in_esz;
    const uintptr_t hA = reinterpret_cast<uintptr_t>(src.hist);
    const int hAl = fmt == kFmtStereo ? 8 : (fmt == kFmtRow16 ? 16 : 4), hLd = fmt == kFmtStereo ? 2 : (fmt == kFmtRow16 ? 4 : 1);
    const bool histOk = !src.hist || src.hist_len <= 0 ||
                        ((hA % hAl) == 0 && src.hist_ld % hLd == 0 && src.hist_len * src.hist_ld * 4 < (int64_t(1) << 31));
    // any other f32 / f64 layout: per-column element loads, every offset from the block's first row < 2^31
    const int64_t spanRows = (16 / C + 2) * pl.Np * p.Qc + pl.Wg;
    const bool gen = fmt == kFmtGather && !src.in_pcm && src.in_fs >= 0 && src.in_cs >= 0 &&
                     (spanRows * src.in_fs + static_cast<int64_t>(C) * src.in_cs) * inEsz < (int64_t(1) << 31);
    // history keep through buffer loads from row ht0: offsets < 2^31
    const bool hkOk = histN <= 0 || (histN * src.in_fs + static_cast<int64_t>(C) * src.in_cs) * inEsz < (int64_t(1) << 31);
    const bool loadsOk = (fmt == kFmtStereo || fmt == kFmtRow16) ? rawSpan : gen;
    if (!(pl.small && k.hxq && loadsOk && histOk && hkOk && p.nw <= 12 && pl.Np == 1)) return 0;
    if (k.hxqNr > 0) return std::min(k.hxqNr, p.nw);
    for (int cand = p.nw; cand >= 1; --cand)
        if (pl.nblocks * static_cast<int64_t>(ceilDiv(p.nw, cand)) >= static_cast<int64_t>(ncu)) return cand;
    return 1;
}

}  // namespace

bool hxsPlanFits(const HxDev& p) {
    if (!p.rb || p.nw > kHxRbMaxWaves || !hxsNsBuilt(p.NS)) return false;
    return hxsRingFits(p.Qc, 1, hxsRingFor(p.Qc, p.Kread, 1).Rt);
}

HxsLaunchPlan hxsPlanLaunch(const HxDev& p, const SrcDesc& src, const OutDesc& od, int C, int ncu, const HxsKnobs& k,
                            bool histKeep, int64_t histN) {
    HxsLaunchPlan pl;
    if (!p.rb || p.nw > kHxRbMaxWaves || !hxsNsBuilt(p.NS)) return pl;
    pl.a_lo = floorDiv(od.o_lo, p.Pc);
    pl.a_hi = ceilDiv(od.o_hi, p.Pc);
    const int64_t nmac = pl.a_hi - pl.a_lo;
    const bool small = isSmall(nmac, C, ncu, k);
    const bool wideWanted = wantsWideBlocks(p, src, od, C, small, k);
    pl.in_esz = sampleBytes(src.in_pcm, src.in_f64);
    pl.out_esz = sampleBytes(od.pcm, od.f64);
    const HxsChunks ch = chunkLaunch(p, src, C, ncu, nmac, small, wideWanted ? 32 : 16, pl.in_esz, k);
    if (ch.ncols > (int64_t(1) << 30) || ch.Np > (int64_t(1) << 24)) return pl;
    // integer arithmetic: either base may point outside the caller's buffer, only rows inside it are dereferenced
    pl.inBase = reinterpret_cast<uintptr_t>(src.in) - static_cast<uintptr_t>(src.in_base * src.in_fs * pl.in_esz);
    pl.outBase = reinterpret_cast<uintptr_t>(od.out) - static_cast<uintptr_t>(od.o0 * od.fs * pl.out_esz);
    const int fmt = loadLayout(src, C);
    pl.vst = storeLayout(od, C, p.Pc, pl.outBase);
    const bool hxtWanted = hxtApplies(src, od, small, fmt, pl.vst, k);
    const bool leanPlan = isLeanPlan(p, src, hxtWanted, fmt, pl.vst, pl.in_esz, ch.Np, k);
    const HxtRoles roles = hxtWanted ? hxtRoles(p.nw, p.NS, leanPlan, k) : HxtRoles{};
    const bool wide = wideWanted && hxtWanted && fmt == kFmtRow16 && pl.vst == kVstAny;
    const HxsChoice c = chooseKernel(p, fmt, hxtWanted, wide, roles, small, ch.Np, k);
    if (c.grp.G == 0) return pl;

    pl.ok = true;
    pl.fmt = c.fmt;
    pl.small = small ? 1 : 0;
    pl.bigSmall = k.smallK ? 0 : 1;
    pl.Np = ch.Np; pl.nchunk = ch.nchunk; pl.ncols = ch.ncols;
    pl.nblocks = static_cast<int>(c.fmt == kFmtRow32 ? (ch.ncols + 31) / 32 : (ch.ncols + 15) / 16);
    pl.G = c.grp.G;
    pl.ngroups = static_cast<int>(ceilDiv(ch.Np, pl.G));
    pl.Wg = c.grp.ring.Wg;
    pl.groupR = c.grp.ring.R; pl.groupRt = c.grp.ring.Rt;
    // small launches stage only the window [0, Wg) of one period: no ring wrap, no mirror rows
    const bool window = small && !pl.bigSmall;
    const int w16 = (pl.Wg + 15) / 16 * 16;
    pl.R = window ? w16 : pl.groupR;
    pl.Rt = window ? w16 : pl.groupRt;
    pl.mirror = window ? 0 : std::max(0, pl.Wg - pl.G * p.Qc);
    pl.ncomp = c.roles.ncomp; pl.maxStride = c.roles.maxStride;
    for (int w = 0; w < kHxtMaxComp; ++w) pl.role[w] = c.roles.role[w];
    pl.loaders = c.hxt ? hxtLoadersFor(pl.ncomp) : 0;
    // lean loaders: an exact match of the plan and ring fields; everything else runs the generic loaders
    pl.lean = leanPlan && c.hxt && (pl.loaders == 6 ? leanGeoIs<6>(p, pl.G, c.grp.ring) : leanGeoIs<4>(p, pl.G, c.grp.ring));
    pl.xcdPair = xcdOrder(pl.fmt, C, pl.nblocks, k);
    pl.qRbs = hxqRowBlocks(p, src, C, ncu, pl, ch.rawSpan, histN, k);
    pl.qGroups = pl.qRbs ? static_cast<int>(ceilDiv(p.nw, pl.qRbs)) : 0;
    pl.qOpt = pl.qRbs ? k.hxqOpt : 0;
    // raw input: element (t, c) at inBase + (t*in_fs + c*in_cs)*in_esz for t in [fastLo, fastHi); hxq_kernel's
    // gathered path checks per lane, so it takes the caller's rows whatever the strides
    const bool rawOk = src.in && pl.fmt != kFmtGather && src.in_len > 0 && src.in_fs > 0 && src.in_cs >= 0 && ch.rawSpan;
    if (rawOk || (pl.qRbs && pl.fmt == kFmtGather && src.in)) {
        pl.fastLo = src.in_base;
        pl.fastHi = std::min(src.in_base + src.in_len, src.valid_end);
    }
    pl.kernel = c.hxt ? HxsKernel::Hxt : pl.qRbs ? HxsKernel::Hxq : window ? HxsKernel::HxsSmall : HxsKernel::Hxs;
    pl.lds = pl.fmt == kFmtRow32 ? hxtLdsWide(pl.Rt) : hxsLds(pl.Rt);
    pl.histFolded = histKeep && histN > 0;
    return pl;
}

int hxsTraceLines(const HxsLaunchPlan& pl, const OutDesc& od, int C, char* buf, size_t cap) {
    // R, Rt: the ring of G periods (before a small launch's trim to one window); fast: the raw-load rows
    // (a gathered layout has none, whatever hxq_kernel's checked loads may touch)
    const bool raw = pl.fmt != kFmtGather;
    int n = std::snprintf(buf, cap, "%s: small=%d o[%lld,%lld) C=%d G=%d Np=%lld ngroups=%d nblocks=%d R=%d Rt=%d Wg=%d fmt=%d vst=%d fast[%lld,%lld) ncomp=%d lean=%d\n",
                          pl.kernel == HxsKernel::Hxt ? "hxt" : "hxs", pl.small, (long long)od.o_lo, (long long)od.o_hi, C, pl.G,
                          (long long)pl.Np, pl.ngroups, pl.nblocks, pl.groupR, pl.groupRt, pl.Wg, pl.fmt, pl.vst,
                          (long long)(raw ? pl.fastLo : 0), (long long)(raw ? pl.fastHi : 0), pl.ncomp, pl.lean ? 1 : 0);
    if (n < 0 || static_cast<size_t>(n) >= cap) return n;
    if (pl.qGroups > 0)
        n += std::snprintf(buf + n, cap - n, "hxq: qRbs=%d qGroups=%d workgroups=%lld\n", pl.qRbs, pl.qGroups,
                           (long long)pl.nblocks * pl.qGroups);
    return n;
}

}  // namespace gar
