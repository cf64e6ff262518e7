// gar_hxs.hip -- launch geometry of the streaming split-f16 kernel (gar_hxs.hpp)
// for row-block plans.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "gar_hx_launch.hpp"
#include "gar_hxt.hpp"

namespace gar {

// instantiations live in gar_hxs_i1.hip / gar_hxs_i2.hip / gar_hxs_i3.hip / gar_hxs_i4.hip (compiled in parallel)
#define GAR_HXS_EXT(NS, V) extern template hipError_t hxsLaunch<NS, V>(const HxsArgs&, size_t, int64_t, hipStream_t, int);
GAR_HXS_FOR_ALL(GAR_HXS_EXT)
#undef GAR_HXS_EXT
// the dither instantiations: gar_hxs_i4.hip
#define GAR_HXS_EXT_DITHER(NS, V) extern template hipError_t hxsLaunchDither<NS, V>(const HxsArgs&, size_t, int64_t, hipStream_t, int);
GAR_HXS_FOR_DITHER(GAR_HXS_EXT_DITHER)
#undef GAR_HXS_EXT_DITHER
// the metered instantiations (declared in gar_hxs.hpp, defined in their units only): gar_hxs_i5.hip / gar_hxs_i6.hip
// hxt_kernel instantiations: gar_hxt_i1.hip / gar_hxt_i2.hip
#define GAR_HXT_EXT(NS, F, V, L) extern template hipError_t hxtLaunch<NS, F, V, L>(const HxsArgs&, size_t, int64_t, hipStream_t);
GAR_HXT_FOR_A(GAR_HXT_EXT)
GAR_HXT_FOR_B(GAR_HXT_EXT)
#undef GAR_HXT_EXT
// lean-loader kernels: gar_hxt_i3.hip
#define GAR_HXT_EXT_LEAN(NS, F, V, L, E) extern template hipError_t hxtLaunch<NS, F, V, L, E>(const HxsArgs&, size_t, int64_t, hipStream_t);
GAR_HXT_FOR_LEAN(GAR_HXT_EXT_LEAN)
#undef GAR_HXT_EXT_LEAN

namespace {
constexpr int kProfWords = 64 + 2 * 4096;
// development: GAR_HXS_PROF=1 sums per-phase s_memtime cycles of every launch and prints them at exit
unsigned long long* profBuf(bool on) {
    static unsigned long long* p = nullptr;
    static bool init = false;
    if (!init) {
        init = true;
        if (on && hipMalloc(&p, kProfWords * sizeof(unsigned long long)) == hipSuccess) {
            (void)hipMemset(p, 0, kProfWords * sizeof(unsigned long long));
            (void)hipMemset(p + 10, 0xff, sizeof(unsigned long long));
            (void)hipMemset(p + 13, 0xff, sizeof(unsigned long long));
            std::atexit([] {
                static unsigned long long h[kProfWords] = {};
                if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h, p, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
                    const double nl = h[3] ? static_cast<double>(h[3]) : 1, nc = h[6] ? static_cast<double>(h[6]) : 1;
                    fprintf(stderr, "hxs prof per wave (cycles): loaders convert %.0f issue+wait %.0f (issue %.0f) barrier %.0f (life %.1f us) | compute convert+mfma %.0f barrier %.0f\n",
                            h[0] / nl, h[1] / nl, h[7] / nl, h[2] / nl, h[9] / nl / 100.0, h[4] / nc, h[5] / nc);
                    fprintf(stderr, "hxs loader pre-loop %.2f us, post-loop %.2f us; compute convert %.0f\n", h[8] / nl / 100.0, h[12] / nl / 100.0, h[15] / nc);
                    if (h[23]) fprintf(stderr, "hxs wave-0 first block (cycles): entry->window %.0f, window->steps done %.0f, ->exit (stores drained) %.0f, n %llu\n",
                                       static_cast<double>(h[20]) / h[23], static_cast<double>(h[21]) / h[23], static_cast<double>(h[22]) / h[23], h[23]);
                    if (h[23]) fprintf(stderr, "hxs wave-0: entry->A landed %.0f, entry->barrier 1 %.0f; wave entry spread in a workgroup %.0f, wave 0 after first wave %.0f\n",
                                       static_cast<double>(h[24]) / h[23], static_cast<double>(h[25]) / h[23], static_cast<double>(h[26]) / h[23], static_cast<double>(h[27]) / h[23]);
                    if (h[34]) fprintf(stderr, "hxt roles per block (cycles): compute wave 0 %.0f (waiting %.0f), loader 0 %.0f (waiting %.0f), n %llu\n",
                                       static_cast<double>(h[30]) / h[34], static_cast<double>(h[32]) / h[34], static_cast<double>(h[31]) / h[34],
                                       static_cast<double>(h[33]) / h[34], h[34]);
                    if (h[34]) fprintf(stderr, "hxt compute wave 0: entry -> first group %.0f cycles, last group -> exit %.0f cycles, periods %.0f, arrivals %.0f\n",
                                       static_cast<double>(h[35]) / h[34], static_cast<double>(h[36]) / h[34],
                                       static_cast<double>(h[37]) / h[34], static_cast<double>(h[38]) / h[34]);
                    if (h[34] && h[57]) fprintf(stderr, "hxt fill (cycles): entry -> A issued %.0f, -> fill barrier %.0f, -> first group %.0f; in-kernel clock %.3f GHz\n",
                                       static_cast<double>(h[53]) / h[34], static_cast<double>(h[54]) / h[34], static_cast<double>(h[55]) / h[34],
                                       0.1 * static_cast<double>(h[56]) / static_cast<double>(h[57]));
                    if (h[34]) fprintf(stderr, "hxt loader 0 phases (cycles): load data wait %.0f, conversion %.0f, arrival %.0f\n",
                                       static_cast<double>(h[50]) / h[34], static_cast<double>(h[51]) / h[34], static_cast<double>(h[52]) / h[34]);
                    if (h[44]) fprintf(stderr, "hxq wave 0 (cycles): entry->barrier 1 %.0f, ->image %.0f, ->MFMA+stores issued %.0f, ->drained %.0f, n %llu\n",
                                       static_cast<double>(h[40]) / h[44], static_cast<double>(h[41]) / h[44], static_cast<double>(h[42]) / h[44],
                                       static_cast<double>(h[43]) / h[44], h[44]);
                    fprintf(stderr, "hxs span: first start -> last end %.1f us; loader wave life min %.1f max %.1f us\n",
                            (h[11] - h[10]) / 100.0, h[13] / 100.0, h[14] / 100.0);
                    // per-workgroup life (last launch): percentiles, by blockIdx % 8, slowest
                    std::vector<std::pair<double, int>> v;
                    unsigned long long t0 = ~0ull;
                    for (int b = 0; b < 4096; ++b)
                        if (h[65 + 2 * b]) { v.push_back({h[65 + 2 * b] / 100.0, b}); t0 = std::min(t0, h[64 + 2 * b]); }
                    if (!v.empty()) {
                        std::vector<std::pair<double, int>> sv = v;
                        std::sort(sv.begin(), sv.end());
                        auto pc = [&](double q) { return sv[std::min(sv.size() - 1, static_cast<size_t>(q * sv.size()))].first; };
                        fprintf(stderr, "hxs WG life us: n %zu min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f |", sv.size(), sv.front().first, pc(0.1), pc(0.5), pc(0.9), sv.back().first);
                        for (int m = 0; m < 8; ++m) {
                            double s = 0; int n = 0;
                            for (auto& e : v) if (e.second % 8 == m) { s += e.first; ++n; }
                            fprintf(stderr, " x%d %.1f", m, n ? s / n : 0.0);
                        }
                        fprintf(stderr, "\n  slowest:");
                        for (size_t k = sv.size(); k-- > 0 && k + 8 >= sv.size();)
                            fprintf(stderr, " b%d %.1fus@+%.1f", sv[k].second, sv[k].first, (h[64 + 2 * sv[k].second] - t0) / 100.0);
                        fprintf(stderr, "\n");
                    }
                }
            });
        }
    }
    return p;
}

// hxt_kernel by load / store layout, loader count and loaders (lean: HxtLeanGeo<NL>, matched by the planner)
template <int NS, int NL>
hipError_t hxtFmtL(const HxsArgs& x, size_t lds, int64_t blocks, hipStream_t st, bool lean) {
    if constexpr (NS == kHxtLeanNS)
        if (lean && x.fmt == kFmtStereo && x.vst == kVstStereo) return hxtLaunch<NS, kFmtStereo, kVstStereo, NL, 1>(x, lds, blocks, st);
    if (x.fmt == kFmtStereo && x.vst == kVstStereo) return hxtLaunch<NS, kFmtStereo, kVstStereo, NL>(x, lds, blocks, st);
    if (x.fmt == kFmtRow16 && x.vst == kVstAny) return hxtLaunch<NS, kFmtRow16, kVstAny, NL>(x, lds, blocks, st);
    if (x.fmt == kFmtRow16 && x.vst == kVstRows) return hxtLaunch<NS, kFmtRow16, kVstRows, NL>(x, lds, blocks, st);
    if (x.fmt == kFmtRow32 && x.vst == kVstAny) return hxtLaunch<NS, kFmtRow32, kVstAny, NL>(x, lds, blocks, st);
    return hipErrorNotSupported;
}
template <int NS>
hipError_t hxtFmt(const HxsArgs& x, size_t lds, int64_t blocks, hipStream_t st, bool lean) {
    return hxtLoadersFor(x.ncomp) == 6 ? hxtFmtL<NS, 6>(x, lds, blocks, st, lean) : hxtFmtL<NS, 4>(x, lds, blocks, st, lean);
}

template <int NS>
hipError_t hxsVst(const HxsArgs& x, size_t lds, int64_t blocks, hipStream_t st, int qWaves, uint64_t* meter) {
    if (meter) {  // integer PCM output (launchHxsPlan): the two store layouts that take it
        if (x.vst == kVstAny) return hxsLaunchMeter<NS, kVstAny>(x, meter, lds, blocks, st, qWaves);
        if (x.vst == kVstStereoPcm16) return hxsLaunchMeter<NS, kVstStereoPcm16>(x, meter, lds, blocks, st, qWaves);
        return hipErrorNotSupported;
    }
    switch (x.vst) {
        case kVstAny:
            return x.dither ? hxsLaunchDither<NS, kVstAny>(x, lds, blocks, st, qWaves) : hxsLaunch<NS, kVstAny>(x, lds, blocks, st, qWaves);
        case kVstRows: return hxsLaunch<NS, kVstRows>(x, lds, blocks, st, qWaves);
        case kVstStereo: return hxsLaunch<NS, kVstStereo>(x, lds, blocks, st, qWaves);
        case kVstStereoPcm16:
            return x.dither ? hxsLaunchDither<NS, kVstStereoPcm16>(x, lds, blocks, st, qWaves)
                            : hxsLaunch<NS, kVstStereoPcm16>(x, lds, blocks, st, qWaves);
        case kVstStereoHalf: return hxsLaunch<NS, kVstStereoHalf>(x, lds, blocks, st, qWaves);
        default: return hxsLaunch<NS, kVstF64>(x, lds, blocks, st, qWaves);
    }
}

// HxsArgs of a planned launch: every decision from the plan, the tables and pointers from the device plan.
HxsArgs hxsArgsOf(const HxsLaunchPlan& pl, const HxDev& p, const SrcDesc& src, const OutDesc& od, int C, const HxsKnobs& k) {
    HxsArgs x{};
    x.A = static_cast<const h8v*>(p.A);
    x.progs = p.progs;
    x.ea = p.ea;
    x.Pc = p.Pc; x.Qc = p.Qc; x.Kc = p.Kc; x.Kread = p.Kread; x.G = pl.G; x.C = C;
    x.nprog = p.nw;
    x.ncols = static_cast<int>(pl.ncols);
    x.nblocks = pl.nblocks;
    x.Np = static_cast<int>(pl.Np);
    x.ngroups = pl.ngroups;
    x.R = pl.R; x.Rt = pl.Rt; x.mirror = pl.mirror; x.Wg = pl.Wg;
    x.a_lo = pl.a_lo; x.a_hi = pl.a_hi;
    x.dbg = k.dbg;
    x.prof = profBuf(k.prof != 0);
    x.o_lo = od.o_lo; x.o_hi = od.o_hi;
    x.in_esz = pl.in_esz;
    x.in_pcm = src.in_pcm;
    x.in = reinterpret_cast<const char*>(pl.inBase);
    x.in_fs = src.in_fs;
    x.in_cs = src.in_cs;
    x.fastLo = pl.fastLo;
    x.fastHi = pl.fastHi;
    x.fmt = pl.fmt;
    x.small = pl.small;
    x.bigSmall = pl.bigSmall;
    x.nt = k.nt;
    x.xcdPair = pl.xcdPair;
    // output (o, c) at out + o*out_fs + c*out_cs bytes (o absolute)
    x.out_pcm = od.pcm;
    x.out_f64 = od.f64;
    x.out = reinterpret_cast<char*>(pl.outBase);
    x.out_fs = od.fs * pl.out_esz;
    x.out_cs = od.cs * pl.out_esz;
    x.dither = pcmIsInt(od.pcm) ? od.dither : 0;
    x.dseedLo = od.dseedLo;
    x.dseedHi = od.dseedHi;
    x.dpos = od.dpos0 - od.o0;
    x.vst = pl.vst;
    x.ncomp = pl.ncomp;
    for (int w = 0; w < kHxtMaxComp; ++w) x.role[w] = pl.role[w];
    // progress-wait bound and the device status word; development knob GAR_HXT_FAULT=1 makes the compute
    // waves' load count unreachable and the bound short: the launch must end with GAR_ERR_DEVICE, not with output
    const bool fault = pl.kernel == HxsKernel::Hxt && k.fault;
    x.err = od.err;
    x.pollMax = fault ? 1 << 12 : 1 << 24;
    x.faultNeed = fault ? 1 << 28 : 0;
    x.coop = std::max(0, std::min(2, k.coop));
    x.src = src;
    x.od = od;
    x.ex = p.ex;
    if (pl.qGroups > 0) {  // hxq_kernel takes each row-block program's first row / row block by value
        x.qOpt = pl.qOpt;
        x.qRbs = pl.qRbs;
        x.qGroups = pl.qGroups;
        for (int w = 0; w < p.nw; ++w) { x.qU0[w] = p.hU0[w]; x.qRbw[w] = p.hRbw[w]; }
    }
    return x;
}
}  // namespace

hipError_t launchHxsPlan(const HxsLaunchPlan& pl, const HxsKnobs& k, const HxDev& p, const SrcDesc& src, const OutDesc& od, int C,
                         hipStream_t stream, HistCopy* hc, uint64_t* meter) {
    if (!pcmIsInt(od.pcm)) meter = nullptr;  // only the clamping stores are metered
    if (meter && pl.kernel == HxsKernel::Hxt) return hipErrorNotSupported;  // hxt_kernel stores no PCM (its planner declines od.pcm)
    if (k.trace) {
        char line[512];
        hxsTraceLines(pl, od, C, line, sizeof(line));
        fputs(line, stderr);
    }
    HxsArgs x = hxsArgsOf(pl, p, src, od, C, k);
    if (pl.histFolded) {  // history keep folded into this launch (no gather_kernel after it)
        x.hdst = static_cast<float*>(hc->dst);
        x.ht0 = hc->t0;
        x.hn = hc->n;
        hc->done = true;
    }
    const int64_t blocks = pl.nblocks;
    if (pl.kernel == HxsKernel::Hxt) {
        switch (p.NS) {
#define GAR_HXT_NS(n) case n: return hxtFmt<n>(x, pl.lds, blocks, stream, pl.lean);
#if !GAR_HXS_QUICK
            GAR_HXT_NS(1) GAR_HXT_NS(2) GAR_HXT_NS(3) GAR_HXT_NS(4) GAR_HXT_NS(5) GAR_HXT_NS(6) GAR_HXT_NS(7)
            GAR_HXT_NS(8)
#endif
            GAR_HXT_NS(9) GAR_HXT_NS(10)
#undef GAR_HXT_NS
            default: return hipErrorNotSupported;
        }
    }
    switch (p.NS) {
#define GAR_HXS_NS(n) case n: return hxsVst<n>(x, pl.lds, blocks, stream, k.hxqW, meter);
#if !GAR_HXS_QUICK
        GAR_HXS_NS(1) GAR_HXS_NS(2) GAR_HXS_NS(3) GAR_HXS_NS(4) GAR_HXS_NS(5) GAR_HXS_NS(6) GAR_HXS_NS(7)
        GAR_HXS_NS(8)
#endif
        GAR_HXS_NS(9) GAR_HXS_NS(10)
#undef GAR_HXS_NS
        default: return hipErrorNotSupported;
    }
}

}  // namespace gar
