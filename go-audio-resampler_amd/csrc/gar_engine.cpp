// gar_engine.cpp -- the run path of the host state machine behind the C ABI (gar_abi.cpp).
//
// The reference keeps, per channel, a chain of engine.Resampler stages
// (constant.go:16-85) whose streaming state is history slices plus integer
// counters (dft_stage.go:156-207, polyphase_stage.go:186-312,
// dft_stage.go:488-554).  Here the *counters* are tracked on the host with the
// reference's exact integer arithmetic (gar_counters.cpp) -- so every call returns exactly the
// reference's number of samples -- while the sample histories live in HBM as
// interleaved [t][channel] rows and all sample arithmetic runs in HIP kernels
// (gar_kernels.hip).  Channels in lockstep share one group and one launch.
#include <cstring>

#include "gar_engine.hpp"

namespace gar {

namespace {
thread_local std::string g_err;
thread_local int* g_curErr = nullptr;  // device status word of the handle whose call is running (callOn's ErrScope)
}  // namespace

void setError(std::string msg) { g_err = std::move(msg); }
const char* lastError() { return g_err.c_str(); }

gar_status guard(gar_status s, const char* msg) {
    if (s != GAR_OK) g_err = msg;
    return s;
}

ErrScope::ErrScope(int* e) : prev(g_curErr) { g_curErr = e; }
ErrScope::~ErrScope() { g_curErr = prev; }

namespace {

struct Ctx {
    Handle* h;
    Group* g;
    hipStream_t s;
    bool launch;
};

// A launch bracketed by HIP events on its stream when profiling is on (tag = gar_profile_read kind).
template <class L>
hipError_t timed(Ctx& x, int tag, L&& launch) {
    if (!x.h->profile || !((x.h->profileKinds >> tag) & 1u)) return launch();
    hipEvent_t a, b;
    if (!x.h->evPool.empty()) {  // reuse event pairs (creation is not free)
        a = x.h->evPool.back().first;
        b = x.h->evPool.back().second;
        x.h->evPool.pop_back();
    } else {
        // timing events without the system-scope release: a default event's record writes back the
        // L2 for host visibility, which costs stream time the measured kernel does not own
        HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableSystemFence));
        HIPCHK(hipEventCreateWithFlags(&b, hipEventDisableSystemFence));
    }
    HIPCHK(hipEventRecord(a, x.s));
    const hipError_t e = launch();
    HIPCHK(hipEventRecord(b, x.s));
    x.h->events.push_back({tag, a, b});
    return e;
}

hipError_t timedBg(Ctx& x, int tag, const BgDev& p, const SrcDesc& src, const OutDesc& od, int C,
                   HistCopy* hc = nullptr) {
    // the meter on and an integer PCM view (the fused store of a device call): the launch tallies what it stores
    uint64_t* meter = (x.h->meterOn && pcmIsInt(od.pcm)) ? static_cast<uint64_t*>(x.h->meterBuf.p) : nullptr;
    return timed(x, tag, [&] { return launchBg(p, src, od, C, x.s, hc, meter); });
}

SrcDesc mkSrc(const Hist& hs, int C, int64_t x0, const InView& in) {
    SrcDesc s{};
    s.hist = hs.ptr();
    s.hist_base = hs.base;
    s.hist_len = hs.len;
    s.hist_ld = C;
    s.in = in.zeros ? nullptr : in.p;
    s.in_base = x0;
    s.in_len = in.zeros ? 0 : in.n;
    s.in_fs = in.fs;
    s.in_cs = in.cs;
    s.in_f64 = in.f64;
    s.in_pcm = in.zeros ? 0 : in.pcm;
    s.valid_end = in.zeros ? x0 : x0 + in.n;
    return s;
}

OutDesc mkOut(const OutView& o, int64_t o0, int64_t n) {
    OutDesc d{};
    d.err = g_curErr;
    d.out = o.p;
    d.o0 = o0;
    d.fs = o.fs;
    d.cs = o.cs;
    d.f64 = o.f64;
    d.pcm = o.pcm;
    d.o_lo = o0;
    d.o_hi = o0 + n;
    d.dither = o.dz.mode;
    d.dseedLo = o.dz.seedLo;
    d.dseedHi = o.dz.seedHi;
    d.dpos0 = o.dz.pos0;
    return d;
}

void hist_update(Ctx& x, Hist& hs, const SrcDesc& src, int64_t k0, int64_t k1) {
    const int C = x.g->C;
    if (k1 < k0) k1 = k0;
    if (!x.launch) { hs.base = k0; hs.len = k1 - k0; hs.zero = false; return; }
    const int other = 1 - hs.cur;
    hs.buf[other].ensure(static_cast<size_t>(std::max<int64_t>(k1 - k0, 1)) * C * x.h->tc());
    HIPCHK(launchGather(x.h->f64, src, hs.buf[other].p, k0, k1 - k0, C, x.s));
    hs.cur = other;
    hs.base = k0;
    hs.len = k1 - k0;
    hs.zero = false;
}

// A FIR launch `l(HistCopy*)` (when `launch`) with the history keep hs <- src[k0, k1) folded into it
// when the kernel takes it (hxs_kernel, bg_kernel); otherwise the keep is a gather launch after it.
template <class L>
void withHist(Ctx& x, Hist& hs, const SrcDesc& src, int64_t k0, int64_t k1, bool launch, L&& l) {
    HistCopy hc;
    const int other = 1 - hs.cur;
    if (x.launch && launch && k1 > k0) {
        hs.buf[other].ensure(static_cast<size_t>(k1 - k0) * x.g->C * x.h->tc());
        hc.dst = hs.buf[other].p;
        hc.t0 = k0;
        hc.n = k1 - k0;
    }
    if (x.launch && launch) HIPCHK(l(&hc));
    if (hc.done) {
        hs.cur = other;
        hs.base = k0;
        hs.len = k1 - k0;
        hs.zero = false;
    } else {
        hist_update(x, hs, src, k0, k1);
    }
}

// FUSED -> STAGED: rebuild the poly-stream history u[u_base, u_count) from x by
// the DFT plan and keep the DFT's own history x[x_count - dft_hist, x_count).
void materialize(Ctx& x, StageRT& rt, Counters& c, StageDev& dv, const SrcDesc& xsrc) {
    const int C = x.g->C;
    if (x.launch) {
        Hist& uh = dv.uh;
        const int other = 1 - uh.cur;
        const int64_t n = c.u_count - c.u_base;
        uh.buf[other].ensure(static_cast<size_t>(std::max<int64_t>(n, 1)) * C * rt.tc());
        const OutView ov = OutView::rows(uh.buf[other].p, C, rt.cf());
        HIPCHK(timedBg(x, 1, rt.dftD, xsrc, mkOut(ov, c.u_base, n), C));
        uh.cur = other;
        uh.base = c.u_base;
        uh.len = n;
    } else {
        dv.uh.base = c.u_base;
        dv.uh.len = c.u_count - c.u_base;
    }
    hist_update(x, dv.xh, xsrc, c.x_count - c.dft_hist, c.x_count);
    c.staged = true;
}

// The staged polyphase launch: nout outputs from y0 of the poly stream `usrc`, from the position the
// counters `before` the call hold.
void polyLaunch(Ctx& x, const StageRT& rt, const Counters& before, const SrcDesc& usrc, const OutView& out, int64_t y0,
                int64_t nout) {
    if (!x.launch || nout <= 0) return;
    PolyDev p = rt.polyD;
    p.at0 = before.at;
    p.u_base = before.u_base;
    p.m0 = before.y_count;
    HIPCHK(timed(x, 4, [&] { return launchPoly(p, usrc, mkOut(out, y0, nout), nout, x.g->C, x.s); }));
}

// engine.Resampler.ProcessZeroCopy for one stage (resampler.go:232-272).
int64_t stageProcess(Ctx& x, int si, const InView& in, const OutView& out) {
    StageRT& rt = *x.h->stages[si];
    Counters& c = x.g->cnt[si];
    StageDev& dv = x.g->dev[si];
    const int C = x.g->C;
    const EngineDesign& d = rt.d;
    const int64_t n = in.n;
    if (n == 0) return 0;
    switch (d.kind) {
        case EngineKind::Cubic: {
            // CubicStage.Process (cubic.go:33-64); Flush emits nothing (cubic.go:93-96)
            const int64_t x0 = c.x_count;
            std::vector<CubicSeg>* segs = x.launch ? &x.g->cubSegs : nullptr;
            if (segs) segs->clear();
            const SrcDesc src = mkSrc(dv.xh, C, x0, in);
            const int64_t y0 = c.y_count;
            // short calls (streaming chunks): short segments, so each GPU thread re-walks only a few
            // inputs from registers (a 4096-frame call would otherwise be 16 serial 256-input walks)
            int segLen = n * C <= (int64_t(1) << 20) ? kCubicSegInputsShort : static_cast<int>(kCubicSegInputs);
            const int64_t nout = cntCubic(c, d.ratio, n, segs, &segLen);
            if (x.launch && nout > 0) {
                PinBuf& pb = x.g->cubPin[x.g->cubCur];
                x.g->cubCur ^= 1;
                void* hp = pb.acquire(segs->size() * sizeof(CubicSeg));
                std::memcpy(hp, segs->data(), segs->size() * sizeof(CubicSeg));
                HIPCHK(timed(x, 5, [&] {
                    return launchCubic(rt.cf(), static_cast<const CubicSeg*>(hp), static_cast<int64_t>(segs->size()),
                                       c.x_count, 1.0 / d.ratio, src, mkOut(out, y0, nout), C, x.s, segLen);
                }));
                pb.issued(x.s);
            }
            hist_update(x, dv.xh, src, std::max<int64_t>(0, c.x_count - 3), c.x_count);
            c.y_count += nout;
            return nout;
        }
        case EngineKind::Passthrough: {
            if (x.launch && !in.zeros) {
                HIPCHK(launchCopy(in.p, in.f64, in.fs, in.cs, out.p, out.f64, out.fs, out.cs, n, C, x.s));
            }
            c.y_count += n;
            return n;
        }
        case EngineKind::DftOnly: {
            const int64_t x0 = c.x_count;
            const int64_t y0 = c.y_count;
            const int64_t nout = cntDft(c, d.dft, n);
            const SrcDesc src = mkSrc(dv.xh, C, x0, in);
            withHist(x, dv.xh, src, c.x_count - c.dft_hist, c.x_count, nout > 0,
                     [&](HistCopy* hc) { return timedBg(x, 1, rt.dftD, src, mkOut(out, y0, nout), C, hc); });
            c.y_count += nout;
            return nout;
        }
        case EngineKind::Decim: {
            const int64_t x0 = c.x_count;
            const int64_t y0 = c.y_count;
            const int64_t nout = cntDecim(c, d.decim, n);
            const SrcDesc src = mkSrc(dv.xh, C, x0, in);
            withHist(x, dv.xh, src, c.x_count - c.dec_hist, c.x_count, nout > 0,
                     [&](HistCopy* hc) { return timedBg(x, 2, rt.decimD, src, mkOut(out, y0, nout), C, hc); });
            c.y_count += nout;
            return nout;
        }
        case EngineKind::DftPoly: {
            const int64_t x0 = c.x_count;
            const int64_t y0 = c.y_count;
            const Counters before = c;
            const SrcDesc xsrc = mkSrc(dv.xh, C, x0, in);
            const int64_t nu = cntDft(c, d.dft, n);
            bool quirk = false;
            const int64_t nout = cntPoly(c, d.poly, nu, quirk);
            if (!c.staged) {
                // Fused: DFT x2 and polyphase composed into one MFMA FIR over x; the history keep
                // x[u_base/2, x_count) rides along in the same launch when the kernel takes it.
                if (quirk) {
                    if (x.launch && nout > 0) HIPCHK(timedBg(x, 0, rt.fusedD, xsrc, mkOut(out, y0, nout), C));
                    materialize(x, rt, c, dv, xsrc);
                } else {
                    withHist(x, dv.xh, xsrc, c.u_base / 2, c.x_count, nout > 0, [&](HistCopy* hc) {
                        return timedBg(x, 0, rt.fusedD, xsrc, mkOut(out, y0, nout), C, hc);
                    });
                }
            } else {
                // Staged: DFT (MFMA FIR) into u scratch, polyphase with live cubic interpolation.
                const int64_t p0 = before.x_count - before.dft_hist;   // DFT positions done before
                const int64_t dy0 = p0 * d.dft.factor;
                if (x.launch) x.g->utmp.ensure(static_cast<size_t>(std::max<int64_t>(nu, 1)) * C * rt.tc());
                const OutView uv = OutView::rows(x.g->utmp.p, C, rt.cf());
                // the x history keep depends on x only: it rides in the DFT launch
                withHist(x, dv.xh, xsrc, c.x_count - c.dft_hist, c.x_count, nu > 0,
                         [&](HistCopy* hc) { return timedBg(x, 1, rt.dftD, xsrc, mkOut(uv, dy0, nu), C, hc); });
                const SrcDesc usrc = mkSrc(dv.uh, C, before.u_count, InView::of(uv, nu));
                polyLaunch(x, rt, before, usrc, out, y0, nout);
                if (nu > 0) hist_update(x, dv.uh, usrc, c.u_base, c.u_count);
            }
            c.y_count += nout;
            return nout;
        }
        default:
            throw DevError{hipErrorNotSupported, "unsupported stage"};
    }
}

// The view `rows` frames further on; the dither position travels with the base.
OutView offsetView(const OutView& o, int64_t rows) {
    OutView r = o;
    if (o.p) r.p = static_cast<char*>(o.p) + rows * o.fs * (o.pcm ? pcmBytes(o.pcm) : (o.f64 ? 8 : 4));
    r.dz.pos0 += rows;
    return r;
}

// engine.Resampler.Flush for one stage (resampler.go:275-322).
int64_t stageFlush(Ctx& x, int si, const OutView& out) {
    StageRT& rt = *x.h->stages[si];
    Counters& c = x.g->cnt[si];
    StageDev& dv = x.g->dev[si];
    const int C = x.g->C;
    const EngineDesign& d = rt.d;
    InView z;
    z.zeros = true;
    switch (d.kind) {
        case EngineKind::Passthrough:
            return 0;
        case EngineKind::DftOnly:
            if (c.dft_hist == 0) return 0;
            z.n = d.dft.taps;
            return stageProcess(x, si, z, out);
        case EngineKind::Decim:
            if (c.dec_hist == 0) return 0;
            z.n = d.decim.taps;
            return stageProcess(x, si, z, out);
        case EngineKind::DftPoly: {
            if (!c.staged) {
                InView none;
                none.zeros = true;
                const SrcDesc xsrc = mkSrc(dv.xh, C, c.x_count, none);
                // Fused flush: DFTStage.Flush + PolyphaseStage.Process + PolyphaseStage.Flush
                // counted exactly, all samples by one composite launch over x zero-extended
                // (the zero pads of both flushes are zero samples of the same composite FIR).
                Counters t = c;
                bool quirk = false;
                int64_t nA = 0, nB = 0;
                if (t.dft_hist > 0) nA = cntPoly(t, d.poly, cntDft(t, d.dft, d.dft.taps), quirk);
                if (t.poly_hist > 0) nB = cntPoly(t, d.poly, d.poly.taps, quirk);
                if (!quirk) {
                    const int64_t y0 = c.y_count, n = nA + nB;
                    if (x.launch && n > 0) HIPCHK(timedBg(x, 3, rt.fusedD, xsrc, mkOut(out, y0, n), C));
                    c = t;
                    c.y_count = y0 + n;
                    c.staged = true;
                    // both delay lines now hold only flush zeros (their last T-1 pad samples)
                    dv.xh.base = c.x_count - c.dft_hist;
                    dv.xh.len = c.dft_hist;
                    dv.xh.zero = true;
                    dv.uh.base = c.u_base;
                    dv.uh.len = c.u_count - c.u_base;
                    dv.uh.zero = true;
                    return n;
                }
                materialize(x, rt, c, dv, xsrc);
            }
            int64_t total = 0;
            // DFTStage.Flush -> PolyphaseStage.Process(intermediate)
            if (c.dft_hist > 0) {
                z.n = d.dft.taps;
                total += stageProcess(x, si, z, out);
            }
            // PolyphaseStage.Flush: tapsPerPhase zeros into the poly stream
            if (c.poly_hist > 0) {
                const int64_t y0 = c.y_count;
                const Counters before = c;
                bool quirk = false;
                const int64_t nout = cntPoly(c, d.poly, d.poly.taps, quirk);
                InView uz;
                uz.zeros = true;
                uz.n = d.poly.taps;
                const SrcDesc usrc = mkSrc(dv.uh, C, before.u_count, uz);
                const OutView o2 = offsetView(out, total);
                polyLaunch(x, rt, before, usrc, o2, y0, nout);
                hist_update(x, dv.uh, usrc, c.u_base, c.u_count);
                c.y_count += nout;
                total += nout;
            }
            return total;
        }
        default:
            return 0;
    }
}

// Where stage i of the chain writes: the caller's output for the last stage, else (when launching) the
// group's scratch of that stage boundary, sized by the counts of the dry run before (scratchSizes).
OutView stageOut(Ctx& x, int i, const OutView& out) {
    if (i == static_cast<int>(x.h->stages.size()) - 1 || !x.launch) return out;
    x.g->tmp[i].ensure(static_cast<size_t>(std::max<int64_t>(x.h->scratchSizes[i], 1)) * x.g->C * x.h->tc());
    return OutView::rows(x.g->tmp[i].p, x.g->C, x.h->cf());
}

// constantRateResampler.processChannel[Into] (constant.go:255-345): the whole
// chain; sizes[i] = samples produced by stage i (buffer i+1).
int64_t chainProcess(Ctx& x, const InView& in, const OutView& out, std::vector<int64_t>& sizes) {
    const int ns = static_cast<int>(x.h->stages.size());
    sizes.assign(ns, 0);
    if (ns == 0) {  // ratio within 0.1% of 1: no stages, the ring buffer passes input through
        if (x.launch && in.n > 0)
            HIPCHK(launchCopy(in.p, in.f64, in.fs, in.cs, out.p, out.f64, out.fs, out.cs, in.n, x.g->C, x.s));
        return in.n;
    }
    InView cur = in;
    for (int i = 0; i < ns; ++i) {
        const OutView o = stageOut(x, i, out);
        int64_t m = 0;
        if (cur.n >= 1) m = stageProcess(x, i, cur, o);  // Available() >= GetMinInput() (constant.go:277,314)
        sizes[i] = m;
        cur = InView::of(o, m);
    }
    return cur.n;
}

// flushChannel (constant.go:360-386)
int64_t chainFlush(Ctx& x, const OutView& out, std::vector<int64_t>& sizes) {
    const int ns = static_cast<int>(x.h->stages.size());
    sizes.assign(ns, 0);
    if (ns == 0) return 0;
    InView pending;  // previous stage's flushed tail
    for (int i = 0; i < ns; ++i) {
        const OutView o = stageOut(x, i, out);
        int64_t m = 0;
        if (pending.n > 0) m += stageProcess(x, i, pending, o);
        m += stageFlush(x, i, offsetView(o, m));
        sizes[i] = m;
        pending = InView::of(o, m);
    }
    return pending.n;
}

// Copy channels [k0, k0+kc) of group g into a new group (Process on channel 0
// of a multi-channel handle advances only that channel, constant.go:88-95).
Group splitCopy(Handle* h, Group& g, int k0, int kc) {
    Group ng = freshGroup(h, g.c0 + k0, kc);
    const int tc = h->tc();
    for (size_t i = 0; i < h->stages.size(); ++i) {
        ng.cnt[i] = g.cnt[i];
        ng.statIn = g.statIn;
        ng.statOut = g.statOut;
        Hist* src[2] = {&g.dev[i].xh, &g.dev[i].uh};
        Hist* dst[2] = {&ng.dev[i].xh, &ng.dev[i].uh};
        for (int k = 0; k < 2; ++k) {
            dst[k]->base = src[k]->base;
            dst[k]->len = src[k]->len;
            dst[k]->zero = src[k]->zero;
            if (!h->dry && src[k]->len > 0 && !src[k]->zero) {
                dst[k]->buf[0].ensure(static_cast<size_t>(src[k]->len) * kc * tc);
                const char* sp = static_cast<const char*>(src[k]->ptr()) + static_cast<size_t>(k0) * tc;
                HIPCHK(launchCopy(sp, h->f64, g.C, 1, dst[k]->buf[0].p, h->f64, kc, 1, src[k]->len, kc, h->stream));
            }
        }
    }
    return ng;
}

// GetStatistics bookkeeping of one successful call (resampler.go:182-322): Process counts its
// input only when non-empty (the early return of an empty call counts nothing); the cubic
// engine's Flush returns CubicStage.Flush directly, uncounted (resampler.go:276-279).
void countStats(const Handle* h, Group& g, int64_t nIn, int64_t nOut, bool flush) {
    if (!flush) {
        if (nIn <= 0) return;
        g.statIn += nIn;
        g.statOut += nOut;
        return;
    }
    const bool cubicEngine = !h->newPath && h->stages.size() == 1 && h->stages[0]->d.kind == EngineKind::Cubic;
    if (!cubicEngine) g.statOut += nOut;
}

}  // namespace

Group* groupOf(Handle* h, int ch) {
    for (auto& g : h->groups)
        if (ch >= g.c0 && ch < g.c0 + g.C) return &g;
    return nullptr;
}

void freshCounters(const Handle* h, Group& g) {
    g.cnt.assign(h->stages.size(), Counters());
    for (size_t i = 0; i < g.cnt.size(); ++i) g.cnt[i].staged = !h->stages[i]->fused;
}

Group freshGroup(Handle* h, int c0, int C) {
    Group g;
    g.c0 = c0;
    g.C = C;
    freshCounters(h, g);
    g.dev.resize(h->stages.size());
    g.tmp.resize(h->stages.size());
    return g;
}

void isolate(Handle* h, int ch) {
    Group* g = groupOf(h, ch);
    if (!g || g->C == 1) return;
    std::vector<Group> out;
    for (auto& gg : h->groups) {
        if (&gg != g) { out.push_back(std::move(gg)); continue; }
        const int k = ch - gg.c0;
        if (k > 0) out.push_back(splitCopy(h, gg, 0, k));
        out.push_back(splitCopy(h, gg, k, 1));
        if (k + 1 < gg.C) out.push_back(splitCopy(h, gg, k + 1, gg.C - k - 1));
    }
    if (!h->dry) HIPCHK(hipStreamSynchronize(h->stream));
    h->groups = std::move(out);
}

int64_t simulate(Handle* h, Group& g, int64_t n, bool flush, std::vector<int64_t>& sizes) {
    Group sim;
    sim.c0 = g.c0;
    sim.C = g.C;
    sim.cnt = g.cnt;
    sim.dev.resize(g.dev.size());
    for (size_t i = 0; i < g.dev.size(); ++i) {
        sim.dev[i].xh.base = g.dev[i].xh.base; sim.dev[i].xh.len = g.dev[i].xh.len;
        sim.dev[i].uh.base = g.dev[i].uh.base; sim.dev[i].uh.len = g.dev[i].uh.len;
    }
    Ctx x{h, &sim, nullptr, false};
    InView in;
    in.n = n;
    OutView o;
    return flush ? chainFlush(x, o, sizes) : chainProcess(x, in, o, sizes);
}

bool fusedFlushQuirk(const Handle* h, const Group& g) {
    if (h->stages.size() != 1 || g.cnt.empty() || g.cnt[0].staged) return false;
    const EngineDesign& d = h->stages[0]->d;
    if (d.kind != EngineKind::DftPoly) return false;
    Counters t = g.cnt[0];  // stageFlush's count of the fused flush
    bool quirk = false;
    if (t.dft_hist > 0) cntPoly(t, d.poly, cntDft(t, d.dft, d.dft.taps), quirk);
    if (t.poly_hist > 0) cntPoly(t, d.poly, d.poly.taps, quirk);
    return quirk;
}

int64_t runGroup(Handle* h, Group& g, const InView& in, const OutView& out, bool flush, hipStream_t s,
                 int64_t cap, gar_status& st) {
    std::vector<int64_t> sizes;
    const int64_t n = simulate(h, g, in.n, flush, sizes);
    if (n > cap) { st = GAR_ERR_BUFFER_TOO_SMALL; return n; }
    st = GAR_OK;
    if (h->dry) {
        Ctx x{h, &g, nullptr, false};
        std::vector<int64_t> s2;
        OutView o;
        if (flush) chainFlush(x, o, s2); else chainProcess(x, in, o, s2);
        countStats(h, g, in.n, n, flush);
        return n;
    }
    h->scratchSizes = sizes;
    Ctx x{h, &g, s, true};
    std::vector<int64_t> s2;
    const int64_t got = flush ? chainFlush(x, out, s2) : chainProcess(x, in, out, s2);
    if (got != n) { st = GAR_ERR_INTERNAL; g_err = "size mismatch between count and launch"; }
    else countStats(h, g, in.n, got, flush);
    return got;
}

gar_status caught(bool* launchLimit) {
    try {
        throw;
    } catch (const DevError& e) {
        if (e.e == hipErrorInvalidConfiguration && !launchLimitMsg().empty()) {  // a launch the device cannot run
            g_err = launchLimitMsg() + " (at " + e.what + ")";
            launchLimitMsg().clear();
            if (launchLimit) *launchLimit = true;
            return GAR_ERR_INVALID_ARGUMENT;
        }
        g_err = std::string("HIP error ") + hipGetErrorString(e.e) + " at " + e.what;
        return GAR_ERR_DEVICE;
    } catch (const std::bad_alloc&) {
        g_err = "out of host memory";
        return GAR_ERR_INTERNAL;
    }
}

bool devFault(Handle* h) {
    if (!h->errHost) return false;
    const int v = __atomic_load_n(h->errHost, __ATOMIC_ACQUIRE);
    if (!v) return false;
    h->poisoned = true;
    const char* what = v == kHxtErrLoadWait   ? "hxt_kernel: a compute wave's LDS load-progress wait expired"
                       : v == kHxtErrSlotWait ? "hxt_kernel: a loader's LDS ring-slot wait expired"
                                              : "unknown code";
    g_err = std::string("device error reported by ") + what + " (code " + std::to_string(v) +
            "); outputs of the launch are invalid; call Reset";
    return true;
}

void drainOrder(Handle* h) {
    if (h->orderValid) (void)hipEventSynchronize(h->orderEv);
    else if (h->unordered) (void)hipDeviceSynchronize();
    h->unordered = false;
}

void waitEnqueued(Handle* h) {
    if (h->orderValid) HIPCHK(hipEventSynchronize(h->orderEv));
    else if (h->unordered) HIPCHK(hipDeviceSynchronize());
    h->unordered = false;
    if (h->stream) HIPCHK(hipStreamSynchronize(h->stream));
}

}  // namespace gar
