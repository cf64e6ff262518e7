// gar_stage.cpp -- stage construction: the MFMA FIR plans and polyphase banks of one engine design,
// built on the host and uploaded (StageRT); nothing here runs per call.
#include <cstring>

#include "gar_engine.hpp"

namespace gar {
namespace {

// The exact rows of a plan as the device sees them: [rows (f64) | off | len | ph | par] in X; the two
// stages' banks of a composite are uploaded once per stage (xBankA / xBankC) and shared by its plans.
// A dry-run handle uploads nothing and gets the host-side scalars.
ExactDev uploadExact(const ExactRows& x, StageRT& s, DevBuf& X, bool dry) {
    ExactDev d{};
    d.rowMax = x.rowMax;
    d.twoStage = x.twoStage ? 1 : 0;
    d.T1 = s.d.dft.taps;
    d.T2 = s.d.poly.taps;
    if (dry) return d;
    const size_t nr = x.rows.size(), Pc = x.off.size();
    std::vector<int> info = x.off;
    for (const std::vector<int>* v : {&x.len, &x.ph, &x.par}) info.insert(info.end(), v->begin(), v->end());
    X.ensure(nr * 8 + info.size() * 4);
    HIPCHK(hipMemcpy(X.p, x.rows.data(), nr * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(static_cast<char*>(X.p) + nr * 8, info.data(), info.size() * 4, hipMemcpyHostToDevice));
    d.rows = static_cast<const double*>(X.p);
    d.rowOff = reinterpret_cast<const int*>(d.rows + nr);
    d.rowLen = d.rowOff + Pc;
    d.rowPh = d.rowOff + 2 * Pc;
    d.rowPar = d.rowOff + 3 * Pc;
    if (x.twoStage) {
        if (!s.xBankA.p) s.xBankA.upload(s.d.poly.a);
        if (!s.xBankC.p) s.xBankC.upload(s.d.dft.c);
        d.polyA = static_cast<const double*>(s.xBankA.p);
        d.dftC = static_cast<const double*>(s.xBankC.p);
    }
    return d;
}

// Builds + uploads the split-f16 plan of `f` and points bg.hx at it.
bool attachHx(const FirPeriodic& f, StageRT::HxRT& h, BgDev& bg, bool dry, StageRT& s) {
    if (!buildHxPlan(f, h.plan)) return false;
    HxDev& d = h.d;
    const HxPlan& p = h.plan;
    // two double-buffered hi/lo images of one macro period + one partial-slot buffer must fit LDS;
    // longer filters (e.g. the 1223-tap decimator) stay on the exact-f32 kernel
    const size_t ws1 = (static_cast<size_t>(p.Kread) + 63) / 64 * 64;
    if (ws1 > static_cast<size_t>(kHxMaxRows)) return false;
    if (hxLdsBytes(static_cast<int>(ws1), p.nslots, 0) > 160 * 1024) return false;
    d = HxDev{};
    d.Pc = p.Pc; d.Qc = p.Qc; d.Kc = p.Kc; d.Kread = p.Kread; d.NS = p.NS; d.nrb = p.nrb;
    d.nw = p.nw; d.kch = p.kch; d.nred = static_cast<int>(p.reds.size()); d.nslots = p.nslots;
    d.ea = p.ea; d.rb = p.rbMode ? 1 : 0;
    d.ex = uploadExact(p.ex, s, h.X, dry);
    if (p.rbMode && p.nw <= 16) {  // hxq_kernel takes them by value
        const std::vector<int> pt = p.progTable();
        for (int w = 0; w < p.nw; ++w) { d.hU0[w] = pt[kBgProgInts * w + 4]; d.hRbw[w] = pt[kBgProgInts * w + 3]; }
    }
    if (!dry) {
        h.A.upload(p.A);
        std::vector<int> t = p.progTable();
        const std::vector<int> rt = p.redTable();
        const size_t redOff = t.size();
        t.insert(t.end(), rt.begin(), rt.end());
        h.T.upload(t);
        d.A = h.A.p;
        d.progs = static_cast<const int*>(h.T.p);
        d.reds = static_cast<const int*>(h.T.p) + redOff;
        d.fixCap = 1 << 16;
        h.fix.upload(std::vector<int>(1 + d.fixCap, 0));
        d.fix = static_cast<int*>(h.fix.p);
    }
    d.hxsOk = hxsPlanFits(d) ? 1 : 0;  // PCM / half stores and loads fuse only into hxs_kernel (pcmFusable)
    bg.hx = &h.d;
    return true;
}

BgDev uploadPlan(const BgPlan& p, DevBuf& A, DevBuf& T, bool dry) {
    BgDev d{};
    d.f64 = p.f64 ? 1 : 0;
    d.Pc = p.Pc; d.Qc = p.Qc; d.Kc = p.Kc; d.Kread = p.Kread; d.NS = p.NS; d.nrb = p.nrb;
    d.nprog = static_cast<int>(p.progs.size());
    d.kch = p.kch;
    d.nw = p.nw;
    d.ncg = p.ncg;
    d.nred = static_cast<int>(p.reds.size());
    d.nslots = p.nslots;
    d.rbAligned = p.rbAligned ? 1 : 0;
    d.hRbStart = p.rbAligned ? p.rbStart.data() : nullptr;  // the plan lives as long as the stage
    d.hRbK0 = p.rbAligned ? p.rbK0.data() : nullptr;
    for (size_t rb = 0; p.rbAligned && rb + 1 < p.rbStart.size(); ++rb)
        d.maxPrb = std::max(d.maxPrb, p.rbStart[rb + 1] - p.rbStart[rb]);
    if (dry) return d;
    if (p.f64) A.upload(p.A64); else A.upload(p.A32);
    std::vector<int> t = p.progTable();
    const std::vector<int> rt = p.redTable();
    const size_t redOff = t.size();
    t.insert(t.end(), rt.begin(), rt.end());
    const size_t rbOff = t.size();
    t.insert(t.end(), p.rbStart.begin(), p.rbStart.end());
    T.upload(t);
    d.A = A.p;
    d.progs = static_cast<const int*>(T.p);
    d.reds = static_cast<const int*>(T.p) + redOff;
    d.rbStart = p.rbAligned ? static_cast<const int*>(T.p) + rbOff : nullptr;
    return d;
}

// A bg plan's exact rows and bg_kernel's non-finite fix list (kBgNfInts ints, zeroed).
void attachExact(const BgPlan& p, StageRT::BgX& x, StageRT& s, BgDev& d, bool dry) {
    d.ex = uploadExact(p.ex, s, x.rows, dry);
    if (dry) return;
    x.nfList.ensure(kBgNfListBytes);
    HIPCHK(hipMemset(x.nfList.p, 0, kBgNfListBytes));
    d.nfList = static_cast<int*>(x.nfList.p);
}

template <class T>
void uploadBank(const std::vector<double>& v, DevBuf& b) {
    std::vector<T> c(v.begin(), v.end());
    b.upload(c);
}

}  // namespace

bool buildStage(StageRT& s, bool f64, bool hx, bool dry, std::string& err) {
    s.f64 = f64;
    hx = hx && !f64;
    const EngineDesign& d = s.d;
    if (d.kind == EngineKind::Cubic) return true;  // no filter banks (cubic.go:75-90)
    if (d.kind == EngineKind::DftOnly || d.kind == EngineKind::DftPoly) {
        if (!buildBgPlan(firFromDft(d.dft), f64, s.dftP)) { err = "DFT plan"; return false; }
        s.dftD = uploadPlan(s.dftP, s.dftA, s.dftT, dry);
        attachExact(s.dftP, s.dftX, s, s.dftD, dry);
        if (hx) attachHx(firFromDft(d.dft), s.dftH, s.dftD, dry, s);
    }
    if (d.kind == EngineKind::Decim) {
        if (!buildBgPlan(firFromDecim(d.decim), f64, s.decimP)) { err = "decimator plan"; return false; }
        s.decimD = uploadPlan(s.decimP, s.decimA, s.decimT, dry);
        attachExact(s.decimP, s.decimX, s, s.decimD, dry);
        if (hx) attachHx(firFromDecim(d.decim), s.decimH, s.decimD, dry, s);
    }
    if (d.kind == EngineKind::DftPoly) {
        if (firComposite(d.dft, d.poly, s.compositeFir) && buildBgPlan(s.compositeFir, f64, s.fusedP)) {
            s.fused = true;
            s.fusedD = uploadPlan(s.fusedP, s.fusedA, s.fusedT, dry);
            attachExact(s.fusedP, s.fusedX, s, s.fusedD, dry);
            if (hx) attachHx(s.compositeFir, s.fusedH, s.fusedD, dry, s);
        }
        PolyDev& p = s.polyD;
        p.f64 = s.cf();
        p.L = d.poly.L;
        p.T = d.poly.taps;
        p.step = d.poly.step;
        if (!dry) {
            if (f64) {
                uploadBank<double>(d.poly.a, s.pa); uploadBank<double>(d.poly.b, s.pb);
                uploadBank<double>(d.poly.cc, s.pc); uploadBank<double>(d.poly.d, s.pd);
            } else {
                uploadBank<float>(d.poly.a, s.pa); uploadBank<float>(d.poly.b, s.pb);
                uploadBank<float>(d.poly.cc, s.pc); uploadBank<float>(d.poly.d, s.pd);
            }
            p.a = s.pa.p; p.b = s.pb.p; p.c = s.pc.p; p.d = s.pd.p;
            std::vector<double> il(4 * d.poly.a.size());
            for (size_t i = 0; i < d.poly.a.size(); ++i) {
                il[4 * i] = d.poly.a[i]; il[4 * i + 1] = d.poly.b[i]; il[4 * i + 2] = d.poly.cc[i]; il[4 * i + 3] = d.poly.d[i];
            }
            if (f64) uploadBank<double>(il, s.pabcd); else uploadBank<float>(il, s.pabcd);
            p.abcd = s.pabcd.p;
        }
    }
    return true;
}

void fillGeometry(const EngineDesign& d, gar_engine_geometry* geom) {
    std::memset(geom, 0, sizeof(*geom));
    geom->kind = static_cast<int32_t>(d.kind);
    geom->dft_factor = d.dft.factor;
    geom->dft_taps = d.dft.taps;
    geom->poly_phases = d.poly.L;
    geom->poly_taps = d.poly.taps;
    geom->poly_step = d.poly.step;
    geom->decim_factor = d.decim.factor;
    geom->decim_taps = d.decim.taps;
    FirPeriodic f;
    bool have = false;
    if (d.kind == EngineKind::DftPoly && firComposite(d.dft, d.poly, f)) { geom->fused = 1; have = true; }
    else if (d.kind == EngineKind::DftOnly) { f = firFromDft(d.dft); have = true; }
    else if (d.kind == EngineKind::Decim) { f = firFromDecim(d.decim); have = true; }
    if (have) {
        geom->fir_period_out = f.P;
        geom->fir_period_in = f.Q;
        for (const auto& row : f.rows) geom->fir_taps_max = std::max<int32_t>(geom->fir_taps_max, static_cast<int32_t>(row.size()));
        BgPlan p;
        if (buildBgPlan(f, false, p)) {
            geom->useful_macs_per_output = p.usefulMacsPerOutput;
            geom->mfma_macs_per_output = p.mfmaMacsPerOutput;
        }
    }
}

}  // namespace gar
