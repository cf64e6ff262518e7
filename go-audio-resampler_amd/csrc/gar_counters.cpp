// gar_counters.cpp -- per-stage streaming counters (exact reference integer semantics).  Host only:
// nothing of HIP is included, so the arithmetic compiles and is checked on its own.
#include "gar_counters.hpp"

#include <cmath>

namespace gar {

int stageLatency(const EngineDesign& d) {
    if (d.kind == EngineKind::Cubic) return 2;  // cubicLatencySamples (internal/engine/constants.go:12)
    int lat = 0;
    if ((d.kind == EngineKind::DftOnly || d.kind == EngineKind::DftPoly) && d.dft.factor > 1)
        lat += (d.dft.taps * d.dft.factor) / 2;
    if (d.kind == EngineKind::DftPoly) lat += d.poly.taps / 2;
    return lat;
}

int64_t cntDft(Counters& s, const DftBank& b, int64_t n) {
    if (b.factor == 1) return n;
    if (n == 0) return 0;
    s.x_count += n;
    s.dft_hist += n;
    if (s.dft_hist < b.taps) return 0;
    const int64_t p = s.dft_hist - b.taps + 1;
    s.dft_hist -= p;
    return p * b.factor;
}

int64_t cntPoly(Counters& s, const PolyBank& b, int64_t m, bool& quirk) {
    if (m == 0) return 0;
    s.poly_hist += m;
    s.u_count += m;
    const int64_t numIn = s.poly_hist - b.taps + 1;
    if (numIn <= 0) return 0;
    const int64_t L = b.L;
    const int64_t limit = (numIn * L) << 16;
    const int64_t nout = (limit - s.at + b.step - 1) / b.step;
    if (nout <= 0) return 0;
    const int64_t at = s.at + nout * b.step;
    const int64_t consumed = (at >> 16) / L;
    if (consumed > 0 && consumed <= s.poly_hist) {
        s.poly_hist -= consumed;
        s.u_base += consumed;
    } else if (consumed > s.poly_hist) {
        quirk = true;  // history left untrimmed, `at` still rebased (polyphase_stage.go:300-307)
    }
    s.at = at - ((consumed * L) << 16);
    return nout;
}

int64_t cntDecim(Counters& s, const DecimBank& b, int64_t n) {
    if (b.factor == 1) return n;
    if (n == 0) return 0;
    s.x_count += n;
    s.dec_hist += n;
    if (s.dec_hist < b.taps) return 0;
    const int64_t nf = s.dec_hist - b.taps + 1;
    const int64_t nout = s.dec_phase < nf ? (nf - s.dec_phase + b.factor - 1) / b.factor : 0;
    if (nout == 0) return 0;  // early return leaves history and phase untouched (dft_stage.go:516-518)
    s.dec_phase = static_cast<int>(((s.dec_phase - nf) % b.factor + b.factor) % b.factor);
    s.dec_hist -= nf;
    return nout;
}

// Exact closed form of the CubicStage phase walk.  In units of 2^-F (F = 53 - exponent of step,
// so step = S units exactly) every value the walk forms -- ph, ph + k*step < 1, the first sum >= 1,
// that sum minus 1 -- is an integer.  When S, the start phase P0 and 2^F are all multiples of the
// rounding grid of the largest binade a sum reaches (sums < 1 + step), no float64 addition of the
// walk rounds (the "- 1" never does: Sterbenz), so the walk is the exact rotation
//     P_{i+1} = P_i + n_i*S - 2^F in [0, S)   =>   P_i = (P0 - i*2^F) mod S,
//     outputs before input i: N_i = (i*2^F + P_i - P0) / S,
// the same phases and counts as the sequential loop, in O(1) per checkpoint (e.g. 44.1k->48k:
// S even, grid 2 units).  Ratios whose step has a low set bit on a coarser grid (48k->44.1k) walk.
namespace {
struct CubicRot {
    int F = 0;
    int64_t S = 0, P0 = 0;
};
bool cubicRotation(double step, double ph, CubicRot& r) {
    int e = 0;
    (void)std::frexp(step, &e);  // step = m * 2^e, m in [0.5, 1)
    r.F = 53 - e;
    if (r.F < 1 || r.F > 60) return false;
    const double Sd = std::ldexp(step, r.F), Pd = std::ldexp(ph, r.F);  // exact (powers of two)
    if (Sd != std::floor(Sd) || Pd != std::floor(Pd) || Pd < 0.0 || Pd >= Sd) return false;
    r.S = static_cast<int64_t>(Sd);
    r.P0 = static_cast<int64_t>(Pd);
    const int64_t one = int64_t(1) << r.F;
    // bits of the largest sum (< one + S): its binade's grid is 2^(bits - 53) units
    int bits = 0;
    for (uint64_t v = static_cast<uint64_t>(one + r.S - 1); v; v >>= 1) ++bits;
    const int64_t grid = bits > 53 ? (int64_t(1) << (bits - 53)) : 1;
    return r.S % grid == 0 && r.P0 % grid == 0 && one % grid == 0;
}
}  // namespace

int64_t cntCubic(Counters& s, double ratio, int64_t n, std::vector<CubicSeg>* segs, int* segLen) {
    const double step = 1.0 / ratio;
    CubicRot rot;
    if (n > 0 && cubicRotation(step, s.cub_phase, rot)) {
        const __int128 one = static_cast<__int128>(1) << rot.F, S = rot.S, P0 = rot.P0;
        auto phaseAt = [&](int64_t i) {  // P_i in [0, S)
            __int128 v = (P0 - static_cast<__int128>(i) * one) % S;
            return v < 0 ? v + S : v;
        };
        auto outsBefore = [&](int64_t i, __int128 Pi) {
            return static_cast<int64_t>((static_cast<__int128>(i) * one + Pi - P0) / S);
        };
        if (segs)
            for (int64_t i = 0; i < n; i += (segLen ? *segLen : kCubicSegInputs)) {
                const __int128 Pi = phaseAt(i);
                segs->push_back({std::ldexp(static_cast<double>(static_cast<int64_t>(Pi)), -rot.F), s.y_count + outsBefore(i, Pi),
                                 s.x_count + i});
            }
        const __int128 Pn = phaseAt(n);
        const int64_t nout = outsBefore(n, Pn);
        s.cub_phase = std::ldexp(static_cast<double>(static_cast<int64_t>(Pn)), -rot.F);
        s.x_count += n;
        return nout;
    }
    if (segLen) *segLen = static_cast<int>(kCubicSegInputs);
    double ph = s.cub_phase;
    int64_t nout = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (segs && i % kCubicSegInputs == 0) segs->push_back({ph, s.y_count + nout, s.x_count + i});
        while (ph < 1.0) {
            ++nout;
            ph += step;
        }
        ph -= 1.0;
    }
    s.cub_phase = ph;
    s.x_count += n;
    return nout;
}

}  // namespace gar
