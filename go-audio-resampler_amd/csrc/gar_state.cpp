// gar_state.cpp -- state snapshots (gar.h gar_state_size / gar_state_save / gar_state_load; layout:
// DESIGN.md "State snapshots").  A blob is little-endian:
//   header   kStHdr bytes: magic, version, flags, total bytes, fingerprint, group count
//   records  per group kStGroupRec bytes, then per stage kStStageRec bytes (counters, xh, uh)
//   rows     the live histories as [len][C] of the compute type, each from a 16-byte boundary, in
//            record order (xh before uh); zero histories, empty ones and dry-run handles store none
//   checksum 64 bits over everything before it
// Every offset follows from the records, so a state has exactly one blob.
#include <cmath>
#include <cstring>

#include "gar_engine.hpp"

namespace gar {
namespace {

constexpr uint64_t kStMagic = 0x4554415453524147ull;  // "GARSTATE"
constexpr uint32_t kStVersion = 1;
constexpr uint32_t kStFlagDry = 1;
constexpr int64_t kStFpBytes = 72;
constexpr int64_t kStHdr = 24 + kStFpBytes + 8;  // 104
constexpr int64_t kStGroupRec = 24;
constexpr int64_t kStStageRec = 80 + 32 + 32;
constexpr int64_t kStMaxCount = int64_t(1) << 56;  // no stream reaches it; keeps every sum of counters in int64
// Longest untrimmed polyphase history accepted (stCountersBad): only designs with the no-trim quirk
// keep one, as long as the largest call that made it; 2^31 rows x 2048 channels x 8 bytes stays far
// inside size_t and cntPoly's (numIn * L) << 16 inside int64.
constexpr int64_t kStMaxQuirkRows = int64_t(1) << 31;

struct SnapHist {
    int64_t base = 0, len = 0;
    bool zero = false;
    int64_t off = 0;  // byte offset of the rows in the blob, 0: none stored
};
struct SnapStage {
    Counters c;
    SnapHist x, u;
};
struct SnapGroup {
    int c0 = 0, C = 1;
    int64_t statIn = 0, statOut = 0;
    std::vector<SnapStage> st;
};
struct Snap {
    bool dry = false;
    std::vector<SnapGroup> g;
    int64_t rowsBase = 0, rowsEnd = 0, total = 0;
};

int64_t align16(int64_t v) { return (v + 15) & ~int64_t(15); }

// Assigns the row offsets and the total size; false when the blob would pass `limit` bytes (an
// untrusted blob's lengths are checked against its own size here, before anything is allocated).
bool snapLayout(Snap& s, size_t ns, int tc, int64_t limit) {
    int64_t pos = kStHdr;
    for (size_t i = 0; i < s.g.size(); ++i) pos += kStGroupRec + static_cast<int64_t>(ns) * kStStageRec;
    if (pos > limit) return false;
    pos = align16(pos);
    s.rowsBase = pos;
    for (SnapGroup& g : s.g)
        for (SnapStage& st : g.st)
            for (SnapHist* h : {&st.x, &st.u}) {
                h->off = 0;
                if (s.dry || h->zero || h->len <= 0) continue;
                const int64_t rowBytes = static_cast<int64_t>(g.C) * tc;
                if (h->len > (limit - pos) / rowBytes) return false;
                h->off = pos;
                pos = align16(pos + h->len * rowBytes);
                if (pos > limit) return false;
            }
    s.rowsEnd = pos;
    s.total = pos + 8;
    return s.total <= limit;
}

struct StWriter {
    std::vector<uint8_t> b;
    void u32(uint32_t v) { for (int i = 0; i < 4; ++i) b.push_back(static_cast<uint8_t>(v >> (8 * i))); }
    void u64(uint64_t v) { for (int i = 0; i < 8; ++i) b.push_back(static_cast<uint8_t>(v >> (8 * i))); }
    void i32(int32_t v) { u32(static_cast<uint32_t>(v)); }
    void i64(int64_t v) { u64(static_cast<uint64_t>(v)); }
    void f64(double v) { u64(__builtin_bit_cast(uint64_t, v)); }
};
// Bounds-checked reader of untrusted bytes: past the end every read gives 0 and clears ok.
struct StReader {
    const uint8_t* p;
    int64_t n, pos = 0;
    bool ok = true;
    StReader(const void* buf, int64_t len) : p(static_cast<const uint8_t*>(buf)), n(len) {}
    uint64_t get(int bytes) {
        if (pos < 0 || bytes > n - pos) { ok = false; return 0; }
        uint64_t v = 0;
        for (int i = 0; i < bytes; ++i) v |= static_cast<uint64_t>(p[pos + i]) << (8 * i);
        pos += bytes;
        return v;
    }
    uint32_t u32() { return static_cast<uint32_t>(get(4)); }
    uint64_t u64() { return get(8); }
    int32_t i32() { return static_cast<int32_t>(u32()); }
    int64_t i64() { return static_cast<int64_t>(u64()); }
    double f64() { return __builtin_bit_cast(double, u64()); }
};

// 64-bit checksum of nbytes (a multiple of 8) as little-endian words: h = mix((h ^ w) * K).  Each step
// is a bijection of h for a fixed word and of the word for a fixed h, so two inputs that differ in one
// word never collide.
uint64_t stChecksum(const uint8_t* p, int64_t nbytes) {
    uint64_t h = 0x6a09e667f3bcc908ull;
    for (int64_t i = 0; i + 8 <= nbytes; i += 8) {
        uint64_t w;
        std::memcpy(&w, p + i, 8);  // little-endian hosts only (x86-64, like the AVX2 host staging)
        h = (h ^ w) * 0x9e3779b97f4a7c15ull;
        h ^= h >> 32;
    }
    return h;
}

// What a blob must match besides its own consistency: the constructor's arguments as the handle
// keeps them (device excluded: restoring on another GPU is the migration case).
void stFingerprint(const Handle* h, StWriter& w) {
    const size_t at = w.b.size();
    w.f64(h->fpInRate);
    w.f64(h->fpOutRate);
    w.i32(h->channels);
    w.i32(h->newPath ? h->cfg.channels : 1);
    w.i32(h->newPath ? 1 : 0);
    w.i32(h->f64 ? GAR_F64 : (h->hx ? GAR_F32 : GAR_F32_EXACT));
    w.i32(static_cast<int32_t>(h->stages.size()));
    const gar_quality_spec q = h->newPath ? h->cfg.quality : gar_quality_spec{};
    w.i32(h->newPath ? q.preset : h->fpQuality);
    w.i32(q.precision);
    w.u32(q.flags);
    w.f64(q.phase_response);
    w.f64(q.passband_end);
    w.f64(q.stopband_begin);
    while (static_cast<int64_t>(w.b.size() - at) < kStFpBytes) w.b.push_back(0);
}

// The history spans the engine keeps for these counters (stageProcess / stageFlush / materialize):
// xh = [xb, xb + xl), uh = [ub, ub + ul).
void stHistSpans(const StageRT& rt, const Counters& c, int64_t& xb, int64_t& xl, int64_t& ub, int64_t& ul) {
    xb = xl = ub = ul = 0;
    auto span = [](int64_t k0, int64_t k1, int64_t& b, int64_t& l) { b = k0; l = std::max<int64_t>(k1 - k0, 0); };
    switch (rt.d.kind) {
        case EngineKind::Cubic: span(std::max<int64_t>(0, c.x_count - 3), c.x_count, xb, xl); break;
        case EngineKind::DftOnly: span(c.x_count - c.dft_hist, c.x_count, xb, xl); break;
        case EngineKind::Decim: span(c.x_count - c.dec_hist, c.x_count, xb, xl); break;
        case EngineKind::DftPoly:
            if (!c.staged) {
                span(c.u_base / 2, c.x_count, xb, xl);
            } else {
                span(c.x_count - c.dft_hist, c.x_count, xb, xl);
                span(c.u_base, c.u_count, ub, ul);
            }
            break;
        default: break;
    }
}

// Counters a stream of this design can reach (cntDft / cntPoly / cntDecim / cntCubic invariants).
const char* stCountersBad(const StageRT& rt, const Counters& c, bool uhZero) {
    const EngineDesign& d = rt.d;
    for (int64_t v : {c.x_count, c.dft_hist, c.poly_hist, c.at, c.u_base, c.u_count, c.dec_hist, c.y_count})
        if (v < 0 || v > kStMaxCount) return "a counter is out of range";
    if (!rt.fused && !c.staged) return "fused mode on a stage without a composite plan";
    const bool dft = d.kind == EngineKind::DftOnly || d.kind == EngineKind::DftPoly;
    const bool poly = d.kind == EngineKind::DftPoly;
    const bool dec = d.kind == EngineKind::Decim;
    const bool cub = d.kind == EngineKind::Cubic;
    if (!dft && c.dft_hist != 0) return "DFT history on a stage without a DFT";
    if (!poly && (c.poly_hist != 0 || c.at != 0 || c.u_base != 0 || c.u_count != 0)) return "polyphase counters on a stage without a polyphase";
    if (!dec && (c.dec_hist != 0 || c.dec_phase != 0)) return "decimator counters on a stage without a decimator";
    if (!cub && c.cub_phase != 0.0) return "cubic phase on a stage without a cubic interpolator";
    if (!dft && !dec && !cub && c.x_count != 0) return "input count on a pass-through stage";
    if (dft) {
        if (d.dft.factor == 1) {
            if (c.x_count != 0 || c.dft_hist != 0) return "DFT counters on a factor-1 DFT";
        } else {
            if (c.dft_hist != std::min<int64_t>(c.x_count, d.dft.taps - 1)) return "DFT history length";
            const int64_t made = (c.x_count - c.dft_hist) * d.dft.factor;
            // the poly stream also receives poly.taps zeros per PolyphaseStage.Flush (stageFlush)
            if (poly ? (c.u_count < made || (c.u_count - made) % d.poly.taps != 0) : c.y_count != made) return "DFT output count";
        }
    }
    if (poly) {
        // a Flush leaves the fused mode, so a fused stage's poly stream is the DFT's output alone
        if (!c.staged && d.dft.factor > 1 && c.u_count != (c.x_count - c.dft_hist) * d.dft.factor) return "fused mode after a flush";
        if (c.u_base > c.u_count || c.poly_hist != c.u_count - c.u_base) return "polyphase history length";
        const int64_t period = static_cast<int64_t>(d.poly.L) << 16;
        if (c.at >= period) return "polyphase position";
        // cntPoly ends on at < limit + step, so it consumes at most numIn + (step - 1) / period inputs of a
        // history of numIn + taps - 1: while that excess is below taps every call trims the history to
        // fewer than taps rows (and the no-trim quirk, consumed > history, cannot occur)
        const bool trims = (d.poly.step - 1) / period < d.poly.taps;
        if (trims || !c.staged || uhZero) {
            if (c.poly_hist > d.poly.taps - 1) return "polyphase history longer than the design keeps";
        } else if (c.poly_hist > kStMaxQuirkRows) {  // untrimmed history: as long as the largest call made it
            return "polyphase history length out of range";
        }
        // without the quirk `at` and u_base move together: the poly stream position of output y_count
        if (trims && static_cast<__int128>(c.y_count) * d.poly.step != static_cast<__int128>(c.u_base) * period + c.at)
            return "polyphase output count";
    }
    if (dec) {
        if (d.decim.factor == 1) {
            if (c.x_count != 0 || c.dec_hist != 0 || c.dec_phase != 0) return "decimator counters on a factor-1 decimator";
        } else {
            if (c.dec_hist > c.x_count || c.dec_hist > static_cast<int64_t>(d.decim.taps) + d.decim.factor - 2) return "decimator history length";
            if (c.dec_phase < 0 || c.dec_phase >= d.decim.factor) return "decimator phase";
            if (c.dec_hist >= d.decim.taps && c.dec_phase < c.dec_hist - d.decim.taps + 1) return "decimator phase behind its history";
            // outputs sit on the filter positions that are multiples of the factor; P positions are done
            const int64_t P = c.x_count - c.dec_hist;
            if (c.y_count != (P + d.decim.factor - 1) / d.decim.factor) return "decimator output count";
            if (c.dec_phase != (d.decim.factor - P % d.decim.factor) % d.decim.factor) return "decimator phase against its position";
        }
    }
    if (cub) {
        const double step = 1.0 / d.ratio;
        // the walk leaves fl(ph + step) - 1 with ph < 1: at most fl(1 + step) - 1 (step plus its rounding)
        if (!(c.cub_phase >= 0.0) || !(c.cub_phase <= (1.0 + step) - 1.0)) return "cubic phase";
        // exactly, y_count * step = x_count + phase; each of the walk's x_count + y_count additions rounds
        // by at most 2^-52 of a value below 2 + step (a closed form exists only for exact rotations)
        const double drift = static_cast<double>(c.y_count) * step - static_cast<double>(c.x_count) - c.cub_phase;
        const double tol = (2.0 + step) * (2.0 + static_cast<double>(c.x_count + c.y_count)) * 0x1p-50;
        if (!(std::fabs(drift) <= tol)) return "cubic output count";
    }
    return nullptr;
}

void stPutHist(StWriter& w, const SnapHist& h) {
    w.i64(h.base);
    w.i64(h.len);
    w.u32(h.zero ? 1 : 0);
    w.u32(0);
    w.i64(h.off);
}

// The handle's state as a Snap (offsets assigned) -- host only, valid at once: the counters and spans
// are the host's own bookkeeping, whatever the device still has queued.
Snap snapOf(const Handle* h) {
    Snap s;
    s.dry = h->dry;
    for (const Group& g : h->groups) {
        SnapGroup sg;
        sg.c0 = g.c0;
        sg.C = g.C;
        sg.statIn = g.statIn;
        sg.statOut = g.statOut;
        for (size_t i = 0; i < h->stages.size(); ++i) {
            SnapStage st;
            st.c = g.cnt[i];
            st.x.base = g.dev[i].xh.base; st.x.len = g.dev[i].xh.len; st.x.zero = g.dev[i].xh.zero;
            st.u.base = g.dev[i].uh.base; st.u.len = g.dev[i].uh.len; st.u.zero = g.dev[i].uh.zero;
            sg.st.push_back(st);
        }
        s.g.push_back(std::move(sg));
    }
    snapLayout(s, h->stages.size(), h->tc(), INT64_MAX / 2);
    return s;
}

// Header + records of a laid-out Snap (the bytes [0, records end)).
void stPutHead(const Handle* h, const Snap& s, StWriter& w) {
    w.u64(kStMagic);
    w.u32(kStVersion);
    w.u32(s.dry ? kStFlagDry : 0);
    w.i64(s.total);
    stFingerprint(h, w);
    w.i32(static_cast<int32_t>(s.g.size()));
    w.i32(0);
    for (const SnapGroup& g : s.g) {
        w.i32(g.c0);
        w.i32(g.C);
        w.i64(g.statIn);
        w.i64(g.statOut);
        for (const SnapStage& st : g.st) {
            const Counters& c = st.c;
            w.u32(c.staged ? 1 : 0);
            w.i32(c.dec_phase);
            w.i64(c.x_count); w.i64(c.dft_hist); w.i64(c.poly_hist); w.i64(c.at);
            w.i64(c.u_base); w.i64(c.u_count); w.i64(c.dec_hist); w.i64(c.y_count);
            w.f64(c.cub_phase);
            stPutHist(w, st.x);
            stPutHist(w, st.u);
        }
    }
}

gar_status stRefuse(const std::string& why) {
    setError("state blob refused: " + why);
    return GAR_ERR_INVALID_ARGUMENT;
}

bool stGetHist(StReader& r, SnapHist& h) {
    h.base = r.i64();
    h.len = r.i64();
    const uint32_t z = r.u32();
    const uint32_t pad = r.u32();
    h.off = r.i64();
    h.zero = z == 1;
    return z <= 1 && pad == 0;
}

// Parses and validates an untrusted blob against the handle's design; on GAR_OK `s` is a state the
// engine itself could have reached, laid out exactly as the blob is.  Touches nothing of the handle.
gar_status stParse(const Handle* h, const void* buf, int64_t n, Snap& s) {
    if (!buf || n < kStHdr + 8) return stRefuse("shorter than a header");
    StReader r(buf, n);
    if (r.u64() != kStMagic) return stRefuse("wrong magic");
    const uint32_t ver = r.u32();
    if (ver != kStVersion) return stRefuse("version " + std::to_string(ver) + ", this build reads version " + std::to_string(kStVersion));
    const uint32_t flags = r.u32();
    const int64_t total = r.i64();
    if (total != n) return stRefuse("length " + std::to_string(n) + " differs from the recorded " + std::to_string(total));
    if (n % 8 != 0) return stRefuse("length is not a multiple of 8");
    const uint8_t* p = static_cast<const uint8_t*>(buf);
    uint64_t sum;
    std::memcpy(&sum, p + n - 8, 8);
    if (sum != stChecksum(p, n - 8)) return stRefuse("checksum mismatch");
    StWriter fp;
    stFingerprint(h, fp);
    if (std::memcmp(fp.b.data(), p + r.pos, static_cast<size_t>(kStFpBytes)) != 0)
        return stRefuse("fingerprint mismatch (rates, channels, quality, path, compute type or stage count differ from this handle's)");
    r.pos += kStFpBytes;
    if (flags & ~kStFlagDry) return stRefuse("unknown flags");
    s.dry = (flags & kStFlagDry) != 0;
    if (s.dry != h->dry) return stRefuse(s.dry ? "a dry-run handle's blob on a real handle" : "a real handle's blob on a dry-run handle");
    const int32_t ng = r.i32();
    if (r.i32() != 0) return stRefuse("reserved field set");
    const size_t ns = h->stages.size();
    const int64_t perGroup = kStGroupRec + static_cast<int64_t>(ns) * kStStageRec;
    if (ng < 1 || ng > h->channels || ng > (n - 8 - kStHdr) / perGroup) return stRefuse("group count");
    const int tc = h->tc();
    int next = 0;
    for (int32_t gi = 0; gi < ng; ++gi) {
        SnapGroup g;
        g.c0 = r.i32();
        g.C = r.i32();
        g.statIn = r.i64();
        g.statOut = r.i64();
        if (g.c0 != next || g.C < 1 || g.C > h->channels - g.c0) return stRefuse("channel ranges overlap or leave a gap");
        next = g.c0 + g.C;
        if (g.statIn < 0 || g.statOut < 0) return stRefuse("negative statistics");
        for (size_t i = 0; i < ns; ++i) {
            SnapStage st;
            Counters& c = st.c;
            const uint32_t staged = r.u32();
            c.dec_phase = r.i32();
            c.x_count = r.i64(); c.dft_hist = r.i64(); c.poly_hist = r.i64(); c.at = r.i64();
            c.u_base = r.i64(); c.u_count = r.i64(); c.dec_hist = r.i64(); c.y_count = r.i64();
            c.cub_phase = r.f64();
            c.staged = staged == 1;
            const bool histOk = stGetHist(r, st.x) && stGetHist(r, st.u);
            if (!r.ok) return stRefuse("truncated records");
            const std::string where = " (group " + std::to_string(gi) + ", stage " + std::to_string(i) + ")";
            if (staged > 1 || !histOk) return stRefuse("flag field out of range" + where);
            const StageRT& rt = *h->stages[i];
            if (const char* bad = stCountersBad(rt, c, st.u.zero)) return stRefuse(std::string("counters inconsistent with the design: ") + bad + where);
            int64_t xb, xl, ub, ul;
            stHistSpans(rt, c, xb, xl, ub, ul);
            if (st.x.base != xb || st.x.len != xl || st.u.base != ub || st.u.len != ul)
                return stRefuse("history span differs from the one its counters give" + where);
            const bool mayZero = rt.d.kind == EngineKind::DftPoly && c.staged;
            if ((st.x.zero || st.u.zero) && !mayZero) return stRefuse("zero history on a stage that keeps none" + where);
            g.st.push_back(st);
        }
        s.g.push_back(std::move(g));
    }
    if (next != h->channels) return stRefuse("channel ranges leave [0, channels) uncovered");
    // the layout these records give must be the blob's own: recorded offsets, total, zero padding
    Snap want = s;
    if (!snapLayout(want, ns, tc, n) || want.total != n) return stRefuse("recorded lengths disagree with the blob's size");
    int64_t end = r.pos;  // end of the bytes accounted for so far
    auto padZero = [&](int64_t from, int64_t to) {
        for (int64_t i = from; i < to; ++i)
            if (p[i] != 0) return false;
        return true;
    };
    if (!padZero(end, want.rowsBase)) return stRefuse("padding not zero");
    end = want.rowsBase;
    for (size_t gi = 0; gi < s.g.size(); ++gi)
        for (size_t i = 0; i < ns; ++i) {
            const SnapHist* got[2] = {&s.g[gi].st[i].x, &s.g[gi].st[i].u};
            const SnapHist* exp[2] = {&want.g[gi].st[i].x, &want.g[gi].st[i].u};
            for (int k = 0; k < 2; ++k) {
                if (got[k]->off != exp[k]->off) return stRefuse("segment offset differs from the layout its records give");
                if (!exp[k]->off) continue;
                const int64_t stop = exp[k]->off + exp[k]->len * s.g[gi].C * tc;
                if (!padZero(stop, align16(stop))) return stRefuse("padding not zero");
                end = align16(stop);
            }
        }
    if (end != want.rowsEnd) return stRefuse("recorded lengths disagree with the blob's size");
    s.rowsBase = want.rowsBase;
    s.rowsEnd = want.rowsEnd;
    s.total = want.total;
    return GAR_OK;
}

// Segment table of a laid-out Snap over the histories `hist(gi, si, k)` (k = 0 xh, 1 uh); offsets
// relative to the row image (blob offset rowsBase).  Returns the chunk total.
template <class F>
int64_t stSegTable(const Snap& s, int tc, F&& hist, std::vector<StateSeg>& tab) {
    int64_t chunks = 0;
    for (size_t gi = 0; gi < s.g.size(); ++gi)
        for (size_t i = 0; i < s.g[gi].st.size(); ++i) {
            const SnapHist* hs[2] = {&s.g[gi].st[i].x, &s.g[gi].st[i].u};
            for (int k = 0; k < 2; ++k) {
                if (!hs[k]->off) continue;
                StateSeg e{};
                e.ptr = hist(gi, i, k);
                e.rows = hs[k]->len;
                e.C = s.g[gi].C;
                e.es = tc;
                e.off = hs[k]->off - s.rowsBase;
                e.chunk0 = chunks;
                chunks += (e.rows * e.C * e.es + 15) / 16;
                tab.push_back(e);
            }
        }
    return chunks;
}

gar_status stSave(Handle* h, void* buf, int64_t cap, int64_t* nWritten) {
    const Snap s = snapOf(h);
    if (nWritten) *nWritten = s.total;
    if (cap < s.total) return guard(GAR_ERR_BUFFER_TOO_SMALL, "state buffer too small");
    uint8_t* out = static_cast<uint8_t*>(buf);
    StWriter w;
    stPutHead(h, s, w);
    const int64_t rowBytes = s.rowsEnd - s.rowsBase;
    std::vector<StateSeg> tab;
    const int64_t chunks = stSegTable(s, h->tc(), [&](size_t gi, size_t i, int k) {
        const StageDev& d = h->groups[gi].dev[i];
        return (k ? d.uh : d.xh).ptr();
    }, tab);
    for (const StateSeg& e : tab)
        if (!e.ptr) { setError("a live history without a buffer"); return GAR_ERR_INTERNAL; }
    if (!tab.empty()) {  // one gather launch into the device image, one copy to the host
        h->stateTab.ensure(tab.size() * sizeof(StateSeg));
        h->stateImg.ensure(static_cast<size_t>(rowBytes));
        HIPCHK(hipMemcpyAsync(h->stateTab.p, tab.data(), tab.size() * sizeof(StateSeg), hipMemcpyHostToDevice, h->stream));
        HIPCHK(launchStatePack(static_cast<const StateSeg*>(h->stateTab.p), static_cast<int>(tab.size()), chunks, h->stateImg.p, h->stream));
        HIPCHK(hipMemcpyAsync(out + s.rowsBase, h->stateImg.p, static_cast<size_t>(rowBytes), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    std::memcpy(out, w.b.data(), w.b.size());
    std::memset(out + w.b.size(), 0, static_cast<size_t>(s.rowsBase) - w.b.size());
    for (const StateSeg& e : tab) {  // the image's pad bytes were never written: canonical zeros
        const int64_t stop = s.rowsBase + e.off + e.rows * e.C * e.es;
        std::memset(out + stop, 0, static_cast<size_t>(align16(stop) - stop));
    }
    const uint64_t sum = stChecksum(out, s.rowsEnd);
    std::memcpy(out + s.rowsEnd, &sum, 8);
    return GAR_OK;
}

gar_status stLoad(Handle* h, const Snap& s, const void* buf) {
    const int tc = h->tc();
    std::vector<Group> fresh;
    for (const SnapGroup& sg : s.g) {
        Group g = freshGroup(h, sg.c0, sg.C);
        g.statIn = sg.statIn;
        g.statOut = sg.statOut;
        for (size_t i = 0; i < sg.st.size(); ++i) {
            g.cnt[i] = sg.st[i].c;
            const SnapHist* src[2] = {&sg.st[i].x, &sg.st[i].u};
            Hist* dst[2] = {&g.dev[i].xh, &g.dev[i].uh};
            for (int k = 0; k < 2; ++k) {
                dst[k]->cur = 0;
                dst[k]->base = src[k]->base;
                dst[k]->len = src[k]->len;
                dst[k]->zero = src[k]->zero;
                if (src[k]->off) dst[k]->buf[0].ensure(static_cast<size_t>(src[k]->len) * sg.C * tc);
            }
        }
        fresh.push_back(std::move(g));
    }
    std::vector<StateSeg> tab;
    const int64_t chunks = stSegTable(s, tc, [&](size_t gi, size_t i, int k) {
        StageDev& d = fresh[gi].dev[i];
        return (k ? d.uh : d.xh).buf[0].p;
    }, tab);
    if (!tab.empty()) {  // one copy to the device image, one scatter launch
        const int64_t rowBytes = s.rowsEnd - s.rowsBase;
        h->stateTab.ensure(tab.size() * sizeof(StateSeg));
        h->stateImg.ensure(static_cast<size_t>(rowBytes));
        HIPCHK(hipMemcpyAsync(h->stateTab.p, tab.data(), tab.size() * sizeof(StateSeg), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->stateImg.p, static_cast<const uint8_t*>(buf) + s.rowsBase, static_cast<size_t>(rowBytes),
                              hipMemcpyHostToDevice, h->stream));
        HIPCHK(launchStateUnpack(static_cast<const StateSeg*>(h->stateTab.p), static_cast<int>(tab.size()), chunks, h->stateImg.p, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    h->groups = std::move(fresh);  // the old histories are idle (drained): freed here
    return GAR_OK;
}

// A state call on a real handle: refused while poisoned, the handle's device current, every earlier
// call drained first; a HIP failure poisons the handle like any other call's.
template <class F>
gar_status stCall(Handle* h, F&& f) {
    if (h->poisoned) return guard(GAR_ERR_DEVICE, "handle unusable after an earlier device error; call Reset");
    if (h->dry) return wrap(f);
    if (devFault(h)) return GAR_ERR_DEVICE;
    DeviceGuard dg(h->device);
    gar_status st = wrap([&]() -> gar_status {
        waitEnqueued(h);
        if (devFault(h)) return GAR_ERR_DEVICE;  // a kernel of the calls just drained reported
        return f();
    });
    if (st == GAR_ERR_DEVICE) h->poisoned = true;
    return st;
}

}  // namespace

int64_t stateSize(const Handle* h) { return snapOf(h).total; }

gar_status stateSave(Handle* h, void* buf, int64_t cap, int64_t* nWritten) {
    return stCall(h, [&]() -> gar_status { return stSave(h, buf, cap, nWritten); });
}

gar_status stateLoad(Handle* h, const void* buf, int64_t n) {
    if (h->poisoned) return guard(GAR_ERR_DEVICE, "handle unusable after an earlier device error; call Reset");
    Snap s;
    const gar_status ps = wrap([&]() -> gar_status { return stParse(h, buf, n, s); });  // host only; nothing changed on refusal
    if (ps != GAR_OK) return ps;
    return stCall(h, [&]() -> gar_status { return stLoad(h, s, buf); });
}

}  // namespace gar
