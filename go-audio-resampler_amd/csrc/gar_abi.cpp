// gar_abi.cpp -- the C ABI (include/gar.h): argument checks, configuration and constructors, the host
// staging of the host entry points, and the entry points themselves.  The state machine they drive is
// gar_engine.cpp's; every refusal text of a process / flush entry point is pinned by
// tests/test_abi_refusals.py.
#include <immintrin.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <type_traits>

#include "gar_engine.hpp"
#include "gar_hx_launch.hpp"
#include "gar_pool.hpp"

namespace gar {
namespace {

// Precision carried by a preset (resample.go:217-267).
gar_quality_spec presetSpec(int32_t preset) {
    gar_quality_spec q{};
    switch (preset) {
        case GAR_QUALITY_QUICK: q = {GAR_QUALITY_QUICK, 8, 50.0, 0.7, 1.0, 0}; break;
        case GAR_QUALITY_LOW: q = {GAR_QUALITY_LOW, 16, 50.0, 0.80, 0.95, 0}; break;
        case GAR_QUALITY_MEDIUM: q = {GAR_QUALITY_MEDIUM, 16, 50.0, 0.90, 0.98, 0}; break;
        case GAR_QUALITY_HIGH: q = {GAR_QUALITY_HIGH, 24, 50.0, 0.95, 0.99, 0}; break;
        case GAR_QUALITY_VERYHIGH: q = {GAR_QUALITY_VERYHIGH, 32, 50.0, 0.99, 0.995, 0}; break;
        default: q = {GAR_QUALITY_MEDIUM, 0, 0, 0, 0, 0}; break;
    }
    return q;
}

gar_status validate(const gar_config* c) {
    if (!c) return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: config is nil");
    if (!(c->input_rate > 0) || !(c->output_rate > 0))
        return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: sample rates must be positive");
    if (c->channels < 1) return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: channels must be at least 1");
    if (c->channels > 256) return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: too many channels (max 256)");
    if (c->compute_dtype == GAR_F16 || c->compute_dtype == GAR_BF16)
        return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: f16 / bf16 are sample types of the device entry points, not compute types");
    if (c->compute_dtype == GAR_PCM24_PACKED)
        return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: packed 24-bit PCM is a sample type of the device entry points, not a compute type");
    const double r = c->output_rate / c->input_rate;
    if (r < 1.0 / 256.0 || r > 256.0)
        return guard(GAR_ERR_INVALID_CONFIG, "invalid resampler configuration: resampling ratio out of range");
    const gar_quality_spec& q = c->quality;
    if (q.preset == GAR_QUALITY_CUSTOM) {
        if (q.precision < 8 || q.precision > 33) return guard(GAR_ERR_INVALID_CONFIG, "precision must be 8-33 bits");
        if (q.phase_response < 0 || q.phase_response > 100) return guard(GAR_ERR_INVALID_CONFIG, "phase response must be 0-100");
        if (q.passband_end <= 0 || q.passband_end >= 1) return guard(GAR_ERR_INVALID_CONFIG, "passband end must be in (0, 1)");
        if (q.stopband_begin <= q.passband_end || q.stopband_begin > 1)
            return guard(GAR_ERR_INVALID_CONFIG, "stopband begin must be in (passband_end, 1]");
    }
    return GAR_OK;
}

// GAR_HX=0 in the environment routes GAR_F32 compute to the exact-f32 MFMA kernel (A/B comparisons).
bool hxEnabled() {
    static const bool on = [] {
        const char* e = std::getenv("GAR_HX");
        return !(e && e[0] == '0');
    }();
    return on;
}

gar_status initDevice(Handle* h) {
    if (h->dry) return GAR_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= h->device)
        return guard(GAR_ERR_DEVICE, "no HIP device visible (the GPU path requires an MI355X / gfx950)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // device-scope release: the event only orders this handle's calls across streams of its
    // device (host visibility of results goes through the stream syncs of the host paths); a
    // system-scope release would write back every dirty L2 line after each call
    HIPCHK(hipEventCreateWithFlags(&h->orderEv, hipEventDisableTiming | hipEventDisableSystemFence));
    HIPCHK(hipEventCreateWithFlags(&h->failEv, hipEventDisableTiming));
    // the device status word: coherent pinned host memory, so a kernel's system-scope store is seen by
    // the next ABI call without a synchronisation
    void* w = nullptr;
    HIPCHK(hipHostMalloc(&w, 64, hipHostMallocMapped | hipHostMallocCoherent));
    h->errHost = static_cast<int*>(w);
    *h->errHost = 0;
    void* d = nullptr;
    HIPCHK(hipHostGetDevicePointer(&d, w, 0));
    h->errDev = static_cast<int*>(d);
    return GAR_OK;
}

gar_status addStage(Handle* h, double inRate, double outRate, Quality q) {
    auto rt = std::make_unique<StageRT>();
    std::string err;
    if (!designEngine(inRate, outRate, q, rt->d, err)) return guard(GAR_ERR_INVALID_CONFIG, err.c_str());
    if (!buildStage(*rt, h->f64, h->hx, h->dry, err)) return guard(GAR_ERR_INTERNAL, err.c_str());
    h->stages.push_back(std::move(rt));
    return GAR_OK;
}

gar_status newCommon(gar_config* cfg, int32_t nstreams, gar_resampler** out) {
    if (!out) return guard(GAR_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    gar_status s = validate(cfg);
    if (s != GAR_OK) return s;
    if (nstreams < 1) return guard(GAR_ERR_INVALID_CONFIG, "n_streams must be >= 1");
    if (cfg->quality.preset != GAR_QUALITY_CUSTOM) cfg->quality = presetSpec(cfg->quality.preset);
    auto h = std::make_unique<Handle>();
    h->newPath = true;
    h->cfg = *cfg;
    h->channels = cfg->channels * nstreams;
    h->ratio = cfg->output_rate / cfg->input_rate;
    h->f64 = cfg->compute_dtype != GAR_F32 && cfg->compute_dtype != GAR_F32_EXACT;
    h->hx = cfg->compute_dtype == GAR_F32 && hxEnabled();
    h->dry = cfg->dry_run != 0;
    h->device = cfg->device;
    h->fpInRate = cfg->input_rate;
    h->fpOutRate = cfg->output_rate;
    DeviceGuard dg(h->dry ? -1 : cfg->device);
    return wrap([&]() -> gar_status {
        gar_status st = initDevice(h.get());
        if (st != GAR_OK) return st;
        const int prec = cfg->quality.precision;
        const std::vector<StageSpec> specs = buildPipeline(h->ratio, prec);
        for (const StageSpec& sp : specs) {
            // createStage -> engine.NewResampler[float64](48000, 48000*ratio, q) (stages.go:54-70)
            if (sp.type == StageType::Cubic) {
                // newCubicStage(ratio) -> engine.NewCubicStage[float64] at the total ratio (stages.go:21-23)
                st = addStage(h.get(), 1.0, sp.ratio, Quality::Quick);
                if (st != GAR_OK) return st;
                continue;
            }
            const double ir = 48000.0;
            st = addStage(h.get(), ir, ir * sp.ratio, precisionToEngineQuality(prec));
            if (st != GAR_OK) return st;
        }
        h->groups.push_back(freshGroup(h.get(), 0, h->channels));
        *out = h.release();
        return GAR_OK;
    });
}

// engine.NewResampler[F] behind NewEngine / NewEngineFloat32 / the engine seam
// (convenience.go:125-135, :329-336; internal/engine/resampler.go:51-179).
gar_status newEngineCommon(double in_rate, double out_rate, Quality q, int32_t dtype, bool dry, gar_resampler** out) {
    if (!out) return guard(GAR_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (dtype != GAR_F64 && dtype != GAR_F32 && dtype != GAR_F32_EXACT) return guard(GAR_ERR_INVALID_ARGUMENT, "unknown dtype");
    if (!(in_rate > 0) || !(out_rate > 0)) return guard(GAR_ERR_INVALID_CONFIG, "sample rates must be positive");
    auto h = std::make_unique<gar_resampler>();
    h->newPath = false;
    h->channels = 1;
    h->dry = dry;
    h->f64 = dtype == GAR_F64;
    h->hx = dtype == GAR_F32 && hxEnabled();
    h->engineF32Io = dtype != GAR_F64;
    h->ratio = out_rate / in_rate;
    h->fpInRate = in_rate;
    h->fpOutRate = out_rate;
    h->fpQuality = static_cast<int32_t>(q);
    DeviceGuard dg(dry ? -1 : 0);
    return wrap([&]() -> gar_status {
        gar_status st = initDevice(h.get());
        if (st != GAR_OK) return st;
        st = addStage(h.get(), in_rate, out_rate, q);
        if (st != GAR_OK) return st;
        h->ratio = h->stages[0]->d.ratio;
        h->groups.push_back(freshGroup(h.get(), 0, 1));
        *out = h.release();
        return GAR_OK;
    });
}

int64_t estimate(const Handle* h, int64_t n) {
    return static_cast<int64_t>(static_cast<double>(n) * h->ratio) + 64;
}

// Pinned host staging above kPinKeep bytes is released when the call that grew it returns, so a
// one-shot call on a long stream does not keep hundreds of MB of page-locked memory per handle.
constexpr size_t kPinKeep = size_t(64) << 20;
// Called only after the call's stream has been synchronised (no kernel still reads the buffers).
void trimHost(Handle* h) {
    if (h->hostIn.cap > kPinKeep) h->hostIn.release();
    if (h->hostOut.cap > kPinKeep) h->hostOut.release();
}

// Runs f(c, lo, hi) over channels x [0, n) samples: inline below ~1 MiB of data, else split over
// the pool -- whole channels per job when there are many channels (2 jobs per worker), else
// slices of channels.
void forSlices(int C, int64_t n, size_t bytesPerSample, const std::function<void(int, int64_t, int64_t)>& f) {
    const size_t total = static_cast<size_t>(C) * static_cast<size_t>(std::max<int64_t>(n, 0)) * bytesPerSample;
    if (total < (size_t(1) << 20)) {
        for (int c = 0; c < C; ++c) f(c, 0, n);
        return;
    }
    Pool& pool = Pool::get();
    const int J = pool.workers() * 2;
    if (C >= J) {
        pool.run(J, [&](int j) {
            for (int c = static_cast<int>(static_cast<int64_t>(C) * j / J); c < static_cast<int64_t>(C) * (j + 1) / J; ++c) f(c, 0, n);
        });
        return;
    }
    const int per = std::max<int>(1, (J + C - 1) / C);  // slices per channel
    const int64_t step = (n + per - 1) / per;
    pool.run(C * per, [&](int i) {
        const int c = i / per, k = i - c * per;
        const int64_t lo = k * step, hi = std::min<int64_t>(n, lo + step);
        if (lo < hi) f(c, lo, hi);
    });
}

// Host input -> pinned staging in the compute dtype (f64 -> f32 rounds exactly as the kernels'
// loads would: the result is bit-identical to handing them the f64 input).
// Host conversions of the staging copies, AVX2 where the CPU has it.  The output copy into the
// caller's arrays uses streaming stores (no read-for-ownership of 8.9 MB per 256-channel 4096-frame
// call); each job ends with an sfence so the stores are globally visible before the pool's hand-off.
__attribute__((target("avx2"))) void cvtD2F(float* d, const double* s, int64_t n) {
    int64_t i = 0;
    for (; i + 8 <= n; i += 8)
        _mm256_storeu_ps(d + i, _mm256_set_m128(_mm256_cvtpd_ps(_mm256_loadu_pd(s + i + 4)),
                                                _mm256_cvtpd_ps(_mm256_loadu_pd(s + i))));
    for (; i < n; ++i) d[i] = static_cast<float>(s[i]);
}
__attribute__((target("avx2"))) void cvtF2DStream(double* d, const float* s, int64_t n) {
    int64_t i = 0;
    for (; i < n && (reinterpret_cast<uintptr_t>(d + i) & 31); ++i) d[i] = static_cast<double>(s[i]);
    for (; i + 8 <= n; i += 8) {
        _mm256_stream_pd(d + i, _mm256_cvtps_pd(_mm_loadu_ps(s + i)));
        _mm256_stream_pd(d + i + 4, _mm256_cvtps_pd(_mm_loadu_ps(s + i + 4)));
    }
    for (; i < n; ++i) d[i] = static_cast<double>(s[i]);
    _mm_sfence();
}
__attribute__((target("avx2"))) void copyD2DStream(double* d, const double* s, int64_t n) {
    int64_t i = 0;
    for (; i < n && (reinterpret_cast<uintptr_t>(d + i) & 31); ++i) d[i] = s[i];
    for (; i + 8 <= n; i += 8) {
        _mm256_stream_pd(d + i, _mm256_loadu_pd(s + i));
        _mm256_stream_pd(d + i + 4, _mm256_loadu_pd(s + i + 4));
    }
    for (; i < n; ++i) d[i] = s[i];
    _mm_sfence();
}
bool hostAvx2() {
    static const bool a = __builtin_cpu_supports("avx2");
    return a;
}

template <class T>
void packChannel(void* dst, bool f64, const T* src, int64_t lo, int64_t hi) {
    if constexpr (std::is_same<T, double>::value) {
        if (!f64 && hostAvx2()) {
            cvtD2F(static_cast<float*>(dst) + lo, src + lo, hi - lo);
            return;
        }
    }
    if (f64) {
        double* d = static_cast<double*>(dst);
        for (int64_t i = lo; i < hi; ++i) d[i] = static_cast<double>(src[i]);
    } else {
        float* d = static_cast<float*>(dst);
        for (int64_t i = lo; i < hi; ++i) d[i] = static_cast<float>(src[i]);
    }
}
template <class T>
void unpackChannel(T* dst, bool f64, const void* src, int64_t lo, int64_t hi) {
    if constexpr (std::is_same<T, double>::value) {
        if (hostAvx2() && hi - lo >= 64) {
            if (f64) copyD2DStream(dst + lo, static_cast<const double*>(src) + lo, hi - lo);
            else cvtF2DStream(dst + lo, static_cast<const float*>(src) + lo, hi - lo);
            return;
        }
    }
    if (f64) {
        const double* s = static_cast<const double*>(src);
        for (int64_t i = lo; i < hi; ++i) dst[i] = static_cast<T>(s[i]);
    } else {
        const float* s = static_cast<const float*>(src);
        for (int64_t i = lo; i < hi; ++i) dst[i] = static_cast<T>(s[i]);
    }
}

// The per-channel host calls (Process / ProcessInto / Flush and their f32 twins) on channel `ch`.
template <class T>
gar_status monoCall(Handle* h, int ch, const T* in, int64_t n, T* out, int64_t cap, int64_t* nOut, bool flush,
                    bool intoSemantics) {
    if (!h) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (ch < 0 || ch >= h->channels) return guard(GAR_ERR_INVALID_ARGUMENT, "channel out of range");
    if (nOut) *nOut = 0;
    if (!flush && n < 0) return guard(GAR_ERR_INVALID_ARGUMENT, "negative length");
    if (!flush && intoSemantics && cap < estimate(h, n)) return guard(GAR_ERR_BUFFER_TOO_SMALL, "output buffer too small");
    const size_t es = h->tc();  // compute dtype: the staging holds exactly what the kernels compute in
    return callOn(h, h->stream, [&]() -> gar_status {
        isolate(h, ch);
        Group* g = groupOf(h, ch);
        std::vector<int64_t> sizes;
        const int64_t need = simulate(h, *g, flush ? 0 : n, flush, sizes);
        if (need > cap) {
            if (intoSemantics && !flush) return guard(GAR_ERR_INTERNAL, "EstimateOutput underestimated actual output length");
            return guard(GAR_ERR_BUFFER_TOO_SMALL, "output buffer too small");
        }
        InView iv;
        iv.n = flush ? 0 : n;
        iv.f64 = h->cf();
        iv.fs = 1;
        iv.cs = 0;
        OutView ov;
        ov.fs = 1;
        ov.cs = 0;
        ov.f64 = h->cf();
        if (!h->dry) {
            if (!flush && n > 0) {
                void* hp = h->hostIn.ensure(static_cast<size_t>(n) * es);
                forSlices(1, n, es + sizeof(T), [&](int, int64_t lo, int64_t hi) { packChannel<T>(hp, h->f64, in, lo, hi); });
                iv.p = hp;
            }
            ov.p = h->hostOut.ensure(static_cast<size_t>(std::max<int64_t>(need, 1)) * es);
        }
        gar_status st;
        const int64_t got = runGroup(h, *g, iv, ov, flush, h->stream, cap, st);
        if (st != GAR_OK) return st;
        if (!h->dry) {
            HIPCHK(hipStreamSynchronize(h->stream));
            forSlices(1, got, es + sizeof(T), [&](int, int64_t lo, int64_t hi) { unpackChannel<T>(out, h->f64, ov.p, lo, hi); });
            trimHost(h);
        }
        if (nOut) *nOut = got;
        return GAR_OK;
    }, true);
}

// Development (GAR_HOST_TRACE=1, read once): per-call phase times of the host multi-channel path on
// stderr (pack into the pinned staging, launches, wait for the device, unpack), microseconds.
struct HostTrace {
    bool on;
    std::chrono::steady_clock::time_point t0;
    double ph[4] = {0, 0, 0, 0};
    HostTrace() : on(enabled()), t0(std::chrono::steady_clock::now()) {}
    static bool enabled() {
        static const bool e = [] { const char* v = std::getenv("GAR_HOST_TRACE"); return v && v[0] == '1'; }();
        return e;
    }
    void add(int k) {  // the time since the previous mark belongs to phase k
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        ph[k] += std::chrono::duration<double, std::micro>(t - t0).count();
        t0 = t;
    }
    ~HostTrace() {
        if (on) fprintf(stderr, "host-trace pack %.1f launch %.1f device-wait %.1f unpack %.1f us\n", ph[0], ph[1], ph[2], ph[3]);
    }
};

// ProcessMulti / FlushMulti over every group of the handle: `in` is NULL and n is 0 when flushing.
gar_status hostMulti(Handle* h, const double* const* in, int64_t n, double* const* out, int64_t cap, int64_t* n_out,
                     bool flush) {
    return callOn(h, h->stream, [&]() -> gar_status {
        // exact sizes first: no state changes on BUFFER_TOO_SMALL
        int64_t need = 0;
        for (auto& g : h->groups) {
            std::vector<int64_t> s;
            const int64_t m = simulate(h, g, n, flush, s);
            if (m > cap) return guard(GAR_ERR_BUFFER_TOO_SMALL, "output buffer too small");
            need = std::max(need, m);
        }
        const int C = h->channels;
        const size_t es = h->tc();
        // planar [channel][frame] in the compute dtype, staged for the exact output length (not the
        // caller's capacity); output rows 16-B aligned (vector stores)
        const int64_t ocap = (std::max<int64_t>(need, 1) + 3) / 4 * 4;
        char* hin = nullptr;
        char* hout = nullptr;
        HostTrace tr;
        if (!h->dry) {
            if (n > 0) {
                hin = static_cast<char*>(h->hostIn.ensure(static_cast<size_t>(n) * C * es));
                forSlices(C, n, es + 8, [&](int c, int64_t lo, int64_t hi) {
                    packChannel<double>(hin + static_cast<size_t>(c) * n * es, h->f64, in[c], lo, hi);
                });
            }
            hout = static_cast<char*>(h->hostOut.ensure(static_cast<size_t>(ocap) * C * es));
        }
        tr.add(0);
        std::vector<int64_t> got(h->groups.size());
        for (size_t gi = 0; gi < h->groups.size(); ++gi) {
            Group& g = h->groups[gi];
            InView iv;
            iv.n = n;
            iv.f64 = h->cf();
            iv.fs = 1;
            iv.cs = n;
            if (hin) iv.p = hin + static_cast<size_t>(g.c0) * n * es;
            OutView ov;
            ov.f64 = h->cf();
            ov.fs = 1;
            ov.cs = ocap;
            if (hout) ov.p = hout + static_cast<size_t>(g.c0) * ocap * es;
            gar_status st;
            got[gi] = runGroup(h, g, iv, ov, flush, h->stream, cap, st);
            if (st != GAR_OK) return st;
            for (int c = g.c0; c < g.c0 + g.C; ++c)
                if (n_out) n_out[c] = got[gi];
        }
        tr.add(1);
        if (!h->dry) {
            HIPCHK(hipStreamSynchronize(h->stream));
            tr.add(2);
            const int64_t gmax = got.empty() ? 0 : *std::max_element(got.begin(), got.end());
            forSlices(C, gmax, es + 8, [&](int c, int64_t lo, int64_t hi) {
                const int64_t m = got[groupOf(h, c) - h->groups.data()];
                if (lo < m) unpackChannel<double>(out[c], h->f64, hout + static_cast<size_t>(c) * ocap * es, lo, std::min(hi, m));
            });
            tr.add(3);
            trimHost(h);
        }
        return GAR_OK;
    }, true);
}

bool isPcm(int32_t t) { return t == GAR_PCM16 || t == GAR_PCM24 || t == GAR_PCM32 || t == GAR_PCM24_PACKED; }
bool isHalf(int32_t t) { return t == GAR_F16 || t == GAR_BF16; }
// sample types converted at the device entry points: integer PCM and f16 / bf16 (InView::pcm / OutView::pcm
// carry the ABI code, which is also launchConvert's code for them)
bool isNarrow(int32_t t) { return isPcm(t) || isHalf(t); }
bool ioTypeOk(int32_t t) { return t == GAR_F64 || t == GAR_F32 || t == GAR_F32_EXACT || isNarrow(t); }
// PCM / half conversion fused into hxs_kernel's loads and stores: one fused split-f16 stage streaming
// through the row-block kernel (hxsPlanFits); anything else stages the conversion.
bool pcmFusable(const Handle* h) {
    if (h->dry || h->f64 || !h->hx || h->stages.size() != 1 || h->groups.size() != 1) return false;
    const StageRT& st = *h->stages[0];
    if (!st.fused || h->groups[0].cnt.empty() || h->groups[0].cnt[0].staged) return false;
    const HxDev* hx = st.fusedD.hx;
    return hx && hx->hxsOk;
}

// A caller's device buffer: base, sample type, frame and channel stride.
struct DevIo {
    void* p;
    int32_t dtype;
    int64_t fs, cs;
};

// gar_process_device / gar_flush_device on the handle's one lockstep group (the arguments are
// checked); `in` is NULL and frames is 0 when flushing.
gar_status deviceCall(Handle* r, const DevIo* in, int64_t frames, const DevIo& out, int64_t out_cap, int64_t* out_frames,
                      void* stream) {
    const bool flush = !in;
    return callOn(r, static_cast<hipStream_t>(stream), [&]() -> gar_status {
        hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = legacy default stream
        const int C = r->channels;
        // packed 24-bit PCM is always staged (pack24_kernel / unpack24_kernel / convert_kernel): hxs_kernel has no
        // 3-byte load or store layout
        const bool fuseAny = pcmFusable(r);
        InView iv;
        if (in) {
            iv.p = in->p;
            iv.f64 = in->dtype == GAR_F64 ? 1 : 0;
            iv.fs = in->fs;
            iv.cs = in->cs;
            iv.n = frames;
            if (isNarrow(in->dtype)) {
                iv.f64 = 0;
                if (fuseAny && in->dtype != GAR_PCM24_PACKED) {
                    iv.pcm = in->dtype;
                } else if (!r->dry) {  // staged: PCM / half -> compute dtype, then the ordinary path
                    r->inStage.ensure(static_cast<size_t>(std::max<int64_t>(frames, 1)) * C * r->tc());
                    HIPCHK(launchConvert(in->p, in->dtype, in->fs, in->cs, r->inStage.p, r->cf(), C, 1, frames, C, s));
                    iv = InView::of(OutView::rows(r->inStage.p, C, r->cf()), frames);
                }
            }
        }
        // a flush that would leave the composite launch (fusedFlushQuirk) ends in kernels that store no PCM
        const bool fuse = fuseAny && out.dtype != GAR_PCM24_PACKED &&
                          !(flush && isNarrow(out.dtype) && fusedFlushQuirk(r, r->groups[0]));
        // dither of an integer PCM output: the position of the call's first frame is the group's samplesOut now
        Dither dz;
        if (r->ditherMode != GAR_DITHER_NONE && isPcm(out.dtype)) {
            dz.mode = r->ditherMode;
            dz.seedLo = static_cast<uint32_t>(r->ditherSeed);
            dz.seedHi = static_cast<uint32_t>(r->ditherSeed >> 32);
            dz.pos0 = r->groups[0].statOut;
        }
        OutView ov;
        ov.p = out.p;
        ov.f64 = out.dtype == GAR_F64 ? 1 : 0;
        ov.fs = out.fs;
        ov.cs = out.cs;
        const bool stageOut = isNarrow(out.dtype) && !fuse && !r->dry;
        if (isNarrow(out.dtype)) {
            ov.f64 = 0;
            if (fuse) {
                ov.pcm = out.dtype;
                ov.dz = dz;
            }
        }
        if (stageOut) {
            std::vector<int64_t> sz;
            const int64_t need = simulate(r, r->groups[0], frames, flush, sz);
            r->outStage.ensure(static_cast<size_t>(std::max<int64_t>(need, 1)) * C * r->tc());
            ov = OutView::rows(r->outStage.p, C, r->cf());
        }
        gar_status st;
        const int64_t got = runGroup(r, r->groups[0], iv, ov, flush, s, out_cap, st);
        if (st == GAR_OK && stageOut && got > 0)
            HIPCHK(launchConvert(r->outStage.p, r->cf(), C, 1, out.p, out.dtype, out.fs, out.cs, got, C, s, dz,
                                 (r->meterOn && isPcm(out.dtype)) ? static_cast<uint64_t*>(r->meterBuf.p) : nullptr));
        if (st == GAR_OK && out_frames) *out_frames = got;
        return st;
    });
}

// Zeroes the tallies of channels [ch0, ch0 + n) after the handle's enqueued work (gar_synchronize's wait), on the
// handle's own stream, and returns once that stream has done it: ordered before any later call whichever stream it
// uses, without a wait for anything else on the device.  Throws DevError.
void meterZero(Handle* h, int32_t ch0, int32_t n) {
    if (h->dry || !h->meterBuf.p || n <= 0) return;
    waitEnqueued(h);
    HIPCHK(hipMemsetAsync(static_cast<char*>(h->meterBuf.p) + 16 * static_cast<size_t>(ch0), 0, 16 * static_cast<size_t>(n), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
}

gar_status channelMismatch(const Handle* h, int32_t got) {
    setError("expected " + std::to_string(h->channels) + " channels, got " + std::to_string(got));
    return GAR_ERR_CHANNEL_MISMATCH;
}

}  // namespace
}  // namespace gar

// ===========================================================================
// C ABI
// ===========================================================================
using namespace gar;

extern "C" {

gar_status gar_config_validate(const gar_config* cfg) { return validate(cfg); }

gar_quality_spec gar_preset_spec(int32_t preset) { return presetSpec(preset); }

gar_status gar_new(gar_config* cfg, gar_resampler** out) { return newCommon(cfg, 1, out); }

gar_status gar_new_batch(gar_config* cfg, int32_t n_streams, gar_resampler** out) {
    return newCommon(cfg, n_streams, out);
}

gar_status gar_new_engine(double in_rate, double out_rate, int32_t preset, int32_t dtype, gar_resampler** out) {
    return newEngineCommon(in_rate, out_rate, presetToEngineQuality(preset), dtype, false, out);
}

gar_status gar_new_engine_quality(double in_rate, double out_rate, int32_t engine_quality, int32_t dtype,
                                  gar_resampler** out) {
    if (engine_quality < GAR_ENGINE_QUICK || engine_quality > GAR_ENGINE_32BIT) {
        if (out) *out = nullptr;
        return guard(GAR_ERR_INVALID_CONFIG, "unknown engine quality");
    }
    return newEngineCommon(in_rate, out_rate, static_cast<Quality>(engine_quality), dtype, false, out);
}

gar_status gar_new_engine_dry(double in_rate, double out_rate, int32_t preset, int32_t dtype, gar_resampler** out) {
    // Host-only engine (used by CPU tests of the stream-length state machine).
    return newEngineCommon(in_rate, out_rate, presetToEngineQuality(preset), dtype, true, out);
}

void gar_free(gar_resampler* r) {
    if (!r) return;
    DeviceGuard dg(r->dry ? -1 : r->device);
    try {
        if (r->stream) (void)hipStreamSynchronize(r->stream);
        drainOrder(r);
        if (r->orderEv) (void)hipEventDestroy(r->orderEv);
        for (auto& ev : r->events) {
            (void)hipEventDestroy(ev.a);
            (void)hipEventDestroy(ev.b);
        }
        for (auto& ev : r->evPool) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
        r->groups.clear();
        r->stages.clear();
        if (r->failEv) (void)hipEventDestroy(r->failEv);
        if (r->errHost) (void)hipHostFree(r->errHost);
        if (r->stream) (void)hipStreamDestroy(r->stream);
    } catch (...) {
    }
    delete r;
}

gar_status gar_synchronize(gar_resampler* r) {
    if (!r) return GAR_ERR_INVALID_ARGUMENT;
    if (r->dry) return GAR_OK;
    DeviceGuard dg(r->device);
    const gar_status st = wrap([&]() -> gar_status {
        waitEnqueued(r);
        return GAR_OK;
    });
    if (st != GAR_OK) {
        r->poisoned = true;
        return st;
    }
    if (devFault(r)) return GAR_ERR_DEVICE;
    if (r->poisoned) return guard(GAR_ERR_DEVICE, "handle unusable after an earlier device error; call Reset");
    return GAR_OK;
}

int64_t gar_state_size(const gar_resampler* r) { return r ? stateSize(r) : -1; }

gar_status gar_state_save(gar_resampler* r, void* buf, int64_t cap, int64_t* n_written) {
    if (n_written) *n_written = 0;
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (cap < 0 || (cap > 0 && !buf)) return guard(GAR_ERR_INVALID_ARGUMENT, "bad state buffer");
    return stateSave(r, buf, cap, n_written);
}

gar_status gar_state_load(gar_resampler* r, const void* buf, int64_t n) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    return stateLoad(r, buf, n);
}

int64_t gar_estimate_output(const gar_resampler* r, int64_t n) { return r ? estimate(r, n) : -1; }

int64_t gar_output_size(const gar_resampler* r, int32_t ch, int64_t n) {
    if (!r || ch < 0 || ch >= r->channels) return -1;
    gar_resampler* h = const_cast<gar_resampler*>(r);
    Group* g = groupOf(h, ch);
    std::vector<int64_t> s;
    return simulate(h, *g, n, false, s);
}

int64_t gar_flush_size(const gar_resampler* r, int32_t ch) {
    if (!r || ch < 0 || ch >= r->channels) return -1;
    gar_resampler* h = const_cast<gar_resampler*>(r);
    Group* g = groupOf(h, ch);
    std::vector<int64_t> s;
    return simulate(h, *g, 0, true, s);
}

gar_status gar_process_f64(gar_resampler* r, const double* in, int64_t n, double* out, int64_t cap, int64_t* n_out) {
    return monoCall<double>(r, 0, in, n, out, cap, n_out, false, false);
}
gar_status gar_process_f32(gar_resampler* r, const float* in, int64_t n, float* out, int64_t cap, int64_t* n_out) {
    return monoCall<float>(r, 0, in, n, out, cap, n_out, false, false);
}
gar_status gar_process_into_f64(gar_resampler* r, const double* in, int64_t n, double* out, int64_t cap,
                                int64_t* n_out) {
    return monoCall<double>(r, 0, in, n, out, cap, n_out, false, true);
}
gar_status gar_process_into_f32(gar_resampler* r, const float* in, int64_t n, float* out, int64_t cap,
                                int64_t* n_out) {
    return monoCall<float>(r, 0, in, n, out, cap, n_out, false, true);
}
gar_status gar_flush_f64(gar_resampler* r, double* out, int64_t cap, int64_t* n_out) {
    return monoCall<double>(r, 0, nullptr, 0, out, cap, n_out, true, false);
}
gar_status gar_flush_f32(gar_resampler* r, float* out, int64_t cap, int64_t* n_out) {
    return monoCall<float>(r, 0, nullptr, 0, out, cap, n_out, true, false);
}

gar_status gar_process_multi_f64(gar_resampler* r, const double* const* in, int32_t nch, int64_t n,
                                 double* const* out, int64_t cap, int64_t* n_out) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (nch != r->channels) return channelMismatch(r, nch);
    if (n < 0) return guard(GAR_ERR_INVALID_ARGUMENT, "negative length");
    return hostMulti(r, in, n, out, cap, n_out, false);
}

gar_status gar_flush_multi_f64(gar_resampler* r, double* const* out, int32_t nch, int64_t cap, int64_t* n_out) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (nch != r->channels) return guard(GAR_ERR_CHANNEL_MISMATCH, "channel count mismatch");
    return hostMulti(r, nullptr, 0, out, cap, n_out, true);
}

int64_t gar_device_output_size(const gar_resampler* r, int64_t frames) {
    if (!r || r->groups.size() != 1) return -1;
    gar_resampler* h = const_cast<gar_resampler*>(r);
    std::vector<int64_t> s;
    return simulate(h, h->groups[0], frames, false, s);
}

int64_t gar_device_flush_size(const gar_resampler* r) {
    if (!r || r->groups.size() != 1) return -1;
    gar_resampler* h = const_cast<gar_resampler*>(r);
    std::vector<int64_t> s;
    return simulate(h, h->groups[0], 0, true, s);
}

gar_status gar_process_device(gar_resampler* r, const void* in, int32_t in_dtype, int64_t in_fs, int64_t in_cs,
                              int64_t frames, int32_t channels, void* out, int32_t out_dtype, int64_t out_fs,
                              int64_t out_cs, int64_t out_cap, int64_t* out_frames, void* stream) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (out_frames) *out_frames = 0;
    if (channels != r->channels) return channelMismatch(r, channels);
    if (frames < 0) return guard(GAR_ERR_INVALID_ARGUMENT, "negative length");
    if (frames > 0 && !in) return guard(GAR_ERR_INVALID_ARGUMENT, "input is NULL");
    if (!ioTypeOk(in_dtype) || !ioTypeOk(out_dtype)) return guard(GAR_ERR_INVALID_ARGUMENT, "unknown sample type");
    if (r->groups.size() != 1) return guard(GAR_ERR_NOT_SUPPORTED, "channels are not in lockstep (per-channel calls were made)");
    const DevIo src{const_cast<void*>(in), in_dtype, in_fs, in_cs};
    return deviceCall(r, &src, frames, DevIo{out, out_dtype, out_fs, out_cs}, out_cap, out_frames, stream);
}

gar_status gar_flush_device(gar_resampler* r, int32_t channels, void* out, int32_t out_dtype, int64_t out_fs,
                            int64_t out_cs, int64_t out_cap, int64_t* out_frames, void* stream) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (out_frames) *out_frames = 0;
    if (channels != r->channels) return channelMismatch(r, channels);
    if (!ioTypeOk(out_dtype)) return guard(GAR_ERR_INVALID_ARGUMENT, "unknown sample type");
    if (r->groups.size() != 1) return guard(GAR_ERR_NOT_SUPPORTED, "channels are not in lockstep");
    return deviceCall(r, nullptr, 0, DevIo{out, out_dtype, out_fs, out_cs}, out_cap, out_frames, stream);
}

void gar_reset(gar_resampler* r) {
    if (!r) return;
    DeviceGuard dg(r->dry ? -1 : r->device);
    try {
        if (r->meterBuf.p && !r->poisoned) meterZero(r, 0, r->channels);  // the tallies describe what was stored since the last reset
    } catch (...) {
        // a device error here poisons nothing by itself: the next call meets it and the recovery path below, which
        // zeroes the tallies again once everything has drained
    }
    try {
        if (!r->dry) (void)devFault(r);  // a raised status word takes the recovery path (and is cleared there)
        if (r->poisoned) {  // recover: drain the handle's streams, fresh state
            // the failing call recorded no order event, and launches it already queued on its
            // caller stream may still read the histories and scratch freed below: drain the failing
            // call's stream through the event recorded on it (the caller may have destroyed it), then
            // the earlier calls (drainOrder: their order event, or -- a handle used on one stream
            // records none -- the whole device, gar.h gar_process_device)
            if (r->failEvValid) (void)hipEventSynchronize(r->failEv);
            if (r->stream) (void)hipStreamSynchronize(r->stream);
            drainOrder(r);
            (void)hipGetLastError();
            if (r->errHost) __atomic_store_n(r->errHost, 0, __ATOMIC_RELEASE);  // every launch that could write it has drained
            r->groups.clear();
            r->groups.push_back(freshGroup(r, 0, r->channels));
            if (r->meterBuf.p && r->stream) {  // everything has drained; done before the next call on any stream
                (void)hipMemsetAsync(r->meterBuf.p, 0, 16 * static_cast<size_t>(r->channels), r->stream);
                (void)hipStreamSynchronize(r->stream);
            }
            r->poisoned = false;
            r->failEvValid = false;
            r->orderValid = false;
            return;
        }
        // one group over every channel: reset in place, keeping its device buffers
        // (stream order covers kernels still reading them; no allocation, no sync)
        if (r->groups.size() == 1 && r->groups[0].c0 == 0 && r->groups[0].C == r->channels) {
            gar::Group& g = r->groups[0];
            freshCounters(r, g);
            for (auto& d : g.dev) {
                d.xh.clear();
                d.uh.clear();
            }
            g.statIn = g.statOut = 0;
            return;
        }
        if (r->stream) (void)hipStreamSynchronize(r->stream);
        drainOrder(r);
        r->groups.clear();
        r->groups.push_back(freshGroup(r, 0, r->channels));
    } catch (...) {
    }
}

double gar_get_ratio(const gar_resampler* r) { return r ? r->ratio : 0.0; }

int32_t gar_get_latency(const gar_resampler* r) {
    if (!r || r->stages.empty()) return 0;
    int tot = 0;
    for (const auto& s : r->stages) tot += static_cast<int>(static_cast<double>(stageLatency(s->d)) * s->d.ratio);
    return tot;
}

int32_t gar_channels(const gar_resampler* r) { return r ? r->channels : 0; }

gar_status gar_get_statistics(const gar_resampler* r, int32_t ch, int64_t* samples_in, int64_t* samples_out) {
    if (samples_in) *samples_in = 0;
    if (samples_out) *samples_out = 0;
    if (!r || ch < 0 || ch >= r->channels) return guard(GAR_ERR_INVALID_ARGUMENT, "channel out of range");
    const Group* g = groupOf(const_cast<gar_resampler*>(r), ch);
    if (!g) return guard(GAR_ERR_INTERNAL, "channel without a group");
    if (samples_in) *samples_in = g->statIn;
    if (samples_out) *samples_out = g->statOut;
    return GAR_OK;
}

gar_status gar_get_info(const gar_resampler* r, gar_info* info) {
    if (!r || !info) return GAR_ERR_INVALID_ARGUMENT;
    std::memset(info, 0, sizeof(*info));
    std::snprintf(info->algorithm, sizeof(info->algorithm), "%s", "multi-stage");
    info->latency = gar_get_latency(r);
    // MemoryUsage as the reference counts it for a fresh handle (constant.go:457-468), per channel:
    //  * every ring buffer's capacity in float64 -- defaultBufferSize 8192, buffer 0 sized
    //    MaxInputSize * bufferSizeMultiplier when set (constant.go:72-78, constants.go:55-57);
    //  * StageAdapter.GetMemoryUsage (stage_adapter.go:66-96) of each stage, whose elements are
    //    float64 on the New path (Resampler[float64], stages.go:63): the DFT pre-stage's
    //    factor x taps coefficients + history capacity taps * historyBufferMultiplier (2,
    //    dft_stage.go:142), the polyphase stage's `a` bank L x taps + history capacity 2 * taps
    //    (polyphase_stage.go:167); decimation stages are not counted.
    // The reference's history capacities then grow with use (appendStable, polyphase.go:36-44);
    // the device histories here are shared per group, so the figure stays the fresh one.
    const int64_t es = 8;
    int64_t perCh = 0;
    for (size_t j = 0; j <= r->stages.size(); ++j)
        perCh += (j == 0 && r->cfg.max_input_size > 0 ? r->cfg.max_input_size * 2 : 8192) * 8;
    for (const auto& s : r->stages) {
        const EngineDesign& d = s->d;
        if ((d.kind == EngineKind::DftOnly || d.kind == EngineKind::DftPoly) && d.dft.factor > 1)
            perCh += static_cast<int64_t>(d.dft.factor) * d.dft.taps * es + 2 * static_cast<int64_t>(d.dft.taps) * es;
        if (d.kind == EngineKind::DftPoly)
            perCh += static_cast<int64_t>(d.poly.L) * d.poly.taps * es + 2 * static_cast<int64_t>(d.poly.taps) * es;
    }
    info->memory_usage = perCh * r->channels;
    if (!r->stages.empty()) {
        const EngineDesign& d = r->stages[0]->d;
        int len = 0;
        if ((d.kind == EngineKind::DftOnly || d.kind == EngineKind::DftPoly) && d.dft.factor > 1) len += d.dft.taps * d.dft.factor;
        if (d.kind == EngineKind::DftPoly) len += d.poly.taps * d.poly.L;
        if (d.kind == EngineKind::Cubic) {
            // CubicStage: 4 points, no phases, no SIMD info (cubic.go:119-137)
            info->filter_length = 4;
            info->phases = 0;
            info->memory_usage += 64 * r->channels;  // cubicMemoryUsage (internal/engine/constants.go:15)
        } else {
            info->filter_length = len;
            info->phases = d.kind == EngineKind::DftPoly ? d.poly.L : 0;
            info->simd_enabled = 1;
            std::snprintf(info->simd_type, sizeof(info->simd_type), "%s", "gfx950 MFMA (HIP)");
        }
    }
    return GAR_OK;
}

const char* gar_status_string(gar_status s) {
    switch (s) {
        case GAR_OK: return "ok";
        case GAR_ERR_INVALID_CONFIG: return "invalid resampler configuration";
        case GAR_ERR_BUFFER_TOO_SMALL: return "output buffer too small";
        case GAR_ERR_NOT_SUPPORTED: return "operation not supported";
        case GAR_ERR_CHANNEL_MISMATCH: return "channel count mismatch";
        case GAR_ERR_DEVICE: return "device error";
        case GAR_ERR_INTERNAL: return "internal error";
        case GAR_ERR_INVALID_ARGUMENT: return "invalid argument";
    }
    return "unknown";
}

const char* gar_last_error(void) { return lastError(); }

void gar_profile_enable(gar_resampler* r, int32_t on) {
    if (!r) return;
    r->profile = on != 0;
}

gar_status gar_dev_half_convert(int32_t half_type, const double* in, int64_t n, uint16_t* from_f64, uint16_t* from_f32,
                                float* widened) {
    if (!isHalf(half_type) || n < 0 || (n > 0 && !in)) return guard(GAR_ERR_INVALID_ARGUMENT, "bad half conversion arguments");
    for (int64_t i = 0; i < n; ++i) {
        const uint16_t b = halfOfF64(in[i], half_type);
        if (from_f64) from_f64[i] = b;
        if (from_f32) from_f32[i] = halfOfF32(static_cast<float>(in[i]), half_type);
        if (widened) widened[i] = halfToF32(b, half_type);
    }
    return GAR_OK;
}

gar_status gar_set_dither(gar_resampler* r, int32_t mode, uint64_t seed) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (mode != GAR_DITHER_NONE && mode != GAR_DITHER_TPDF) return guard(GAR_ERR_INVALID_ARGUMENT, "unknown dither mode");
    static_assert(kDitherNone == GAR_DITHER_NONE && kDitherTpdf == GAR_DITHER_TPDF, "the kernels' dither modes are the ABI's");
    r->ditherMode = mode;
    r->ditherSeed = seed;
    return GAR_OK;
}

gar_status gar_set_meter(gar_resampler* r, int32_t on) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (on != 0 && on != 1) return guard(GAR_ERR_INVALID_ARGUMENT, "meter setting must be 0 or 1");
    if (on && !r->dry && !r->meterBuf.p) {  // [channels] x {clips, peak bits}, zeroed
        DeviceGuard dg(r->device);
        const gar_status st = wrap([&]() -> gar_status {
            r->meterBuf.ensure(16 * static_cast<size_t>(r->channels));
            HIPCHK(hipMemsetAsync(r->meterBuf.p, 0, 16 * static_cast<size_t>(r->channels), r->stream));
            HIPCHK(hipStreamSynchronize(r->stream));
            return GAR_OK;
        });
        if (st != GAR_OK) {
            r->meterBuf.release();
            return st;
        }
    }
    r->meterOn = on != 0;
    return GAR_OK;
}

gar_status gar_get_meter(const gar_resampler* r, int32_t* on) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (on) *on = r->meterOn ? 1 : 0;
    return GAR_OK;
}

gar_status gar_meter_read(gar_resampler* r, int32_t ch0, int32_t n_ch, uint64_t* clips, double* peak, int32_t reset) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (ch0 < 0 || n_ch < 0 || static_cast<int64_t>(ch0) + n_ch > r->channels)
        return guard(GAR_ERR_INVALID_ARGUMENT, "meter channel range outside the handle");
    const gar_status sy = gar_synchronize(r);  // the handle's enqueued calls; a raised status word: GAR_ERR_DEVICE
    if (sy != GAR_OK) return sy;
    std::vector<uint64_t> w(2 * static_cast<size_t>(n_ch), 0);
    if (!r->dry && r->meterBuf.p && n_ch > 0) {
        DeviceGuard dg(r->device);
        const gar_status st = wrap([&]() -> gar_status {
            HIPCHK(hipMemcpy(w.data(), static_cast<const char*>(r->meterBuf.p) + 16 * static_cast<size_t>(ch0), 16 * static_cast<size_t>(n_ch),
                             hipMemcpyDeviceToHost));
            if (reset) meterZero(r, ch0, n_ch);
            return GAR_OK;
        });
        if (st != GAR_OK) return st;
    }
    for (int32_t i = 0; i < n_ch; ++i) {
        if (clips) clips[i] = w[2 * i];
        if (peak) peak[i] = __builtin_bit_cast(double, w[2 * i + 1]);
    }
    return GAR_OK;
}

gar_status gar_dev_meter_tally(int32_t pcm_type, int32_t dither_mode, uint64_t seed, int32_t channel, int64_t position0,
                               const double* in, int64_t n, uint64_t* clips, double* peak) {
    if (!isPcm(pcm_type) || (dither_mode != GAR_DITHER_NONE && dither_mode != GAR_DITHER_TPDF) || n < 0 || (n > 0 && !in) || channel < 0)
        return guard(GAR_ERR_INVALID_ARGUMENT, "bad meter tally arguments");
    uint64_t total = 0, pk = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t c = 0;
        // what the kernels tally (meterTallyAt: the checked stores and the staged kernels call it as is)
        meterTallyAt(in[i], pcm_type, dither_mode, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32),
                     static_cast<uint32_t>(channel), static_cast<uint64_t>(position0) + static_cast<uint64_t>(i), c, pk);
        total += c;
    }
    if (clips) *clips = total;
    if (peak) *peak = __builtin_bit_cast(double, pk);
    return GAR_OK;
}

gar_status gar_get_dither(const gar_resampler* r, int32_t* mode, uint64_t* seed, int64_t* position) {
    if (!r) return guard(GAR_ERR_INVALID_ARGUMENT, "nil resampler");
    if (mode) *mode = r->ditherMode;
    if (seed) *seed = r->ditherSeed;
    if (position) *position = r->groups.size() == 1 ? r->groups[0].statOut : -1;
    return GAR_OK;
}

gar_status gar_dev_dither_quantize(int32_t pcm_type, uint64_t seed, int32_t channel, int64_t position0, const double* in,
                                   int64_t n, int32_t* out, double* noise) {
    if (!isPcm(pcm_type) || n < 0 || (n > 0 && !in && out) || channel < 0)
        return guard(GAR_ERR_INVALID_ARGUMENT, "bad dither quantizer arguments");
    const uint32_t lo = static_cast<uint32_t>(seed), hi = static_cast<uint32_t>(seed >> 32);
    const uint32_t key = ditherKey(lo, hi, static_cast<uint32_t>(channel));
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t p = static_cast<uint64_t>(position0) + static_cast<uint64_t>(i);
        if (noise) noise[i] = ditherNoise(ditherKeyHi(key, static_cast<uint32_t>(p >> 32)), static_cast<uint32_t>(p));
        // what the kernels store (pcmDitherAt: the checked stores and the staged kernels call it as is)
        if (out) out[i] = pcmDitherAt(in[i], pcm_type, lo, hi, static_cast<uint32_t>(channel), p);
    }
    return GAR_OK;
}

gar_status gar_dev_pcm24_convert(const double* in, int64_t n, uint8_t* packed, int32_t* unpacked) {
    if (n < 0 || (n > 0 && !in)) return guard(GAR_ERR_INVALID_ARGUMENT, "bad packed 24-bit conversion arguments");
    static_assert(kSampPcm24P == GAR_PCM24_PACKED, "the kernels' packed 24-bit code is the ABI's");
    for (int64_t i = 0; i < n; ++i) {
        uint8_t b[3];
        pcmWrite(b, 0, kSampPcm24P, in[i]);  // what convert_kernel / pack24_kernel store from f64
        if (packed) std::memcpy(packed + 3 * i, b, 3);
        if (unpacked) unpacked[i] = pcm24Load(b);
    }
    return GAR_OK;
}

namespace {
// The call description of the launch-plan entry points as the launchers' descriptors (addresses as integers).
void planDescs(int32_t in_type, int64_t in_fs, int64_t in_cs, uint64_t in_addr, int64_t in_base, int64_t in_len,
               int64_t valid_end, uint64_t hist_addr, int64_t hist_len, int64_t hist_ld, int32_t out_type, uint64_t out_addr,
               int64_t o0, int64_t out_fs, int64_t out_cs, int64_t o_lo, int64_t o_hi, SrcDesc& src, OutDesc& od) {
    src = SrcDesc{};
    src.hist = reinterpret_cast<const void*>(static_cast<uintptr_t>(hist_addr));
    src.hist_len = hist_len;
    src.hist_ld = hist_ld;
    src.in = reinterpret_cast<const void*>(static_cast<uintptr_t>(in_addr));
    src.in_base = in_base; src.in_len = in_len; src.in_fs = in_fs; src.in_cs = in_cs;
    src.in_f64 = in_type == GAR_F64;
    src.in_pcm = isNarrow(in_type) ? in_type : 0;
    src.valid_end = valid_end;
    od = OutDesc{};
    od.out = reinterpret_cast<void*>(static_cast<uintptr_t>(out_addr));
    od.o0 = o0; od.fs = out_fs; od.cs = out_cs;
    od.f64 = out_type == GAR_F64;
    od.pcm = isNarrow(out_type) ? out_type : 0;
    od.o_lo = o_lo; od.o_hi = o_hi;
}
}  // namespace

gar_status gar_dev_hxs_plan(const gar_resampler* r, int32_t stage, int32_t in_type, int64_t in_fs, int64_t in_cs,
                            uint64_t in_addr, int64_t in_base, int64_t in_len, int64_t valid_end, uint64_t hist_addr,
                            int64_t hist_len, int64_t hist_ld, int32_t out_type, uint64_t out_addr, int64_t o0,
                            int64_t out_fs, int64_t out_cs, int64_t o_lo, int64_t o_hi, int32_t channels,
                            int32_t cu_count, int64_t hist_keep, char* buf, int64_t cap) {
    if (!r || !buf || cap < 1 || stage < 0 || stage >= static_cast<int32_t>(r->stages.size()) || channels < 1 ||
        cu_count < 1 || !ioTypeOk(in_type) || !ioTypeOk(out_type))
        return guard(GAR_ERR_INVALID_ARGUMENT, "bad launch-plan arguments");
    const gar::StageRT& st = *r->stages[stage];
    const HxDev* hx = st.fusedD.hx ? st.fusedD.hx : (st.dftD.hx ? st.dftD.hx : st.decimD.hx);
    if (!hx) return guard(GAR_ERR_INVALID_ARGUMENT, "the stage has no split-f16 plan");
    SrcDesc src;
    OutDesc od;
    planDescs(in_type, in_fs, in_cs, in_addr, in_base, in_len, valid_end, hist_addr, hist_len, hist_ld, out_type, out_addr, o0,
              out_fs, out_cs, o_lo, o_hi, src, od);
    buf[0] = 0;
    if (o_hi <= o_lo) return GAR_OK;  // nothing to launch
    const gar::HxsLaunchPlan pl = gar::hxsPlanLaunch(*hx, src, od, channels, cu_count, gar::hxsReadKnobs(), hist_keep > 0, hist_keep);
    if (!pl.ok) std::snprintf(buf, static_cast<size_t>(cap), "not supported\n");
    else gar::hxsTraceLines(pl, od, channels, buf, static_cast<size_t>(cap));
    return GAR_OK;
}

gar_status gar_dev_fir_plan(const gar_resampler* r, int32_t stage, int32_t which, int32_t in_type, int64_t in_fs, int64_t in_cs,
                            uint64_t in_addr, int64_t in_base, int64_t in_len, int64_t valid_end, uint64_t hist_addr,
                            int64_t hist_len, int64_t hist_ld, int32_t out_type, uint64_t out_addr, int64_t o0,
                            int64_t out_fs, int64_t out_cs, int64_t o_lo, int64_t o_hi, int32_t channels,
                            int32_t cu_count, int64_t hist_keep, char* buf, int64_t cap) {
    if (!r || !buf || cap < 1 || stage < 0 || stage >= static_cast<int32_t>(r->stages.size()) || channels < 1 ||
        cu_count < 1 || which < 0 || which > 2 || !ioTypeOk(in_type) || !ioTypeOk(out_type))
        return guard(GAR_ERR_INVALID_ARGUMENT, "bad launch-plan arguments");
    const gar::StageRT& st = *r->stages[stage];
    BgDev p = which == 0 ? st.fusedD : (which == 1 ? st.dftD : st.decimD);
    if (p.Pc <= 0) return guard(GAR_ERR_INVALID_ARGUMENT, "the stage has no such FIR plan");
    // a dry-run handle uploads no tables: its row-block-aligned plans get the non-null table pointer they
    // have on a device (the planner tests it, nothing dereferences it)
    if (p.rbAligned && !p.rbStart) p.rbStart = p.hRbStart;
    SrcDesc src;
    OutDesc od;
    planDescs(in_type, in_fs, in_cs, in_addr, in_base, in_len, valid_end, hist_addr, hist_len, hist_ld, out_type, out_addr, o0,
              out_fs, out_cs, o_lo, o_hi, src, od);
    const gar::FirLaunchPlan pl = gar::firPlanLaunch(p, src, od, channels, cu_count, gar::firReadKnobs(), hist_keep > 0, hist_keep);
    gar::firTraceLines(pl, p, src, od, channels, buf, static_cast<size_t>(cap));
    return GAR_OK;
}

int64_t gar_dev_pool_selftest(int32_t threads, int32_t iters, int32_t channels, int64_t frames) {
    if (threads < 1 || iters < 0 || channels < 1 || frames < 0) return -1;
    std::atomic<int64_t> bad{0};
    // thread t uses channels + t channels, so consecutive jobs on the pool have different job
    // counts (whole-channel jobs for C >= 2 * workers, channel slices below) -- the case where a
    // stale ticket could claim an index of the next job
    auto body = [&](int t) {
        const int channels_t = channels + t;
        std::vector<double> src(static_cast<size_t>(channels_t) * frames), dst(src.size());
        std::vector<float> mid(src.size());
        for (size_t i = 0; i < src.size(); ++i) src[i] = static_cast<double>((i * 2654435761u + t) % 65536) / 65536.0 - 0.5;
        for (int k = 0; k < iters; ++k) {
            std::fill(dst.begin(), dst.end(), -9.0);
            forSlices(channels_t, frames, 12, [&](int c, int64_t lo, int64_t hi) {
                packChannel<double>(mid.data() + static_cast<size_t>(c) * frames, false,
                                    src.data() + static_cast<size_t>(c) * frames, lo, hi);
            });
            forSlices(channels_t, frames, 12, [&](int c, int64_t lo, int64_t hi) {
                unpackChannel<double>(dst.data() + static_cast<size_t>(c) * frames, false,
                                      mid.data() + static_cast<size_t>(c) * frames, lo, hi);
            });
            int64_t b = 0;
            for (size_t i = 0; i < src.size(); ++i) b += dst[i] != static_cast<double>(static_cast<float>(src[i]));
            bad += b;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < threads; ++t) th.emplace_back(body, t);
    body(0);
    for (auto& x : th) x.join();
    return bad.load();
}

void gar_profile_kinds(gar_resampler* r, uint32_t kinds) {
    if (!r) return;
    r->profileKinds = kinds & 0x3fu;
}

gar_status gar_stage_state(const gar_resampler* r, int32_t stage, int32_t* fused_plan, int32_t* fused_now) {
    if (!r || !fused_plan || !fused_now || stage < 0 || stage >= static_cast<int32_t>(r->stages.size()))
        return GAR_ERR_INVALID_ARGUMENT;
    const gar::StageRT& st = *r->stages[stage];
    *fused_plan = st.fused ? 1 : 0;
    const gar::Group* g = r->groups.empty() ? nullptr : &r->groups[0];
    *fused_now = (st.fused && g && !g->cnt[stage].staged) ? 1 : 0;
    return GAR_OK;
}

gar_status gar_stage_geometry(const gar_resampler* r, int32_t stage, double* stage_ratio, gar_engine_geometry* geom) {
    if (!r || !geom || stage < 0 || stage >= static_cast<int32_t>(r->stages.size())) return GAR_ERR_INVALID_ARGUMENT;
    const gar::EngineDesign& d = r->stages[stage]->d;
    fillGeometry(d, geom);
    if (stage_ratio) *stage_ratio = d.ratio;
    return GAR_OK;
}

int32_t gar_num_stages(const gar_resampler* r) { return r ? static_cast<int32_t>(r->stages.size()) : 0; }

gar_status gar_profile_read(gar_resampler* r, int32_t kind, double* ms, int64_t* launches) {
    if (!r || kind < 0 || kind > 5) return GAR_ERR_INVALID_ARGUMENT;
    DeviceGuard dg(r->dry ? -1 : r->device);
    return wrap([&]() -> gar_status {
        for (auto& ev : r->events) {
            HIPCHK(hipEventSynchronize(ev.b));
            float t = 0;
            HIPCHK(hipEventElapsedTime(&t, ev.a, ev.b));
            r->profiledMs[ev.tag] += t;
            r->profiledLaunches[ev.tag] += 1;
            r->launchMs[ev.tag].push_back(t);
            r->evPool.emplace_back(ev.a, ev.b);
        }
        r->events.clear();
        if (ms) *ms = r->profiledMs[kind];
        if (launches) *launches = r->profiledLaunches[kind];
        r->profiledMs[kind] = 0;
        r->profiledLaunches[kind] = 0;
        r->readMs[kind].swap(r->launchMs[kind]);
        r->launchMs[kind].clear();
        return GAR_OK;
    });
}

gar_status gar_profile_launch_stats(gar_resampler* r, int32_t kind, double* min_ms, double* median_ms, double* max_ms) {
    if (!r || kind < 0 || kind > 5) return GAR_ERR_INVALID_ARGUMENT;
    std::vector<float> v = r->readMs[kind];
    if (v.empty()) {
        if (min_ms) *min_ms = 0;
        if (median_ms) *median_ms = 0;
        if (max_ms) *max_ms = 0;
        return GAR_OK;
    }
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    if (min_ms) *min_ms = v.front();
    if (max_ms) *max_ms = v.back();
    if (median_ms) *median_ms = n % 2 ? v[n / 2] : 0.5 * (static_cast<double>(v[n / 2 - 1]) + v[n / 2]);
    return GAR_OK;
}

gar_status gar_design_engine(double in_rate, double out_rate, int32_t q, gar_engine_geometry* geom, double* dft,
                             double* pa, double* pb, double* pc, double* pd, double* decim) {
    EngineDesign d;
    std::string err;
    if (!designEngine(in_rate, out_rate, static_cast<Quality>(q), d, err)) return guard(GAR_ERR_INVALID_CONFIG, err.c_str());
    if (geom) fillGeometry(d, geom);
    if (dft && !d.dft.c.empty()) std::memcpy(dft, d.dft.c.data(), d.dft.c.size() * 8);
    if (pa && !d.poly.a.empty()) std::memcpy(pa, d.poly.a.data(), d.poly.a.size() * 8);
    if (pb && !d.poly.b.empty()) std::memcpy(pb, d.poly.b.data(), d.poly.b.size() * 8);
    if (pc && !d.poly.cc.empty()) std::memcpy(pc, d.poly.cc.data(), d.poly.cc.size() * 8);
    if (pd && !d.poly.d.empty()) std::memcpy(pd, d.poly.d.data(), d.poly.d.size() * 8);
    if (decim && !d.decim.c.empty()) std::memcpy(decim, d.decim.c.data(), d.decim.c.size() * 8);
    return GAR_OK;
}

gar_status gar_design_composite(double in_rate, double out_rate, int32_t q, double* rows, int64_t* offsets) {
    EngineDesign d;
    std::string err;
    if (!designEngine(in_rate, out_rate, static_cast<Quality>(q), d, err)) return guard(GAR_ERR_INVALID_CONFIG, err.c_str());
    FirPeriodic f;
    if (d.kind != EngineKind::DftPoly || !firComposite(d.dft, d.poly, f)) return guard(GAR_ERR_NOT_SUPPORTED, "no composite FIR");
    size_t w = 0;
    for (const auto& r : f.rows) w = std::max(w, r.size());
    for (int r = 0; r < f.P; ++r) {
        if (offsets) offsets[r] = f.off[r];
        if (rows)
            for (size_t k = 0; k < w; ++k) rows[r * w + k] = k < f.rows[r].size() ? f.rows[r][k] : 0.0;
    }
    return GAR_OK;
}

}  // extern "C"
