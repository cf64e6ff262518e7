// gar_engine.hpp -- internal types of the host engine and what its units need from each other (never
// installed; the interface is include/gar.h).  The units:
//   gar_counters.cpp  the reference's integer stream arithmetic (host only, no HIP)
//   gar_stage.cpp     stage construction: plans and banks of one engine design, uploaded
//   gar_engine.cpp    the run path: histories, stage / chain process and flush, groups, call plumbing
//   gar_state.cpp     state snapshots (blob layout, parser, save / load)
//   gar_abi.cpp       the C ABI: argument checks, constructors, host staging, the entry points
// Everything here has hidden visibility: none of it enters the library's dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "gar.h"
#include "gar_counters.hpp"
#include "gar_design.hpp"
#include "gar_kernels.hpp"
#include "gar_plan.hpp"

#pragma GCC visibility push(hidden)
namespace gar {

struct DevError {
    hipError_t e;
    std::string what;
};
#define HIPCHK(x)                                                   \
    do {                                                            \
        hipError_t e_ = (x);                                        \
        if (e_ != hipSuccess) throw DevError{e_, #x};               \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    void ensure(size_t bytes) {
        if (bytes <= cap) return;
        release();
        const size_t nb = bytes + bytes / 4 + 256;
        HIPCHK(hipMalloc(&p, nb));
        cap = nb;
    }
    template <class T>
    void upload(const std::vector<T>& v) {
        ensure(sizeof(T) * std::max<size_t>(v.size(), 1));
        if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    }
};

// ---------------------------------------------------------------------------
// Stage runtime: one engine design + its device plans, shared by all channels
// (the reference designs the same filters once per channel, constant.go:57-70).
// ---------------------------------------------------------------------------
struct StageRT {
    EngineDesign d;
    bool f64 = false;
    bool fused = false;
    FirPeriodic compositeFir;
    BgPlan fusedP, dftP, decimP;
    DevBuf fusedA, fusedT, dftA, dftT, decimA, decimT;
    struct BgX { DevBuf rows, nfList; } fusedX, dftX, decimX;  // a bg plan's exact rows and fix list (attachExact)
    DevBuf xBankA, xBankC;  // the two stages' banks of a composite: every plan's exact recompute (uploadExact)
    BgDev fusedD{}, dftD{}, decimD{};
    DevBuf pa, pb, pc, pd, pabcd;
    PolyDev polyD{};
    // split-f16 variants (f32 compute), referenced from the BgDev's .hx
    struct HxRT {
        HxPlan plan;
        DevBuf A, T, X, fix;  // X: the plan's exact rows (uploadExact)
        HxDev d{};
    } fusedH, dftH, decimH;

    int tc() const { return f64 ? 8 : 4; }  // bytes of a compute-type sample
    int cf() const { return f64 ? 1 : 0; }  // the kernels' flag of the compute type
};

// gar_stage.cpp: the plans and banks of s.d, uploaded unless `dry`.
bool buildStage(StageRT& s, bool f64, bool hx, bool dry, std::string& err);
void fillGeometry(const EngineDesign& d, gar_engine_geometry* geom);

struct Hist {
    DevBuf buf[2];
    int cur = 0;
    int64_t base = 0, len = 0;
    bool zero = false;  // rows known to be all zero (post-flush state); nothing stored
    void* ptr() const { return zero ? nullptr : buf[cur].p; }
    void clear() { base = 0; len = 0; zero = false; }
};

struct StageDev {
    Hist xh;  // stage input stream history
    Hist uh;  // poly-stream history (staged DFT+poly)
};

struct OutView {
    void* p = nullptr;
    int64_t fs = 0, cs = 0;
    int f64 = 0;
    int pcm = 0;  // integer PCM output bits, or GAR_F16 / GAR_BF16 (fused into hxs_kernel's stores)
    Dither dz;    // dither of a fused integer PCM store; dz.pos0 = stream position of the view's first frame
    // interleaved [t][C] rows of the compute type (histories, stage-boundary scratch, staged conversions)
    static OutView rows(void* p, int C, int cf) { return OutView{p, C, 1, cf, 0}; }
};

struct InView {
    const void* p = nullptr;
    int64_t fs = 0, cs = 0;
    int f64 = 0;
    int pcm = 0;  // integer PCM input bits, or GAR_F16 / GAR_BF16 (fused into hxs_kernel's loads; gar_process_device only)
    int64_t n = 0;
    bool zeros = false;
    // the first n frames a stage wrote through `o`, as the next stage's input
    static InView of(const OutView& o, int64_t n) {
        InView v;
        v.p = o.p; v.fs = o.fs; v.cs = o.cs; v.f64 = o.f64; v.n = n;
        return v;
    }
};

// Pinned host buffer the device reads in place (CubicStage checkpoints); reused only
// after the launch that read it has completed (event).
struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap), ev(o.ev), pending(o.pending) { o.p = nullptr; o.ev = nullptr; o.cap = 0; o.pending = false; }
    PinBuf& operator=(PinBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p; cap = o.cap; ev = o.ev; pending = o.pending;
            o.p = nullptr; o.ev = nullptr; o.cap = 0; o.pending = false;
        }
        return *this;
    }
    ~PinBuf() { release(); }
    void release() {
        if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); }
        if (p) (void)hipHostFree(p);
        p = nullptr; ev = nullptr; cap = 0; pending = false;
    }
    // Wait for the previous reader, grow if needed; returns the host pointer.
    void* acquire(size_t bytes) {
        if (pending) HIPCHK(hipEventSynchronize(ev));
        pending = false;
        if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (bytes > cap) {
            if (p) HIPCHK(hipHostFree(p));
            p = nullptr;
            cap = 0;
            const size_t nb = bytes + bytes / 2 + 4096;
            HIPCHK(hipHostMalloc(&p, nb, hipHostMallocDefault));
            cap = nb;
        }
        return p;
    }
    void issued(hipStream_t s) {
        HIPCHK(hipEventRecord(ev, s));
        pending = true;
    }
};

// Pinned host buffer the kernels read / write in place (the host C-ABI's staging: the caller's
// pageable arrays are packed into it on the host, the first stage's kernel reads it over PCIe and
// the last stage's kernel writes its outputs into the output one -- no DMA round trip per call).
// Used only between a launch and the stream synchronise of the same call.
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    unsigned flags = 0;
    HostBuf() = default;
    explicit HostBuf(unsigned f) : flags(f) {}
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() { release(); }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    void* ensure(size_t bytes) {
        if (bytes <= cap) return p;
        release();
        const size_t nb = bytes + bytes / 4 + 4096;
        HIPCHK(hipHostMalloc(&p, nb, hipHostMallocMapped | flags));
        cap = nb;
        return p;
    }
};

struct Group {
    int c0 = 0, C = 1;
    std::vector<Counters> cnt;
    // engine.Resampler.GetStatistics counters per channel (resampler.go:187-195,270,320,338-339):
    // samples in per non-empty Process, samples out per Process and Flush, zeroed by Reset
    int64_t statIn = 0, statOut = 0;
    std::vector<StageDev> dev;
    std::vector<DevBuf> tmp;   // per stage-boundary output buffers
    DevBuf utmp;               // staged DFT output (u) scratch
    PinBuf cubPin[2];          // CubicStage checkpoints, double-buffered
    int cubCur = 0;
    std::vector<CubicSeg> cubSegs;
};

}  // namespace gar

struct gar_resampler {
    bool newPath = true;
    int channels = 1;      // total (streams * channels for a batch)
    double ratio = 1.0;
    bool f64 = true;       // compute dtype
    bool hx = false;       // f32 compute on the split-f16 MFMA kernel (GAR_F32) instead of exact-f32 MFMA
    bool dry = false;
    int device = 0;
    bool engineF32Io = false;
    hipStream_t stream = nullptr;
    // cross-stream ordering: every call's work is recorded on orderEv; a call on another
    // stream waits for it first, so one handle's launches never overlap (they share
    // histories, scratch and the fix lists)
    hipEvent_t orderEv = nullptr;
    hipStream_t lastStream = nullptr;
    bool orderValid = false;
    // Recording orderEv costs ~3.5 us of stream time per call (r05f trace: dispatch gaps 7.9 / 8.2 ->
    // 4.3 / 5.8 us without it), so a handle used on one stream only records none: `unordered` marks
    // device work not covered by an event.  The first call on a second stream waits for the device
    // once and turns `multiStream` on; from then on every call records the event.
    bool unordered = false;
    bool multiStream = false;
    // a HIP failure mid-call may leave counters advanced past the histories: refuse
    // further work until Reset (ADVICE: no silent wrong output)
    bool poisoned = false;
    hipEvent_t failEv = nullptr;  // recorded on the failing call's stream (the caller may destroy that stream)
    bool failEvValid = false;
    // device status word (pinned, host-mapped): a kernel that detects a broken invariant of its own
    // (hxt_kernel: an expired progress wait) writes a nonzero code; every ABI call checks it first
    int* errHost = nullptr;
    int* errDev = nullptr;
    gar_config cfg{};
    std::vector<std::unique_ptr<gar::StageRT>> stages;
    std::vector<gar::Group> groups;
    gar::DevBuf inStage, outStage;
    // state snapshots (gar_state_save / gar_state_load): what the constructor was asked for (the blob's
    // fingerprint; the engine constructors keep no gar_config), the device row image and segment table
    // gar_set_dither: configuration (not stream state, not in the state blob); the position is the group's statOut
    int32_t ditherMode = GAR_DITHER_NONE;
    uint64_t ditherSeed = 0;
    // gar_set_meter: configuration like dither; meterBuf = [channels] x {uint64 clips, uint64 peak bits} in device
    // memory, allocated when the meter is first turned on, zeroed by gar_reset and by gar_meter_read's reset
    bool meterOn = false;
    gar::DevBuf meterBuf;
    double fpInRate = 0, fpOutRate = 0;
    int32_t fpQuality = 0;  // engine.Quality of the engine constructors
    gar::DevBuf stateImg, stateTab;
    // host C-ABI staging: pinned, mapped; input write-combined (the host only writes it)
    gar::HostBuf hostIn{hipHostMallocWriteCombined | hipHostMallocCoherent}, hostOut{hipHostMallocCoherent};
    std::vector<int64_t> scratchSizes;
    // optional HIP-event timing of the MFMA FIR launches (bench.py roofline)
    bool profile = false;
    uint32_t profileKinds = 0x3f;  // kinds whose launches get events (gar_profile_kinds)
    struct Ev { int tag; hipEvent_t a, b; };
    std::vector<Ev> events;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evPool;
    double profiledMs[6] = {0, 0, 0, 0, 0, 0};
    int64_t profiledLaunches[6] = {0, 0, 0, 0, 0, 0};
    std::vector<float> launchMs[6], readMs[6];  // per-launch ms since the last read / of the last read

    int tc() const { return f64 ? 8 : 4; }  // bytes of a compute-type sample
    int cf() const { return f64 ? 1 : 0; }  // the kernels' flag of the compute type
};

namespace gar {

using Handle = gar_resampler;

// ---- gar_engine.cpp: the run path ----

// The calling thread's gar_last_error text; guard() sets it for any status but GAR_OK.
void setError(std::string msg);
const char* lastError();
gar_status guard(gar_status s, const char* msg);

Group* groupOf(Handle* h, int ch);
// The counters of a stream that has seen nothing (a stage without a composite plan starts staged).
void freshCounters(const Handle* h, Group& g);
Group freshGroup(Handle* h, int c0, int C);
// Gives channel `ch` a group of its own (Process on one channel advances only that channel).
void isolate(Handle* h, int ch);
// Dry-run a process (or flush) on copies of the group counters.
int64_t simulate(Handle* h, Group& g, int64_t n, bool flush, std::vector<int64_t>& sizes);
// True when a flush of the group's fused DFT+polyphase stage would leave the composite launch for the staged
// kernels (the polyphase history quirk), which store no PCM: such a flush stages its PCM conversion.
bool fusedFlushQuirk(const Handle* h, const Group& g);
// Run one group for real: sizes first (so scratch can be sized), then launches.
int64_t runGroup(Handle* h, Group& g, const InView& in, const OutView& out, bool flush, hipStream_t s, int64_t cap,
                 gar_status& st);

// Makes the handle's device current for one call and restores the caller's.
struct DeviceGuard {
    int prev = -1;
    bool set = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != dev && hipSetDevice(dev) == hipSuccess) set = true;
    }
    ~DeviceGuard() {
        if (set) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// While one lives, the kernels launched by this thread report into status word `e` (OutDesc::err).
struct ErrScope {
    int* prev;
    explicit ErrScope(int* e);
    ~ErrScope();
    ErrScope(const ErrScope&) = delete;
    ErrScope& operator=(const ErrScope&) = delete;
};

// The exception in flight as a status and an error text: DevError and std::bad_alloc; anything else
// goes on.  `launchLimit` (when given) is set when it was a launch the device cannot run.
gar_status caught(bool* launchLimit);

template <class F>
gar_status wrap(F&& f, bool* launchLimit = nullptr) {
    try {
        return f();
    } catch (...) {
        return caught(launchLimit);
    }
}

// A kernel of an earlier (asynchronous) call raised the handle's device status word: the outputs of
// that call are not the reference's, so the handle is poisoned until Reset (no silent wrong output).
bool devFault(Handle* h);
// Waits until no device work of the handle's calls is pending (free / reset / synchronize): the
// order event when one covers the last call, else -- work of single-stream calls left no event --
// the device (the caller's stream may already be destroyed).
void drainOrder(Handle* h);
// The same wait for a call that reports a failure of it (gar_synchronize, gar_state_save / gar_state_load):
// throws DevError, and waits for the handle's own stream (the host calls' and the snapshots' work) too.
void waitEnqueued(Handle* h);

// One ABI call that touches the device: handle's device current, ordered after
// the handle's previous call (any stream), recorded for the next; a device
// error poisons the handle until Reset.
template <class F>
gar_status callOn(Handle* h, hipStream_t s, F&& f, bool hostSynced = false) {
    if (h->poisoned) return guard(GAR_ERR_DEVICE, "handle unusable after an earlier device error; call Reset");
    if (h->dry) return wrap(f);
    if (devFault(h)) return GAR_ERR_DEVICE;
    DeviceGuard dg(h->device);
    ErrScope es(h->errDev);
    bool launchLimit = false;
    gar_status st = wrap([&]() -> gar_status {
        if (h->orderValid && h->lastStream != s) {
            HIPCHK(hipStreamWaitEvent(s, h->orderEv, 0));
        } else if (h->unordered && h->lastStream != s) {  // first switch of stream: earlier calls left no event
            HIPCHK(hipDeviceSynchronize());
            h->unordered = false;
            h->multiStream = true;
        }
        const gar_status r = f();
        if (hostSynced) {  // the call synchronised its stream: nothing of it is left to order after
            h->orderValid = false;
            h->unordered = false;
        } else if (h->multiStream) {
            HIPCHK(hipEventRecord(h->orderEv, s));
            h->lastStream = s;
            h->orderValid = true;
        } else {
            h->lastStream = s;
            h->orderValid = false;
            h->unordered = true;
        }
        return r;
    }, &launchLimit);
    if (st == GAR_ERR_DEVICE || (st == GAR_ERR_INVALID_ARGUMENT && launchLimit)) {  // state may be half-updated
        h->poisoned = true;
        // drained by Reset through an event: the caller may destroy `s` after the failed call
        h->failEvValid = h->failEv && hipEventRecord(h->failEv, s) == hipSuccess;
    } else if (st == GAR_OK && hostSynced && devFault(h)) {  // this call's own kernels reported
        st = GAR_ERR_DEVICE;
    }
    return st;
}

// ---- gar_state.cpp: state snapshots (argument checks are the entry points') ----
int64_t stateSize(const Handle* h);
gar_status stateSave(Handle* h, void* buf, int64_t cap, int64_t* nWritten);
gar_status stateLoad(Handle* h, const void* buf, int64_t n);

}  // namespace gar
#pragma GCC visibility pop
