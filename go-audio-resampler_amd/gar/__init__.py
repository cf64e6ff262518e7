"""gar -- Python mirror of go-audio-resampler's public API over the MI355X engine.

Names, argument meaning and error behaviour follow the Go package `resampler`
(/root/reference resample.go, constant.go, convenience.go) so the parity tests
read like the reference's own tests.  Every sample operation runs in
libgar.so's HIP kernels; there is no CPU fallback -- importing this module
without the built library raises immediately.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GAR_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "libgar.so")  # override: A/B builds

# resampler.QualityPreset (resample.go:104-131)
QualityQuick, QualityLow, QualityMedium, QualityHigh, QualityVeryHigh, QualityCustom = range(6)
# engine.Quality (internal/engine/filter_params.go:16-41)
(EngineQuick, EngineLow, EngineMedium, EngineHigh, EngineVeryHigh,
 Engine16Bit, Engine20Bit, Engine24Bit, Engine28Bit, Engine32Bit) = range(10)
F64, F32, F32_EXACT = 0, 1, 2

GAR_OK, INVALID_CONFIG, BUFFER_TOO_SMALL, NOT_SUPPORTED, CHANNEL_MISMATCH, DEVICE, INTERNAL, INVALID_ARGUMENT = range(8)


class ResamplerError(Exception):
    code = -1


class ErrInvalidConfig(ResamplerError):   # resample.go:158
    code = INVALID_CONFIG


class ErrBufferTooSmall(ResamplerError):  # resample.go:161
    code = BUFFER_TOO_SMALL


class ErrNotSupported(ResamplerError):    # resample.go:164
    code = NOT_SUPPORTED


class ErrChannelMismatch(ResamplerError):
    code = CHANNEL_MISMATCH


class ErrDevice(ResamplerError):
    code = DEVICE


class ErrInternal(ResamplerError):
    code = INTERNAL


_ERRS = {c.code: c for c in (ErrInvalidConfig, ErrBufferTooSmall, ErrNotSupported, ErrChannelMismatch,
                             ErrDevice, ErrInternal)}


class QualitySpec(C.Structure):
    _fields_ = [("Preset", C.c_int32), ("Precision", C.c_int32), ("PhaseResponse", C.c_double),
                ("PassbandEnd", C.c_double), ("StopbandBegin", C.c_double), ("Flags", C.c_uint32)]


class _Config(C.Structure):
    _fields_ = [("InputRate", C.c_double), ("OutputRate", C.c_double), ("Channels", C.c_int32),
                ("Quality", QualitySpec), ("MaxInputSize", C.c_int64), ("EnableSIMD", C.c_int32),
                ("EnableParallel", C.c_int32), ("ComputeDtype", C.c_int32), ("Device", C.c_int32),
                ("DryRun", C.c_int32)]


class Info(C.Structure):
    _fields_ = [("Algorithm", C.c_char * 32), ("FilterLength", C.c_int32), ("Phases", C.c_int32),
                ("Latency", C.c_int32), ("MemoryUsage", C.c_int64), ("SIMDEnabled", C.c_int32),
                ("SIMDType", C.c_char * 48)]


class EngineGeometry(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dft_factor", C.c_int32), ("dft_taps", C.c_int32),
                ("poly_phases", C.c_int32), ("poly_taps", C.c_int32), ("poly_step", C.c_int64),
                ("decim_factor", C.c_int32), ("decim_taps", C.c_int32), ("fused", C.c_int32),
                ("fir_period_out", C.c_int32), ("fir_period_in", C.c_int32), ("fir_taps_max", C.c_int32),
                ("useful_macs_per_output", C.c_double), ("mfma_macs_per_output", C.c_double)]


EXPORTED = [
    "gar_config_validate", "gar_preset_spec", "gar_new", "gar_new_batch", "gar_new_engine", "gar_new_engine_quality", "gar_new_engine_dry", "gar_free",
    "gar_estimate_output", "gar_output_size", "gar_flush_size", "gar_process_f64", "gar_process_f32",
    "gar_process_into_f64", "gar_process_into_f32", "gar_process_multi_f64", "gar_flush_f64", "gar_flush_f32",
    "gar_flush_multi_f64", "gar_process_device", "gar_flush_device", "gar_device_output_size",
    "gar_device_flush_size", "gar_reset", "gar_get_ratio", "gar_get_latency", "gar_get_info", "gar_channels",
    "gar_status_string", "gar_last_error", "gar_design_engine", "gar_design_composite", "gar_profile_enable",
    "gar_profile_read", "gar_stage_state", "gar_num_stages", "gar_stage_geometry", "gar_get_statistics",
    "gar_synchronize", "gar_profile_launch_stats", "gar_profile_kinds", "gar_dev_half_convert",
    "gar_dev_pcm24_convert", "gar_dev_hxs_plan", "gar_dev_fir_plan", "gar_state_size", "gar_state_save", "gar_state_load",
    "gar_set_dither", "gar_get_dither", "gar_dev_dither_quantize",
    "gar_set_meter", "gar_get_meter", "gar_meter_read", "gar_dev_meter_tally",
]

_lib = None


def lib():
    """Load libgar.so (raises if the HIP library was not built -- no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libgar.so not built ({LIB_PATH}); run __graft_entry__.build()")
    # One HIP runtime per process: libgar.so and torch both depend on the
    # soname libamdhip64.so.7, and whichever is loaded first serves both.  Load
    # torch's first (it carries its own libhsa-runtime64) so the two stay in
    # step; the standalone C ABI (cgo) simply uses the system ROCm.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, d, dp = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.POINTER(C.c_double)
    sig = {
        "gar_config_validate": (i32, [C.POINTER(_Config)]),
        "gar_preset_spec": (QualitySpec, [i32]),
        "gar_new": (i32, [C.POINTER(_Config), C.POINTER(vp)]),
        "gar_new_batch": (i32, [C.POINTER(_Config), i32, C.POINTER(vp)]),
        "gar_new_engine": (i32, [d, d, i32, i32, C.POINTER(vp)]),
        "gar_new_engine_quality": (i32, [d, d, i32, i32, C.POINTER(vp)]),
        "gar_new_engine_dry": (i32, [d, d, i32, i32, C.POINTER(vp)]),
        "gar_free": (None, [vp]),
        "gar_estimate_output": (i64, [vp, i64]),
        "gar_output_size": (i64, [vp, i32, i64]),
        "gar_flush_size": (i64, [vp, i32]),
        "gar_process_f64": (i32, [vp, vp, i64, vp, i64, C.POINTER(i64)]),
        "gar_process_f32": (i32, [vp, vp, i64, vp, i64, C.POINTER(i64)]),
        "gar_process_into_f64": (i32, [vp, vp, i64, vp, i64, C.POINTER(i64)]),
        "gar_process_into_f32": (i32, [vp, vp, i64, vp, i64, C.POINTER(i64)]),
        "gar_process_multi_f64": (i32, [vp, vp, i32, i64, vp, i64, vp]),
        "gar_flush_f64": (i32, [vp, vp, i64, C.POINTER(i64)]),
        "gar_flush_f32": (i32, [vp, vp, i64, C.POINTER(i64)]),
        "gar_flush_multi_f64": (i32, [vp, vp, i32, i64, vp]),
        "gar_process_device": (i32, [vp, vp, i32, i64, i64, i64, i32, vp, i32, i64, i64, i64, C.POINTER(i64), vp]),
        "gar_flush_device": (i32, [vp, i32, vp, i32, i64, i64, i64, C.POINTER(i64), vp]),
        "gar_device_output_size": (i64, [vp, i64]),
        "gar_device_flush_size": (i64, [vp]),
        "gar_reset": (None, [vp]),
        "gar_get_ratio": (d, [vp]),
        "gar_get_latency": (i32, [vp]),
        "gar_get_info": (i32, [vp, C.POINTER(Info)]),
        "gar_channels": (i32, [vp]),
        "gar_status_string": (C.c_char_p, [i32]),
        "gar_last_error": (C.c_char_p, []),
        "gar_design_engine": (i32, [d, d, i32, C.POINTER(EngineGeometry), vp, vp, vp, vp, vp, vp]),
        "gar_design_composite": (i32, [d, d, i32, vp, vp]),
        "gar_profile_enable": (None, [vp, i32]),
        "gar_profile_read": (i32, [vp, i32, C.POINTER(d), C.POINTER(i64)]),
        "gar_stage_state": (i32, [vp, i32, C.POINTER(i32), C.POINTER(i32)]),
        "gar_num_stages": (i32, [vp]),
        "gar_stage_geometry": (i32, [vp, i32, C.POINTER(d), C.POINTER(EngineGeometry)]),
        "gar_get_statistics": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i64)]),
        "gar_synchronize": (i32, [vp]),
        "gar_profile_kinds": (None, [vp, C.c_uint32]),
        "gar_profile_launch_stats": (i32, [vp, i32, C.POINTER(d), C.POINTER(d), C.POINTER(d)]),
        "gar_dev_half_convert": (i32, [i32, vp, i64, vp, vp, vp]),
        "gar_dev_pcm24_convert": (i32, [vp, i64, vp, vp]),
        "gar_dev_hxs_plan": (i32, [vp, i32, i32, i64, i64, C.c_uint64, i64, i64, i64, C.c_uint64, i64, i64, i32, C.c_uint64,
                                   i64, i64, i64, i64, i64, i32, i32, i64, C.c_char_p, i64]),
        "gar_dev_fir_plan": (i32, [vp, i32, i32, i32, i64, i64, C.c_uint64, i64, i64, i64, C.c_uint64, i64, i64, i32, C.c_uint64,
                                   i64, i64, i64, i64, i64, i32, i32, i64, C.c_char_p, i64]),
        "gar_state_size": (i64, [vp]),
        "gar_state_save": (i32, [vp, vp, i64, C.POINTER(i64)]),
        "gar_state_load": (i32, [vp, vp, i64]),
        "gar_set_dither": (i32, [vp, i32, C.c_uint64]),
        "gar_get_dither": (i32, [vp, C.POINTER(i32), C.POINTER(C.c_uint64), C.POINTER(i64)]),
        "gar_dev_dither_quantize": (i32, [i32, C.c_uint64, i32, i64, vp, i64, vp, vp]),
        "gar_set_meter": (i32, [vp, i32]),
        "gar_get_meter": (i32, [vp, C.POINTER(i32)]),
        "gar_meter_read": (i32, [vp, i32, i32, vp, vp, i32]),
        "gar_dev_meter_tally": (i32, [i32, i32, C.c_uint64, i32, i64, vp, i64, C.POINTER(C.c_uint64), C.POINTER(d)]),
    }
    ab = os.environ.get("GAR_LIB_PATH") is not None
    for name, (res, args) in sig.items():
        if ab and not hasattr(L, name):  # development A/B against an older build: entry points it lacks are no-ops
            setattr(L, name, lambda *a, _r=res: None if _r is None else 0)
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc):
    if rc != GAR_OK:
        msg = lib().gar_last_error().decode(errors="replace")
        err = _ERRS.get(rc, ResamplerError)(msg or lib().gar_status_string(rc).decode())
        err.code = rc  # the plain ResamplerError of a status without a class of its own carries it too
        raise err


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else C.c_void_p(0)


def Config(InputRate, OutputRate, Channels=1, Quality=None, MaxInputSize=0, EnableSIMD=True,
           EnableParallel=False, ComputeDtype=F64, Device=0, DryRun=False):
    """resampler.Config (resample.go:46-73) plus engine extensions."""
    c = _Config()
    c.InputRate, c.OutputRate, c.Channels = float(InputRate), float(OutputRate), int(Channels)
    if Quality is None:
        Quality = QualitySpec(Preset=QualityHigh)
    elif isinstance(Quality, int):
        Quality = QualitySpec(Preset=Quality)
    c.Quality = Quality
    c.MaxInputSize, c.EnableSIMD, c.EnableParallel = int(MaxInputSize), int(EnableSIMD), int(EnableParallel)
    c.ComputeDtype, c.Device, c.DryRun = int(ComputeDtype), int(Device), int(bool(DryRun))
    return c


def GetPresetSpec(preset):
    return lib().gar_preset_spec(preset)


class Resampler:
    """resampler.Resampler (resample.go:14-43) + ProcessInto/EstimateOutput/FlushMulti."""

    def __init__(self, handle, f32_io=False):
        self._h = C.c_void_p(handle)
        self._f32_io = f32_io
        # bound now: at interpreter exit the module globals (lib) may already be torn down
        self._free = lib().gar_free

    def __del__(self):
        h = getattr(self, "_h", None)
        free = getattr(self, "_free", None)
        if h is not None and h.value and free is not None:
            free(h)
            self._h = None

    # -- streaming, channel 0 --
    def Process(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = lib().gar_output_size(self._h, 0, len(x))
        out = np.empty(max(n, 1))
        got = C.c_int64(0)
        _check(lib().gar_process_f64(self._h, _p(x), len(x), _p(out), len(out), C.byref(got)))
        return out[: got.value].copy()

    def ProcessFloat32(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        n = lib().gar_output_size(self._h, 0, len(x))
        out = np.empty(max(n, 1), dtype=np.float32)
        got = C.c_int64(0)
        _check(lib().gar_process_f32(self._h, _p(x), len(x), _p(out), len(out), C.byref(got)))
        return out[: got.value].copy()

    def ProcessInto(self, x, out):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous
        got = C.c_int64(0)
        _check(lib().gar_process_into_f64(self._h, _p(x), len(x), _p(out), len(out), C.byref(got)))
        return got.value

    def ProcessFloat32Into(self, x, out):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous
        got = C.c_int64(0)
        _check(lib().gar_process_into_f32(self._h, _p(x), len(x), _p(out), len(out), C.byref(got)))
        return got.value

    def EstimateOutput(self, n):
        return lib().gar_estimate_output(self._h, n)

    def OutputSize(self, n, channel=0):
        return lib().gar_output_size(self._h, channel, n)

    def FlushSize(self, channel=0):
        return lib().gar_flush_size(self._h, channel)

    def ProcessMulti(self, xs):
        nch = len(xs)
        n = len(xs[0]) if nch else 0
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
        if any(len(a) != n for a in arrs):
            raise ValueError("ProcessMulti requires equal channel lengths")
        cap = max([lib().gar_output_size(self._h, c, n) for c in range(self.Channels)] + [1]) if nch == self.Channels else 1
        outs = [np.empty(cap) for _ in range(nch)]
        inp = (C.c_void_p * max(nch, 1))(*[_p(a) for a in arrs])
        outp = (C.c_void_p * max(nch, 1))(*[_p(o) for o in outs])
        counts = np.zeros(max(nch, 1), dtype=np.int64)
        _check(lib().gar_process_multi_f64(self._h, inp, nch, n, outp, cap, _p(counts)))
        return [o[: counts[c]].copy() for c, o in enumerate(outs)]

    def Flush(self):
        n = lib().gar_flush_size(self._h, 0)
        out = np.empty(max(n, 1), dtype=np.float32 if self._f32_io else np.float64)
        got = C.c_int64(0)
        fn = lib().gar_flush_f32 if self._f32_io else lib().gar_flush_f64
        _check(fn(self._h, _p(out), len(out), C.byref(got)))
        return out[: got.value].copy()

    def FlushMulti(self):
        nch = self.Channels
        cap = max([lib().gar_flush_size(self._h, c) for c in range(nch)] + [1])
        outs = [np.empty(cap) for _ in range(nch)]
        outp = (C.c_void_p * nch)(*[_p(o) for o in outs])
        counts = np.zeros(nch, dtype=np.int64)
        _check(lib().gar_flush_multi_f64(self._h, outp, nch, cap, _p(counts)))
        return [o[: counts[c]].copy() for c, o in enumerate(outs)]

    def Reset(self):
        lib().gar_reset(self._h)

    def GetRatio(self):
        return lib().gar_get_ratio(self._h)

    def GetLatency(self):
        return lib().gar_get_latency(self._h)

    def GetStatistics(self, channel=0):
        """engine.Resampler.GetStatistics (internal/engine/resampler.go:348-353)."""
        a, b = C.c_int64(0), C.c_int64(0)
        _check(lib().gar_get_statistics(self._h, channel, C.byref(a), C.byref(b)))
        return {"samplesIn": a.value, "samplesOut": b.value}

    def GetInfo(self):
        info = Info()
        _check(lib().gar_get_info(self._h, C.byref(info)))
        return info

    def profile(self, on=True, kinds=None):
        """HIP-event timing of the FIR launches; `kinds` (iterable of kind numbers) limits it."""
        lib().gar_profile_enable(self._h, int(on))
        lib().gar_profile_kinds(self._h, 0x3F if kinds is None else sum(1 << k for k in kinds))

    def profile_read(self, kind=0):
        """(total ms, launches) of one kernel kind (0 fused FIR, 1 DFT FIR, 2 decimator FIR, 3 fused FIR
        of a flush, 4 polyphase with cubic coefficients, 5 cubic stage) since the last read."""
        ms, n = C.c_double(0), C.c_int64(0)
        _check(lib().gar_profile_read(self._h, kind, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_launch_stats(self, kind=0):
        """(min, median, max) ms per launch of the launches the last profile_read(kind) summed."""
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        _check(lib().gar_profile_launch_stats(self._h, kind, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def synchronize(self):
        """Wait for the handle's enqueued device work; raises ResamplerError (GAR_ERR_DEVICE) when a
        kernel reported a broken invariant (gar.h gar_synchronize)."""
        _check(lib().gar_synchronize(self._h))

    # -- state snapshots (gar.h gar_state_size / gar_state_save / gar_state_load) --
    def state_size(self):
        """Bytes save_state() would return now."""
        return lib().gar_state_size(self._h)

    def save_state(self, cap=None):
        """The handle's streaming state (groups, counters, histories, statistics) as bytes, after every
        enqueued call has run.  `cap` (default: state_size()) is the buffer offered; one too small
        raises ErrBufferTooSmall whose `needed` attribute is the size required."""
        cap = self.state_size() if cap is None else int(cap)
        buf = (C.c_ubyte * max(cap, 1))()
        got = C.c_int64(0)
        try:
            _check(lib().gar_state_save(self._h, buf, cap, C.byref(got)))
        except ErrBufferTooSmall as e:
            e.needed = got.value
            raise
        return bytes(memoryview(buf)[: got.value])

    def load_state(self, blob):
        """Replace the handle's streaming state with a save_state() blob of a handle constructed with
        the same arguments; anything else raises ResamplerError (code INVALID_ARGUMENT) and changes
        nothing."""
        blob = bytes(blob)
        _check(lib().gar_state_load(self._h, blob, len(blob)))

    # -- dithered integer PCM output (gar.h gar_set_dither / gar_get_dither) --
    def set_dither(self, mode, seed=0):
        """DITHER_TPDF: the integer PCM outputs of process_device / flush_device enqueued from now on are
        rounded to nearest with a +-1 LSB triangular dither, a function of (seed, channel, position in
        the output stream) alone; DITHER_NONE (the default): the reference's truncation.  Configuration,
        not stream state: it survives Reset and load_state.  Float and half outputs and the host-memory
        calls ignore it."""
        _check(lib().gar_set_dither(self._h, int(mode), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def get_dither(self):
        """(mode, seed, position): position = the stream position the next device call starts at
        (GetStatistics samplesOut), -1 when the channels are not in lockstep."""
        m, s, p = C.c_int32(0), C.c_uint64(0), C.c_int64(0)
        _check(lib().gar_get_dither(self._h, C.byref(m), C.byref(s), C.byref(p)))
        return m.value, s.value, p.value

    # -- clip counter / peak meter of the integer PCM output (gar.h gar_set_meter / gar_meter_read) --
    def set_meter(self, on):
        """on = True: every integer PCM sample process_device / flush_device store from now on updates the
        channel's clip count and peak |y| in device memory (gar.h: the definition).  Configuration like
        dither: survives Reset and load_state; Reset zeroes the tallies, load_state leaves them."""
        _check(lib().gar_set_meter(self._h, int(on)))

    def get_meter(self):
        v = C.c_int32(0)
        _check(lib().gar_get_meter(self._h, C.byref(v)))
        return bool(v.value)

    def meter_read(self, ch0=0, n_ch=None, reset=False):
        """(clips uint64 [n_ch], peak float64 [n_ch]) of channels ch0 .. ch0 + n_ch - 1 (default: to the last
        channel), after waiting for the handle's enqueued calls; reset zeroes exactly those channels."""
        if n_ch is None:
            n_ch = self.Channels - ch0
        clips = np.zeros(max(n_ch, 0), dtype=np.uint64)
        peak = np.zeros(max(n_ch, 0), dtype=np.float64)
        _check(lib().gar_meter_read(self._h, int(ch0), int(n_ch), _p(clips), _p(peak), int(bool(reset))))
        return clips, peak

    def num_stages(self):
        return lib().gar_num_stages(self._h)

    def stage_geometry(self, stage):
        """(engine ratio, EngineGeometry) of pipeline stage `stage`."""
        ratio, g = C.c_double(0), EngineGeometry()
        _check(lib().gar_stage_geometry(self._h, stage, C.byref(ratio), C.byref(g)))
        return ratio.value, g

    def stage_state(self, stage):
        """(fused_plan, fused_now) of pipeline stage `stage` (channel 0's group)."""
        a, b = C.c_int32(0), C.c_int32(0)
        _check(lib().gar_stage_state(self._h, stage, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    @property
    def Channels(self):
        return lib().gar_channels(self._h)

    # -- device-resident (torch tensors on cuda) --
    def process_device(self, x, out=None, stream=None, pcm_bits=None):
        """x: [frames, channels] device tensor (float32/float64, float16/bfloat16, or integer PCM:
        int16 = PCM16, int32 = PCM24/PCM32 per pcm_bits, default 32), any strides.  Returns out[:n]
        (out allocated with x's dtype if None; x and out may differ in dtype).  Integer PCM follows
        cmd/resample-wav/main.go:444-543 (input i * (1/maxVal), output int(clamp(y, -1, 1) * maxVal)).
        float16 / bfloat16 samples are widened exactly on input and rounded once, to nearest even, on
        output (overflow gives +-Inf, no clamp; gar.h GAR_F16 / GAR_BF16).
        Packed 24-bit PCM (gar.h GAR_PCM24_PACKED, the 3-byte little-endian samples of a 24-bit WAV) is a
        uint8 tensor [frames, channels, 3]: last stride 1, the other strides multiples of 3, any base
        address; values are PCM24's.  An output allocated here has x's form.
        x.shape[1] (and out.shape[1]) must equal Channels (ErrChannelMismatch)."""
        import torch
        _check_form(x)
        if out is not None:
            _check_form(out)
        assert x.is_cuda
        if x.shape[1] != self.Channels or (out is not None and out.shape[1] != self.Channels):
            raise ErrChannelMismatch(f"expected {self.Channels} channels, got {x.shape[1]}"
                                     + ("" if out is None else f" (out {out.shape[1]})"))
        frames = x.shape[0]
        n = lib().gar_device_output_size(self._h, frames)
        if n < 0:
            raise ErrNotSupported("channels not in lockstep")
        if out is None:
            out = torch.empty((max(n, 1),) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        got = C.c_int64(0)
        dt = _io_type(x.dtype, pcm_bits)
        odt = _io_type(out.dtype, pcm_bits)
        (xfs, xcs), (ofs, ocs) = _sample_strides(x), _sample_strides(out)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream)
        _check(lib().gar_process_device(self._h, C.c_void_p(x.data_ptr()), dt, xfs, xcs, frames,
                                        x.shape[1], C.c_void_p(out.data_ptr()), odt, ofs, ocs,
                                        out.shape[0], C.byref(got), st))
        return out[: got.value]

    def flush_device(self, out=None, dtype=None, stream=None, pcm_bits=None):
        """Flush all channels into a device tensor (FlushMulti semantics): `out`, or a new tensor of
        `dtype` (default float32; any sample type process_device takes, float16 / bfloat16 included;
        torch.uint8 allocates packed 24-bit PCM, [frames, channels, 3])."""
        import torch
        if out is not None:
            _check_form(out)
        if out is not None and out.shape[1] != self.Channels:
            raise ErrChannelMismatch(f"expected {self.Channels} channels, got {out.shape[1]}")
        n = lib().gar_device_flush_size(self._h)
        if n < 0:
            raise ErrNotSupported("channels not in lockstep")
        if out is None:
            shape = (max(n, 1), self.Channels) + ((3,) if dtype == torch.uint8 else ())
            out = torch.empty(shape, dtype=dtype or torch.float32, device="cuda")
        got = C.c_int64(0)
        odt = _io_type(out.dtype, pcm_bits)
        ofs, ocs = _sample_strides(out)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(out.device).cuda_stream)
        _check(lib().gar_flush_device(self._h, out.shape[1], C.c_void_p(out.data_ptr()), odt, ofs,
                                      ocs, out.shape[0], C.byref(got), st))
        return out[: got.value]


PCM16, PCM24, PCM32 = 16, 24, 32
F16, BF16 = 4, 5  # device sample types only (gar.h GAR_F16 / GAR_BF16), not compute types
PCM24_PACKED = 280  # device sample type only (gar.h GAR_PCM24_PACKED): 3 bytes per sample, little-endian
DITHER_NONE, DITHER_TPDF = 0, 1  # gar.h GAR_DITHER_*


def _io_type(dtype, pcm_bits=None):
    """Device sample type code of a torch dtype (gar.h GAR_F32/GAR_F64/GAR_F16/GAR_BF16/GAR_PCM*);
    uint8 is packed 24-bit PCM (tensors of shape [frames, channels, 3])."""
    import torch
    if dtype == torch.uint8:
        return PCM24_PACKED
    if dtype == torch.float64:
        return F64
    if dtype == torch.float32:
        return F32
    if dtype == torch.float16:
        return F16
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.int16:
        return PCM16
    if dtype == torch.int32:
        bits = pcm_bits or PCM32
        if bits not in (PCM24, PCM32):
            raise ValueError("int32 PCM holds 24- or 32-bit samples")
        return bits
    raise TypeError(f"unsupported sample dtype {dtype}")


def _check_form(t):
    """A device sample tensor is [frames, channels], or for packed 24-bit PCM (uint8) [frames, channels, 3]
    with the 3 bytes of a sample adjacent and the other strides whole samples."""
    import torch
    if t.dtype == torch.uint8:
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"packed 24-bit PCM is a uint8 tensor [frames, channels, 3], got shape {tuple(t.shape)}")
        if t.stride(2) != 1 or t.stride(0) % 3 or t.stride(1) % 3:
            raise ValueError(f"packed 24-bit PCM needs strides (3 a, 3 b, 1), got {tuple(t.stride())}")
    elif t.dim() != 2:
        raise ValueError(f"sample tensors are [frames, channels], got shape {tuple(t.shape)}")


def _sample_strides(t):
    """(frame_stride, channel_stride) in samples (units of 3 bytes for packed 24-bit PCM)."""
    if t.dim() == 3:
        return t.stride(0) // 3, t.stride(1) // 3
    return t.stride(0), t.stride(1)


def pack_pcm24(i):
    """int32 samples (numpy array or tensor, any shape) -> uint8 [..., 3]: the low three bytes of each,
    little-endian (the layout of GAR_PCM24_PACKED and of 24-bit WAV data).  Host, numpy."""
    a = np.ascontiguousarray(i.cpu().numpy() if hasattr(i, "cpu") else i).astype(np.int32)
    u = a.astype(np.uint32)
    return np.stack([(u & 0xFF), ((u >> 8) & 0xFF), ((u >> 16) & 0xFF)], axis=-1).astype(np.uint8)


def unpack_pcm24(b):
    """uint8 [..., 3] packed 24-bit samples (numpy array or tensor) -> sign-extended int32 [...].  Host, numpy."""
    a = np.asarray(b.cpu().numpy() if hasattr(b, "cpu") else b, dtype=np.uint8)
    if a.ndim < 1 or a.shape[-1] != 3:
        raise ValueError(f"packed 24-bit samples have a last dimension of 3, got shape {a.shape}")
    u = a[..., 0].astype(np.uint32) | (a[..., 1].astype(np.uint32) << 8) | (a[..., 2].astype(np.uint32) << 16)
    return ((u << 8).astype(np.int32) >> 8).astype(np.int32)


def pcm24_convert(x):
    """Host run of the kernels' packed 24-bit conversions (gar.h gar_dev_pcm24_convert) on the float64
    array x: (uint8 [n, 3] bytes a float64-compute handle stores, those bytes read back as int32)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = np.zeros((x.size, 3), dtype=np.uint8)
    i = np.zeros(x.size, dtype=np.int32)
    _check(lib().gar_dev_pcm24_convert(_p(x), x.size, _p(b), _p(i)))
    return b, i


def dither_quantize(y, pcm_bits, seed, channel, position0):
    """Host run of the kernels' dithered quantizer (gar.h gar_dev_dither_quantize) on the float64 array y, taken
    as the samples of channel `channel` from stream position position0: (int32 integers stored, float64 noise d)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    q = np.zeros(y.size, dtype=np.int32)
    d = np.zeros(y.size, dtype=np.float64)
    _check(lib().gar_dev_dither_quantize(int(pcm_bits), int(seed) & 0xFFFFFFFFFFFFFFFF, int(channel), int(position0),
                                         _p(y), y.size, _p(q), _p(d)))
    return q, d


def meter_tally(y, pcm_bits, dither_mode, seed, channel, position0):
    """Host run of the kernels' meter tally (gar.h gar_dev_meter_tally) on the float64 array y, taken as the samples
    of channel `channel` from stream position position0: (clips, peak)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    c, p = C.c_uint64(0), C.c_double(0)
    _check(lib().gar_dev_meter_tally(int(pcm_bits), int(dither_mode), int(seed) & 0xFFFFFFFFFFFFFFFF, int(channel),
                                     int(position0), _p(y), y.size, C.byref(c), C.byref(p)))
    return c.value, p.value


def half_convert(x, half_type):
    """Host run of the kernels' half conversions (gar.h gar_dev_half_convert) on the float64 array x:
    (bits of one f64 -> half rounding, bits of float32(x) -> half, those first bits widened to f32)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    a, b = np.zeros(x.size, dtype=np.uint16), np.zeros(x.size, dtype=np.uint16)
    w = np.zeros(x.size, dtype=np.float32)
    _check(lib().gar_dev_half_convert(int(half_type), _p(x), x.size, _p(a), _p(b), _p(w)))
    return a, b, w


def hxs_plan(r, in_type, in_fs, in_cs, in_addr, in_base, in_len, valid_end, hist_addr, hist_len, hist_ld,
             out_type, out_addr, o0, out_fs, out_cs, o_lo, o_hi, channels, cu_count, hist_keep=0, stage=0):
    """Host run of the streaming FIR launch planner (gar.h gar_dev_hxs_plan) for one call on the handle r
    (a dry-run handle will do): the GAR_HX_TRACE line(s) of that launch, "not supported\\n", or "" for an
    empty output range.  The knobs are read from the environment on every call."""
    buf = C.create_string_buffer(1024)
    _check(lib().gar_dev_hxs_plan(r._h, int(stage), int(in_type), int(in_fs), int(in_cs), int(in_addr), int(in_base),
                                  int(in_len), int(valid_end), int(hist_addr), int(hist_len), int(hist_ld), int(out_type),
                                  int(out_addr), int(o0), int(out_fs), int(out_cs), int(o_lo), int(o_hi), int(channels),
                                  int(cu_count), int(hist_keep), buf, len(buf)))
    return buf.value.decode()


FIR_FUSED, FIR_DFT, FIR_DECIM = 0, 1, 2


def fir_plan(r, in_type, in_fs, in_cs, in_addr, in_base, in_len, valid_end, hist_addr, hist_len, hist_ld,
             out_type, out_addr, o0, out_fs, out_cs, o_lo, o_hi, channels, cu_count, hist_keep=0, stage=0, which=FIR_FUSED):
    """Host run of the x == 0 FIR launch planner (gar.h gar_dev_fir_plan) for one call of the stage's fused,
    DFT or decimator plan on the handle r (a dry-run handle of any compute type will do): the "hxs:" / "hxt:" /
    "hxq:", "hx:" or "bg:" trace line(s) of that launch, "not supported\\n", "invalid configuration\\n", or ""
    when nothing launches.  The knobs are read from the environment on every call."""
    buf = C.create_string_buffer(2048)
    _check(lib().gar_dev_fir_plan(r._h, int(stage), int(which), int(in_type), int(in_fs), int(in_cs), int(in_addr), int(in_base),
                                  int(in_len), int(valid_end), int(hist_addr), int(hist_len), int(hist_ld), int(out_type),
                                  int(out_addr), int(o0), int(out_fs), int(out_cs), int(o_lo), int(o_hi), int(channels),
                                  int(cu_count), int(hist_keep), buf, len(buf)))
    return buf.value.decode()


def New(config):
    """resampler.New (resample.go:272-292)."""
    if config is None:
        raise ErrInvalidConfig("config is nil")
    h = C.c_void_p(0)
    _check(lib().gar_new(C.byref(config), C.byref(h)))
    return Resampler(h.value)


def NewBatch(config, n_streams):
    """n_streams independent New(config) resamplers as one lockstep GPU batch."""
    h = C.c_void_p(0)
    _check(lib().gar_new_batch(C.byref(config), int(n_streams), C.byref(h)))
    return Resampler(h.value)


def NewEngine(inputRate, outputRate, quality):
    """resampler.NewEngine (convenience.go:125-135), float64."""
    h = C.c_void_p(0)
    _check(lib().gar_new_engine(float(inputRate), float(outputRate), quality, F64, C.byref(h)))
    return Resampler(h.value)


def NewEngineFloat32(inputRate, outputRate, quality):
    """resampler.NewEngineFloat32 (convenience.go:329-336)."""
    h = C.c_void_p(0)
    _check(lib().gar_new_engine(float(inputRate), float(outputRate), quality, F32, C.byref(h)))
    return Resampler(h.value, f32_io=True)


def EngineNewResampler(inputRate, outputRate, quality, dtype=F64):
    """engine.NewResampler[F](inputRate, outputRate, quality) with an engine.Quality
    (internal/engine/resampler.go:51-179; the seam cmd/resample-wav/helpers.go:77-97
    drives).  dtype F64 = Resampler[float64]; F32 / F32_EXACT = Resampler[float32]."""
    h = C.c_void_p(0)
    _check(lib().gar_new_engine_quality(float(inputRate), float(outputRate), int(quality), int(dtype), C.byref(h)))
    return Resampler(h.value, f32_io=dtype != F64)


def NewEngineDry(inputRate, outputRate, quality, dtype=F64):
    """Host-only NewEngine: exact stream lengths, no GPU work (CPU tests)."""
    h = C.c_void_p(0)
    _check(lib().gar_new_engine_dry(float(inputRate), float(outputRate), quality, dtype, C.byref(h)))
    return Resampler(h.value, f32_io=dtype == F32)


def ResampleMono(x, inputRate, outputRate, quality):
    """resampler.ResampleMono (convenience.go:204-229): Process + Flush."""
    r = NewEngine(inputRate, outputRate, quality)
    return np.concatenate([r.Process(x), r.Flush()])


def ResampleMonoFloat32(x, inputRate, outputRate, quality):
    r = NewEngineFloat32(inputRate, outputRate, quality)
    return np.concatenate([r.ProcessFloat32(x), r.Flush()])


def ResampleStereo(left, right, inputRate, outputRate, quality):
    """resampler.ResampleStereo (convenience.go:233-257): one engine reused with Reset."""
    r = NewEngine(inputRate, outputRate, quality)
    lo = np.concatenate([r.Process(left), r.Flush()])
    r.Reset()
    ro = np.concatenate([r.Process(right), r.Flush()])
    return lo, ro


def design_engine(in_rate, out_rate, engine_quality):
    """Host-only engine design introspection (no GPU): geometry + coefficient banks."""
    g = EngineGeometry()
    _check(lib().gar_design_engine(in_rate, out_rate, engine_quality, C.byref(g), None, None, None, None, None, None))
    dft = np.zeros(max(g.dft_factor * g.dft_taps, 1))
    n = g.poly_phases * g.poly_taps
    pa, pb, pc, pd = (np.zeros(max(n, 1)) for _ in range(4))
    dec = np.zeros(max(g.decim_taps, 1))
    _check(lib().gar_design_engine(in_rate, out_rate, engine_quality, C.byref(g), _p(dft), _p(pa), _p(pb), _p(pc),
                                   _p(pd), _p(dec)))
    return g, {"dft": dft[: g.dft_factor * g.dft_taps], "a": pa[:n], "b": pb[:n], "c": pc[:n], "d": pd[:n],
               "decim": dec[: g.decim_taps]}


def design_composite(in_rate, out_rate, engine_quality):
    g, _ = design_engine(in_rate, out_rate, engine_quality)
    if not g.fused:
        raise ErrNotSupported("engine has no fused composite FIR")
    rows = np.zeros((g.fir_period_out, g.fir_taps_max))
    offs = np.zeros(g.fir_period_out, dtype=np.int64)
    _check(lib().gar_design_composite(in_rate, out_rate, engine_quality, _p(rows), _p(offs)))
    return rows, offs, g
