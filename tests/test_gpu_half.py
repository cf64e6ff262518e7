"""GPU: half-precision (float16 / bfloat16) sample I/O of the device entry points (gar.h GAR_F16 /
GAR_BF16) -- samples widened exactly in the resampling kernel's loads, results rounded once (to
nearest even) in its stores.

Parity bars:
  * bit-exact against the "float path": the same handle configuration fed x.float(), its output
    rounded on the host (torch's float32 -> half cast is one RNE) -- fused loads / stores change
    nothing but the bytes moved;
  * float64 compute: bit-exact against numpy's single f64 -> f16 rounding of the float64 path
    (a numpy helper does the same for bf16), and within one half ulp of the single-rounded oracle on
    at most 1e-4 of the samples (the bar of test_pcm_staged_f64);
  * fused float32 path against the oracle: rms <= rms of half an ulp of the outputs + F32_RMS_TOL
    (triangle inequality over one RNE rounding and the project's float32 bar);
  * ragged chunks == one shot, flush tail included.

Launch sizes: a launch of at most 8192 columns (periods x channels) runs the compact small-launch
kernels, whose window is gathered per element; the streaming kernel's register loaders (one dword
per stereo frame, 32-B rows of 16 channels) need more, so two cases use longer streams.
"""
import numpy as np
import pytest

from helpers import F32_RMS_TOL, chunk_sizes, oracle_new, signal

pytestmark = pytest.mark.gpu

HALF = ["float16", "bfloat16"]


def bits16(t):
    """int16 bit view of a half tensor as numpy."""
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy()


def same_bits(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    a, b = bits16(got), bits16(want)
    assert np.array_equal(a, b), (int(np.count_nonzero(a != b)), a.size)


def bf16_bits_of_f64(v):
    """float64 -> bfloat16 bit patterns with ONE rounding, ties to even (finite values and +-Inf;
    exact arithmetic: |v| is scaled by the bf16 spacing at its binade, rounded by rint)."""
    v = np.asarray(v, dtype=np.float64)
    fin = np.isfinite(v) & (v != 0)
    _, e = np.frexp(np.where(fin, np.abs(v), 1.0))       # |v| = m * 2^e, m in [0.5, 1)
    q = np.maximum(e - 8, -133)                          # spacing 2^q: 8 significant bits, subnormals 2^-133
    val = np.ldexp(np.rint(np.ldexp(np.abs(v), -q)), q)  # exact: a multiple of the spacing
    with np.errstate(over="ignore"):
        b = (np.where(fin, val, np.abs(v)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return np.where(np.signbit(v), b | 0x8000, b).astype(np.uint16)


def ordered(b):
    """Half bit patterns (sign-magnitude) -> integers in value order; +0 and -0 both 0."""
    m = (b & 0x7fff).astype(np.int64)
    return np.where(b & 0x8000, -m, m)


def half_ulp(tdtype, y):
    """Spacing of the half type at each value of the float64 array y (np.spacing for f16)."""
    import torch
    if tdtype == torch.float16:
        return np.abs(np.spacing(y.astype(np.float16))).astype(np.float64)
    _, e = np.frexp(np.where(y != 0, np.abs(y), 1.0))
    return np.ldexp(1.0, np.maximum(e - 8, -133))


def run(gar, torch, xd, in_rate, out_rate, preset, compute, chunks=None, out_dtype=None, bits=None, into=None):
    """Process (+ chunks) + Flush of the device tensor xd [frames, channels]; outputs of out_dtype
    (default xd's), written into successive parts of `into` when given.  Returns a host tensor."""
    ch = xd.shape[1]
    r = gar.New(gar.Config(in_rate, out_rate, ch, preset, ComputeDtype=compute))
    od = out_dtype or xd.dtype
    outs, s, pos = [], 0, 0

    def dest(n):
        if into is not None:
            return into[pos:]
        return torch.empty((max(n, 1), ch), dtype=od, device="cuda")

    for n in (chunks or [xd.shape[0]]):
        y = r.process_device(xd[s:s + n], out=dest(gar.lib().gar_device_output_size(r._h, n)), pcm_bits=bits)
        outs.append(y)
        pos += y.shape[0]
        s += n
    outs.append(r.flush_device(out=dest(gar.lib().gar_device_flush_size(r._h)), pcm_bits=bits))
    torch.cuda.synchronize()
    return torch.cat(outs).cpu()


def cfg2(gar, torch, xd, **kw):
    return run(gar, torch, xd, 44100, 48000, gar.QualityHigh, gar.F32, **kw)


def half_signal(torch, tdtype, n, ch, seed=4242, amp=1.0):
    return torch.from_numpy(signal(n, ch, seed=seed) * amp).to(tdtype).cuda()


@pytest.mark.parametrize("name", HALF)
def test_half_fused_equals_float_path(gar, cuda, name):
    """cfg2 geometry (stereo 44.1k -> 48k QualityHigh, float32 split-f16 path), half in and out ==
    the float kernel fed x.float(), rounded on the host."""
    torch = cuda
    td = getattr(torch, name)
    x = half_signal(torch, td, 3 * 44100 + 123, 2)
    got = cfg2(gar, torch, x)
    assert got.dtype == td
    same_bits(got, cfg2(gar, torch, x.float()).to(td))


@pytest.mark.parametrize("name,ch,n", [("float16", 2, 15 * 44100 + 77), ("bfloat16", 2, 15 * 44100 + 77),
                                       ("float16", 16, 2 * 44100 + 3), ("bfloat16", 16, 2 * 44100 + 3)])
def test_half_streaming_loaders_equal_float_path(gar, cuda, name, ch, n):
    """Streams long enough (more than 8192 columns) for the streaming kernel: its register loaders
    take stereo half frames as one dword per frame and 16-channel half rows as 32-B rows."""
    torch = cuda
    td = getattr(torch, name)
    x = half_signal(torch, td, n, ch, seed=5)
    same_bits(cfg2(gar, torch, x), cfg2(gar, torch, x.float()).to(td))


@pytest.mark.parametrize("name", HALF)
def test_half_quiet_material(gar, cuda, name):
    """Amplitude 1e-5: the f16 inputs and outputs are subnormal -- values, never flushed."""
    torch = cuda
    td = getattr(torch, name)
    x = half_signal(torch, td, 3 * 44100 + 123, 2, amp=1e-5)
    got = cfg2(gar, torch, x)
    if td == torch.float16:
        a = got.float().abs()
        assert float(a.max()) < 2.0 ** -14 and int(torch.count_nonzero(a)) > got.numel() // 2  # subnormal, not zero
    same_bits(got, cfg2(gar, torch, x.float()).to(td))


def test_half_chunked_is_bit_identical(gar, cuda):
    """Ragged chunks == one shot, flush tail included; the chunk list starts with [1, 0, 7, 2, 4800],
    so launches start at odd frame offsets of the input.  Written back to back into one buffer
    that starts one frame (4 bytes) into its allocation, no frame-pair store is 8-byte aligned: they
    take the checked per-element path."""
    torch = cuda
    n = 2 * 44100 + 777
    x = half_signal(torch, torch.float16, n, 2, seed=7)
    one = cfg2(gar, torch, x)
    head = [1, 0, 7, 2, 4800]
    chunks = head + chunk_sizes(n - sum(head), 4096 + 17)
    same_bits(cfg2(gar, torch, x, chunks=chunks), one)
    buf = torch.zeros((one.shape[0] + 9, 2), dtype=torch.float16, device="cuda")
    same_bits(cfg2(gar, torch, x, chunks=chunks, into=buf[1:]), one)
    assert not bits16(buf[0]).any() and not bits16(buf[1 + one.shape[0]:]).any()  # nothing written around it
    same_bits(cfg2(gar, torch, x, into=buf[1:]), one)


@pytest.mark.parametrize("name", HALF)
@pytest.mark.parametrize("ch", [1, 16, 3])
def test_half_other_layouts(gar, cuda, name, ch):
    """Mono, 16-channel and 3-channel rows == the float path + host rounding."""
    torch = cuda
    td = getattr(torch, name)
    x = half_signal(torch, td, 44100 + 5, ch, seed=11)
    same_bits(cfg2(gar, torch, x), cfg2(gar, torch, x.float()).to(td))


def test_half_input_views(gar, cuda):
    """A planar (channel-major) input view and a view that starts one element (2 bytes) into its
    buffer == the float path of the contiguous tensor + host rounding."""
    torch = cuda
    n = 44100 + 5
    x = half_signal(torch, torch.float16, n, 2, seed=13)
    want = cfg2(gar, torch, x.float()).to(torch.float16)
    planar = x.t().contiguous().t()
    assert planar.stride() == (1, n)
    same_bits(cfg2(gar, torch, planar), want)
    buf = torch.zeros(2 * n + 1, dtype=torch.float16, device="cuda")
    off = buf[1:].view(n, 2)
    off.copy_(x)
    assert off.data_ptr() % 4 == 2
    same_bits(cfg2(gar, torch, off), want)


def test_half_mixed_types(gar, cuda):
    """Input and output types are independent."""
    torch = cuda
    n = 44100 + 5
    x = half_signal(torch, torch.float16, n, 2, seed=17)
    yf = cfg2(gar, torch, x.float())
    got = cfg2(gar, torch, x, out_dtype=torch.float32)  # f16 in, f32 out: the float path's bits
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), yf.view(torch.int32))
    xf = torch.from_numpy(signal(n, 2, seed=19).astype(np.float32)).cuda()
    same_bits(cfg2(gar, torch, xf, out_dtype=torch.bfloat16), cfg2(gar, torch, xf).to(torch.bfloat16))
    pcm = torch.from_numpy(np.round(signal(n, 2, seed=23) * 32767 * 0.98).astype(np.int16)).cuda()
    same_bits(cfg2(gar, torch, pcm, out_dtype=torch.float16), cfg2(gar, torch, pcm, out_dtype=torch.float32).to(torch.float16))


def test_half_loud_and_nonfinite(gar, cuda):
    """+Inf, NaN, -Inf and a sample of 1000.0 in the f16 input: the outputs are NaN / +-Inf exactly
    where the float path's are (their recompute writes 2-byte elements), bit-equal elsewhere."""
    torch = cuda
    n = 44100
    x = half_signal(torch, torch.float16, n, 2, seed=29)
    x[5000, 0] = float("inf")
    x[12000, 1] = float("nan")
    x[20001, 0] = float("-inf")
    x[30003, 1] = 1000.0
    got = cfg2(gar, torch, x)
    yf = cfg2(gar, torch, x.float())
    want = yf.to(torch.float16)
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn) and int(wn.sum()) > 0
    assert int(torch.isinf(want).sum()) > 0
    g, w = bits16(got), bits16(want)
    keep = ~wn.numpy()
    assert np.array_equal(g[keep], w[keep])  # +-Inf and every finite sample


@pytest.mark.parametrize("name", HALF)
def test_half_overflow_is_inf_not_clamped(gar, cuda, name):
    """A square wave of amplitude 60000 overshoots past 65504 after resampling: +Inf in f16 (no
    clamp), finite in bf16 -- what rounding the float path on the host gives."""
    torch = cuda
    td = getattr(torch, name)
    t = np.arange(44100)
    sq = np.where((t // 50) % 2 == 0, 60000.0, -60000.0)
    x = torch.from_numpy(np.stack([sq, -sq], axis=1)).to(td).cuda()
    got = cfg2(gar, torch, x)
    yf = cfg2(gar, torch, x.float())
    assert float(yf.max()) > 65520.0 and bool(torch.isfinite(yf).all())
    if td == torch.float16:
        assert int(torch.isinf(got).sum()) > 0 and float(got[torch.isfinite(got)].max()) <= 65504.0
    else:
        assert bool(torch.isfinite(got).all())
    same_bits(got, yf.to(td))


@pytest.mark.parametrize("name", HALF)
def test_half_staged_f64(gar, cuda, O, name):
    """float64 compute (conversion staged by convert_kernel): the half output == ONE rounding of the
    float64 path's output (numpy rounds f64 -> f16 once; torch on the CPU goes through f32), and is
    within one half ulp of the single-rounded oracle on at most 1e-4 of the samples."""
    torch = cuda
    td = getattr(torch, name)
    n = 44100
    x = half_signal(torch, td, n, 2, seed=3)
    got = bits16(run(gar, torch, x, 44100, 48000, gar.QualityHigh, gar.F64)).view(np.uint16)
    yd = run(gar, torch, x.double(), 44100, 48000, gar.QualityHigh, gar.F64).numpy()

    def once(v):
        return v.astype(np.float16).view(np.uint16) if td == torch.float16 else bf16_bits_of_f64(v)

    assert got.shape == yd.shape
    assert np.array_equal(got, once(yd)), int(np.count_nonzero(got != once(yd)))
    ref = oracle_new(O, 44100, 48000, x.double().cpu().numpy(), O.P_HIGH)
    for c in range(2):
        want = once(ref[c])
        assert len(want) == got.shape[0]
        d = np.abs(ordered(got[:, c]) - ordered(want))  # neighbouring half values differ by 1
        assert d.max() <= 1 and np.mean(d != 0) <= 1e-4, (int(d.max()), float(np.mean(d != 0)))


@pytest.mark.parametrize("i,o", [(96000, 16000), (16000, 44100)])
def test_half_staged_f32_plans(gar, cuda, i, o):
    """A multi-stage pipeline (96k -> 16k) and a fractional-step polyphase stage (16k -> 44.1k) on
    float32 compute, f16 in and out: staged conversion == the float path + host rounding."""
    torch = cuda
    x = half_signal(torch, torch.float16, 44100, 2, seed=31)
    got = run(gar, torch, x, i, o, gar.QualityHigh, gar.F32)
    same_bits(got, run(gar, torch, x.float(), i, o, gar.QualityHigh, gar.F32).to(torch.float16))


@pytest.mark.parametrize("name", HALF)
def test_half_vs_oracle(gar, cuda, O, name):
    """Fused path against the oracle fed the widened input: one RNE rounding (at most half an ulp
    of each output) on top of the project's float32 bar."""
    torch = cuda
    td = getattr(torch, name)
    n = 2 * 44100
    x = half_signal(torch, td, n, 2)
    got = cfg2(gar, torch, x).double().numpy()
    ref = np.stack(oracle_new(O, 44100, 48000, x.double().cpu().numpy(), O.P_HIGH), axis=1)
    assert ref.shape == got.shape
    err = float(np.sqrt(np.mean((got - ref) ** 2)))
    bound = float(np.sqrt(np.mean((0.5 * half_ulp(td, got)) ** 2))) + F32_RMS_TOL
    print(f"{name}: rms {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)
