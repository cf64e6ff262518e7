"""GPU: packed 24-bit PCM sample I/O of the device entry points (gar.h GAR_PCM24_PACKED) -- 3 bytes
per sample, little-endian, as a 24-bit WAV file holds them; torch.uint8 tensors [frames, channels, 3].

The sample semantics are GAR_PCM24's (int32 storage), only the byte layout is new, so every result is
compared BIT FOR BIT with the int32 path (or the float path plus the host conversion) -- no tolerance
of its own.  The one oracle comparison reuses the bar of test_gpu_pcm.test_pcm_vs_oracle (24-bit).

Packed samples are converted by the pack / unpack kernels around the float path (4 samples <-> 3
dwords per thread for interleaved contiguous buffers from a 4-byte aligned base, the per-element
kernel otherwise).  Launch sizes: a launch of at most 8192 columns (periods x channels) runs the
compact small-launch FIR kernels, a longer one the streaming kernels: SHORT and LONG.
"""
import numpy as np
import pytest

from helpers import F32_RMS_TOL, chunk_sizes, oracle_new, signal

pytestmark = pytest.mark.gpu

MAX24 = 8388607.0
SHORT = 3 * 44100 + 123
LONG = 15 * 44100 + 77
GUARD = 0xA5
_cache = {}


def pcm24(n, ch, seed=4242):
    """24-bit integer samples (int32) of the deterministic test signal."""
    key = ("pcm", n, ch, seed)
    if key not in _cache:
        _cache[key] = np.round(np.clip(signal(n, ch, seed=seed), -1, 1) * MAX24 * 0.98).astype(np.int32)
    return _cache[key]


def from_float(y):
    """int(clamp(float64(y), -1, 1) * 8388607), truncating -- main.go:497-541."""
    return np.trunc(np.clip(np.asarray(y, dtype=np.float64), -1.0, 1.0) * MAX24).astype(np.int32)


def shape_of(n, ch, dtype, torch):
    return (max(n, 1), ch, 3) if dtype == torch.uint8 else (max(n, 1), ch)


def run(gar, torch, xd, rates=(44100, 48000), preset=None, compute=None, chunks=None, out_dtype=None, bits=None,
        into=None):
    """Process (+ chunks) + Flush of the device tensor xd; outputs of out_dtype (default xd's), written
    into successive parts of `into` when given (so output bases follow the produced frame counts).
    Returns the host array of all output frames."""
    ch = xd.shape[1]
    L = gar.lib()
    r = gar.New(gar.Config(rates[0], rates[1], ch, gar.QualityHigh if preset is None else preset,
                           ComputeDtype=gar.F32 if compute is None else compute))
    od = out_dtype or xd.dtype
    outs, s, pos = [], 0, 0

    def dest(n):
        if into is not None:
            return into[pos:pos + n]
        return torch.empty(shape_of(n, ch, od, torch), dtype=od, device="cuda")

    for n in (chunks or [xd.shape[0]]):
        y = r.process_device(xd[s:s + n], out=dest(L.gar_device_output_size(r._h, n)), pcm_bits=bits)
        outs.append(y)
        pos += y.shape[0]
        s += n
    outs.append(r.flush_device(out=dest(L.gar_device_flush_size(r._h)), pcm_bits=bits))
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy()


def int32_path(gar, torch, n, ch=2, seed=4242, rates=(44100, 48000), compute=None, preset=None):
    """The GAR_PCM24 (int32 storage) path's output for pcm24(n, ch, seed), packed on the host: the
    reference bytes of every packed run of the same integers.  Computed once per case."""
    key = ("ref", n, ch, seed, rates, compute, preset)
    if key not in _cache:
        xd = torch.from_numpy(pcm24(n, ch, seed)).cuda()
        y = run(gar, torch, xd, rates=rates, compute=compute, preset=preset, bits=24)
        assert y.dtype == np.int32
        _cache[key] = gar.pack_pcm24(y)
    return _cache[key]


def packed_ref(gar, torch, n, seed=4242):
    """The packed path's own output for pcm24(n, 2, seed) from 16-byte aligned bases, computed once:
    the reference of the alignment, guard-byte and chunking cases (identical to the aligned run)."""
    key = ("pref", n, seed)
    if key not in _cache:
        _cache[key] = run(gar, torch, packed_dev(gar, torch, pcm24(n, 2, seed)))
    return _cache[key]


def at_offset(torch, nbytes, off):
    """(allocation, view): a uint8 device view of nbytes that starts `off` bytes past a 16-byte
    boundary, inside a larger allocation filled with the guard byte."""
    buf = torch.full((nbytes + 96,), GUARD, dtype=torch.uint8, device="cuda")
    lead = (-buf.data_ptr()) % 16 + 16 + off
    v = buf[lead:lead + nbytes]
    assert v.data_ptr() % 16 == off % 16
    return buf, v


def packed_dev(gar, torch, pcm, off=0):
    """pcm (int32 [n, ch]) as a packed device tensor [n, ch, 3] whose base is `off` bytes past a
    16-byte boundary."""
    b = gar.pack_pcm24(pcm)
    _, v = at_offset(torch, b.size, off)
    v.copy_(torch.from_numpy(b.reshape(-1)))
    return v.view(b.shape)


def same_bytes(got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (int(np.count_nonzero(got != want)), got.size)


@pytest.mark.parametrize("n", [SHORT, LONG])
def test_packed_fused_equals_int32_path(gar, cuda, n):
    """cfg2 geometry (stereo 44.1k -> 48k QualityHigh, float32 split-f16 path): packed in / out bytes
    == pack_pcm24 of the GAR_PCM24 int32 path's output for the same integers, at a small-launch and a
    streaming size.

    LONG is also the first test of the int32 path's streaming loader (hxs_kernel FMT 4): it used to
    return channel 0 in both channels (719813 of 1440172 samples off the float path), see
    test_int32_pcm24_streaming_equals_float_path."""
    torch = cuda
    want = int32_path(gar, torch, n)
    xd = packed_dev(gar, torch, pcm24(n, 2))
    assert xd.dtype == torch.uint8 and xd.data_ptr() % 16 == 0
    got = run(gar, torch, xd)
    same_bytes(got, want)
    # and the default allocation has the input's form
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))
    y = r.process_device(xd[:4410])
    assert y.dtype == torch.uint8 and y.dim() == 3 and y.shape[1:] == (2, 3)
    f = r.flush_device(dtype=torch.uint8)
    assert f.dtype == torch.uint8 and f.shape[1:] == (2, 3)


@pytest.mark.parametrize("which", ["in", "out", "both"])
@pytest.mark.parametrize("off", [0, 2, 6, 1, 4, 12])
def test_packed_alignment_variants(gar, cuda, off, which):
    """Input and / or output base at byte offset 0, 2, 6, 1 (and 4, 12) from a 16-byte boundary.  A
    4-byte aligned base (0, 4, 12) runs the vector pack / unpack kernels, 2, 6 and 1 the per-element
    kernel's byte loads and stores.  Identical bytes to the aligned run every time."""
    torch = cuda
    want = packed_ref(gar, torch, LONG)
    xd = packed_dev(gar, torch, pcm24(LONG, 2), off if which != "out" else 0)
    _, ob = at_offset(torch, want.size, off if which != "in" else 0)
    got = run(gar, torch, xd, into=ob.view(want.shape))
    same_bytes(got, want)
    assert np.array_equal(ob.cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize("case", ["fused_long", "fused_long_off2", "fused_short", "staged_f64", "planar_pitch"])
def test_packed_no_stray_writes(gar, cuda, case):
    """`out` is a slice inside a larger buffer filled with 0xA5, exactly as long as the produced
    samples: every byte before and after them is unchanged after process and flush; in a strided
    planar output the gap bytes between the channels are unchanged too."""
    torch = cuda
    n = LONG if case.startswith("fused_long") else SHORT
    compute = gar.F64 if case == "staged_f64" else gar.F32
    want = int32_path(gar, torch, n, compute=compute) if n == SHORT else packed_ref(gar, torch, n)
    m = want.shape[0]
    xd = packed_dev(gar, torch, pcm24(n, 2))
    if case == "planar_pitch":
        pitch = m + 5
        buf, ob = at_offset(torch, 2 * pitch * 3, 0)
        out = ob.view(2, pitch, 3).permute(1, 0, 2)[:m]  # strides (3, 3 * pitch, 1)
        assert out.stride() == (3, 3 * pitch, 1)
    else:
        buf, ob = at_offset(torch, want.size, 2 if case.endswith("off2") else 0)
        out = ob.view(want.shape)
    got = run(gar, torch, xd, compute=compute, into=out)
    same_bytes(got, want)
    host = buf.cpu().numpy()
    lead = ob.data_ptr() - buf.data_ptr()
    assert (host[:lead] == GUARD).all() and (host[lead + ob.numel():] == GUARD).all()
    if case == "planar_pitch":
        body = host[lead:lead + ob.numel()].reshape(2, pitch, 3)
        assert np.array_equal(body[:, :m].transpose(1, 0, 2), want)
        assert (body[:, m:] == GUARD).all()


@pytest.mark.parametrize("chunks", ["ragged", "small_then_long", "long_then_small"])
def test_packed_chunked_equals_one_shot(gar, cuda, chunks):
    """Ragged chunks == one shot, flush tail included.  Odd chunk lengths make the chunk bases (input,
    and the outputs written back to back) alternate between 4-byte and 2-byte alignment; the LONG
    splits put the history seam and the odd base on a streaming launch."""
    torch = cuda
    if chunks == "ragged":
        n = 2 * 44100 + 777
        sizes = chunk_sizes(n, 4096 + 17)
    else:
        n = LONG
        sizes = [44101, n - 44101] if chunks == "small_then_long" else [14 * 44100 + 1, n - 14 * 44100 - 1]
    assert sum(sizes) == n and any(s % 2 for s in sizes[:-1])
    want = packed_ref(gar, torch, n, seed=7)
    xd = packed_dev(gar, torch, pcm24(n, 2, seed=7))
    out = torch.full(want.shape, GUARD, dtype=torch.uint8, device="cuda")
    got = run(gar, torch, xd, chunks=sizes, into=out)
    same_bytes(got, want)


def test_packed_mixed_types(gar, cuda):
    """Packed in -> f32 out == the float path fed float32(unpack * (1 / 8388607)), bit for bit;
    f32 in -> packed out == the float path's output converted on the host."""
    torch = cuda
    pcm = pcm24(LONG, 2)
    xf = torch.from_numpy((pcm.astype(np.float64) * (1.0 / MAX24)).astype(np.float32)).cuda()
    yf = run(gar, torch, xf)
    assert yf.dtype == np.float32
    got = run(gar, torch, packed_dev(gar, torch, pcm), out_dtype=torch.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), yf.view(np.uint32))
    got = run(gar, torch, xf, out_dtype=torch.uint8)
    same_bytes(got, gar.pack_pcm24(from_float(yf)))
    # PCM16 in -> packed out: the PCM16 float path converted on the host
    p16 = torch.from_numpy(np.round(np.clip(signal(SHORT, 2), -1, 1) * 32767 * 0.98).astype(np.int16)).cuda()
    y16 = run(gar, torch, p16, out_dtype=torch.float32)
    same_bytes(run(gar, torch, p16, out_dtype=torch.uint8), gar.pack_pcm24(from_float(y16)))


@pytest.mark.parametrize("ch,n", [(2, SHORT), (5, SHORT), (5, SHORT - 2), (3, SHORT)])
def test_packed_staged_f64(gar, cuda, ch, n):
    """float64 compute (bg_kernel between the pack / unpack kernels): bytes == the GAR_PCM24
    float64 path packed on the host.  frames * channels % 4 is 2, 3, 1, 1: the vector kernels' tail."""
    torch = cuda
    assert (n * ch) % 4 in (1, 2, 3)
    want = int32_path(gar, torch, n, ch=ch, seed=3, compute=gar.F64)
    got = run(gar, torch, packed_dev(gar, torch, pcm24(n, ch, seed=3)), compute=gar.F64)
    same_bytes(got, want)
    # the same through the per-element kernel: an input base 1 byte past a boundary
    xd = packed_dev(gar, torch, pcm24(n, ch, seed=3), off=1)
    same_bytes(run(gar, torch, xd, compute=gar.F64), want)


def test_packed_staged_two_stage_f32(gar, cuda):
    """A two-stage plan (96k -> 16k QualityHigh) in float32: staged conversion, bytes == int32 path."""
    torch = cuda
    n = 96000 + 333
    want = int32_path(gar, torch, n, seed=5, rates=(96000, 16000))
    got = run(gar, torch, packed_dev(gar, torch, pcm24(n, 2, seed=5)), rates=(96000, 16000))
    same_bytes(got, want)


@pytest.mark.parametrize("layout", ["mono", "ch16", "planar_pitch"])
def test_packed_other_layouts(gar, cuda, layout):
    """Mono, 16-channel interleaved rows and a planar input with a pitch (gathered byte loads, checked
    stores) == the int32 path."""
    torch = cuda
    n = 44100 + 5
    ch = {"mono": 1, "ch16": 16, "planar_pitch": 2}[layout]
    want = int32_path(gar, torch, n, ch=ch, seed=11)
    if layout == "planar_pitch":
        pitch = n + 3
        b = gar.pack_pcm24(pcm24(n, ch, seed=11))
        buf = torch.full((ch, pitch, 3), GUARD, dtype=torch.uint8, device="cuda")
        buf[:, :n] = torch.from_numpy(np.ascontiguousarray(b.transpose(1, 0, 2))).cuda()
        xd = buf.permute(1, 0, 2)[:n]
        assert xd.stride() == (3, 3 * pitch, 1)
    else:
        xd = packed_dev(gar, torch, pcm24(n, ch, seed=11))
    same_bytes(run(gar, torch, xd), want)


def test_packed_clipping(gar, cuda):
    """The overshooting full-scale square of test_pcm_clipping: the bytes are the packed +-8388607
    clamp of the float path (no wrap-around into the sign bit)."""
    torch = cuda
    n = 44100
    t = np.arange(n)
    sq = np.where((t // 50) % 2 == 0, 8388607, -8388607).astype(np.int32)
    pcm = np.stack([sq, -sq], axis=1)
    got = run(gar, torch, packed_dev(gar, torch, pcm))
    vals = gar.unpack_pcm24(got)
    assert vals.max() == 8388607 and vals.min() == -8388607
    xf = torch.from_numpy((pcm.astype(np.float64) * (1.0 / MAX24)).astype(np.float32)).cuda()
    yf = run(gar, torch, xf)
    assert np.abs(yf).max() > 1.0  # the float path does overshoot
    same_bytes(got, gar.pack_pcm24(from_float(yf)))


def test_packed_vs_oracle(gar, cuda, O):
    """Packed in -> packed out vs the oracle fed the same scaled floats: the 24-bit bar of
    test_gpu_pcm.test_pcm_vs_oracle (the 24-bit LSB is at the float32 error level: RMS <= F32_RMS_TOL
    of full scale, plus its per-sample cap)."""
    torch = cuda
    n = 2 * 44100
    pcm = pcm24(n, 2)
    got = gar.unpack_pcm24(run(gar, torch, packed_dev(gar, torch, pcm))).astype(np.int64)
    xs = (pcm.astype(np.float64) * (1.0 / MAX24)).astype(np.float32).astype(np.float64)
    ref = oracle_new(O, 44100, 48000, xs, O.P_HIGH)
    for c in range(2):
        want = from_float(ref[c]).astype(np.int64)
        assert len(want) == got.shape[0]
        d = np.abs(got[:, c] - want)
        assert np.sqrt(np.mean(d.astype(np.float64) ** 2)) / MAX24 <= F32_RMS_TOL
        assert d.max() <= 16, d.max()


@pytest.mark.parametrize("bits", [24, 32])
def test_int32_pcm24_streaming_equals_float_path(gar, cuda, bits):
    """int32-held PCM at a streaming size (hxs_kernel's FMT 4 register loader; test_gpu_pcm runs only
    small launches): int32 in -> f32 out == the float path fed float32(float64(i) / maxVal), bit for
    bit, both channels.  The loader once carried the integers through a float vector and the second
    channel's conversion was dropped: channel 1 came out as channel 0."""
    torch = cuda
    maxv = MAX24 if bits == 24 else 2147483647.0
    pcm = pcm24(LONG, 2) if bits == 24 else (pcm24(LONG, 2).astype(np.int64) * 256).astype(np.int32)
    xf = torch.from_numpy((pcm.astype(np.float64) * (1.0 / maxv)).astype(np.float32)).cuda()
    yf = run(gar, torch, xf)
    got = run(gar, torch, torch.from_numpy(pcm).cuda(), bits=bits, out_dtype=torch.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), yf.view(np.uint32))
    assert not np.array_equal(got[:, 0], got[:, 1])
