"""GPU: TPDF-dithered integer PCM output (gar.h gar_set_dither) on every store path of the device entry points.

The expected integers are always the SAME handle configuration's float output (test_gpu_pcm.py establishes
that identity for truncation), quantized by the numpy restatement of the header's definition in dither_ref.py
with the sample's channel and its index in the output stream -- so every test below also checks that the
noise does not depend on the chunking, the fused or staged path, the layout or the launch that stored it.

Streams are 44100 + 123 frames (44.1k -> 48k QualityHigh unless said): interior row blocks (the vector
store), edge blocks (the checked store) and a flush tail.
"""
import numpy as np
import pytest

import dither_ref as D
from helpers import chunk_sizes, signal

pytestmark = pytest.mark.gpu

N = 44100 + 123
SEED = 7
_float_ref = {}


def _new(gar, ch, compute, rates=(44100, 48000), batch=0):
    cfg = gar.Config(rates[0], rates[1], ch, gar.QualityHigh, ComputeDtype=compute)
    return gar.NewBatch(cfg, batch) if batch else gar.New(cfg)


def interleaved(torch, dtype):
    def make(cap, ch):
        shape = (cap, ch, 3) if dtype == torch.uint8 else (cap, ch)
        return torch.zeros(shape, dtype=dtype, device="cuda")
    return make


def planar(torch, dtype):
    """[frames, channels] view of a [channels, pitch] buffer: channel_stride = pitch, frame_stride = 1."""
    return lambda cap, ch: torch.zeros((ch, cap + 5), dtype=dtype, device="cuda").t()[:cap]


def packed_offset(torch):
    """Packed 24-bit from a base 1 byte into an allocation: the byte-wise kernel."""
    return lambda cap, ch: torch.zeros(cap * ch * 3 + 1, dtype=torch.uint8, device="cuda")[1:].view(cap, ch, 3)


def packed_strided(torch):
    """Packed 24-bit rows with one unused sample per frame (frame stride ch + 1 samples)."""
    return lambda cap, ch: torch.zeros((cap, ch + 1, 3), dtype=torch.uint8, device="cuda")[:, :ch]


def stream(gar, torch, r, xd, make, bits=None, chunks=None, flush=True, start=0):
    """Process xd[start:] (in chunks) and flush into outputs from make(cap, channels); host array, calls' sizes."""
    L = gar.lib()
    ch = xd.shape[1]
    outs, s = [], start
    for n in (chunks or [xd.shape[0] - start]):
        cap = max(L.gar_device_output_size(r._h, n), 1)
        outs.append(r.process_device(xd[s:s + n], out=make(cap, ch), pcm_bits=bits).clone())
        s += n
    if flush:
        cap = max(L.gar_device_flush_size(r._h), 1)
        outs.append(r.flush_device(out=make(cap, ch), pcm_bits=bits).clone())
    torch.cuda.synchronize()
    y = torch.cat(outs)
    sizes = [int(o.shape[0]) for o in outs]
    if y.dtype == torch.uint8:
        return gar.unpack_pcm24(y).astype(np.int64), sizes
    a = y.cpu().numpy() if y.dtype != torch.bfloat16 else y.view(torch.int16).cpu().numpy()
    return (a.astype(np.int64) if not y.dtype.is_floating_point else a), sizes


def case(gar, torch, ch=2, compute="F32", rates=(44100, 48000), batch=0, n=N, kind="signal"):
    """The input tensor and the float output of one configuration, computed once per session."""
    key = (ch, compute, rates, batch, n, kind)
    if key not in _float_ref:
        total = ch * max(batch, 1)
        if kind == "square":  # full scale: overshoots after resampling (test_gpu_pcm.py test_pcm_clipping)
            sq = np.where((np.arange(n) // 50) % 2 == 0, 1.0, -1.0)
            x = np.stack([sq if c % 2 == 0 else -sq for c in range(total)], axis=1)
        else:
            x = signal(n, total, seed=11 + total)
        fdt = np.float64 if compute == "F64" else np.float32
        xd = torch.from_numpy(np.ascontiguousarray(x.astype(fdt))).cuda()
        r = _new(gar, ch, getattr(gar, compute), rates, batch)
        yf, _ = stream(gar, torch, r, xd, interleaved(torch, xd.dtype))
        _float_ref[key] = (xd, yf, r.num_stages())
    return _float_ref[key]


def dithered(gar, torch, xd, make, bits, ch=2, compute="F32", rates=(44100, 48000), batch=0, chunks=None, seed=SEED):
    r = _new(gar, ch, getattr(gar, compute), rates, batch)
    r.set_dither(gar.DITHER_TPDF, seed)
    return stream(gar, torch, r, xd, make, bits=bits, chunks=chunks)


def int_dtype(torch, bits):
    return torch.int16 if bits == 16 else torch.int32


def check(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_fused_equals_quantized_float_path(gar, cuda, bits):
    """Stereo f32 in, fused PCM out (bits 16: the stereo vector store; 24 / 32: the per-element store)."""
    xd, yf, _ = case(gar, cuda)
    got, _ = dithered(gar, cuda, xd, interleaved(cuda, int_dtype(cuda, bits)), bits)
    check(got, D.quantize_frames(yf, bits, SEED))


def test_ragged_chunks_are_bit_identical(gar, cuda):
    xd, yf, _ = case(gar, cuda)
    got, sizes = dithered(gar, cuda, xd, interleaved(cuda, cuda.int16), 16, chunks=chunk_sizes(N, 4096 + 17))
    assert len(sizes) > 10
    check(got, D.quantize_frames(yf, 16, SEED))


@pytest.mark.parametrize("layout", ["mono", "ch16", "planar"])
def test_layouts(gar, cuda, layout):
    ch = {"mono": 1, "ch16": 16, "planar": 2}[layout]
    xd, yf, _ = case(gar, cuda, ch=ch)
    make = planar(cuda, cuda.int16) if layout == "planar" else interleaved(cuda, cuda.int16)
    got, _ = dithered(gar, cuda, xd, make, 16, ch=ch)
    check(got, D.quantize_frames(yf, 16, SEED))


def test_staged_f64_pcm16(gar, cuda):
    """float64 compute: the conversion is staged through convert_kernel, quantizing the f64 samples."""
    xd, yf, _ = case(gar, cuda, compute="F64")
    got, _ = dithered(gar, cuda, xd, interleaved(cuda, cuda.int16), 16, compute="F64")
    check(got, D.quantize_frames(yf, 16, SEED))


@pytest.mark.parametrize("form", ["contiguous", "offset1", "strided"])
def test_staged_packed24(gar, cuda, form):
    """Packed 24-bit: interleaved contiguous with frames * channels % 4 != 0 (vector quads plus the byte-wise
    tail), from a base offset by one byte and with a strided layout (the per-element kernel)."""
    ch = 3
    xd, yf, _ = case(gar, cuda, ch=ch, n=N + 1)  # 47865 frames out of the process call: 3 samples after the last quad
    make = {"contiguous": interleaved(cuda, cuda.uint8), "offset1": packed_offset(cuda), "strided": packed_strided(cuda)}[form]
    got, sizes = dithered(gar, cuda, xd, make, None, ch=ch)
    assert any((s * ch) % 4 for s in sizes), sizes
    check(got, D.quantize_frames(yf, 24, SEED))


def test_staged_multi_stage_plan(gar, cuda):
    """96k -> 16k QualityHigh on the New path: more than one stage, the last one's output converted."""
    xd, yf, stages = case(gar, cuda, rates=(96000, 16000), n=96000 + 123)
    assert stages > 1
    got, _ = dithered(gar, cuda, xd, interleaved(cuda, cuda.int16), 16, rates=(96000, 16000))
    check(got, D.quantize_frames(yf, 16, SEED))


def test_batch_channel_keys(gar, cuda):
    """NewBatch of 3 stereo streams: channel stream * 2 + ch of the handle has key(stream * 2 + ch)."""
    xd, yf, _ = case(gar, cuda, batch=3)
    assert yf.shape[1] == 6
    got, _ = dithered(gar, cuda, xd, interleaved(cuda, cuda.int16), 16, batch=3)
    check(got, D.quantize_frames(yf, 16, SEED))
    assert not np.array_equal(got[:, 0], D.quantize(yf[:, 0].astype(np.float64), 16, SEED, 2, 0))


def test_state_resume_and_reset(gar, cuda):
    """Process A, save_state, fresh handle + set_dither + load_state, process B + flush == the uninterrupted
    run; Reset followed by the same input == a fresh handle."""
    xd, yf, _ = case(gar, cuda)
    want = D.quantize_frames(yf, 16, SEED)
    make = interleaved(cuda, cuda.int16)
    a = _new(gar, 2, gar.F32)
    a.set_dither(gar.DITHER_TPDF, SEED)
    cut = 20000 + 1
    ya, _ = stream(gar, cuda, a, xd[:cut], make, bits=16, flush=False)
    blob = a.save_state()
    b = _new(gar, 2, gar.F32)
    b.set_dither(gar.DITHER_TPDF, SEED)
    b.load_state(blob)
    assert b.get_dither() == (gar.DITHER_TPDF, SEED, ya.shape[0])
    yb, _ = stream(gar, cuda, b, xd, make, bits=16, start=cut)
    check(np.concatenate([ya, yb]), want)
    b.Reset()
    assert b.get_dither() == (gar.DITHER_TPDF, SEED, 0)
    again, _ = stream(gar, cuda, b, xd, make, bits=16)
    check(again, want)


def test_off_means_off(gar, cuda):
    """TPDF then NONE: today's truncated bytes; f32 and f16 outputs are bit-identical with dither on and off."""
    xd, yf, _ = case(gar, cuda)
    r = _new(gar, 2, gar.F32)
    r.set_dither(gar.DITHER_TPDF, SEED)
    r.set_dither(gar.DITHER_NONE, 0)
    got, _ = stream(gar, cuda, r, xd, interleaved(cuda, cuda.int16), bits=16)
    trunc = np.trunc(np.clip(yf.astype(np.float64), -1.0, 1.0) * 32767.0).astype(np.int64)
    check(got, trunc)
    on32, _ = dithered(gar, cuda, xd, interleaved(cuda, cuda.float32), None)
    assert np.array_equal(on32.view(np.uint32), yf.view(np.uint32))
    on16, _ = dithered(gar, cuda, xd, interleaved(cuda, cuda.float16), None)
    off16, _ = stream(gar, cuda, _new(gar, 2, gar.F32), xd, interleaved(cuda, cuda.float16))
    assert np.array_equal(on16.view(np.uint16), off16.view(np.uint16))


def test_seeds(gar, cuda):
    """Two seeds give different bytes, the same seed twice the same bytes."""
    xd, yf, _ = case(gar, cuda)
    make = interleaved(cuda, cuda.int16)
    a, _ = dithered(gar, cuda, xd, make, 16, seed=1)
    b, _ = dithered(gar, cuda, xd, make, 16, seed=2)
    c, _ = dithered(gar, cuda, xd, make, 16, seed=1)
    assert np.array_equal(a, c)
    assert np.mean(a != b) > 0.2
    check(b, D.quantize_frames(yf, 16, 2))


def test_full_scale_square_clips(gar, cuda):
    """A full-scale square overshoots after resampling: the dithered output reaches exactly +-32767, never wraps."""
    xd, yf, _ = case(gar, cuda, n=44100, kind="square")
    assert np.abs(yf).max() > 1.0
    got, _ = dithered(gar, cuda, xd, interleaved(cuda, cuda.int16), 16)
    assert got.max() == 32767 and got.min() == -32767
    check(got, D.quantize_frames(yf, 16, SEED))


def _with_samples_out(blob, pos):
    """A state blob with group 0's samplesOut replaced (DESIGN.md "State snapshots": 104 header bytes, then the
    group's c0, C, samplesIn, samplesOut; the last 8 bytes are the checksum of everything before them)."""
    import struct
    b = bytearray(blob)
    b[104 + 16:104 + 24] = struct.pack("<q", pos)
    h, mask = 0x6A09E667F3BCC908, (1 << 64) - 1
    for (w,) in struct.iter_unpack("<Q", bytes(b[:-8])):
        h = ((h ^ w) * 0x9E3779B97F4A7C15) & mask
        h ^= h >> 32
    b[-8:] = struct.pack("<Q", h)
    return bytes(b)


@pytest.mark.parametrize("back", [1000, 1001])
def test_positions_across_2_pow_32(gar, cuda, back):
    """A fresh stream whose samplesOut is set (through a state blob) just below 2^32: the first call's stores
    cross the boundary where hi32(n) changes -- with an odd start inside one lane's frame pair of the stereo
    vector store."""
    xd, yf, _ = case(gar, cuda)
    n0 = 2 ** 32 - back
    r = _new(gar, 2, gar.F32)
    r.set_dither(gar.DITHER_TPDF, SEED)
    r.load_state(_with_samples_out(r.save_state(), n0))
    assert r.get_dither()[2] == n0
    got, _ = stream(gar, cuda, r, xd, interleaved(cuda, cuda.int16), bits=16)
    check(got, D.quantize_frames(yf, 16, SEED, n0=n0))
    assert r.get_dither()[2] == n0 + got.shape[0]
