"""GPU: the clip counter / peak meter (gar.h gar_set_meter) on every integer PCM store path of the device calls.

Expected values never come from the meter: they are computed from the SAME configuration's float output
(test_gpu_pcm.py / test_gpu_dither.py establish that the PCM stores quantize exactly those samples) --
clips = count(|yf| > 1) per channel, peak = max |yf| per channel as float64 -- plus, with dither on, the
second-clamp hits counted by the numpy restatement in meter_ref.py.  Expected and measured rest on the same
float samples, so every comparison is exact equality.

Streams are 44100 + 123 frames of a full-scale square (meter_gpu_helpers.case, the shapes of test_gpu_dither.py) (44.1k -> 48k QualityHigh unless
said), which overshoots after resampling: interior row blocks, edge blocks and a flush tail.  Kernels reached
(GAR_HX_TRACE): a one-shot f32 stereo call and its flush run hxs_kernel and hxs_small_kernel; the ragged
4096 + 17 frame f32 calls run hxq_kernel; int16 input calls run hxs_small_kernel (hxq_kernel takes f32 input only).
"""
import numpy as np
import pytest

import meter_gpu_helpers as TD
import meter_ref as M
from helpers import chunk_sizes, signal

pytestmark = pytest.mark.gpu

N = TD.N
SEED = 7


def run(gar, torch, r, xd, make, bits=None, chunks=None, per_call=False, flush=True):
    """Process xd (in chunks) and flush through handle r; (host integers, [(clips, peak) read with reset after each call])."""
    L = gar.lib()
    ch = xd.shape[1]
    outs, parts, s = [], [], 0
    for n in (chunks or [xd.shape[0]]):
        cap = max(L.gar_device_output_size(r._h, n), 1)
        outs.append(r.process_device(xd[s:s + n], out=make(cap, ch), pcm_bits=bits).clone())
        s += n
        if per_call:
            parts.append(r.meter_read(reset=True))
    if flush:
        cap = max(L.gar_device_flush_size(r._h), 1)
        outs.append(r.flush_device(out=make(cap, ch), pcm_bits=bits).clone())
        if per_call:
            parts.append(r.meter_read(reset=True))
    torch.cuda.synchronize()
    y = torch.cat(outs)
    if y.dtype == torch.uint8:
        return gar.unpack_pcm24(y).astype(np.int64), parts
    return y.cpu().numpy().astype(np.int64), parts


def expect(yf, bits=16, dither=False, clipping=None):
    """(clips, peak) per channel from the float output; asserts the expectation itself clips where it is meant to."""
    clips, peak = M.tally_frames(yf, bits, dither, SEED)
    for c in (range(yf.shape[1]) if clipping is None else clipping):
        assert clips[c] > 0, (c, clips.tolist())
    return clips, peak


def same(got, want):
    assert got[0].dtype == np.uint64 and got[1].dtype == np.float64
    assert got[0].tolist() == want[0].tolist(), (got[0].tolist(), want[0].tolist())
    assert got[1].view(np.uint64).tolist() == want[1].view(np.uint64).tolist(), (got[1].tolist(), want[1].tolist())


def metered(gar, ch=2, compute="F32", rates=(44100, 48000), batch=0, dither=False):
    r = TD._new(gar, ch, getattr(gar, compute), rates, batch)
    r.set_meter(True)
    if dither:
        r.set_dither(gar.DITHER_TPDF, SEED)
    return r


def sum_parts(parts):
    return (np.sum([p[0] for p in parts], axis=0, dtype=np.uint64), np.max([p[1] for p in parts], axis=0))


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_fused_stereo_one_shot_and_ragged_chunks(gar, cuda, bits):
    """Stereo f32 in, fused PCM out (16: the stereo frame-pair vector store, VST 4; 24 / 32: the per-element store,
    VST 0).  One shot: hxs_kernel (+ hxs_small_kernel for the flush tail); chunks of 4096 + 17 frames: hxq_kernel.
    The totals over the calls equal the one-shot totals, and so do the sum and the maximum of per-call reads with reset."""
    xd, yf, _ = TD.case(gar, cuda, kind="square")
    want = expect(yf, bits)
    make = TD.interleaved(cuda, TD.int_dtype(cuda, bits))
    r = metered(gar)
    run(gar, cuda, r, xd, make, bits)
    same(r.meter_read(), want)
    same(r.meter_read(reset=True), want)  # a read without reset left them
    same(r.meter_read(), (np.zeros(2, np.uint64), np.zeros(2)))
    chunks = chunk_sizes(N, 4096 + 17)
    r = metered(gar)
    run(gar, cuda, r, xd, make, bits, chunks=chunks)
    same(r.meter_read(), want)
    r = metered(gar)
    _, parts = run(gar, cuda, r, xd, make, bits, chunks=chunks, per_call=True)
    assert len(parts) == len(chunks) + 1 and sum(int(p[0].sum() > 0) for p in parts) > 3
    same(sum_parts(parts), want)
    same(r.meter_read(), (np.zeros(2, np.uint64), np.zeros(2)))


def test_fused_pcm16_in_small_calls(gar, cuda):
    """PCM16 in, PCM16 out, calls of 1024 + 3 frames: hxs_small_kernel (integer input is not hxq_kernel's)."""
    n = 12000 + 5
    sq = np.where((np.arange(n) // 50) % 2 == 0, 32767, -32767).astype(np.int16)
    xd = cuda.from_numpy(np.stack([sq, -sq], axis=1)).cuda()
    chunks = chunk_sizes(n, 1024 + 3)
    yf, _ = TD.stream(gar, cuda, TD._new(gar, 2, gar.F32), xd, TD.interleaved(cuda, cuda.float32), chunks=chunks)
    want = expect(yf)
    r = metered(gar)
    _, parts = run(gar, cuda, r, xd, TD.interleaved(cuda, cuda.int16), 16, chunks=chunks, per_call=True)
    same(sum_parts(parts), want)


@pytest.mark.parametrize("layout", ["mono", "ch3", "ch16", "planar"])
def test_layouts(gar, cuda, layout):
    ch = {"mono": 1, "ch3": 3, "ch16": 16, "planar": 2}[layout]
    xd, yf, _ = TD.case(gar, cuda, ch=ch, kind="square")
    make = TD.planar(cuda, cuda.int16) if layout == "planar" else TD.interleaved(cuda, cuda.int16)
    r = metered(gar, ch)
    run(gar, cuda, r, xd, make, 16)
    same(r.meter_read(), expect(yf))


def test_staged_f64_pcm16(gar, cuda):
    """float64 compute: the conversion is staged (the metered twin of convert_kernel), tallying the f64 samples."""
    xd, yf, _ = TD.case(gar, cuda, compute="F64", kind="square")
    r = metered(gar, compute="F64")
    run(gar, cuda, r, xd, TD.interleaved(cuda, cuda.int16), 16, chunks=chunk_sizes(N, 20000 + 1))
    same(r.meter_read(), expect(yf))


@pytest.mark.parametrize("form", ["contiguous", "offset1", "strided"])
def test_staged_packed24(gar, cuda, form):
    """Packed 24-bit, 3 channels: contiguous with frames * channels % 4 != 0 (the vector quads and the byte-wise tail
    of pack24's metered twin), from a base offset by one byte and strided (the per-element kernel's twin)."""
    ch = 3
    xd, yf, _ = TD.case(gar, cuda, ch=ch, n=N + 1, kind="square")
    make = {"contiguous": TD.interleaved(cuda, cuda.uint8), "offset1": TD.packed_offset(cuda),
            "strided": TD.packed_strided(cuda)}[form]
    r = metered(gar, ch)
    L = gar.lib()
    assert (L.gar_device_output_size(r._h, N + 1) * ch) % 4
    run(gar, cuda, r, xd, make)
    same(r.meter_read(), expect(yf, 24))


def test_staged_multi_stage_plan(gar, cuda):
    """96k -> 16k QualityHigh: more than one stage, the last one's output converted and tallied."""
    xd, yf, stages = TD.case(gar, cuda, rates=(96000, 16000), n=96000 + 123, kind="square")
    assert stages > 1
    r = metered(gar, rates=(96000, 16000))
    run(gar, cuda, r, xd, TD.interleaved(cuda, cuda.int16), 16)
    same(r.meter_read(), expect(yf))


def test_batch_channel_separation(gar, cuda):
    """NewBatch of 3 stereo streams, handle channel = stream * 2 + ch: the odd channels carry the square, the even
    ones a signal at 0.25 scale -- 0 clips and their own peak there, the exact counts on the odd ones; and a read
    with reset of channels 1 .. 2 zeroes exactly those."""
    sq = np.where((np.arange(N) // 50) % 2 == 0, 1.0, -1.0)
    quiet = 0.25 * signal(N, 6, seed=5)
    x = np.stack([sq if c % 2 else quiet[:, c] for c in range(6)], axis=1).astype(np.float32)
    xd = cuda.from_numpy(np.ascontiguousarray(x)).cuda()
    yf, _ = TD.stream(gar, cuda, TD._new(gar, 2, gar.F32, batch=3), xd, TD.interleaved(cuda, cuda.float32))
    want = expect(yf, clipping=[1, 3, 5])
    assert want[0][0::2].tolist() == [0, 0, 0] and len(set(want[1].tolist())) >= 4
    r = metered(gar, batch=3)
    run(gar, cuda, r, xd, TD.interleaved(cuda, cuda.int16), 16, chunks=chunk_sizes(N, 16384 + 3))
    same(r.meter_read(), want)
    same(r.meter_read(1, 2, reset=True), (want[0][1:3], want[1][1:3]))
    left = (want[0].copy(), want[1].copy())
    left[0][1:3] = 0
    left[1][1:3] = 0.0
    same(r.meter_read(), left)


@pytest.mark.parametrize("ch", [2, 3])
@pytest.mark.parametrize("chunked", [False, True])
def test_exact_fallback_is_tallied_once(gar, cuda, ch, chunked):
    """f32 input with one sample of 20.0, one +Inf and one NaN in different blocks (and different channels; with two
    channels the NaN shares the 20.0's), the +Inf ten frames before a 4096-frame chunk boundary.  The blocks holding
    them store MFMA values first, then the exact fallback overwrites the outputs whose windows hold them: clips and
    peak equal those of the float output (NaN excluded), so nothing is counted twice or with the overwritten value;
    the +Inf channel's peak is +Inf."""
    x = (0.9 * signal(N, ch, seed=23)).astype(np.float32)
    x[5000, 0] = 20.0
    x[3 * 4096 - 10, 1] = np.inf
    x[30000, ch - 1 if ch > 2 else 0] = np.nan
    xd = cuda.from_numpy(np.ascontiguousarray(x)).cuda()
    chunks = chunk_sizes(N, 4096) if chunked else None
    yf, _ = TD.stream(gar, cuda, TD._new(gar, ch, gar.F32), xd, TD.interleaved(cuda, cuda.float32), chunks=chunks)
    assert np.isnan(yf).any() and np.isinf(yf[:, 1]).any()
    want = expect(yf, clipping=[0, 1])
    assert want[1][1] == np.inf and np.isfinite(want[1][0]) and want[1][0] > 1.0
    r = metered(gar, ch)
    got, _ = run(gar, cuda, r, xd, TD.interleaved(cuda, cuda.int16), 16, chunks=chunks)
    same(r.meter_read(), want)
    with np.errstate(invalid="ignore"):
        trunc = np.trunc(np.clip(yf.astype(np.float64), -1.0, 1.0) * 32767.0)
    assert np.array_equal(got, np.where(np.isnan(trunc), 0.0, trunc).astype(np.int64))


@pytest.mark.parametrize("path", ["fused16", "fused24", "staged_f64", "packed24"])
def test_dither_on_adds_second_clamp_hits(gar, cuda, path):
    """With TPDF dither the clips are the numpy count including the second clamp; the peak is that of dither off."""
    ch, compute, bits, dt = {"fused16": (2, "F32", 16, cuda.int16), "fused24": (2, "F32", 24, cuda.int32),
                             "staged_f64": (2, "F64", 16, cuda.int16), "packed24": (3, "F32", 24, cuda.uint8)}[path]
    n = N + 1 if path == "packed24" else N
    xd, yf, _ = TD.case(gar, cuda, ch=ch, compute=compute, n=n, kind="square")
    want = expect(yf, bits, dither=True)
    plain = expect(yf, bits)
    assert want[1].tolist() == plain[1].tolist() and (want[0] >= plain[0]).all()
    r = metered(gar, ch, compute, dither=True)
    run(gar, cuda, r, xd, TD.interleaved(cuda, dt), None if path == "packed24" else bits, chunks=chunk_sizes(n, 16384 + 3))
    same(r.meter_read(), want)


def test_second_clamp_on_the_device(gar, cuda):
    """A DC input of 0.99999 settles just below full scale, where the first clamp never fires and only the dithered
    quantizer's second clamp decides (d >= 0.83 or so: about 1.4 % of the samples).  The numpy side shows those hits
    beyond the first clamp's; the device count equals it."""
    xd = cuda.full((N, 2), 0.99999, dtype=cuda.float32, device="cuda")
    yf, _ = TD.stream(gar, cuda, TD._new(gar, 2, gar.F32), xd, TD.interleaved(cuda, cuda.float32))
    want = M.tally_frames(yf, 16, True, SEED)
    assert (want[0] > M.tally_frames(yf, 16, False)[0] + 100).all()
    r = metered(gar, dither=True)
    run(gar, cuda, r, xd, TD.interleaved(cuda, cuda.int16), 16)
    same(r.meter_read(), want)


@pytest.mark.parametrize("path", ["fused16", "staged_f64", "packed24"])
def test_stored_bytes_do_not_change(gar, cuda, path):
    """Meter on and meter off store identical bytes; with the meter off (never on) a read gives zeros."""
    ch, compute, bits, dt = {"fused16": (2, "F32", 16, cuda.int16), "staged_f64": (2, "F64", 16, cuda.int16),
                             "packed24": (3, "F32", None, cuda.uint8)}[path]
    n = N + 1 if path == "packed24" else N
    xd, _, _ = TD.case(gar, cuda, ch=ch, compute=compute, n=n, kind="square")
    chunks = chunk_sizes(n, 8192 + 5)
    off = TD._new(gar, ch, getattr(gar, compute))
    a, _ = run(gar, cuda, off, xd, TD.interleaved(cuda, dt), bits, chunks=chunks)
    same(off.meter_read(), (np.zeros(ch, np.uint64), np.zeros(ch)))
    on = metered(gar, ch, compute)
    b, _ = run(gar, cuda, on, xd, TD.interleaved(cuda, dt), bits, chunks=chunks)
    assert np.array_equal(a, b)
    assert on.meter_read()[0].min() > 0


def test_reset_zeroes_load_state_leaves(gar, cuda):
    """Reset zeroes the tallies and keeps the setting; load_state leaves the tallies alone; turning the meter off
    stops the tallying."""
    xd, yf, _ = TD.case(gar, cuda, kind="square")
    want = expect(yf)
    make = TD.interleaved(cuda, cuda.int16)
    r = metered(gar)
    blob = r.save_state()
    run(gar, cuda, r, xd, make, 16)
    same(r.meter_read(), want)
    r.load_state(blob)
    assert r.get_meter() is True
    same(r.meter_read(), want)
    r.Reset()
    assert r.get_meter() is True
    same(r.meter_read(), (np.zeros(2, np.uint64), np.zeros(2)))
    run(gar, cuda, r, xd, make, 16)
    same(r.meter_read(), want)
    r.set_meter(False)
    r.Reset()
    run(gar, cuda, r, xd, make, 16)
    same(r.meter_read(), (np.zeros(2, np.uint64), np.zeros(2)))
