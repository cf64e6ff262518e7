"""GPU: state snapshots (gar.h gar_state_save / gar_state_load) of real handles -- the history rows
gathered by one launch (launchStatePack) and scattered by one (launchStateUnpack).

Scheme of every case: handle A processes chunk 1, saves, processes chunk 2 and flushes; a fresh
handle B loads the blob, processes chunk 2 and flushes; then A loads its own blob (rewind) and does
the same again.  All three continuations must be byte-identical (np.array_equal on the raw arrays)
with equal statistics, and B's state after them must be A's.  The bar is exact equality: a snapshot
holds the histories bit for bit, and the kernels are deterministic.

Shapes are the smallest that reach each path: chunk 1 of 1000 and 4099 frames (4099 rows of an odd
channel count end off a 16-byte boundary: the element-wise tail of the copy kernel), chunk 2 of
3000 frames; 33 and 5 channels give rows that are no multiple of 16 bytes.

The host Process of the ABI (gar_process_f64, Go's Process) advances channel 0; that is the
per-channel call that splits a multi-channel handle here.  No test provokes a device error.
"""
import numpy as np
import pytest

from helpers import signal

pytestmark = pytest.mark.gpu

CHUNK2 = 3000


def raw(t):
    """A device tensor's bytes as numpy (half types through their bit patterns)."""
    import torch
    t = t.contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        t = t.view(torch.int16)
    return t.cpu().numpy().copy()


def tdtype(torch, compute, gar):
    return torch.float64 if compute == gar.F64 else torch.float32


def process(r, x, out_dtype=None):
    """process_device with an output of out_dtype (default: x's)."""
    import torch
    if out_dtype is None:
        return r.process_device(x)
    n = r.OutputSize(x.shape[0])
    return r.process_device(x, out=torch.empty((max(n, 1), x.shape[1]), dtype=out_dtype, device="cuda"))


def tail(r, x2, out_dtype=None):
    """chunk 2 + flush on the device; raw outputs and the statistics after them."""
    od = out_dtype or x2.dtype
    a = raw(process(r, x2, out_dtype))
    b = raw(r.flush_device(dtype=od))
    r.synchronize()
    return a, b, [r.GetStatistics(c) for c in (0, r.Channels - 1)]


def same(p, q):
    assert len(p) == len(q)
    for a, b in zip(p[:2], q[:2]):
        assert a.dtype == b.dtype and a.shape == b.shape, (a.shape, b.shape)
        assert np.array_equal(a, b), int(np.count_nonzero(a != b))
    assert p[2] == q[2]


def scheme(gar, torch, mk, x, n1, head=None, out_dtype=None):
    """The common scheme; `head(r, x1)` brings a handle to the save point (default: process chunk 1).
    Returns the blob."""
    x1, x2 = x[:n1], x[n1:n1 + CHUNK2]
    assert x2.shape[0] == CHUNK2
    head = head or (lambda r, x1: r.process_device(x1))
    a = mk()
    head(a, x1)
    size = a.state_size()
    blob = a.save_state()
    assert len(blob) == size and a.save_state() == blob
    ya = tail(a, x2, out_dtype)
    assert ya[0].shape[0] > 0 or n1 == 0
    b = mk()
    b.load_state(blob)
    assert b.save_state() == blob                     # save -> load -> save: identical bytes
    yb = tail(b, x2, out_dtype)
    same(ya, yb)
    assert a.save_state() == b.save_state()
    a.load_state(blob)                                # rewind
    same(ya, tail(a, x2, out_dtype))
    return blob


def material(torch, n1, ch, dtype, rate):
    x = signal(n1 + CHUNK2, ch, rate=float(rate), seed=77 + ch)
    return torch.from_numpy(x).to(dtype).cuda()


# (id, in rate, out rate, preset, channels, compute)
def _cases():
    F64, F32, EX = 0, 1, 2
    return [
        ("44k1_48k_high_stereo_f32", 44100, 48000, 3, 2, F32),       # split-f16 streaming kernels
        ("44k1_48k_high_stereo_f64", 44100, 48000, 3, 2, F64),
        ("44k1_48k_high_stereo_f32exact", 44100, 48000, 3, 2, EX),
        ("48k_44k1_veryhigh_33ch_f32", 48000, 44100, 4, 33, F32),    # wide rows, odd C
        ("16k_44k1_high_5ch_f64", 16000, 44100, 3, 5, F64),          # stage-by-stage: xh and uh live, odd C
        ("96k_44k1_veryhigh_8ch_f64", 96000, 44100, 4, 8, F64),
        ("96k_16k_high_2ch_f32", 96000, 16000, 3, 2, F32),
        ("24k_48k_high_mono_f32", 24000, 48000, 3, 1, F32),
        ("44k1_48k_quick_stereo_f32", 44100, 48000, 0, 2, F32),
    ]


CASES = _cases()


@pytest.mark.parametrize("n1", [1000, 4099])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_save_load_continues_bit_identically(gar, cuda, case, n1):
    torch = cuda
    _, i, o, preset, ch, compute = case
    x = material(torch, n1, ch, tdtype(torch, compute, gar), i)
    blob = scheme(gar, torch, lambda: gar.New(gar.Config(i, o, ch, preset, ComputeDtype=compute)), x, n1)
    assert blob[12] == 0                              # a real handle's blob
    dry = gar.New(gar.Config(i, o, ch, preset, ComputeDtype=compute, DryRun=True))
    assert len(blob) > dry.state_size()               # rows are in it


@pytest.mark.parametrize("n1", [1000, 4099])
def test_batch_of_streams(gar, cuda, n1):
    torch = cuda
    x = material(torch, n1, 6, torch.float32, 44100)
    scheme(gar, torch, lambda: gar.NewBatch(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32), 3), x, n1)


@pytest.mark.parametrize("n1", [1000, 4099])
def test_io_types_are_not_state(gar, cuda, n1):
    """PCM16 in, f16 out: the blob equals the one of the float-I/O run fed the same material converted
    to PCM16 on the host first, and the continuation (f16 outputs) is byte-identical."""
    torch = cuda
    mk = lambda: gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))  # noqa: E731
    pcm = np.round(np.clip(signal(n1 + CHUNK2, 2, seed=5), -1, 1) * 32767.0 * 0.98).astype(np.int16)
    xp = torch.from_numpy(pcm).cuda()
    xf = torch.from_numpy((pcm.astype(np.float64) * (1.0 / 32767.0)).astype(np.float32)).cuda()

    blob_pcm = scheme(gar, torch, mk, xp, n1, head=lambda r, x1: process(r, x1, torch.float16), out_dtype=torch.float16)
    f = mk()
    f.process_device(xf[:n1])
    assert f.save_state() == blob_pcm


def test_short_history(gar, cuda):
    """chunk 1 of 50 frames: every history is shorter than its stage's taps."""
    torch = cuda
    for compute, ch in ((gar.F32, 2), (gar.F64, 3)):
        x = material(torch, 50, ch, tdtype(torch, compute, gar), 44100)
        scheme(gar, torch, lambda: gar.New(gar.Config(44100, 48000, ch, gar.QualityHigh, ComputeDtype=compute)), x, 50)


def test_never_used_handle(gar, cuda):
    torch = cuda
    x = material(torch, 0, 2, torch.float32, 44100)
    mk = lambda: gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))  # noqa: E731
    blob = scheme(gar, torch, mk, x, 0, head=lambda r, x1: None)
    used = mk()
    used.process_device(x[:777])
    used.Reset()
    assert used.save_state() == blob


@pytest.mark.parametrize("compute", [1, 0], ids=["f32", "f64"])
def test_save_after_flush_then_process(gar, cuda, compute):
    """Flush then Process: the fused stage has fallen back to stage-by-stage with zero histories, then
    live ones; both save points continue byte-identically."""
    torch = cuda
    x = material(torch, 1000, 2, tdtype(torch, compute, gar), 44100)
    mk = lambda: gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=compute))  # noqa: E731

    def flushed(r, x1):
        r.process_device(x1)
        r.flush_device(dtype=x1.dtype)
        assert not r.stage_state(0)[1]                 # no longer on the fused plan

    def flushed_then_processed(r, x1):
        flushed(r, x1)
        r.process_device(x1[:600])

    zero = scheme(gar, torch, mk, x, 1000, head=flushed)
    live = scheme(gar, torch, mk, x, 1000, head=flushed_then_processed)
    assert len(live) > len(zero)                      # zero histories store no rows


@pytest.mark.parametrize("compute", [0, 1], ids=["f64", "f32"])
def test_split_handle(gar, cuda, compute):
    cfg = dict(InputRate=44100, OutputRate=48000, Channels=3, Quality=3, ComputeDtype=compute)
    x = signal(1200 + 640 + CHUNK2, 3, seed=9)
    a = gar.New(gar.Config(**cfg))
    a.ProcessMulti([x[:1200, c] for c in range(3)])
    a.Process(x[1200:1840, 0])                         # channel 0 alone: groups {0}, {1, 2}
    blob = a.save_state()
    b = gar.New(gar.Config(**cfg))
    b.load_state(blob)
    assert b.save_state() == blob
    assert gar.lib().gar_device_output_size(a._h, 100) == -1 == gar.lib().gar_device_output_size(b._h, 100)
    x2 = [x[1840:, c] for c in range(3)]
    ya, yb = a.ProcessMulti(x2) + a.FlushMulti(), b.ProcessMulti(x2) + b.FlushMulti()
    assert a.GetStatistics(0) != a.GetStatistics(1)
    for p, q in zip(ya, yb):
        assert p.shape == q.shape and p.size and np.array_equal(p, q)
    assert [a.GetStatistics(c) for c in range(3)] == [b.GetStatistics(c) for c in range(3)]
    a.load_state(blob)                                 # rewind
    for p, q in zip(ya, a.ProcessMulti(x2) + a.FlushMulti()):
        assert np.array_equal(p, q)


def test_save_is_ordered_after_enqueued_calls(gar, cuda):
    """process_device on a non-default stream, save_state at once: the blob is the one saved after a
    synchronize()."""
    torch = cuda
    n = 200000
    x = torch.from_numpy(signal(n, 2, seed=3).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    mk = lambda: gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))  # noqa: E731
    s = torch.cuda.Stream()
    a, b = mk(), mk()
    ya = a.process_device(x, stream=s.cuda_stream)
    blob = a.save_state()                              # no explicit synchronise
    yb = b.process_device(x, stream=s.cuda_stream)
    b.synchronize()
    assert b.save_state() == blob
    torch.cuda.synchronize()
    assert np.array_equal(raw(ya), raw(yb))
    # a load right after an enqueued call on another stream is ordered after it too
    s2 = torch.cuda.Stream()
    a.process_device(x[:5000], stream=s2.cuda_stream)
    a.load_state(blob)
    assert a.save_state() == blob


def test_save_is_ordered_after_calls_on_two_streams(gar, cuda):
    """A handle used on a second stream orders its calls by an event from then on: save_state and
    load_state right after such calls wait for that event (the other branch of the wait above)."""
    torch = cuda
    x = torch.from_numpy(signal(150000, 2, seed=4).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    mk = lambda: gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))  # noqa: E731
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c, d = mk(), mk()
    outs = []
    for r in (c, d):
        outs.append(r.process_device(x[:50000], stream=s1.cuda_stream))
        outs.append(r.process_device(x[50000:], stream=s2.cuda_stream))   # the switch: events from here on
        if r is d:
            r.synchronize()
        blob = r.save_state()                          # c: no explicit synchronise
        outs.append(blob)
    assert outs[2] == outs[5]
    torch.cuda.synchronize()
    assert np.array_equal(raw(outs[0]), raw(outs[3])) and np.array_equal(raw(outs[1]), raw(outs[4]))
    y = c.process_device(x[:70000], stream=s1.cuda_stream)                 # records the event again
    c.load_state(outs[2])                              # ordered after it, then rewinds
    assert c.save_state() == outs[2]
    y2 = c.process_device(x[:70000], stream=s2.cuda_stream)
    c.synchronize()
    assert np.array_equal(raw(y), raw(y2))
