"""Streams, layouts and cached float references for test_gpu_meter.py (its own copy, so an edit of another test
module's helpers does not change what the meter tests cover).

case(): the input tensor and the float output of one configuration, computed once per session and never modified.
"""
import numpy as np

from helpers import signal

N = 44100 + 123
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


def int_dtype(torch, bits):
    return torch.int16 if bits == 16 else torch.int32
