"""Wall time of gar_state_save / gar_state_load on the GPU.

Handles: the stereo 44.1k -> 48k QualityHigh GAR_F32 handle, a batch of 1024 such streams (2048
channels) -- one live history each -- and two handles with several segments: a batch of 128 stereo
96k -> 16k QualityHigh streams (multi-stage) and one of 128 stereo 16k -> 44.1k streams (stage-by-stage,
both histories live), each after one 4096-frame process_device call.  Both calls are synchronous, so the time is a
host clock around the C-ABI call (a reused caller buffer: no Python allocation inside the window), the
device idle before it (`synchronize()` first) -- the wait for enqueued work is the caller's pipeline, not
the snapshot's cost.  `--warmup` untimed rounds (the first save allocates the device image), then
`--repeats` rounds of save, load into the same handle (a rewind), load into a second handle; medians
and quartiles in microseconds.

  python tools/state_timing.py [--repeats 50] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "go-audio-resampler_amd")]


def timed(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e6


def quart(v):
    q = statistics.quantiles(v, n=4)
    return {"median_us": round(statistics.median(v), 1), "q1_us": round(q[0], 1), "q3_us": round(q[2], 1),
            "min_us": round(min(v), 1)}


def measure(in_rate, out_rate, streams, repeats, warmup):
    import torch
    import gar

    cfg = gar.Config(in_rate, out_rate, 2, gar.QualityHigh, ComputeDtype=gar.F32)
    mk = (lambda: gar.New(cfg)) if streams == 1 else (lambda: gar.NewBatch(cfg, streams))
    a, b = mk(), mk()
    g = torch.Generator(device="cuda").manual_seed(99)
    x = (torch.rand((4096, 2 * streams), device="cuda", generator=g) - 0.5) * 1.6
    a.process_device(x)
    a.synchronize()
    n = a.state_size()
    buf = (C.c_ubyte * n)()
    got = C.c_int64(0)
    L = gar.lib()

    def save():
        assert L.gar_state_save(a._h, buf, n, C.byref(got)) == 0 and got.value == n

    def load(h):
        assert L.gar_state_load(h._h, buf, n) == 0

    rows = {"save": [], "load_same_handle": [], "load_other_handle": []}
    for k in range(warmup + repeats):
        a.synchronize()
        t = [timed(save), timed(lambda: load(a)), timed(lambda: load(b))]
        if k >= warmup:
            for key, v in zip(rows, t):
                rows[key].append(v)
    assert b.save_state() == bytes(buf)
    segments = sum(1 for i in range(a.num_stages()) for k in (0, 1)
                   if int.from_bytes(bytes(buf)[104 + 24 + 144 * i + 80 + 32 * k + 24:][:8], "little"))
    return {"rates": [in_rate, out_rate], "stages": a.num_stages(), "segments": segments, "streams": streams, "channels": 2 * streams, "blob_bytes": n, **{k: quart(v) for k, v in rows.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "state_timing.py measures on a GPU"
    res = [measure(i, o, s, args.repeats, args.warmup)
           for i, o, s in ((44100, 48000, 1), (44100, 48000, 1024), (96000, 16000, 128), (16000, 44100, 128))]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
