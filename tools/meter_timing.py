"""Wall and FIR-kernel time of the clip / peak meter (gar.h gar_set_meter) on the headline plan's PCM16 store.

Workload: stereo 44.1k -> 48k QualityHigh, GAR_F32 compute, f32 input, PCM16 output fused into the streaming
kernels' stores.  Rows, each with the meter off and on in the SAME build, alternating round by round so the pair
sees the same clocks and neighbours:

  long   a `--seconds` (default 600) stream in one process_device + flush_device (hxs_kernel / hxs_meter_kernel)
  chunk  `--calls` (default 200) process_device calls of 4096 frames (hxq_kernel / hxq_meter_kernel)

Wall time: torch.cuda.Event pairs around a row; `--repeats` (at least 5) timed rounds after `--warmup`.  FIR time
of the long row: gar_profile_read of kind 0 in a separate pass.  Printed per row: median, quartiles and range with
the meter off and on, and the per-round difference on - off.  The spread of the off rounds is what the on - off
difference is judged by.  The tallies are read once at the end (not timed) and printed, so a run shows it metered.

  python tools/meter_timing.py [--seconds 600] [--calls 200] [--repeats 7] [--warmup 2] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "go-audio-resampler_amd")]


def quart(v):
    v = sorted(v)
    q = statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0]] * 3
    return {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": v[0], "max": v[-1]}


def measure(seconds, calls, repeats, warmup):
    import torch
    import gar

    frames = int(seconds * 44100)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = (torch.rand((frames, 2), device="cuda", generator=g) - 0.5) * 2.4  # |x| up to 1.2: some samples clip
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))
    n = gar.lib().gar_device_output_size(r._h, frames)
    r.process_device(x[:4096])
    m = gar.lib().gar_device_flush_size(r._h)
    r.Reset()
    y = torch.empty((n + m, 2), dtype=torch.int16, device="cuda")
    yc = torch.empty((2 * 4096, 2), dtype=torch.int16, device="cuda")  # room for any call of the stream

    def long_row(on):
        r.Reset()
        r.set_meter(on)
        k = r.process_device(x, out=y).shape[0]
        r.flush_device(out=y[k:])

    def chunk_row(on):
        r.Reset()
        r.set_meter(on)
        for i in range(calls):
            r.process_device(x[4096 * i:4096 * (i + 1)], out=yc)

    rows = {"long": long_row, "chunk": chunk_row}
    for _ in range(warmup):
        for f in rows.values():
            f(False)
            f(True)
    torch.cuda.synchronize()
    wall = {(name, on): [] for name in rows for on in (False, True)}
    for _ in range(repeats):
        for name, f in rows.items():
            for on in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f(on)
                e1.record()
                e1.synchronize()
                wall[(name, on)].append(e0.elapsed_time(e1))
    fir = {False: [], True: []}
    r.profile(True, kinds=(0,))
    for _ in range(repeats):
        for on in (False, True):
            torch.cuda.synchronize()
            r.profile_read(0)
            long_row(on)
            torch.cuda.synchronize()
            fir[on].append(r.profile_read(0)[0])
    r.profile(False)
    long_row(True)
    clips, peak = r.meter_read()
    return wall, fir, frames, (clips.tolist(), peak.tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "the median of at least 5 runs"
    wall, fir, frames, tallies = measure(a.seconds, a.calls, a.repeats, a.warmup)
    lines = [f"meter_timing: stereo 44.1k -> 48k QualityHigh, GAR_F32, f32 in, PCM16 out fused; long = {a.seconds:g} s stream "
             f"({frames} frames) in one call + flush, chunk = {a.calls} calls of 4096 frames; {a.repeats} rounds after {a.warmup} warm-ups, "
             "meter off / on alternating",
             f"{'row':<22}{'median ms':>12}{'q1':>10}{'q3':>10}{'min':>10}{'max':>10}"]

    def add(tag, v):
        q = quart(v)
        lines.append(f"{tag:<22}{q['median']:>12.4f}{q['q1']:>10.4f}{q['q3']:>10.4f}{q['min']:>10.4f}{q['max']:>10.4f}")

    for name in ("long", "chunk"):
        add(f"{name} wall, meter off", wall[(name, False)])
        add(f"{name} wall, meter on", wall[(name, True)])
        add(f"{name} wall, on - off", [b - c for c, b in zip(wall[(name, False)], wall[(name, True)])])
    add("long FIR, meter off", fir[False])
    add("long FIR, meter on", fir[True])
    add("long FIR, on - off", [b - c for c, b in zip(fir[False], fir[True])])
    lines.append(f"tallies of one long row: clips {tallies[0]}, peak {tallies[1]}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
