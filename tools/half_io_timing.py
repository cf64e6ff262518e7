"""Wall and FIR-kernel time of half-precision sample I/O against float32 I/O on the headline plan.

Workload: stereo 44.1k -> 48k QualityHigh, GAR_F32 compute, a 60 s stream in one process_device +
flush_device.  Four rows:

  (a) f32 I/O as it runs by default (hxt_kernel);
  (b) f32 I/O forced onto hxs_kernel (GAR_HXT=0);
  (c) f16 I/O fused into hxs_kernel's loads and stores;
  (d) what a caller with f16 tensors did before: x.float(), the f32 call, y.half().

Wall time: torch.cuda.Event pairs around the whole sequence of a row, `--repeats` timed runs after
`--warmup`; the rows of one process run interleaved round by round (a, c, d, a, c, d, ...), so the
differences between them see the same clocks and neighbours.  The library reads GAR_HXT once per
process, so row (b) runs in a child process of its own, which also repeats row (c) (when asked for) as
its link to the parent's rounds.  FIR time: gar_profile_read of kinds 0 and 3 (the process launch and the flush
launch, printed separately; medians over rounds interleaved the same way, each row started on an idle
device) in a separate pass, because the profile's event pairs cost stream time.  A launch of a few tens
of microseconds is bracketed by events the host enqueues around it, so differences of a few microseconds
between rows are not kernel properties; `--seconds 600` gives launches long enough to compare kernels.
Spread: the quartiles of each row, and for (c) against (d) the per-round difference d - c of the
interleaved rounds (each pair ran back to back): its median, quartiles and how many rounds it is
positive in.

  python tools/half_io_timing.py [--seconds 60] [--repeats 20] [--warmup 3] [--out FILE]
  GAR_LIB_PATH=<older libgar.so> python tools/half_io_timing.py --rows a,d     (rows of another build)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "go-audio-resampler_amd")]

LABEL = {
    "a": "(a) f32 I/O, default kernel",
    "b": "(b) f32 I/O, GAR_HXT=0 (hxs_kernel)",
    "c": "(c) f16 I/O fused",
    "d": "(d) x.float() + f32 call + y.half()",
}


def measure(rows, seconds, repeats, warmup):
    import torch
    import gar

    frames = int(seconds * 44100)
    g = torch.Generator(device="cuda").manual_seed(1234)
    xf = (torch.rand((frames, 2), device="cuda", generator=g) - 0.5) * 1.6
    xh = xf.half() if ("c" in rows or "d" in rows) else None
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))
    n = gar.lib().gar_device_output_size(r._h, frames)
    r.process_device(xf[:4096])
    m = gar.lib().gar_device_flush_size(r._h)  # the flush tail of a stream that has had input
    r.Reset()
    yf = torch.empty((n + m, 2), dtype=torch.float32, device="cuda")
    yh = torch.empty((n + m, 2), dtype=torch.float16, device="cuda")

    def call(x, y):
        r.Reset()
        k = r.process_device(x, out=y).shape[0]
        r.flush_device(out=y[k:])

    def row(name):
        if name == "c":
            call(xh, yh)
        elif name == "d":
            y = torch.empty((n + m, 2), dtype=torch.float32, device="cuda")
            call(xh.float(), y)
            return y.half()
        else:
            call(xf, yf)

    for _ in range(warmup):
        for name in rows:
            row(name)
    torch.cuda.synchronize()
    wall = {name: [] for name in rows}
    for _ in range(repeats):
        for name in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            row(name)
            e1.record()
            e1.synchronize()
            wall[name].append(e0.elapsed_time(e1))
    fir = {}
    r.profile(True, kinds=(0, 3))
    per = {name: ([], []) for name in rows}
    for _ in range(repeats):  # interleaved like the wall rounds; every row starts on an idle device
        for name in rows:
            torch.cuda.synchronize()
            r.profile_read(0)
            r.profile_read(3)
            row(name)
            torch.cuda.synchronize()
            per[name][0].append(r.profile_read(0)[0])
            per[name][1].append(r.profile_read(3)[0])
    for name in rows:
        fir[name] = (statistics.median(per[name][0]), statistics.median(per[name][1]))
    r.profile(False)
    res = {}
    for name in rows:
        w = sorted(wall[name])
        q = statistics.quantiles(w, n=4) if len(w) >= 2 else [w[0]] * 3
        res[name] = {"wall_ms_median": statistics.median(w), "wall_ms_min": w[0], "wall_ms_max": w[-1],
                     "wall_ms_q1": q[0], "wall_ms_q3": q[2], "fir_process_ms": fir[name][0], "fir_flush_ms": fir[name][1],
                     "repeats": repeats}
    if "c" in wall and "d" in wall:  # paired: round i's (d) minus round i's (c)
        diff = sorted(d - c for c, d in zip(wall["c"], wall["d"]))
        q = statistics.quantiles(diff, n=4) if len(diff) >= 2 else [diff[0]] * 3
        res["d_minus_c"] = {"median": statistics.median(diff), "q1": q[0], "q3": q[2], "min": diff[0], "max": diff[-1],
                            "positive": sum(1 for v in diff if v > 0), "rounds": len(diff)}
    return res, frames, n + m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    rows = [s for s in a.rows.split(",") if s]
    if a.child:  # GAR_HXT=0 set by the parent: the f32 row is (b)
        res, _, _ = measure(["a", "c"] if "c" in rows else ["a"], a.seconds, a.repeats, a.warmup)
        print(json.dumps({"b": res["a"], **({"c_child": res["c"]} if "c" in res else {})}))
        return
    here = [s for s in rows if s != "b"]
    res, frames, outs = measure(here, a.seconds, a.repeats, a.warmup) if here else ({}, int(a.seconds * 44100), 0)
    if "b" in rows:  # a fresh child process (this one keeps its GPU context; nothing is replaced)
        env = dict(os.environ, GAR_HXT="0")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rows", a.rows, "--seconds", str(a.seconds),
                            "--repeats", str(a.repeats), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True,
                           timeout=600)
        line = [s for s in p.stdout.splitlines() if s.startswith("{")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stderr[-2000:])
            raise SystemExit("row (b): the child process failed")
        res.update(json.loads(line[-1]))
    lines = [f"half_io_timing: stereo 44.1k -> 48k QualityHigh, GAR_F32, {a.seconds:g} s stream ({frames} frames in, "
             f"{outs} out), process_device + flush_device, {a.repeats} timed repeats after {a.warmup} warm-ups",
             f"library: {os.environ.get('GAR_LIB_PATH', 'libgar.so of this tree')}",
             f"{'row':<40}{'wall ms median':>15}{'q1':>9}{'q3':>9}{'min':>9}{'max':>9}{'FIR process ms':>16}{'FIR flush ms':>14}"]
    for name in ("a", "b", "c", "c_child", "d"):
        if name in res:
            v = res[name]
            label = LABEL.get(name, "(c) again, in row (b)'s process")
            lines.append(f"{label:<40}{v['wall_ms_median']:>15.4f}{v['wall_ms_q1']:>9.4f}{v['wall_ms_q3']:>9.4f}{v['wall_ms_min']:>9.4f}"
                         f"{v['wall_ms_max']:>9.4f}{v['fir_process_ms']:>16.4f}{v['fir_flush_ms']:>14.4f}")
    if "d_minus_c" in res:
        c, d, p = res["c"], res["d"], res["d_minus_c"]
        lines.append(f"(c) vs (d): median {c['wall_ms_median'] / d['wall_ms_median']:.3f}x; per-round (d) - (c): median {p['median']:.4f} ms, "
                     f"quartiles {p['q1']:.4f} .. {p['q3']:.4f}, range {p['min']:.4f} .. {p['max']:.4f}, positive in {p['positive']} of "
                     f"{p['rounds']} rounds; (c) q3 {c['wall_ms_q3']:.4f} ms {'<' if c['wall_ms_q3'] < d['wall_ms_q1'] else '>='} (d) q1 {d['wall_ms_q1']:.4f} ms")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
