"""Wall and FIR-kernel time of dithered integer PCM output (gar.h gar_set_dither) on the headline plan.

Workload: stereo 44.1k -> 48k QualityHigh, GAR_F32 compute, f32 input, a 60 s stream in one process_device +
flush_device.  Rows:

  f32      f32 output (no conversion): the floor
  p16_off  PCM16 output fused into hxs_kernel's stores, dither off (the reference's truncation)
  p16_on   the same with GAR_DITHER_TPDF
  p24_off  packed 24-bit output, staged (f32 FIR output + pack24_kernel), dither off
  p24_on   the same with GAR_DITHER_TPDF (the quantizer runs in pack24_kernel)

Wall time: torch.cuda.Event pairs around the whole sequence of a row, `--repeats` timed runs after `--warmup`;
the rows run interleaved round by round, so their differences see the same clocks and neighbours.  FIR time:
gar_profile_read of kinds 0 and 3 (the process launch and the flush launch) in a separate pass, because the
profile's event pairs cost stream time; every row starts on an idle device.  Spread: the quartiles of each row
and, for each on / off pair, the per-round difference on - off (the pair ran back to back).

Two builds (dither off against a build without the feature): `--libs OLD.so,NEW.so --sessions K` runs K
sessions of each library alternately (OLD, NEW, OLD, NEW, ...), each in a fresh child process, with the rows
both builds have (f32, p16_off, p24_off); it prints every session's medians, and for each row the range of the
session medians per library -- OLD against itself is the run-to-run spread NEW is judged by.

  python tools/dither_timing.py [--seconds 60] [--repeats 20] [--warmup 3] [--out FILE]
  python tools/dither_timing.py --libs <older libgar.so>,<libgar.so> --sessions 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "go-audio-resampler_amd")]

ALL = ["f32", "p16_off", "p16_on", "p24_off", "p24_on"]
COMMON = ["f32", "p16_off", "p24_off"]  # rows a build without gar_set_dither has


def quart(v):
    v = sorted(v)
    q = statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0]] * 3
    return {"median": statistics.median(v), "q1": q[0], "q3": q[2], "min": v[0], "max": v[-1]}


def measure(rows, seconds, repeats, warmup):
    import torch
    import gar

    frames = int(seconds * 44100)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = (torch.rand((frames, 2), device="cuda", generator=g) - 0.5) * 1.6
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))
    n = gar.lib().gar_device_output_size(r._h, frames)
    r.process_device(x[:4096])
    m = gar.lib().gar_device_flush_size(r._h)  # the flush tail of a stream that has had input
    r.Reset()
    out = {"f32": torch.empty((n + m, 2), dtype=torch.float32, device="cuda"),
           "p16": torch.empty((n + m, 2), dtype=torch.int16, device="cuda"),
           "p24": torch.empty((n + m, 2, 3), dtype=torch.uint8, device="cuda")}

    def row(name):
        y = out[name[:3]]
        r.Reset()
        if name.endswith("_on"):
            r.set_dither(gar.DITHER_TPDF, 7)
        elif name != "f32":
            r.set_dither(gar.DITHER_NONE, 0)
        k = r.process_device(x, out=y).shape[0]
        r.flush_device(out=y[k:])

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
    r.profile(False)
    res = {}
    for name in rows:
        res[name] = {"wall_ms": quart(wall[name]), "fir_process_ms": quart(per[name][0]), "fir_flush_ms": quart(per[name][1])}
    for p in ("p16", "p24"):
        if p + "_on" in wall and p + "_off" in wall:  # paired: round i's on minus round i's off
            d = [b - a for a, b in zip(wall[p + "_off"], wall[p + "_on"])]
            res[p + "_on_minus_off"] = dict(quart(d), positive=sum(1 for v in d if v > 0), rounds=len(d))
            fd = [b - a for a, b in zip(per[p + "_off"][0], per[p + "_on"][0])]
            res[p + "_fir_on_minus_off"] = dict(quart(fd), positive=sum(1 for v in fd if v > 0), rounds=len(fd))
    return res, frames, n + m


def table(res):
    lines = [f"{'row':<10}{'wall ms median':>15}{'q1':>9}{'q3':>9}{'min':>9}{'max':>9}{'FIR process ms':>16}{'q1':>9}{'q3':>9}{'FIR flush ms':>14}"]
    for name in ALL:
        if name in res:
            w, p, f = res[name]["wall_ms"], res[name]["fir_process_ms"], res[name]["fir_flush_ms"]
            lines.append(f"{name:<10}{w['median']:>15.4f}{w['q1']:>9.4f}{w['q3']:>9.4f}{w['min']:>9.4f}{w['max']:>9.4f}"
                         f"{p['median']:>16.4f}{p['q1']:>9.4f}{p['q3']:>9.4f}{f['median']:>14.4f}")
    for p in ("p16", "p24"):
        for k, what in ((p + "_on_minus_off", "wall"), (p + "_fir_on_minus_off", "FIR process")):
            if k in res:
                d = res[k]
                lines.append(f"{p} on - off, {what}, per round: median {d['median']:.4f} ms, quartiles {d['q1']:.4f} .. {d['q3']:.4f}, "
                             f"range {d['min']:.4f} .. {d['max']:.4f}, positive in {d['positive']} of {d['rounds']} rounds")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default=",".join(ALL))
    ap.add_argument("--libs", default=None, help="OLD.so,NEW.so: alternate sessions of two builds (common rows)")
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    rows = [s for s in a.rows.split(",") if s]
    if a.json:  # a session of --libs: one JSON line
        res, _, _ = measure(rows, a.seconds, a.repeats, a.warmup)
        print(json.dumps(res))
        return
    head = (f"dither_timing: stereo 44.1k -> 48k QualityHigh, GAR_F32, f32 in, {a.seconds:g} s stream, process_device + "
            f"flush_device, {a.repeats} timed repeats after {a.warmup} warm-ups")
    if a.libs:
        libs = a.libs.split(",")
        assert len(libs) == 2
        lines = [head, f"libraries: OLD {libs[0]}  NEW {libs[1]}; {a.sessions} sessions each, alternating, fresh processes"]
        med = {(t, n, k): [] for t in ("OLD", "NEW") for n in COMMON for k in ("wall_ms", "fir_process_ms")}
        for s in range(a.sessions):
            for tag, path in zip(("OLD", "NEW"), libs):
                env = dict(os.environ, GAR_LIB_PATH=os.path.abspath(path))
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--json", "--rows", ",".join(COMMON), "--seconds",
                                    str(a.seconds), "--repeats", str(a.repeats), "--warmup", str(a.warmup)], env=env,
                                   capture_output=True, text=True, timeout=600)
                line = [t for t in p.stdout.splitlines() if t.startswith("{")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stderr[-2000:])
                    raise SystemExit(f"session {s} of {tag} failed")
                res = json.loads(line[-1])
                lines.append(f"-- {tag} session {s}")
                lines += table(res)
                for n in COMMON:
                    for k in ("wall_ms", "fir_process_ms"):
                        med[(tag, n, k)].append(res[n][k]["median"])
        lines.append("-- session medians per library (ms): min .. max over sessions; OLD's own range is the run-to-run spread")
        for n in COMMON:
            for k in ("wall_ms", "fir_process_ms"):
                o, w = med[("OLD", n, k)], med[("NEW", n, k)]
                lines.append(f"{n:<8} {k:<15} OLD {min(o):.4f} .. {max(o):.4f} (median {statistics.median(o):.4f})   "
                             f"NEW {min(w):.4f} .. {max(w):.4f} (median {statistics.median(w):.4f})   "
                             f"NEW median - OLD median {statistics.median(w) - statistics.median(o):+.4f}, OLD range {max(o) - min(o):.4f}")
    else:
        res, frames, outs = measure(rows, a.seconds, a.repeats, a.warmup)
        lines = [head + f" ({frames} frames in, {outs} out)", f"library: {os.environ.get('GAR_LIB_PATH', 'libgar.so of this tree')}"]
        lines += table(res)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
