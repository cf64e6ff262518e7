"""FIR-kernel and wall time of packed 24-bit PCM I/O (GAR_PCM24_PACKED) against GAR_PCM24 in int32
storage, stereo 44.1k -> 48k QualityHigh, one process_device + flush_device of a `--seconds` stream.

Rows (interleaved round by round after `--warmup` rounds, so they see the same clocks and neighbours):

  (p)  packed in / out, GAR_F32 compute: staged through unpack24_kernel / pack24_kernel;
  (i)  GAR_PCM24 int32 in / out, GAR_F32 compute: fused (fmt 4 loads, checked stores);
  (sv) packed in / out, GAR_F64 compute: staged through unpack24_kernel / pack24_kernel;
  (se) the same through the per-element convert_kernel (GAR_PACK24_VEC=0, read per launch);
  (si) GAR_PCM24 int32 in / out, GAR_F64 compute: staged through convert_kernel.

FIR time: gar_profile_read(0) after each round -- the round's process launch, bracketed by events on
its own stream -- and the min / median / max of those figures over the rounds.  Wall time:
torch.cuda.Event pairs around process + flush, in a pass of its own (the profile's events cost stream
time); for the staged rows it is the figure that contains the conversion kernels.

  python tools/pcm24_packed_timing.py [--seconds 600] [--repeats 20] [--warmup 3] [--rows p,i,sv,se,si] [--out FILE]
  GAR_LIB_PATH=<older libgar.so> python tools/pcm24_packed_timing.py --rows i,si     (rows an older build has)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "go-audio-resampler_amd")]

LABEL = {
    "p": "(p)  packed in/out, f32 staged",
    "i": "(i)  int32 PCM24 in/out, f32 fused",
    "sv": "(sv) packed, f64 staged, vector kernels",
    "se": "(se) packed, f64 staged, per-element",
    "si": "(si) int32 PCM24, f64 staged",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", default="p,i,sv,se,si")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [s for s in a.rows.split(",") if s]

    import numpy as np
    import torch
    import gar

    frames = int(a.seconds * 44100)
    g = torch.Generator(device="cuda").manual_seed(1234)
    xi = torch.randint(-8000000, 8000000, (frames, 2), device="cuda", generator=g, dtype=torch.int32)
    xp = None
    if any(r in rows for r in ("p", "sv", "se")):  # pack on the device: the low three bytes of each sample
        sh = torch.tensor([0, 8, 16], device="cuda", dtype=torch.int32)
        xp = ((xi.unsqueeze(-1) >> sh) & 0xFF).to(torch.uint8).contiguous()
        chk = gar.unpack_pcm24(xp[:1000])
        assert np.array_equal(chk, xi[:1000].cpu().numpy())
    hs = {"f32": gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32)),
          "f64": gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F64))}
    r0 = hs["f32"]
    n = gar.lib().gar_device_output_size(r0._h, frames)
    r0.process_device(xi[:4096], pcm_bits=24)
    m = gar.lib().gar_device_flush_size(r0._h)
    r0.Reset()
    yi = torch.empty((n + m, 2), dtype=torch.int32, device="cuda")
    yp = torch.empty((n + m, 2, 3), dtype=torch.uint8, device="cuda") if xp is not None else None

    def row(name):
        r = hs["f32" if name in ("p", "i") else "f64"]
        x, y = (xi, yi) if name in ("i", "si") else (xp, yp)
        os.environ["GAR_PACK24_VEC"] = "0" if name == "se" else "1"
        r.Reset()
        k = r.process_device(x, out=y, pcm_bits=24).shape[0]
        r.flush_device(out=y[k:], pcm_bits=24)
        return r

    for _ in range(a.warmup):
        for name in rows:
            row(name)
    torch.cuda.synchronize()
    wall = {name: [] for name in rows}
    for _ in range(a.repeats):
        for name in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            row(name)
            e1.record()
            e1.synchronize()
            wall[name].append(e0.elapsed_time(e1))
    fir = {}
    for h in hs.values():
        h.profile(True, kinds=(0,))
        h.profile_read(0)
    for _ in range(a.repeats):  # every row starts on an idle device; one handle serves two or three rows,
        for name in rows:       # so each round's launch is read (and kept) on its own
            torch.cuda.synchronize()
            r = row(name)
            torch.cuda.synchronize()
            fir.setdefault(name, []).append(r.profile_read(0)[0])
    for h in hs.values():
        h.profile(False)

    lines = [f"pcm24_packed_timing: stereo 44.1k -> 48k QualityHigh, {a.seconds:g} s stream ({frames} frames in, {n + m} out), "
             f"process_device + flush_device, {a.repeats} timed rounds after {a.warmup} warm-ups, rows interleaved",
             f"library: {os.environ.get('GAR_LIB_PATH', 'libgar.so of this tree')}",
             f"{'row':<42}{'FIR ms min':>11}{'median':>9}{'max':>9}{'wall ms min':>13}{'q1':>9}{'median':>9}{'q3':>9}{'max':>9}"]
    for name in rows:
        w, f = sorted(wall[name]), sorted(fir[name])
        q = statistics.quantiles(w, n=4) if len(w) >= 2 else [w[0]] * 3
        lines.append(f"{LABEL[name]:<42}{f[0]:>11.4f}{statistics.median(f):>9.4f}{f[-1]:>9.4f}{w[0]:>13.4f}{q[0]:>9.4f}"
                     f"{statistics.median(w):>9.4f}{q[2]:>9.4f}{w[-1]:>9.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
