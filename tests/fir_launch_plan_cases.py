#!/usr/bin/env python3
"""The calls of tests/golden/fir_launch_plans.json (cases(): name, design, compute type, knobs, arguments) and the
recorder of their expected lines (the fixture maps case name -> lines).

The fixture pins the launch planners of the x == 0 FIR family -- csrc/gar_bg_launch.cpp (bg kernels),
csrc/gar_hx_launch.cpp (hx_kernel and the routing among bg / streaming split-f16 / hx_kernel) -- against the
launchers they were split out of.  It was recorded from the commit BEFORE the split, with only the plan entry
point added to that commit's unmodified launchBg / launchHx / launchHxs (tools/fir_launch_plan_parent.patch:
plan-only mode returns once the complete line is formed from the launcher's own variables), on a machine
without a GPU:

    git worktree add ../parent <parent commit> && cd ../parent
    git apply <this commit>/tools/fir_launch_plan_parent.patch
    cp <this commit>/include/gar.h include/ && cp <this commit>/go-audio-resampler_amd/gar/__init__.py go-audio-resampler_amd/gar/
    make -C go-audio-resampler_amd -j8
    python tests/fir_launch_plan_cases.py go-audio-resampler_amd tests/golden/fir_launch_plans.json

Every knob set runs in a process of its own (the parent caches the knobs per process).  Sizes are arithmetic
only -- nothing is allocated -- so a 600 s call costs what a 4096-frame call does."""
import json
import os
import subprocess
import sys

F64, F32, F32X = 0, 1, 2  # compute types (F32X: GAR_F32_EXACT); also the ABI's f64 / f32 sample type codes
PCM16 = 16
FUSED, DFT, DECIM = 0, 1, 2
# design -> (input rate, output rate, preset, pipeline stage, which plan, Pc, Qc of that plan)
DESIGNS = {
    "cd48": (44100, 48000, 3, 0, FUSED, 160, 147),   # composite, ten row blocks
    "48cd": (48000, 44100, 4, 0, FUSED, 294, 320),   # composite, nineteen row blocks
    "96dec": (96000, 44100, 4, 0, DECIM, 16, 32),    # integer decimator, one row block; no split-f16 plan (window > 1024 rows)
    "96cd": (96000, 44100, 4, 1, FUSED, 294, 320),   # the composite after that decimator
    "88cd": (88200, 44100, 3, 0, DECIM, 16, 32),     # integer decimator; its split-f16 plan is segmented (hx_kernel)
    "cd88": (44100, 88200, 3, 0, DFT, 16, 8),        # DFT-only
    "16cd": (16000, 44100, 3, 0, DFT, 16, 8),        # the DFT stage of an x != 0 pipeline
}
# designs of the engine API (gar.NewEngineDry, f64): ratios whose fused composite has one very long row block
ENGINE_DESIGNS = {
    "705k8k": (705600, 8000, 3, 0, FUSED, 10, 882),      # one row block, window 15 * 882 + 996 rows: rtLds above 64 KiB
    "768k11k": (768000, 11025, 3, 0, FUSED, 147, 10240),  # 148 partial slots: more than bg_kernel's LDS holds
}
NCU = 256
IN_A, HIST_A, OUT_A = 0x7F0000000000, 0x7F4000000000, 0x7F8000000000  # 256-B aligned
BIG = 3_000_000
ESZ = {F64: 8, F32: 4, PCM16: 2}
BG_KNOBS = [{"GAR_BG_G": "2"}, {"GAR_BG_WGPERCU": "1"}, {"GAR_BG_DBG": "8"}, {"GAR_BG_RT": "0"}, {"GAR_BG_RT": "1"},
            {"GAR_BG_NOVST": "1"}, {"GAR_BG_NOPARITY": "1"}]
HX_KNOBS = [{"GAR_HX_G": "1"}, {"GAR_HX_DWORD": "1"}, {"GAR_HXS": "0"}]


def case(name, design, ct, C, frames, it=None, ot=None, inl="il", outl="il", env=None, twin=None, ncu=NCU, hist_len=900,
         hist_keep=0, nmac=None, in_fs=None, in_off=0, **over):
    """One call: `frames` new frames after `hist_len` history rows (nmac: whole macro periods from an aligned start
    instead).  Sample types default to the compute type's.  inl / outl: il interleaved, pl planar, mis base one
    element past alignment; inl flush: no input."""
    ir, orr, _, stage, which, Pc, Qc = (DESIGNS.get(design) or ENGINE_DESIGNS[design])
    it = (F64 if ct == F64 else F32) if it is None else it
    ot = (F64 if ct == F64 else F32) if ot is None else ot
    o0 = 1088
    if nmac is not None:
        o0 = -(-1088 // Pc) * Pc
        frames, nout = nmac * Qc + 2000, nmac * Pc
    else:
        nout = max(1, frames * Pc // Qc)
    flush = inl == "flush"
    fs = in_fs if in_fs else (1 if inl == "pl" else C)
    base = hist_len + 100
    a = dict(in_type=it, in_fs=fs, in_cs=frames if inl == "pl" else 1,
             in_addr=0 if flush else IN_A + in_off + (ESZ[it] if inl == "mis" else 0), in_base=base, in_len=0 if flush else frames,
             valid_end=base if flush else base + frames, hist_addr=HIST_A, hist_len=hist_len, hist_ld=C, out_type=ot,
             out_addr=OUT_A + (ESZ[ot] if outl == "mis" else 0), o0=o0, out_fs=1 if outl == "pl" else C,
             out_cs=(nout + 3) // 4 * 4 if outl == "pl" else 1, o_lo=o0, o_hi=o0 + nout, channels=C, cu_count=ncu,
             hist_keep=hist_keep, stage=stage, which=which)
    a.update(over)
    return dict(name=name, design=design, ct=ct, env=env or {}, args=a, twin=twin)


def cases():
    cs = []
    chans = (1, 2, 3, 8, 16, 64)
    ctn = {F64: "f64", F32: "f32", F32X: "f32x"}
    for d in DESIGNS:  # every design, compute type and channel count: a stream chunk, a long call, a 600 s call
        for ct in (F64, F32, F32X):
            for C in chans:
                cs.append(case(f"{d}-{ctn[ct]}-c{C}-4096", d, ct, C, 4096))
                cs.append(case(f"{d}-{ctn[ct]}-c{C}-big", d, ct, C, BIG))
            cs.append(case(f"{d}-{ctn[ct]}-c2-600s", d, ct, 2, 600 * DESIGNS[d][0]))
            cs.append(case(f"{d}-{ctn[ct]}-c2-1period", d, ct, 2, 0, nmac=1))
    # bg: every G (one to eight macro periods on a one-CU device, so the launch is not a small one)
    for n in range(1, 10):
        cs.append(case(f"cd88-f64-c64-nmac{n}-1cu", "cd88", F64, 64, 0, nmac=n, ncu=1))
        cs.append(case(f"cd88-f32x-c2-nmac{n}", "cd88", F32X, 2, 0, nmac=n))
    # bg: either side of the small-launch rule (nmac * C + 15) / 16 <= 2 ncu
    for d, C, n in (("cd48", 2, 4096), ("cd48", 64, 128), ("96dec", 8, 1024), ("cd88", 3, 2730)):
        cs.append(case(f"{d}-f64-c{C}-small-at", d, F64, C, 0, nmac=n))
        cs.append(case(f"{d}-f64-c{C}-small-above", d, F64, C, 0, nmac=n + 1))
    # bg: layouts and sample types of the f32 epilogue, history keep
    for d in ("cd48", "88cd", "cd88"):
        for C in (2, 3):
            for inl, outl in (("pl", "il"), ("il", "pl"), ("il", "mis"), ("flush", "il")):
                cs.append(case(f"{d}-f32x-c{C}-in_{inl}-out_{outl}", d, F32X, C, BIG, inl=inl, outl=outl))
            cs.append(case(f"{d}-f32x-c{C}-out_f64", d, F32X, C, BIG, ot=F64))
            cs.append(case(f"{d}-f32x-c{C}-out_pcm16", d, F32X, C, BIG, ot=PCM16))
            cs.append(case(f"{d}-f64-c{C}-4096-histkeep", d, F64, C, 4096, hist_keep=900))
            cs.append(case(f"{d}-f64-c{C}-big-histkeep", d, F64, C, BIG, hist_keep=900))
    for env in BG_KNOBS:  # bg knobs against their twins
        tag = "+".join(f"{k}={v}" for k, v in env.items())
        for d, ct, C, size in (("cd88", F64, 2, "big"), ("cd88", F64, 2, "4096"), ("cd48", F64, 2, "4096"), ("cd48", F32X, 2, "big"),
                               ("cd88", F32X, 2, "big"), ("96dec", F64, 8, "4096")):
            cs.append(case(f"{d}-{ctn[ct]}-c{C}-{size}-{tag}", d, ct, C, BIG if size == "big" else 4096, env=env,
                           twin=f"{d}-{ctn[ct]}-c{C}-{size}"))
    # hx: the segmented plan (88cd) and, with GAR_HXS=0, the row-block plans
    for C in (2, 4, 16):  # load formats: stereo frames, four-channel rows, dword; offsets past 2^31
        cs.append(case(f"88cd-f32-c{C}-mis", "88cd", F32, C, BIG, inl="mis"))
        cs.append(case(f"88cd-f32-c{C}-pl", "88cd", F32, C, BIG, inl="pl", outl="pl"))
        cs.append(case(f"88cd-f32-c{C}-stride64M", "88cd", F32, C, BIG, in_fs=1 << 26))
        cs.append(case(f"88cd-f32-c{C}-stride1M", "88cd", F32, C, BIG, in_fs=1 << 20))
        cs.append(case(f"88cd-f32-c{C}-out_f64", "88cd", F32, C, BIG, ot=F64))
        cs.append(case(f"88cd-f32-c{C}-out_mis", "88cd", F32, C, BIG, outl="mis"))
        cs.append(case(f"88cd-f32-c{C}-in_f64", "88cd", F32, C, BIG, it=F64))
        cs.append(case(f"88cd-f32-c{C}-in_pcm16", "88cd", F32, C, BIG, it=PCM16))
        cs.append(case(f"88cd-f32-c{C}-flush", "88cd", F32, C, 600, inl="flush"))
        cs.append(case(f"88cd-f32-c{C}-out_pcm16", "88cd", F32, C, BIG, ot=PCM16))  # the PCM refusal
    # the empty interior range: 399 frames after 912 history rows (every window crosses the history seam)
    cs.append(case("88cd-f32-c2-399-after-912", "88cd", F32, 2, 399, hist_len=912, in_base=912, valid_end=912 + 399, o0=456 - 228,
                   o_lo=456 - 228, o_hi=456 - 228 + 199))
    cs.append(case("88cd-f32-c2-399-after-912-late", "88cd", F32, 2, 399, hist_len=912, in_base=2000, valid_end=2399, o0=0, o_lo=0, o_hi=199))
    # k0 / k1 clipped at each end: by the output range, by the input's first row, by the last row, by valid_end
    cs.append(case("88cd-f32-c2-k0-by-input", "88cd", F32, 2, BIG))
    cs.append(case("88cd-f32-c2-k0-by-output", "88cd", F32, 2, BIG, hist_len=0, in_base=0, valid_end=BIG, o0=1001, o_lo=1001, o_hi=1001 + 5000))
    cs.append(case("88cd-f32-c2-k0-zero", "88cd", F32, 2, BIG, hist_len=0, in_base=0, valid_end=BIG, o0=1600, o_lo=1600, o_hi=1600 + 16 * 300))
    cs.append(case("88cd-f32-c2-k1-by-output", "88cd", F32, 2, BIG, o_hi=1088 + 5003))
    cs.append(case("88cd-f32-c2-k1-by-validend", "88cd", F32, 2, BIG, valid_end=1000 + 20000, o_hi=1088 + 16 * 2000))
    cs.append(case("88cd-f32-c2-k1-nchunk", "88cd", F32, 2, BIG, in_len=BIG + 5000, valid_end=1000 + BIG + 5000, o_hi=1088 + 16 * 3000))
    # the G search: stopped by the macro periods, the window rows, LDS, the CU count; not stopped
    for n in (1, 2, 3):
        cs.append(case(f"88cd-f32-c64-nmac{n}", "88cd", F32, 64, 0, nmac=n, ncu=1))
    for d in ("cd48", "48cd", "cd88", "16cd"):
        for C, ncu in ((2, 256), (64, 1), (64, 256)):
            cs.append(case(f"{d}-f32-c{C}-big-ncu{ncu}-GAR_HXS=0", d, F32, C, BIG, env={"GAR_HXS": "0"}, ncu=ncu))
        for n in (1, 2, 5):
            cs.append(case(f"{d}-f32-c64-nmac{n}-GAR_HXS=0", d, F32, 64, 0, nmac=n, ncu=1, env={"GAR_HXS": "0"}))
    for env in HX_KNOBS:  # hx knobs against their twins
        tag = "+".join(f"{k}={v}" for k, v in env.items())
        cs.append(case(f"88cd-f32-c2-big-{tag}", "88cd", F32, 2, BIG, env=env, twin="88cd-f32-c2-big"))
        cs.append(case(f"88cd-f32-c16-big-{tag}", "88cd", F32, 16, BIG, env=env, twin="88cd-f32-c16-big"))
        cs.append(case(f"cd48-f32-c2-big-{tag}", "cd48", F32, 2, BIG, env=env, twin="cd48-f32-c2-big"))
        cs.append(case(f"cd48-f32-c2-4096-{tag}", "cd48", F32, 2, 4096, env=env, twin="cd48-f32-c2-4096"))
    cs.append(case("cd48-f32-c2-out_pcm16-GAR_HXS=0", "cd48", F32, 2, BIG, ot=PCM16, env={"GAR_HXS": "0"}))
    cs.append(case("cd48-f32-c2-out_pcm16", "cd48", F32, 2, BIG, ot=PCM16))
    # bg: a plan of one row block whose time-major window exceeds 64 KiB runs bg_rb_kernel, whatever GAR_BG_RT says;
    # a plan whose partial slots exceed bg_kernel's LDS is an invalid configuration at any size
    for n in (1, 64, 4096, 4097):
        cs.append(case(f"705k8k-f64-c2-nmac{n}", "705k8k", F64, 2, 0, nmac=n))
    cs.append(case("705k8k-f64-c8-nmac64", "705k8k", F64, 8, 0, nmac=64))
    cs.append(case("705k8k-f64-c2-nmac64-GAR_BG_RT=1", "705k8k", F64, 2, 0, nmac=64, env={"GAR_BG_RT": "1"}, twin="705k8k-f64-c2-nmac64"))
    for C, n in ((2, 1), (2, 64), (2, 100000), (64, 1)):
        cs.append(case(f"768k11k-f64-c{C}-nmac{n}", "768k11k", F64, C, 0, nmac=n))
    # the streaming planner declines a row-block plan and the launch falls back to hx_kernel: a chunk of more than
    # 2^24 macro periods, reached where the frame stride leaves no raw-load span to clamp it (GAR_HXS_NP sets the
    # chunk length; without the knob the call must be so long that hx_kernel's 2^30 columns are exceeded as well)
    cs.append(case("cd48-f32-c2-stride1M-GAR_HXS_NP=20000000", "cd48", F32, 2, BIG, in_fs=1 << 20, env={"GAR_HXS_NP": "20000000"}))
    cs.append(case("cd48-f32-c2-stride1M", "cd48", F32, 2, BIG, in_fs=1 << 20))
    cs.append(case("cd48-f32-c2-stride1M-2e36periods", "cd48", F32, 2, 0, nmac=(1 << 36) + 1, in_fs=1 << 20))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


def new_handles(gar):
    h = {(d, ct): gar.New(gar.Config(v[0], v[1], 2, v[2], ComputeDtype=ct, DryRun=True))
         for d, v in DESIGNS.items() for ct in (F64, F32, F32X)}
    h.update({(d, F64): gar.NewEngineDry(v[0], v[1], v[2], F64) for d, v in ENGINE_DESIGNS.items()})
    return h


def run_cases(gar, cs, handles=None):
    """The planner's lines for each case (same environment for all: the caller set it)."""
    handles = handles or new_handles(gar)
    return [gar.fir_plan(handles[c["design"], c["ct"]], **c["args"]) for c in cs]


def main():
    pkg, dst = sys.argv[1], sys.argv[2]
    if len(sys.argv) > 3:  # child: one knob set
        sys.path.insert(0, pkg)
        import gar
        env = json.loads(sys.argv[3])
        print(json.dumps(run_cases(gar, [c for c in cases() if c["env"] == env])))
        return
    cs = cases()
    envs = []
    for c in cs:
        if c["env"] not in envs:
            envs.append(c["env"])
    for env in envs:
        base = {k: v for k, v in os.environ.items() if not k.startswith("GAR_")}
        p = subprocess.run([sys.executable, os.path.abspath(__file__), pkg, dst, json.dumps(env)], env=dict(base, **env),
                           capture_output=True, text=True, check=True)
        got = json.loads(p.stdout.splitlines()[-1])
        for c, g in zip([c for c in cs if c["env"] == env], got):
            c["want"] = g
    with open(dst, "w") as f:  # case name -> expected lines; the inputs of a case are cases() above
        f.write("{\n" + ",\n".join(json.dumps(c["name"]) + ": " + json.dumps(c["want"]) for c in cs) + "\n}\n")
    print(f"{len(cs)} cases -> {dst}")


if __name__ == "__main__":
    main()
