#!/usr/bin/env python3
"""The calls of tests/golden/hxs_launch_plans.json (cases(): name, plan, knobs, arguments) and the recorder of
their expected lines (the fixture maps case name -> lines).

The fixture pins the streaming FIR launch planner (csrc/gar_hxs_launch.cpp) against the launcher it
was split out of.  It was recorded from the commit BEFORE the split, with only the plan entry point
added to that commit's unmodified launchHxs (tools/hxs_launch_plan_parent.patch: plan-only mode returns
after the trace lines are formed), on a machine without a GPU:

    git worktree add /tmp/parent <parent commit> && cd /tmp/parent
    git apply tools/hxs_launch_plan_parent.patch   # the patch file of this commit
    cp <this commit>/include/gar.h include/ && cp <this commit>/go-audio-resampler_amd/gar/__init__.py go-audio-resampler_amd/gar/
    make -C go-audio-resampler_amd -j8
    python tests/hxs_launch_plan_cases.py go-audio-resampler_amd tests/golden/hxs_launch_plans.json

Every case runs in a process of its own per knob set (the parent caches most knobs per process).
Sizes are arithmetic only -- nothing is allocated -- so a 600 s call costs what a 4096-frame call does."""
import json
import os
import subprocess
import sys

F64, F32, F16, BF16, PCM16, PCM24, PCM32 = 0, 1, 4, 5, 16, 24, 32
TYPES = {"f32": F32, "f64": F64, "pcm16": PCM16, "pcm24": PCM24, "pcm32": PCM32, "f16": F16, "bf16": BF16}
ESZ = {"f32": 4, "f64": 8, "pcm16": 2, "pcm24": 4, "pcm32": 4, "f16": 2, "bf16": 2}
# (input rate, output rate, preset, pipeline stage): 44.1k -> 48k High is the lean plan; 96k -> 44.1k runs a
# decimator first, its second stage is the FIR; 88.2k -> 44.1k is a plan hxsPlanFits rejects
PLANS = {"cd48": (44100, 48000, 3, 0), "48cd": (48000, 44100, 4, 0), "96cd": (96000, 44100, 4, 1),
         "16cd": (16000, 44100, 3, 0), "reject": (88200, 44100, 3, 0)}
NCU = 256
IN_A, HIST_A, OUT_A = 0x7F0000000000, 0x7F4000000000, 0x7F8000000000  # 256-B aligned
BIG = 3_000_000
KNOBS = [{"GAR_HXT_ROLES": "0"}, {"GAR_HXT_ROLES": "1"}, {"GAR_HXT_LEAN": "0"}, {"GAR_HXT_WIDE": "0"}, {"GAR_HXT": "0"},
         {"GAR_HXS_SMALL": "0"}, {"GAR_HXS_SMALL": "1"}, {"GAR_HXS_G": "1"}, {"GAR_HXQ": "0"},
         {"GAR_HXT_ROLES": "1", "GAR_HXT_LEAN": "0"}]


def case(name, plan, C, frames, it="f32", ot="f32", inl="il", outl="il", env=None, in_fs=None, hist_keep=0, twin=None,
         ncu=NCU):
    """One call: `frames` new frames after 900 history rows.  inl: il interleaved, pl planar, mis base one element
    past alignment, flush / flushmis no input (history aligned / one element past).  outl: il, pl (planes of a
    capacity rounded up to 4 frames), mis."""
    ir, orr, _, stage = PLANS[plan]
    nout = max(1, frames * orr // ir)
    flush = inl.startswith("flush")
    fs = in_fs if in_fs else (1 if inl == "pl" else C)
    a = dict(in_type=TYPES[it], in_fs=fs, in_cs=frames if inl == "pl" else 1,
             in_addr=0 if flush else IN_A + (ESZ[it] if inl == "mis" else 0), in_base=1000, in_len=0 if flush else frames,
             valid_end=1000 if flush else 1000 + frames, hist_addr=HIST_A + (4 if inl == "flushmis" else 0), hist_len=900,
             hist_ld=C, out_type=TYPES[ot], out_addr=OUT_A + (ESZ[ot] if outl == "mis" else 0), o0=1088,
             out_fs=1 if outl == "pl" else C, out_cs=(nout + 3) // 4 * 4 if outl == "pl" else 1, o_lo=1088, o_hi=1088 + nout,
             channels=C, cu_count=ncu, hist_keep=hist_keep, stage=stage)
    return dict(name=name, plan=plan, env=env or {}, args=a, it=it, ot=ot, inl=inl, outl=outl, twin=twin)


def cases():
    cs = []
    chans = (1, 2, 3, 16, 32, 64)
    for C in chans:  # every sample type in and out, streaming and 4096-frame calls, on the lean plan
        for t in TYPES:
            cs.append(case(f"cd48-c{C}-{t}-big", "cd48", C, BIG, t, t))
            cs.append(case(f"cd48-c{C}-{t}-4096", "cd48", C, 4096, t, t))
    for plan in ("48cd", "96cd", "16cd"):
        for C in chans:
            cs.append(case(f"{plan}-c{C}-f32-big", plan, C, BIG))
            cs.append(case(f"{plan}-c{C}-f32-4096", plan, C, 4096))
        for t in ("pcm16", "f16"):
            for C in (2, 16):
                cs.append(case(f"{plan}-c{C}-{t}-big", plan, C, BIG, t, t))
    for t in ("f32", "pcm16", "f16"):  # layouts
        for C in (2, 16, 32):
            for inl, outl in (("pl", "il"), ("mis", "il"), ("il", "pl"), ("il", "mis")):
                cs.append(case(f"cd48-c{C}-{t}-in_{inl}-out_{outl}", "cd48", C, BIG, t, t, inl, outl))
    for plan in ("cd48", "48cd"):  # flushes: history only
        for C in (2, 3, 16, 32):
            for inl in ("flush", "flushmis"):
                for ot in ("f32", "pcm16"):
                    cs.append(case(f"{plan}-c{C}-{inl}-{ot}", plan, C, 600, "f32", ot, inl))
    # sizes.  cd48: Pc = 160, Qc = 147; the small-launch rule is nmac * C <= 32 * ncu macro periods
    for C, nmac in ((2, 4096), (16, 512), (64, 128)):
        lo = -(-1088 // 160) * 160  # first whole macro period at or after o0
        for d, tag in ((0, "at"), (1, "above")):
            c = case(f"cd48-c{C}-threshold-{tag}", "cd48", C, 1)
            c["args"]["o_lo"] = c["args"]["o0"] = lo
            c["args"]["o_hi"] = lo + (nmac + d) * 160
            c["args"]["in_len"] = (nmac + d) * 147 + 500
            c["args"]["valid_end"] = 1000 + c["args"]["in_len"]
            cs.append(c)
    for plan in PLANS:
        if plan != "reject":
            cs.append(case(f"{plan}-c2-600s", plan, 2, 600 * PLANS[plan][0]))
            cs.append(case(f"{plan}-c64-600s", plan, 64, 600 * PLANS[plan][0]))
    cs.append(case("cd48-c16-stride4096-npmax", "cd48", 16, 40_000_000, in_fs=4096))   # npMax clamps Np
    cs.append(case("cd48-c2-stride4096-npmax", "cd48", 2, 40_000_000, in_fs=4096))
    cs.append(case("cd48-c16-stride1M-norawspan", "cd48", 16, BIG, in_fs=1 << 20))     # rawSpan false
    cs.append(case("cd48-c2-stride1M-norawspan", "cd48", 2, BIG, in_fs=1 << 20))
    cs.append(case("cd48-c2-stride1M-norawspan-4096", "cd48", 2, 4096, in_fs=1 << 20))
    cs.append(case("cd48-c2-np3", "cd48", 2, 4100 * 147 + 512))                        # Np below the lean geometry's G
    cs.append(case("cd48-c2-lean", "cd48", 2, 74500 * 147 + 77))                       # Np = 37: the lean launch
    cs.append(case("cd48-c64-wide", "cd48", 64, 88200))
    for C in (2, 3, 64):  # history keep folded into a small launch
        cs.append(case(f"cd48-c{C}-4096-histkeep", "cd48", C, 4096, hist_keep=900))
    cs.append(case("cd48-c3-4096-histkeep-stride", "cd48", 3, 4096, in_fs=1 << 19, hist_keep=5000))
    for env in KNOBS:  # knobs
        tag = "+".join(f"{k}={v}" for k, v in env.items())
        cs.append(case(f"cd48-c2-lean-{tag}", "cd48", 2, 74500 * 147 + 77, env=env, twin="cd48-c2-lean"))
        cs.append(case(f"cd48-c2-4096-{tag}", "cd48", 2, 4096, env=env, twin="cd48-c2-f32-4096"))
        cs.append(case(f"cd48-c64-big-{tag}", "cd48", 64, BIG, env=env, twin="cd48-c64-f32-big"))
        cs.append(case(f"16cd-c2-big-{tag}", "16cd", 2, BIG, env=env, twin="16cd-c2-f32-big"))
        cs.append(case(f"96cd-c32-big-{tag}", "96cd", 32, BIG, env=env, twin="96cd-c32-f32-big"))
    for C in (2, 64):
        cs.append(case(f"reject-c{C}-big", "reject", C, BIG))
        cs.append(case(f"reject-c{C}-4096", "reject", C, 4096))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return cs


def run_cases(gar, cs):
    """The planner's lines for each case (same environment for all: the caller set it)."""
    handles, out = {}, []
    for c in cs:
        if c["plan"] not in handles:
            ir, orr, q, _ = PLANS[c["plan"]]
            handles[c["plan"]] = gar.New(gar.Config(ir, orr, 2, q, ComputeDtype=gar.F32, DryRun=True))
        out.append(gar.hxs_plan(handles[c["plan"]], **c["args"]))
    return out


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
