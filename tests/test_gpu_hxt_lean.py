"""Lean loaders of the balanced streaming kernel (gar_hxt.hpp, round 7).

For the Q24 44.1k -> 48k plan on stereo f32 frames hxt_kernel's loader waves run a step loop compiled for
the plan's ring geometry (ring rows, wrap and mirror as constants, every address base + immediate).  It
must stage the same f16 hi/lo image and loud marks as the generic loaders (knob GAR_HXT_LEAN=0, read per
launch), so every output keeps its bits: one-shot, across a history seam, with loud / NaN samples on the
ring's wrap and mirrored head, on balanced compute roles (GAR_HXT_ROLES, read per launch), and against
the reference (dft_stage.go:156-349 + polyphase_stage.go:186-352 through the oracle).

Shapes.  DESIGN.md 2.4's small-launch rule sends a stereo call to hxt_kernel above 2 blocks per CU, i.e.
above 16 * 2 * 256 / 2 = 4096 macro periods of Qc = 147 input frames: kShort is the first round length past
it (4100 periods + one window).  At that length a chunk holds Np = 3 periods, the launcher picks G = 3 and
the lean geometry (G = 5, or G = 4 beside four loaders) does not match: that case checks the exact-match
dispatch.  The lean step loop itself only runs where a chunk holds several groups of G periods (G = 4 on
the default balanced roles, G = 5 with GAR_HXT_ROLES=0); its unrolled body is 6 steps (3 ring slots x 2
register buffers), so kLong is the next length up with Np = 37: 10 / 8 groups per chunk (9 / 7 lean steps:
every body and the loop's back edge), Np mod G = 1 / 2, and 77 frames of a partial last period.  Np = 37 needs 36 * 2048 < periods <= 37 * 2048 (2048 chunks: 16 columns per CU);
74,500 periods sits in the middle of that range whatever the stream's latency.  All signals are made and
compared on the device, so a case takes well under a second of GPU work."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import F32_RMS_TOL, oracle_new, rms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IR, OR, QC = 44100, 48000, 147
kShort = 4100 * QC + 512            # 603,212 frames: just past the small-launch rule
kLong = 74500 * QC + 77             # 10,951,577 frames: Np = 37, 10 groups of G = 4 per chunk, partial last period


def _signal(torch, frames, seed=11):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.arange(frames, device="cuda", dtype=torch.float64)
    x = torch.rand((frames, 2), generator=g, device="cuda", dtype=torch.float32) * 0.2 - 0.1
    x[:, 0] += (0.6 * torch.sin(2 * np.pi * 440.0 / IR * t)).float()
    x[:, 1] += (0.6 * torch.sin(2 * np.pi * 1750.0 / IR * t + 0.5)).float()
    return x


def _run(gar, torch, x, calls=None, env=None):
    """Process (one call, or calls of the given frame counts) + Flush on the device API, with the knobs
    in `env` set for the launches; one int32 tensor (the bits) per part."""
    env = env or {}
    for k, v in env.items():
        os.environ[k] = v
    try:
        r = gar.New(gar.Config(IR, OR, 2, gar.QualityHigh, ComputeDtype=gar.F32))
        parts, s = [], 0
        for n in (calls or [x.shape[0]]):
            parts.append(r.process_device(x[s:s + n]).clone())
            s += n
        assert s == x.shape[0]
        parts.append(r.flush_device().clone())
        torch.cuda.synchronize()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return [p.contiguous().view(torch.int32) for p in parts]


def _same(torch, a, b):
    return a.shape == b.shape and bool(torch.equal(a, b))


def _trace(frames, env=None, views=False):
    """GAR_HX_TRACE lines of a child process (the trace switch is read once per process) that runs one
    Process call of `frames` stereo frames; with `views`, two more calls on fresh streams whose input is
    an offset view (4 B past 8-B alignment) and a strided view (two channels of three)."""
    code = ("import sys, torch; sys.path.insert(0, %r); import gar\n"
            "def run(x):\n"
            "    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))\n"
            "    r.process_device(x); torch.cuda.synchronize(); print('call done', file=sys.stderr, flush=True)\n"
            "n = %d\n"
            "run(torch.rand((n, 2), device='cuda') - 0.5)\n"
            "if %d:\n"
            "    run((torch.rand(2 * n + 1, device='cuda') - 0.5)[1:].view(n, 2))\n"
            "    run((torch.rand((n, 3), device='cuda') - 0.5)[:, :2])\n"
            % (os.path.join(ROOT, "go-audio-resampler_amd"), frames, 1 if views else 0))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, GAR_HX_TRACE="1", **(env or {})),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    calls, cur = [], []
    for ln in p.stderr.splitlines():
        if ln.startswith(("hxt:", "hxs:")):
            cur.append(ln)
        elif ln.startswith("call done"):
            calls.append(cur)
            cur = []
    return calls


def _field(line, name):
    m = re.search(r"\b%s=(-?\d+)" % name, line)
    assert m, (name, line)
    return int(m.group(1))


@pytest.fixture(scope="module")
def long_trace(cuda):
    """The default launches of the kLong stream: contiguous frames, then the offset and strided views."""
    return _trace(kLong, views=True)


@pytest.fixture(scope="module")
def geometry(long_trace):
    """Launch geometry of the kLong one-shot call, from its trace line."""
    ln = long_trace[0][0]
    m = re.search(r"o\[(-?\d+),(-?\d+)\).*fast\[(-?\d+),(-?\d+)\)", ln)
    assert m, ln
    g = {k: _field(ln, k) for k in ("G", "Np", "ngroups", "R", "Rt", "Wg")}
    g["a_lo"] = int(m.group(1)) // 160 if int(m.group(1)) >= 0 else -((-int(m.group(1)) + 159) // 160)
    g["fastLo"] = int(m.group(3))
    return g


@pytest.fixture(scope="module")
def long_x(cuda):
    return _signal(cuda, kLong)


@pytest.fixture(scope="module")
def long_lean(gar, cuda, long_x):
    """The default (lean) one-shot bits of the kLong stream: computed once, shared, left unchanged."""
    return _run(gar, cuda, long_x)


def test_default_launch_takes_lean_path(long_trace):
    """The kLong call runs hxt_kernel with lean=1 on the default roles -- balanced, twelve compute waves beside
    four lean loaders at G = 4 (ring 3 x 588 rows + 273 mirrored); Np = 37 leaves Np mod G != 0."""
    lines = long_trace[0]
    assert lines and lines[0].startswith("hxt:"), lines
    ln = lines[0]
    assert _field(ln, "lean") == 1, ln
    assert (_field(ln, "ncomp"), _field(ln, "G"), _field(ln, "R"), _field(ln, "Rt"), _field(ln, "Wg")) == (12, 4, 1764, 2048, 861), ln
    assert _field(ln, "Np") == 37 and _field(ln, "Np") % _field(ln, "G") != 0 and _field(ln, "ngroups") >= 8, ln
    assert _field(ln, "fmt") == 1 and _field(ln, "vst") == 2, ln


def test_lean_knob_off_takes_generic_path(cuda):
    """GAR_HXT_LEAN=0 keeps the launch on hxt_kernel's generic loaders and their role default (lean=0, one
    compute wave per row block beside six loaders, G = 5)."""
    lines = _trace(kLong, env={"GAR_HXT_LEAN": "0"})[0]
    assert lines and lines[0].startswith("hxt:"), lines
    assert (_field(lines[0], "lean"), _field(lines[0], "ncomp"), _field(lines[0], "G")) == (0, 10, 5), lines


def test_lean_equals_generic_one_shot(gar, cuda, long_x, long_lean):
    """One Process call + Flush: lean == generic bit for bit, the Process output and the Flush tail both, on the
    default roles (four lean loaders; GAR_HXT_LEAN=0: six generic ones) and with six lean loaders against six
    generic ones (GAR_HXT_ROLES=0)."""
    generic = _run(gar, cuda, long_x, env={"GAR_HXT_LEAN": "0"})
    assert len(generic) == len(long_lean) == 2
    assert long_lean[0].shape[0] > 0 and long_lean[1].shape[0] > 0
    assert _same(cuda, long_lean[0], generic[0])
    assert _same(cuda, long_lean[1], generic[1])
    lean6 = _run(gar, cuda, long_x, env={"GAR_HXT_ROLES": "0"})
    assert _same(cuda, lean6[0], generic[0]) and _same(cuda, lean6[1], generic[1])


def test_lean_equals_generic_chunked(gar, cuda, long_x, long_lean):
    """Two large calls: the second starts on a history seam (its first block's first loads are gathered, the
    lean loop takes over behind them).  Lean == generic, and both == the one-shot bits."""
    calls = [1000003, kLong - 1000003]
    lean = _run(gar, cuda, long_x, calls=calls)
    lean6 = _run(gar, cuda, long_x, calls=calls, env={"GAR_HXT_ROLES": "0"})
    generic = _run(gar, cuda, long_x, calls=calls, env={"GAR_HXT_LEAN": "0"})
    assert len(lean) == 3
    for a, b, c in zip(lean, generic, lean6):
        assert _same(cuda, a, b)
        assert _same(cuda, a, c)
    assert _same(cuda, cuda.cat(lean), cuda.cat(long_lean))


def _hazard_signal(torch, x, geo):
    """x with loud / NaN samples at ring rows the lean loop treats specially.  Column-relative row t of chunk
    k is input frame (a_lo + k Np) Qc + t - fastLo and lands in ring row t mod R; loads are GQ rows from row
    Wg on.  Rows t = 2R - 1 and 2R sit on either side of the ring's wrap (one 64-row piece, split per lane),
    t = 2R + 5 in the mirrored head [0, Wg - GQ) (written twice), t = Wg + GQ - 1 is the last row of a load
    (its partial last piece) and t = Wg + GQ the first of the next ring slot."""
    R, Wg, GQ, Np = geo["R"], geo["Wg"], geo["G"] * QC, geo["Np"]
    assert 2 * R + 5 < Np * QC and Wg - GQ > 5
    y = x.clone()
    spots = [(100, 2 * R + 5, 0, 16.0), (300, Wg + GQ - 1, 1, -40.0), (301, Wg + GQ, 0, 1e9),
             (900, 2 * R - 1, 1, float("nan")), (1500, 2 * R, 0, -16.0), (1501, 2 * R - 1, 1, 17.5)]
    for k, t, c, v in spots:
        f = (geo["a_lo"] + k * Np) * QC + t - geo["fastLo"]
        assert 0 <= f < y.shape[0], (k, t, f)
        y[f, c] = v
    return y


def test_lean_hazard_samples(gar, cuda, long_x, long_lean, geometry):
    """Samples >= 16.0 (loud) and a NaN on the ring's wrap, mirrored head and slot boundary: staged as zero,
    marked and recomputed exactly -- the bits equal the generic loaders', NaN outputs included."""
    y = _hazard_signal(cuda, long_x, geometry)
    lean = _run(gar, cuda, y)
    generic = _run(gar, cuda, y, env={"GAR_HXT_LEAN": "0"})
    for a, b in zip(lean, generic):
        assert _same(cuda, a, b)
    # the same rows of the six-loader ring (G = 5: R 2205, Wg 1008), against the generic loaders of that layout
    y6 = _hazard_signal(cuda, long_x, dict(geometry, G=5, R=2205, Wg=1008))
    lean6 = _run(gar, cuda, y6, env={"GAR_HXT_ROLES": "0"})
    generic6 = _run(gar, cuda, y6, env={"GAR_HXT_LEAN": "0"})
    for a, b in zip(lean6, generic6):
        assert _same(cuda, a, b)
    assert not _same(cuda, lean[0], long_lean[0])  # the samples did reach the outputs
    assert bool(cuda.isnan(lean[0].view(cuda.float32)).any())


def test_generic_fallback_for_views(gar, cuda, long_x, long_lean, long_trace):
    """An offset view (4 B past 8-B alignment) and a strided view (two channels of three) of the same samples
    do not match the lean dispatch (trace: no lean=1 launch) and still give the same bits."""
    for lines in long_trace[1:]:
        assert lines and all(_field(ln, "lean") == 0 for ln in lines), lines
    n = kLong
    flat = cuda.empty(2 * n + 1, device="cuda", dtype=cuda.float32)
    off = flat[1:].view(n, 2)
    off.copy_(long_x)
    assert off.data_ptr() % 8 == 4
    got = _run(gar, cuda, off)
    for a, b in zip(got, long_lean):
        assert _same(cuda, a, b)
    del flat, off, got
    wide = cuda.zeros((n, 3), device="cuda", dtype=cuda.float32)
    strided = wide[:, :2]
    strided.copy_(long_x)
    assert strided.stride(0) == 3
    got = _run(gar, cuda, strided)
    for a, b in zip(got, long_lean):
        assert _same(cuda, a, b)


def test_balanced_roles_equal_one_wave_per_row_block(gar, cuda, long_x, geometry):
    """GAR_HXT_ROLES: twelve compute waves on balanced roles (four lean loaders, G = 4) == one wave per row
    block (six loaders, G = 5), bit for bit, lean and generic, on the hazard signal."""
    y = _hazard_signal(cuda, long_x, geometry)
    one = _run(gar, cuda, y, env={"GAR_HXT_ROLES": "0"})
    bal = _run(gar, cuda, y, env={"GAR_HXT_ROLES": "1"})
    bal_generic = _run(gar, cuda, y, env={"GAR_HXT_ROLES": "1", "GAR_HXT_LEAN": "0"})
    for a, b, c in zip(one, bal, bal_generic):
        assert _same(cuda, a, b)
        assert _same(cuda, a, c)


def test_both_role_layouts_launch_lean(cuda):
    """GAR_HXT_ROLES=1: twelve compute waves at G = 4 on the four-loader lean kernel; GAR_HXT_ROLES=0: ten at G = 5
    (ring 3 x 735 rows + 273 mirrored) on the six-loader one."""
    ln = _trace(kLong, env={"GAR_HXT_ROLES": "1"})[0][0]
    assert ln.startswith("hxt:") and (_field(ln, "ncomp"), _field(ln, "G"), _field(ln, "lean")) == (12, 4, 1), ln
    ln = _trace(kLong, env={"GAR_HXT_ROLES": "0"})[0][0]
    assert ln.startswith("hxt:") and (_field(ln, "ncomp"), _field(ln, "G"), _field(ln, "lean")) == (10, 5, 1), ln
    assert (_field(ln, "R"), _field(ln, "Rt"), _field(ln, "Wg")) == (2205, 2480, 1008), ln


def test_shortest_hxt_launch_falls_through(gar, cuda):
    """kShort, the shortest length past the small-launch rule: hxt_kernel with G = Np = 3, which is not the lean
    geometry -- generic loaders (lean=0), and the knob changes nothing."""
    ln = _trace(kShort)[0][0]
    assert ln.startswith("hxt:") and _field(ln, "lean") == 0 and _field(ln, "G") < 5, ln
    x = _signal(cuda, kShort, seed=5)
    a = _run(gar, cuda, x)
    b = _run(gar, cuda, x, env={"GAR_HXT_LEAN": "0"})
    for p, q in zip(a, b):
        assert _same(cuda, p, q)


def test_lean_parity_with_oracle(O, cuda, long_x, long_lean):
    """The first second of the kLong stream's lean output against the float64 oracle fed the same prefix:
    RMS within the float32 bar (1e-6; 7e-8 measured for this plan before the lean loaders)."""
    n_in = IR + 4096  # 1 s of output needs a little more than 1 s of input (the filter's latency)
    x = long_x[:n_in].cpu().numpy().astype(np.float64)
    want = oracle_new(O, IR, OR, x, O.P_HIGH, flush=False)
    n = min(len(want[0]), OR)
    assert n >= OR - 1024, n
    got = long_lean[0][:n].view(cuda.float32).cpu().numpy().astype(np.float64)
    for c in range(2):
        e = rms(got[:, c], np.asarray(want[c])[:n])
        print("lean vs oracle rms ch%d: %.3e" % (c, e))
        assert e <= F32_RMS_TOL, (c, e)
