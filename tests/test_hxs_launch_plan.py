"""The streaming FIR launch planner (csrc/gar_hxs_launch.cpp) on the CPU, through gar_dev_hxs_plan.

tests/golden/hxs_launch_plans.json pins every decision the GAR_HX_TRACE line names -- kernel, small-launch
rule, group size, chunking, ring, load / store layout, raw-load rows, compute waves, lean loaders, hxq grouping
-- for 280 calls.  The expected lines were recorded from the launcher as it was before the planner was split
out of it (tests/hxs_launch_plan_cases.py says how, and holds the calls), so a line that changes is a launch
decision that changed.  The coverage tests below keep the case table honest: every layout, every kernel
variant and both fallbacks must occur in it.  No GPU: the planner is integer arithmetic on plan fields,
strides, address alignments, the CU count and the knobs."""
import json
import os
import re

import pytest

from hxs_launch_plan_cases import PLANS, cases

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "hxs_launch_plans.json")) as f:
    WANT = json.load(f)
CASES = cases()
assert [c["name"] for c in CASES] == list(WANT), "the fixture does not list the cases of hxs_launch_plan_cases.py"
for _c in CASES:
    _c["want"] = WANT[_c["name"]]
BY_NAME = {c["name"]: c for c in CASES}
F32 = 1


def _field(line, name):
    m = re.search(r"\b%s=(-?\d+)" % name, line)
    assert m, (name, line)
    return int(m.group(1))


def _variant(want):
    """The kernel variant a recorded launch runs, from its lines."""
    if want == "not supported\n":
        return "not supported"
    first = want.splitlines()[0]
    if first.startswith("hxt:"):
        if _field(first, "fmt") == 5:
            return "hxt wide"
        if _field(first, "lean"):
            return "hxt lean"
        return "hxt generic %d" % (6 if _field(first, "ncomp") + 6 <= 16 else 4)
    if "\nhxq:" in want:
        return "hxq"
    return "hxs_small" if _field(first, "small") else "hxs"


@pytest.fixture(scope="module")
def handles(gar):
    return {k: gar.New(gar.Config(ir, orr, 2, q, ComputeDtype=gar.F32, DryRun=True)) for k, (ir, orr, q, _) in PLANS.items()}


def _plan(gar, handles, c, env=None):
    env = c["env"] if env is None else env
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return gar.hxs_plan(handles[c["plan"]], **c["args"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _no_stray_knobs():
    stray = [k for k in os.environ if k.startswith(("GAR_HXS", "GAR_HXT", "GAR_HXQ"))]
    assert not stray, "launch knobs set in the environment of the test run: %s" % stray


def test_every_case_plans_as_recorded(gar, handles):
    assert 200 <= len(CASES) <= 400
    bad = []
    for c in CASES:
        got = _plan(gar, handles, c)
        if got != c["want"]:
            bad.append((c["name"], c["want"], got))
    assert not bad, "%d of %d launch plans changed, first: %r" % (len(bad), len(CASES), bad[:3])


def test_fixture_covers_every_layout():
    lines = [c["want"].splitlines()[0] for c in CASES if c["want"] != "not supported\n"]
    assert {_field(ln, "fmt") for ln in lines} == set(range(8))
    assert {_field(ln, "vst") for ln in lines} == set(range(6))


def test_fixture_covers_every_kernel_variant():
    assert {_variant(c["want"]) for c in CASES} == {"hxs", "hxs_small", "hxq", "hxt generic 4", "hxt generic 6", "hxt lean",
                                                    "hxt wide", "not supported"}


def test_fixture_covers_the_axes():
    assert {c["plan"] for c in CASES} == set(PLANS)
    assert {c["args"]["channels"] for c in CASES} >= {1, 2, 3, 16, 32, 64}
    types = {"f32", "f64", "pcm16", "pcm24", "pcm32", "f16", "bf16"}
    assert {c["it"] for c in CASES} == types and {c["ot"] for c in CASES} == types
    assert {c["inl"] for c in CASES} == {"il", "pl", "mis", "flush", "flushmis"}
    assert {c["outl"] for c in CASES} == {"il", "pl", "mis"}
    knobs = {(k, v) for c in CASES for k, v in c["env"].items()}
    assert knobs >= {("GAR_HXT_ROLES", "0"), ("GAR_HXT_ROLES", "1"), ("GAR_HXT_LEAN", "0"), ("GAR_HXT_WIDE", "0"), ("GAR_HXT", "0"),
                     ("GAR_HXS_SMALL", "0"), ("GAR_HXS_SMALL", "1"), ("GAR_HXS_G", "1"), ("GAR_HXQ", "0")}


def test_fixture_covers_the_sizes():
    """Either side of the small-launch rule nmac * C == 32 * ncu, a 600 s call, Np clamped by the frame stride,
    no raw-load span, Np below the lean geometry's G."""
    for C, nmac in ((2, 4096), (16, 512), (64, 128)):
        at, above = BY_NAME["cd48-c%d-threshold-at" % C], BY_NAME["cd48-c%d-threshold-above" % C]
        assert nmac * C == 32 * at["args"]["cu_count"]
        assert (at["args"]["o_hi"] - at["args"]["o_lo"], above["args"]["o_hi"] - above["args"]["o_lo"]) == (nmac * 160, (nmac + 1) * 160)
        assert (_field(at["want"], "small"), _field(above["want"], "small")) == (1, 0)
    assert BY_NAME["cd48-c2-600s"]["args"]["in_len"] == 600 * 44100
    # 2^31 B / (4096 * 4 B rows) - (3 Qc + Kread + 256) rows = 129955 rows = 884 periods of Qc = 147, below
    # the ~1060 periods (272k periods over 256 chunks) a chunk of this call would otherwise hold
    assert _field(BY_NAME["cd48-c16-stride4096-npmax"]["want"], "Np") == 884
    ln = BY_NAME["cd48-c16-stride1M-norawspan"]["want"]
    assert _field(ln, "fmt") == 2 and "fast[0,0)" in ln
    ln = BY_NAME["cd48-c2-np3"]["want"]
    assert ln.startswith("hxt:") and _field(ln, "Np") == 3 and _field(ln, "lean") == 0


def test_fixture_covers_both_fallbacks():
    """32-channel -> 16-channel blocks: with the group size capped at 1 the launch that ran fmt 5 keeps its
    chunking for 32-channel blocks (twice the 16-channel blocks) and runs fmt 2.  hxt_kernel -> hxs_kernel: the
    same cap leaves the 16k -> 44.1k plan no group size within hxt_kernel's arrival slots."""
    c = BY_NAME["cd48-c64-big-GAR_HXS_G=1"]
    twin = BY_NAME[c["twin"]]
    assert c["args"] == twin["args"] and c["env"] == {"GAR_HXS_G": "1"} and not twin["env"]
    assert _field(twin["want"], "fmt") == 5 and _field(c["want"], "fmt") == 2 and c["want"].startswith("hxt:")
    assert _field(c["want"], "nblocks") == 2 * _field(twin["want"], "nblocks")
    assert _field(c["want"], "Np") == _field(twin["want"], "Np")
    c = BY_NAME["16cd-c2-big-GAR_HXS_G=1"]
    twin = BY_NAME[c["twin"]]
    assert c["args"] == twin["args"] and c["env"] == {"GAR_HXS_G": "1"} and not twin["env"]
    assert twin["want"].startswith("hxt:") and c["want"].startswith("hxs:")
    assert (_field(c["want"], "fmt"), _field(c["want"], "vst"), _field(c["want"], "small")) == (1, 2, 0)


# ---- CPU twins of the geometry assertions of test_gpu_hxt_lean.py and test_gpu_wide.py ----------------
kLong = 74500 * 147 + 77


def _stereo_call(gar, handles, frames, env, in_addr=0x7F0000000000, in_fs=2):
    """A first Process call of `frames` stereo f32 frames on the 44.1k -> 48k High stream."""
    nout = frames * 48000 // 44100
    c = {"plan": "cd48", "args": dict(in_type=F32, in_fs=in_fs, in_cs=1, in_addr=in_addr, in_base=0, in_len=frames, valid_end=frames,
                                      hist_addr=0, hist_len=0, hist_ld=2, out_type=F32, out_addr=0x7F8000000000, o0=0, out_fs=2,
                                      out_cs=1, o_lo=0, o_hi=nout, channels=2, cu_count=256)}
    return _plan(gar, handles, c, env)


def test_default_launch_takes_lean_path(gar, handles):
    ln = _stereo_call(gar, handles, kLong, {})
    assert ln.startswith("hxt:") and ln.count("\n") == 1, ln
    assert _field(ln, "lean") == 1, ln
    assert (_field(ln, "ncomp"), _field(ln, "G"), _field(ln, "R"), _field(ln, "Rt"), _field(ln, "Wg")) == (12, 4, 1764, 2048, 861), ln
    assert _field(ln, "Np") == 37 and _field(ln, "Np") % _field(ln, "G") != 0 and _field(ln, "ngroups") >= 8, ln
    assert _field(ln, "fmt") == 1 and _field(ln, "vst") == 2, ln


def test_lean_knob_off_takes_generic_path(gar, handles):
    ln = _stereo_call(gar, handles, kLong, {"GAR_HXT_LEAN": "0"})
    assert ln.startswith("hxt:") and (_field(ln, "lean"), _field(ln, "ncomp"), _field(ln, "G")) == (0, 10, 5), ln


def test_both_role_layouts_launch_lean(gar, handles):
    ln = _stereo_call(gar, handles, kLong, {"GAR_HXT_ROLES": "1"})
    assert ln.startswith("hxt:") and (_field(ln, "ncomp"), _field(ln, "G"), _field(ln, "lean")) == (12, 4, 1), ln
    ln = _stereo_call(gar, handles, kLong, {"GAR_HXT_ROLES": "0"})
    assert ln.startswith("hxt:") and (_field(ln, "ncomp"), _field(ln, "G"), _field(ln, "lean")) == (10, 5, 1), ln
    assert (_field(ln, "R"), _field(ln, "Rt"), _field(ln, "Wg")) == (2205, 2480, 1008), ln


def test_views_fall_back_to_generic_loaders(gar, handles):
    """An input 4 B past 8-B alignment and a two-of-three-channel strided view do not match the lean dispatch."""
    for kw in ({"in_addr": 0x7F0000000004}, {"in_fs": 3}):
        ln = _stereo_call(gar, handles, kLong, {}, **kw)
        assert ln.startswith(("hxt:", "hxs:")) and _field(ln, "lean") == 0, ln


def test_shortest_hxt_launch_is_not_lean(gar, handles):
    ln = _stereo_call(gar, handles, 4100 * 147 + 512, {})
    assert ln.startswith("hxt:") and _field(ln, "lean") == 0 and _field(ln, "G") < 5, ln


def test_wide_blocks_are_taken(gar, handles):
    """A 64-channel f32 row stream plans fmt=5 by default and fmt=2 with GAR_HXT_WIDE=0."""
    frames = 88200
    c = {"plan": "cd48", "args": dict(in_type=F32, in_fs=64, in_cs=1, in_addr=0x7F0000000000, in_base=0, in_len=frames,
                                      valid_end=frames, hist_addr=0, hist_len=0, hist_ld=64, out_type=F32, out_addr=0x7F8000000000,
                                      o0=0, out_fs=64, out_cs=1, o_lo=0, o_hi=frames * 48000 // 44100, channels=64, cu_count=256)}
    wide, narrow = _plan(gar, handles, c, {"GAR_HXT_WIDE": "1"}), _plan(gar, handles, c, {"GAR_HXT_WIDE": "0"})
    assert wide.startswith("hxt:") and _field(wide, "fmt") == 5, wide
    assert narrow.startswith("hxt:") and _field(narrow, "fmt") == 2, narrow


def test_bad_arguments_are_refused(gar, handles):
    c = BY_NAME["cd48-c2-f32-4096"]
    with pytest.raises(gar.ResamplerError):
        gar.hxs_plan(handles["cd48"], **dict(c["args"], stage=5))
    with pytest.raises(gar.ResamplerError):
        gar.hxs_plan(handles["cd48"], **dict(c["args"], in_type=7))
    assert gar.hxs_plan(handles["cd48"], **dict(c["args"], o_hi=c["args"]["o_lo"])) == ""
