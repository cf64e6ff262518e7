"""The launch planners of the x == 0 FIR family (csrc/gar_bg_launch.cpp, csrc/gar_hx_launch.cpp) on the CPU,
through gar_dev_fir_plan.

tests/golden/fir_launch_plans.json pins the complete trace line -- every field of the launch plan -- of 502 calls:
bg launches (GAR_F64 / GAR_F32_EXACT compute), hx_kernel launches, and the routing among the bg kernels, the
streaming split-f16 kernels and hx_kernel.  The expected lines were recorded from the launchers as they were before
the planners were split out of them (tests/fir_launch_plan_cases.py says how, and holds the calls), so a line that
changes is a launch decision that changed.  The coverage tests keep the case table honest; a value no design of
the engine reaches is named in UNREACHED with the reason.  No GPU: the planners are integer arithmetic on plan
fields, strides, addresses, the CU count and the knobs."""
import collections
import json
import os
import re

import pytest

from fir_launch_plan_cases import BG_KNOBS, DESIGNS, ENGINE_DESIGNS, F32, F32X, F64, HX_KNOBS, cases, new_handles

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "fir_launch_plans.json")) as f:
    WANT = json.load(f)
CASES = cases()
assert [c["name"] for c in CASES] == list(WANT), "the fixture does not list the cases of fir_launch_plan_cases.py"
for _c in CASES:
    _c["want"] = WANT[_c["name"]]
BY_NAME = {c["name"]: c for c in CASES}
BG = [c for c in CASES if c["want"].startswith("bg:")]
HX = [c for c in CASES if c["want"].startswith("hx:")]

UNREACHED = {
    "hx invalid configuration by window rows, LDS or NS": "attachHx (gar_stage.cpp) builds a split-f16 plan only if one macro period fits "
                                                          "hx_kernel's rows and LDS, and buildHxPlan only NS values with a kernel; the "
                                                          "2^30-column limit is reached (a call of 2^36 macro periods)",
    "hx G search stopped by LDS": "row-block plans have no partial slots and the segmented plan (88.2k -> 44.1k, 6 slots, parity) "
                                  "needs 156184 B at the 1024-row limit, which stops the search first",
}


def _field(line, name):
    m = re.search(r"\b%s=(-?\w+)" % name, line)
    assert m, (name, line)
    return m.group(1) if not re.fullmatch(r"-?\d+", m.group(1)) else int(m.group(1))


@pytest.fixture(scope="module")
def handles(gar):
    return new_handles(gar)


def _plan(gar, handles, c):
    saved = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    try:
        return gar.fir_plan(handles[c["design"], c["ct"]], **c["args"])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def _no_stray_knobs():
    stray = [k for k in os.environ if k.startswith(("GAR_BG", "GAR_HX"))]
    assert not stray, "launch knobs set in the environment of the test run: %s" % stray


def test_every_case_plans_as_recorded(gar, handles):
    assert 300 <= len(CASES) <= 600
    bad = []
    for c in CASES:
        got = _plan(gar, handles, c)
        if got != c["want"]:
            bad.append((c["name"], c["want"], got))
    assert not bad, "%d of %d launch plans changed, first: %r" % (len(bad), len(CASES), bad[:3])


def test_fixture_covers_the_axes():
    assert {c["design"] for c in CASES} == set(DESIGNS) | set(ENGINE_DESIGNS)
    for d in DESIGNS:
        assert {c["ct"] for c in CASES if c["design"] == d} == {F64, F32, F32X}
    assert {c["args"]["channels"] for c in CASES} >= {1, 2, 3, 8, 16, 64}
    assert any(c["args"]["in_len"] == 600 * 44100 for c in CASES)
    assert any(c["name"].endswith("1period") for c in CASES)
    kinds = collections.Counter(c["want"].split(":")[0] for c in CASES)
    assert set(kinds) == {"bg", "hx", "hxs", "hxt", "not supported\n", "invalid configuration\n"}, kinds
    assert any("\nhxq:" in c["want"] for c in CASES)


def test_fixture_covers_the_invalid_configurations():
    """bg: 768k -> 11.025k (engine API) has 148 partial slots, 148 * 256 * 8 B = 303104 B in one buffer, above bg_kernel's
    160 KiB - 64 B even with B read from global memory: every call, small ones included (its programs exceed what the
    small kernels take by value), is an invalid configuration.  hx: more than 2^30 columns."""
    for C, n in ((2, 1), (2, 64), (2, 100000), (64, 1)):
        c = BY_NAME["768k11k-f64-c%d-nmac%d" % (C, n)]
        assert c["ct"] == F64 and not c["env"] and c["want"] == "invalid configuration\n"
    c = BY_NAME["cd48-f32-c2-stride1M-2e36periods"]
    assert c["ct"] == F32 and not c["env"] and c["want"] == "invalid configuration\n"
    assert (c["args"]["o_hi"] - c["args"]["o_lo"]) // 160 // 8 * c["args"]["channels"] > 2 ** 30  # columns at G = 8


def test_bg_fixture_covers_kernels_units_and_geometry():
    assert {_field(c["want"], "kernel") for c in BG} == {"bg", "bg_rb", "bg_rt"}
    units = {(_field(c["want"], "unit"), _field(c["want"], "NS") < 56) for c in BG if not _field(c["want"], "f64")}
    assert units == {("f32a", True), ("f32b", False)}, units
    assert {_field(c["want"], "NS") for c in BG if _field(c["want"], "unit") == "f32b"} >= {56}  # the first NS of f32b
    assert {_field(c["want"], "unit") for c in BG if _field(c["want"], "f64")} == {"f64"}
    assert {_field(c["want"], "globalB") for c in BG} == {0, 1}
    assert {_field(c["want"], "parity") for c in BG} == {0, 1}
    assert {_field(c["want"], "vst") for c in BG} == {0, 1, 2}
    assert {_field(c["want"], "G") for c in BG} == set(range(1, 9))
    assert {_field(c["want"], "hist") for c in BG if _field(c["want"], "rbMode")} == {0, 1}
    assert {_field(c["want"], "hist") for c in BG if not _field(c["want"], "rbMode")} == {0, 1}


def test_bg_fixture_covers_the_small_launch_rule():
    """Either side of (nmac * C + 15) / 16 <= 2 ncu; bg_rt_kernel for plans of at most two row blocks, bg_rb_kernel
    above; GAR_BG_RT switches each."""
    for d, C, n in (("cd48", 2, 4096), ("cd48", 64, 128), ("96dec", 8, 1024), ("cd88", 3, 2730)):
        at, above = BY_NAME["%s-f64-c%d-small-at" % (d, C)], BY_NAME["%s-f64-c%d-small-above" % (d, C)]
        ncu = at["args"]["cu_count"]
        assert (n * C + 15) // 16 <= 2 * ncu < ((n + 1) * C + 15) // 16
        assert (_field(at["want"], "nmac"), _field(above["want"], "nmac")) == (n, n + 1)
        assert _field(at["want"], "rbMode") in (1, 2) and _field(above["want"], "rbMode") == 0
    # row blocks: nred is one per row block with a reduction; the composites have ten and nineteen row blocks
    assert _field(BY_NAME["cd48-f64-c2-4096"]["want"], "kernel") == "bg_rb"
    assert _field(BY_NAME["96dec-f64-c8-4096"]["want"], "kernel") == "bg_rt"
    assert _field(BY_NAME["96dec-f64-c8-4096-GAR_BG_RT=0"]["want"], "kernel") == "bg_rb"
    assert _field(BY_NAME["cd48-f64-c2-4096-GAR_BG_RT=1"]["want"], "kernel") == "bg_rt"
    # the rtLds <= 64 KiB limit: 705.6k -> 8k (engine API) is one row block (one reduction, seven programs) whose
    # time-major window, (15 * 882 + 996 rows + padding) * 8 B, is above it: bg_rb_kernel, also under GAR_BG_RT=1
    rt = [_field(c["want"], "lds") for c in BG if _field(c["want"], "kernel") == "bg_rt"]
    assert 0 < max(rt) <= 64 * 1024
    for n in ("705k8k-f64-c2-nmac1", "705k8k-f64-c2-nmac64", "705k8k-f64-c8-nmac64", "705k8k-f64-c2-nmac4096"):
        ln = BY_NAME[n]["want"]
        assert (_field(ln, "kernel"), _field(ln, "nred"), _field(ln, "threads") // 64) == ("bg_rb", 1, _field(ln, "nprog"))
        assert (15 * _field(ln, "Qc") + _field(ln, "Kread")) * 8 > 64 * 1024
    c = BY_NAME["705k8k-f64-c2-nmac64-GAR_BG_RT=1"]
    assert c["env"] == {"GAR_BG_RT": "1"} and c["want"] == BY_NAME[c["twin"]]["want"] and c["args"] == BY_NAME[c["twin"]]["args"]
    assert _field(BY_NAME["705k8k-f64-c2-nmac4097"]["want"], "kernel") == "bg"  # above the small-launch rule


def test_bg_knobs_take_effect():
    assert all(any(c["env"] == env for c in CASES) for env in BG_KNOBS)
    changed = collections.defaultdict(int)
    for c in CASES:
        if c["twin"] and c["env"] in BG_KNOBS:
            twin = BY_NAME[c["twin"]]
            assert c["args"] == twin["args"] and (c["design"], c["ct"]) == (twin["design"], twin["ct"]) and not twin["env"]
            changed[json.dumps(c["env"])] += c["want"] != twin["want"]
    assert all(changed[json.dumps(env)] > 0 for env in BG_KNOBS), changed
    c = BY_NAME["cd88-f64-c2-big-GAR_BG_G=2"]
    assert (_field(c["want"], "G"), _field(BY_NAME[c["twin"]]["want"], "G")) == (2, 8)
    c = BY_NAME["cd88-f64-c2-big-GAR_BG_WGPERCU=1"]
    assert (_field(c["want"], "blocks"), _field(BY_NAME[c["twin"]]["want"], "blocks")) == (256, 512)
    c = BY_NAME["cd48-f64-c2-4096-GAR_BG_DBG=8"]
    assert (_field(c["want"], "rbMode"), _field(BY_NAME[c["twin"]]["want"], "rbMode")) == (0, 1) and _field(c["want"], "dbg") == 8
    c = BY_NAME["cd48-f32x-c2-big-GAR_BG_NOVST=1"]
    assert (_field(c["want"], "vst"), _field(BY_NAME[c["twin"]]["want"], "vst")) == (0, 2)
    c = BY_NAME["cd48-f32x-c2-big-GAR_BG_NOPARITY=1"]
    assert (_field(c["want"], "parity"), _field(BY_NAME[c["twin"]]["want"], "parity")) == (0, 1)


def _hx_stop(c):
    """What ended hx_kernel's search for G at this launch (bounds from the line: the planner's Kread >= Kc)."""
    ln, a = c["want"], c["args"]
    G, W, Ws, lds = (_field(ln, n) for n in ("G", "W", "Ws", "lds"))
    Qc = _field(ln, "in_chunk") // (G * a["in_fs"])
    Pc = _field(ln, "out_chunk") // (G * a["out_fs"] * (8 if a["out_type"] == F64 else 4))
    nmac = -(-a["o_hi"] // Pc) - a["o_lo"] // Pc
    if "GAR_HX_G" in c["env"]:
        return "knob"
    if G == 8:
        return "none"
    if G + 1 > nmac:
        return "nmac"
    rows_lo, rows_hi = (W + Qc + 63) // 64 * 64, (W + Qc + 126) // 64 * 64  # the next window: at least, at most
    if rows_lo > 1024:
        return "rows"
    if lds + 132 * (rows_lo - Ws) > 160 * 1024:
        return "lds"
    nb = ((nmac + G) // (G + 1) * a["channels"] + 15) // 16
    if nb < a["cu_count"] and rows_hi <= 1024 and lds + 132 * (rows_hi - Ws) <= 160 * 1024:
        return "ncu"
    return "rows, lds or ncu"


def test_hx_fixture_covers_plans_layouts_and_the_g_search():
    assert {c["design"] for c in HX} == {"88cd", "cd48", "48cd", "cd88", "16cd"}  # 88cd: segmented, the rest row-block plans
    # a row-block plan reaches hx_kernel under GAR_HXS=0, or where the streaming planner declines (test below)
    assert all(c["env"].get("GAR_HXS") == "0" or "GAR_HXS_NP" in c["env"] for c in HX if c["design"] != "88cd")
    assert {_field(c["want"], "fmt") for c in HX} == {0, 1, 2, 3}
    big = [c for c in HX if _field(c["want"], "fmt") == 3]
    # fmt 3: a block's offsets (16 / C + 2 chunks of in_chunk elements, + the channels) reach 2^31 bytes
    assert big and all((16 / c["args"]["channels"] + 2) * _field(c["want"], "in_chunk") * 4 >= 2 ** 31 - 17 - 4 * c["args"]["channels"] for c in big)
    assert {_field(c["want"], "vst") for c in HX} == {0, 1, 2, 3}
    stops = collections.Counter(_hx_stop(c) for c in HX)
    assert {"nmac", "rows", "ncu", "none", "knob"} <= set(stops), stops
    assert "lds" not in stops, UNREACHED["hx G search stopped by LDS"]
    assert {_field(c["want"], "fixReset") for c in HX} == {0, 1}


def test_hx_fixture_covers_the_interior_range():
    """The empty interior range of the k0 comment (399 frames after 912 history rows: k0 clamped to nchunk), and k0 /
    k1 clipped by the output range, the input's first row, valid_end and the chunk count."""
    ln = BY_NAME["88cd-f32-c2-399-after-912"]["want"]
    assert (_field(ln, "in_len"), _field(ln, "hist_len")) == (399, 912)
    assert _field(ln, "k0") == _field(ln, "k1") == _field(ln, "nchunk") and _field(ln, "ib0") == _field(ln, "ib1") == _field(ln, "nblocks")
    assert _field(ln, "fixReset") == 0
    ln = BY_NAME["88cd-f32-c2-k0-by-input"]["want"]
    assert _field(ln, "k0") == 0 and _field(ln, "a_lo") * 32 >= 1000  # the first window starts inside the input
    ln = BY_NAME["88cd-f32-c2-k0-by-output"]["want"]
    assert _field(ln, "k0") == 1 and 1001 % 16 != 0  # chunk 0 holds outputs before o_lo
    ln = BY_NAME["88cd-f32-c2-k0-zero"]["want"]
    assert (_field(ln, "k0"), _field(ln, "k1")) == (0, _field(ln, "nchunk"))
    ln = BY_NAME["88cd-f32-c2-k1-by-output"]["want"]
    assert _field(ln, "k1") == _field(ln, "nchunk") - 1 and (1088 + 5003) % 16 != 0  # the last chunk holds outputs past o_hi
    ln = BY_NAME["88cd-f32-c2-k1-by-validend"]["want"]
    assert 0 < _field(ln, "k1") < _field(ln, "nchunk") - 1 and _field(ln, "valid_end") == 21000
    ln = BY_NAME["88cd-f32-c2-k1-nchunk"]["want"]
    assert _field(ln, "k1") == _field(ln, "nchunk")
    ln = BY_NAME["88cd-f32-c2-big"]["want"]  # the input's last rows: the windows of the last chunks run past them
    assert _field(ln, "k1") < _field(ln, "nchunk") - 1 and _field(ln, "valid_end") == _field(ln, "in_base") + _field(ln, "in_len")


def test_hx_knobs_routing_and_refusal():
    assert all(any(c["env"] == env for c in CASES) for env in HX_KNOBS)
    c = BY_NAME["88cd-f32-c2-big-GAR_HX_G=1"]
    assert (_field(c["want"], "G"), _field(BY_NAME[c["twin"]]["want"], "G")) == (1, 3)
    c = BY_NAME["88cd-f32-c2-big-GAR_HX_DWORD=1"]
    assert (_field(c["want"], "fmt"), _field(BY_NAME[c["twin"]]["want"], "fmt")) == (0, 1)
    c = BY_NAME["88cd-f32-c16-big-GAR_HX_DWORD=1"]
    assert (_field(c["want"], "fmt"), _field(BY_NAME[c["twin"]]["want"], "fmt")) == (0, 2)
    for n in ("cd48-f32-c2-big", "cd48-f32-c2-4096"):  # GAR_HXS=0 routes a row-block plan to hx_kernel
        assert BY_NAME[n]["want"].startswith(("hxt:", "hxs:")) and BY_NAME[n + "-GAR_HXS=0"]["want"].startswith("hx:")
    # a segmented plan never streams (the routing does not ask the streaming planner): hx_kernel, whatever GAR_HXS says
    assert BY_NAME["88cd-f32-c2-big"]["want"].startswith("hx:")
    assert BY_NAME["88cd-f32-c2-big-GAR_HXS=0"]["want"] == BY_NAME["88cd-f32-c2-big"]["want"]
    # the "not supported" fallback: GAR_HXS on, a row-block plan, the streaming planner declines (a chunk of more than
    # 2^24 macro periods, not clamped because a 4 MiB frame stride leaves no raw-load span) -> hx_kernel.  Its twin
    # streams.  Without the knob the same decline needs a call so long that hx_kernel refuses it too (2^30 columns).
    c, twin = BY_NAME["cd48-f32-c2-stride1M-GAR_HXS_NP=20000000"], BY_NAME["cd48-f32-c2-stride1M"]
    assert c["args"] == twin["args"] and c["env"] == {"GAR_HXS_NP": "20000000"} and not twin["env"]
    assert twin["want"].startswith("hxs:") and "fast[0,0)" in twin["want"] and c["want"].startswith("hx:")
    assert _field(c["want"], "fmt") == 3 and _field(c["want"], "G") == 5
    c = BY_NAME["cd48-f32-c2-stride1M-2e36periods"]
    assert not c["env"] and c["want"] == "invalid configuration\n"
    # PCM output: fused into the streaming kernels, refused by hx_kernel
    assert BY_NAME["cd48-f32-c2-out_pcm16"]["want"].startswith("hxs:")
    assert BY_NAME["cd48-f32-c2-out_pcm16-GAR_HXS=0"]["want"] == "not supported\n"
    assert BY_NAME["88cd-f32-c2-out_pcm16"]["want"] == "not supported\n"
    # a decimator without a split-f16 plan (its window exceeds hx_kernel's rows) runs bg_kernel in f32
    assert BY_NAME["96dec-f32-c2-big"]["want"].startswith("bg:") and _field(BY_NAME["96dec-f32-c2-big"]["want"], "unit") == "f32a"


def test_bad_arguments_are_refused(gar, handles):
    c = BY_NAME["cd48-f64-c2-4096"]
    h = handles["cd48", F64]
    with pytest.raises(gar.ResamplerError):
        gar.fir_plan(h, **dict(c["args"], stage=5))
    with pytest.raises(gar.ResamplerError):
        gar.fir_plan(h, **dict(c["args"], which=3))
    with pytest.raises(gar.ResamplerError):
        gar.fir_plan(h, **dict(c["args"], which=2))  # the stage has no decimator
    with pytest.raises(gar.ResamplerError):
        gar.fir_plan(h, **dict(c["args"], in_type=7))
    assert gar.fir_plan(h, **dict(c["args"], o_hi=c["args"]["o_lo"])) == ""
    # the streaming planner's entry point and this one agree where the launch streams
    c = BY_NAME["cd48-f32-c2-big"]
    a = {k: v for k, v in c["args"].items() if k != "which"}
    assert gar.hxs_plan(handles["cd48", F32], **a) == c["want"]
