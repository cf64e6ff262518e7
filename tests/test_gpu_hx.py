"""GPU: the float32 compute path (split-f16 MFMA kernel, csrc/gar_hx.hpp) against
the oracle and against the exact-f32 MFMA kernel (GAR_F32_EXACT).

Tolerances: BASELINE.json north_star float32 <= 1e-6 RMS vs the reference.
The split path's error must also stay within 2x of exact-f32 arithmetic's
(it is in fact below it: 22-bit operands, f32 accumulation).
Edge cases: Inf/NaN and |x| >= 16 samples (exact f64 fallback of the outputs
whose windows hold one, two-stage for non-finite), extreme magnitudes, ragged
lengths, both directions, the DFT-only / decimator stages and chunked
streaming (bit-identical to one shot).
"""
import numpy as np
import pytest

from helpers import F32_RMS_TOL, chunk_sizes, oracle_new, rms, signal

pytestmark = pytest.mark.gpu


def run(gar, torch, in_rate, out_rate, x, preset, dtype, chunks=None):
    ch = x.shape[1]
    r = gar.New(gar.Config(in_rate, out_rate, ch, preset, ComputeDtype=dtype))
    xd = torch.from_numpy(np.ascontiguousarray(x)).float().cuda()
    outs, s = [], 0
    for n in (chunks or [x.shape[0]]):
        outs.append(r.process_device(xd[s:s + n]).clone())
        s += n
    outs.append(r.flush_device(dtype=torch.float32).clone())
    torch.cuda.synchronize()
    return torch.cat(outs).double().cpu().numpy()


CASES = [
    (44100, 48000, 2, "QualityHigh"),      # cfg2 geometry (fused composite)
    (48000, 44100, 5, "QualityVeryHigh"),  # cfg3 geometry, odd channel count
    (96000, 44100, 3, "QualityVeryHigh"),  # decimator + fused
    (22050, 44100, 1, "QualityHigh"),      # DFT-only (integer up)
    (48000, 16000, 2, "QualityMedium"),    # integer down (decimator)
    (44100, 96000, 4, "QualityLow"),       # halfband x2 + fused
]


@pytest.mark.parametrize("case", CASES)
def test_hx_vs_oracle_and_exact(gar, O, cuda, case):
    ir, orr, ch, q = case
    n = 30011  # ragged
    x = signal(n, ch, ir, seed=ir + ch).astype(np.float32).astype(np.float64)
    got = run(gar, cuda, ir, orr, x, getattr(gar, q), gar.F32)
    ex = run(gar, cuda, ir, orr, x, getattr(gar, q), gar.F32_EXACT)
    want = oracle_new(O, ir, orr, x, getattr(O, "P_" + q[7:].upper()))
    for c in range(ch):
        assert got.shape[0] == ex.shape[0] == len(want[c])
        e_hx, e_ex = rms(got[:, c], want[c]), rms(ex[:, c], want[c])
        assert e_hx <= F32_RMS_TOL, e_hx
        assert e_hx <= max(2.0 * e_ex, 1e-8), (e_hx, e_ex)


@pytest.mark.parametrize("chunk", [4096, 1001])
def test_hx_chunked_equals_oracle(gar, O, cuda, chunk):
    x = signal(50000, 2, 44100).astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32, chunk_sizes(50000, chunk))
    want = oracle_new(O, 44100, 48000, x, O.P_HIGH)
    for c in range(2):
        assert got.shape[0] == len(want[c])
        assert rms(got[:, c], want[c]) <= F32_RMS_TOL


@pytest.mark.parametrize("scale", [1e30, 3.0e4, 1e-6])
def test_hx_extreme_magnitudes(gar, O, cuda, scale):
    """|x| >= 16 takes the exact f64 path; quiet signals keep 22-bit operands down to
    |x| ~ 2^-26 (the lo halves are scaled apart): error stays relative to the level."""
    x = signal(40000, 2, 44100, seed=7)
    xs = (x * scale).astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 44100, 48000, xs, gar.QualityHigh, gar.F32)
    want = oracle_new(O, 44100, 48000, xs, O.P_HIGH)
    for c in range(2):
        assert np.all(np.isfinite(got[:, c]))
        assert rms(got[:, c] / scale, want[c] / scale) <= F32_RMS_TOL


def test_hx_tiny_signal_absolute_floor(gar, O, cuda):
    """Below |x| ~ 2^-26 the fixed split scale leaves an absolute floor of ~2^-47."""
    x = signal(20000, 2, 44100, seed=8) * 1e-30
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32)
    want = oracle_new(O, 44100, 48000, x, O.P_HIGH)
    for c in range(2):
        assert np.max(np.abs(got[:, c] - want[c])) <= 1e-13


def test_hx_mixed_levels(gar, O, cuda):
    """A loud channel beside a very quiet one."""
    x = signal(40000, 2, 44100, seed=9)
    x[:, 1] *= 1e-6
    x = x.astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32)
    want = oracle_new(O, 44100, 48000, x, O.P_HIGH)
    assert rms(got[:, 0], want[0]) <= F32_RMS_TOL
    assert rms(got[:, 1] * 1e6, want[1] * 1e6) <= F32_RMS_TOL


@pytest.mark.parametrize("chunks", [None, 4096, 997])
def test_hx_nonfinite_propagates(gar, O, cuda, chunks):
    """Inf / NaN samples: non-finite exactly where the reference is -- an Inf gives NaN
    where the two-stage reference sums +Inf and -Inf DFT outputs (the exact fallback
    runs the two stages), +-Inf where it does not -- and the oracle's values elsewhere;
    any chunking gives the same bits."""
    n = 60000
    x = signal(n, 2, 44100, seed=11).astype(np.float32).astype(np.float64)
    x[20000, 0] = np.inf
    x[41000, 1] = np.nan
    x[41500, 0] = -np.inf
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32, None if chunks is None else chunk_sizes(n, chunks))
    want = oracle_new(O, 44100, 48000, x, O.P_HIGH)
    for c in range(2):
        w = np.asarray(want[c])
        fin = np.isfinite(w)
        assert not fin.all()
        np.testing.assert_array_equal(np.isnan(got[:, c]), np.isnan(w))
        np.testing.assert_array_equal(np.isposinf(got[:, c]), np.isposinf(w))
        np.testing.assert_array_equal(np.isneginf(got[:, c]), np.isneginf(w))
        assert rms(got[fin, c], w[fin]) <= F32_RMS_TOL
    if chunks is not None:
        one = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32)
        np.testing.assert_array_equal(got, one)


@pytest.mark.parametrize("chunks", [None, 4096, 1231])
def test_hx_loud_samples(gar, O, cuda, chunks):
    """Finite samples beyond the split range (|x| >= 16: clipped/unnormalised audio) next
    to normal ones: outputs whose windows hold one are exact, the rest are split-f16,
    and the result does not depend on the chunking."""
    n = 50000
    x = signal(n, 2, 44100, seed=12).astype(np.float32).astype(np.float64)
    x[10000:10050, 0] *= 1000.0
    x[33333, 1] = -3.0e5
    x[45000:, 0] *= 40.0
    x = x.astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32, None if chunks is None else chunk_sizes(n, chunks))
    want = oracle_new(O, 44100, 48000, x, O.P_HIGH)
    ex = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32_EXACT)
    for c in range(2):
        assert got.shape[0] == len(want[c])
        # error at the level of exact-f32 arithmetic on the same (partly loud) signal
        assert rms(got[:, c], want[c]) <= max(3.0 * rms(ex[:, c], want[c]), F32_RMS_TOL)
        big = np.abs(np.asarray(want[c])) > 20
        if big.any():
            assert np.max(np.abs(got[big, c] - want[c][big]) / np.abs(want[c][big])) <= 1e-6
    if chunks is not None:
        one = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32)
        np.testing.assert_array_equal(got, one)


def test_hx_zero_input(gar, O, cuda):
    x = np.zeros((20000, 2))
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32)
    assert np.all(got == 0.0)


def test_hx_loud_many_columns(gar, O, cuda):
    """Loud samples (|x| >= 16) in several columns of one 16-column block and in many blocks of
    one launch (16 channels: ROW16 loads, every block holds loud columns): each output whose
    window holds one is recomputed exactly after the block (hxsFixup), for every column."""
    n, ch = 120000, 16
    x = signal(n, ch, 48000, seed=21).astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(5)
    for c in range(ch):
        for t in rng.integers(0, n, size=6):
            x[t, c] = (1 if rng.random() < 0.5 else -1) * 10.0 ** rng.uniform(1.3, 5)
    x = x.astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 48000, 44100, x, gar.QualityVeryHigh, gar.F32)
    want = oracle_new(O, 48000, 44100, x, O.P_VERYHIGH)
    ex = run(gar, cuda, 48000, 44100, x, gar.QualityVeryHigh, gar.F32_EXACT)
    for c in range(ch):
        assert got.shape[0] == len(want[c])
        assert rms(got[:, c], want[c]) <= max(3.0 * rms(ex[:, c], want[c]), F32_RMS_TOL)
        big = np.abs(np.asarray(want[c])) > 20
        assert big.any()
        assert np.max(np.abs(got[big, c] - want[c][big]) / np.abs(want[c][big])) <= 1e-6


@pytest.mark.parametrize("chunk", [4096, 1500])
def test_hx_row16_small_launches_loud(gar, O, cuda, chunk):
    """16 channels fed in short calls: every launch is a small ROW16 launch (hxq_kernel: one
    workgroup per block and row-block group, history seam loaded through the history resource),
    with loud samples in many columns -- the same bits as the one-shot call, exact where loud."""
    n, ch = 40000, 16
    x = signal(n, ch, 48000, seed=23).astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(9)
    for c in range(ch):
        for t in rng.integers(0, n, size=3):
            x[t, c] = (1 if rng.random() < 0.5 else -1) * 10.0 ** rng.uniform(1.3, 4)
    x = x.astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 48000, 44100, x, gar.QualityVeryHigh, gar.F32, chunk_sizes(n, chunk))
    one = run(gar, cuda, 48000, 44100, x, gar.QualityVeryHigh, gar.F32)
    np.testing.assert_array_equal(got, one)
    want = oracle_new(O, 48000, 44100, x, O.P_VERYHIGH)
    for c in range(ch):
        big = np.abs(np.asarray(want[c])) > 20
        assert big.any()
        assert np.max(np.abs(got[big, c] - want[c][big]) / np.abs(want[c][big])) <= 1e-6


@pytest.mark.parametrize("chunks", [None, 4096])
def test_hx_values_just_below_16(gar, O, cuda, chunks):
    """Samples in [15.996, 16): x * 2^12 rounds to f16 +-Inf there (65520 ties to even), so the split
    bound is 16 - 2^-8 -- at or above it a sample takes the exact path, just below it the split stays
    finite.  Every output finite and within the float32 bar of the oracle, any chunking the same bits."""
    n = 40000
    x = signal(n, 2, 44100, seed=13).astype(np.float32).astype(np.float64)
    vals = [15.99609375, 15.997, 15.9999, -15.99609375, -15.998, 15.996, -15.9960937, 15.99, 16.0]
    rng = np.random.default_rng(3)
    for i, v in enumerate(vals * 6):
        x[int(rng.integers(100, n - 100)), i % 2] = v
    x = x.astype(np.float32).astype(np.float64)
    got = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32, None if chunks is None else chunk_sizes(n, chunks))
    want = oracle_new(O, 44100, 48000, x, O.P_HIGH)
    ex = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32_EXACT)
    for c in range(2):
        assert np.all(np.isfinite(got[:, c]))
        assert rms(got[:, c], want[c]) <= max(3.0 * rms(ex[:, c], want[c]), F32_RMS_TOL)
    if chunks is not None:
        one = run(gar, cuda, 44100, 48000, x, gar.QualityHigh, gar.F32)
        np.testing.assert_array_equal(got, one)


_HX_CHILD = """
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import gar
ir, orr, src, dst = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
x = torch.from_numpy(np.load(src)).cuda()
def run(ck):
    r = gar.New(gar.Config(ir, orr, x.shape[1], gar.QualityHigh, ComputeDtype=gar.F32))
    parts = [r.process_device(x[s:s + ck]).clone() for s in range(0, x.shape[0], ck)]
    parts.append(r.flush_device(dtype=torch.float32).clone())
    torch.cuda.synchronize()
    return torch.cat(parts).cpu().numpy()
np.savez(dst, one=run(x.shape[0]), chunked=run(997))
"""


def _hazard_input(rate):
    """12,000 stereo frames with one loud run (40 samples x 1000) and a +Inf, a NaN and a -Inf 2,500 frames apart."""
    x = signal(12000, 2, rate, seed=31).astype(np.float32).astype(np.float64)
    x[1500:1540, 0] *= 1000.0
    x[4000, 1] = np.inf
    x[6500, 0] = np.nan
    x[9000, 1] = -np.inf
    return x.astype(np.float32)


@pytest.mark.parametrize("ir,orr,hxs_off", [(44100, 48000, True), (88200, 44100, False)])
def test_hx_kernel_exact_fallback(O, cuda, tmp_path, ir, orr, hxs_off):
    """hx_kernel's exact recompute of loud and non-finite windows (hxFixupBlock -> firExact), which no other GPU test
    reaches for a composite: a row-block plan streams through hxs / hxq / hxt unless GAR_HXS=0, and that knob is read
    once per process, so a fresh child runs the stream (GAR_HX_TRACE=1: its launches are `hx:` lines).
    44.1k -> 48k High with GAR_HXS=0 is a DFT x2 (*) polyphase composite -- the non-finite windows take the two-stage
    half; 88.2k -> 44.1k High is an integer decimator whose split-f16 plan is segmented, hx_kernel by the default
    route (the launch-plan cases' 88cd) -- the single-stage half.  One-shot and in 997-frame calls: every output's
    NaN / +Inf / -Inf class is the oracle's, the finite ones are within the float32 bar, and the two runs are bit-equal.
    The bar leaves room on this input: the loud run's ~45 (~20) outputs reach |y| ~ 900 (ulp 6e-5), so the oracle's own
    values rounded to float32 are already 7.0e-7 (4.4e-7) RMS from it over the ~13,000 (6,000) outputs of channel 0 --
    asserted to be within 0.75 of the bar; the split-f16 arithmetic of the other outputs (~1e-7) adds in quadrature.
    The oracle alone leaves 96 % (85 %: the decimator's longer rows) of the Inf channel's outputs finite."""
    import os
    import subprocess
    import sys
    x = _hazard_input(ir)
    want = oracle_new(O, ir, orr, x.astype(np.float64), O.P_HIGH)
    src, dst = str(tmp_path / "x.npy"), str(tmp_path / "y.npz")
    np.save(src, x)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GAR_HX_TRACE="1")
    if hxs_off:
        env["GAR_HXS"] = "0"
    p = subprocess.run([sys.executable, "-c", _HX_CHILD, os.path.join(root, "go-audio-resampler_amd"), str(ir), str(orr), src, dst],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stderr.splitlines() if ln.startswith(("hx:", "hxs:", "hxt:", "hxq:"))]
    assert any(ln.startswith("hx:") for ln in lines), p.stderr[-2000:]
    assert all(ln.startswith("hx:") for ln in lines), lines[:8]
    y = np.load(dst)
    one, chunked = y["one"], y["chunked"]
    assert one.dtype == np.float32 and one.shape == chunked.shape
    np.testing.assert_array_equal(one.view(np.uint32), chunked.view(np.uint32))
    for c in range(2):
        w = np.asarray(want[c])
        fin = np.isfinite(w)
        assert one.shape[0] == len(w)
        # neither all finite nor mostly non-finite
        assert (0.9 if hxs_off else 0.8) * len(w) < fin.sum() < len(w), (c, int(fin.sum()), len(w))
        assert rms(w[fin].astype(np.float32), w[fin]) <= 0.75 * F32_RMS_TOL
        g = one[:, c].astype(np.float64)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w))
        np.testing.assert_array_equal(np.isposinf(g), np.isposinf(w))
        np.testing.assert_array_equal(np.isneginf(g), np.isneginf(w))
        e = rms(g[fin], w[fin])
        print("hx_kernel exact fallback %d -> %d ch%d: rms %.3e over %d finite of %d" % (ir, orr, c, e, fin.sum(), len(w)))
        assert e <= F32_RMS_TOL, (c, e)


def test_hxt_expired_wait_is_a_device_error(gar, cuda, monkeypatch):
    """An expired progress wait of the streaming kernel (hxt_kernel) is an error, not output
    (VERDICT r04 item 2): the development knob GAR_HXT_FAULT=1 makes the compute waves' load count
    unreachable (and the poll bound short), the status word reaches the host, gar_synchronize and
    the next call return GAR_ERR_DEVICE naming hxt_kernel, and Reset recovers the handle."""
    torch = cuda
    frames = 44100 * 20  # a streaming (non-small) launch: hxt_kernel, stereo frames
    x = torch.from_numpy(signal(frames, 2, 44100, seed=7).astype(np.float32)).cuda()
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32))
    ref = r.process_device(x).clone()
    torch.cuda.synchronize()
    r.Reset()
    monkeypatch.setenv("GAR_HXT_FAULT", "1")
    r.process_device(x)  # asynchronous: enqueued fine
    with pytest.raises(gar.ErrDevice, match="hxt_kernel"):
        r.synchronize()
    monkeypatch.delenv("GAR_HXT_FAULT")
    with pytest.raises(gar.ErrDevice):  # poisoned until Reset
        r.process_device(x)
    r.Reset()
    again = r.process_device(x).clone()
    r.synchronize()
    assert torch.equal(again, ref)


@pytest.mark.parametrize("ch,dtype,mono_first", [(256, "F32", False), (64, "F64", False), (24, "F32", True)])
def test_large_host_calls_equal_device_stream(gar, cuda, ch, dtype, mono_first):
    """Host ProcessMulti calls large enough for the packing pool (AVX2 conversions, streaming
    stores into the caller's arrays, whole channels per job) return exactly the samples and counts
    of the same streams run through the device API in one call each (chunked == one-shot, stereo ==
    monos), including a handle whose channel 0 was advanced alone first (two channel groups), and
    FlushMulti afterwards."""
    import torch
    n = 2 * 4096 if ch >= 256 else 6 * 4096 + 77
    x = signal(n, ch, 44100, seed=ch).astype(np.float32).astype(np.float64)
    dt = getattr(gar, dtype)
    tdt = torch.float32 if dtype == "F32" else torch.float64
    rh = gar.New(gar.Config(44100, 48000, ch, gar.QualityHigh, ComputeDtype=dt))
    pre = 1000 if mono_first else 0
    got = [[] for _ in range(ch)]
    if mono_first:
        got[0].append(rh.Process(x[:pre, 0]))
    # channel 0 continues at frame pre, the others start at 0: every call gives all channels k frames
    lens = [n - pre] if ch >= 256 else [4096 * 5 + 11, n - pre - (4096 * 5 + 11)]
    s = 0
    for k in lens:
        res = rh.ProcessMulti([x[s + (pre if c == 0 else 0):s + (pre if c == 0 else 0) + k, c] for c in range(ch)])
        for c in range(ch):
            got[c].append(res[c])
        s += k
    tails = rh.FlushMulti()
    got = [np.concatenate(got[c] + [tails[c]]) for c in range(ch)]
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(tdt).cuda()
    if mono_first:
        ref = []
        for c in range(ch):
            r1 = gar.New(gar.Config(44100, 48000, 1, gar.QualityHigh, ComputeDtype=dt))
            L = n if c == 0 else n - pre
            y = torch.cat([r1.process_device(xd[:L, c:c + 1].contiguous()), r1.flush_device(dtype=tdt)])
            ref.append(y[:, 0].double().cpu().numpy())
    else:
        rd = gar.New(gar.Config(44100, 48000, ch, gar.QualityHigh, ComputeDtype=dt))
        y = torch.cat([rd.process_device(xd), rd.flush_device(dtype=tdt)]).double().cpu().numpy()
        ref = [y[:, c] for c in range(ch)]
    torch.cuda.synchronize()
    for c in range(ch):
        assert got[c].shape == ref[c].shape, (c, got[c].shape, ref[c].shape)
        np.testing.assert_array_equal(got[c], ref[c])
