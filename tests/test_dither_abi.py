"""CPU (dry-run handles and the host helper): TPDF-dithered integer PCM output, gar.h gar_set_dither.

  * gar_dev_dither_quantize -- the kernels' quantizer run on the host -- against the numpy restatement of
    the header's definition in dither_ref.py: the noise and the stored integers, bit for bit;
  * statistics of the noise (triangular on (-1, 1): mean 0, variance 1/6, white, channels independent),
    DC linearity (the quantized mean of a constant is the constant) and the clamp;
  * the setting: default, round trip, configuration not state (survives Reset and load_state, not in the
    blob), the position follows GetStatistics samplesOut, refusals change nothing.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dither_ref as D

SEEDS = [0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1]
CHANNELS = [0, 1, 255]
STARTS = [0, 2 ** 32 - 100, 2 ** 40]


def _inputs(bits):
    mv = D.MAXV[bits]
    edge = np.array([1.0, -1.0, 1.0 + 1e-9, -(1.0 + 1e-9), 2.0, -2.0, 0.0, 0.5 / mv, -0.5 / mv, np.nan, np.inf, -np.inf])
    rng = np.random.default_rng(bits)
    # the edge values twice over (different noise), values across the full range and values of a few LSB
    return np.concatenate([edge, rng.uniform(-1.1, 1.1, 150), edge, rng.uniform(-4, 4, 38) / mv])


def test_header_enum_values(gar):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gar.h")).read()
    assert re.search(r"enum \{ GAR_DITHER_NONE = 0, GAR_DITHER_TPDF = 1 \};", hdr)
    assert (gar.DITHER_NONE, gar.DITHER_TPDF) == (0, 1)


@pytest.mark.parametrize("bits", [16, 24, 32, 280])
def test_quantizer_equals_numpy_restatement(gar, bits):
    """Noise equal and integers equal for every seed x channel x start (one start crosses a multiple of
    2^32 after 100 positions), on +-1, +-(1 + 1e-9), +-2, 0, +-0.5 / maxVal, NaN, +-Inf and random values."""
    y = _inputs(bits)
    assert y.size > 200
    for seed in SEEDS:
        for c in CHANNELS:
            for n0 in STARTS:
                q, d = gar.dither_quantize(y, bits, seed, c, n0)
                pos = np.uint64(n0) + np.arange(y.size, dtype=np.uint64)
                assert np.array_equal(d, D.noise(seed, c, pos)), (hex(seed), c, n0)
                want = D.quantize(y, bits, seed, c, n0)
                assert np.array_equal(q.astype(np.int64), want), (hex(seed), c, n0, int(np.count_nonzero(q != want)))
    mv = int(D.MAXV[bits])
    # the last combination's integers: full scale and beyond stay within one LSB inside the clamp, NaN is 0
    for i in (0, 2, 4, 10):
        assert mv - 1 <= want[i] <= mv and -mv <= want[i + 1] <= -mv + 1, (i, want[i], want[i + 1])
    assert want[9] == 0 and want[6] in (-1, 0, 1)


def test_quantizer_arguments(gar):
    L = gar.lib()
    y = np.array([0.25, -0.25])
    q = np.zeros(2, dtype=np.int32)
    d = np.zeros(2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for bad in (gar.F32, gar.F64, gar.F16, gar.BF16, 0, 8, 23):
        assert L.gar_dev_dither_quantize(bad, 1, 0, 0, p(y), 2, p(q), p(d)) == gar.INVALID_ARGUMENT, bad
    assert not q.any() and not d.any()
    # either output may be NULL; packed 24-bit gives PCM24's integers
    assert L.gar_dev_dither_quantize(gar.PCM24, 5, 1, 7, p(y), 2, p(q), None) == gar.GAR_OK
    assert L.gar_dev_dither_quantize(gar.PCM24, 5, 1, 7, p(y), 2, None, p(d)) == gar.GAR_OK
    q2 = np.zeros(2, dtype=np.int32)
    assert L.gar_dev_dither_quantize(gar.PCM24_PACKED, 5, 1, 7, p(y), 2, p(q2), None) == gar.GAR_OK
    assert np.array_equal(q, q2) and np.array_equal(q.astype(np.int64), D.quantize(y, 24, 5, 1, 7))


@pytest.mark.parametrize("seed", SEEDS)
def test_noise_statistics(gar, seed):
    """2^20 positions: |mean| <= 2.5e-3, |var - 1/6| <= 2e-3, |lag-1 autocorrelation| <= 6e-3, |channel 0 / 1
    correlation| <= 6e-3 (about six standard errors of these estimators at this N: 4.0e-4, 1.9e-4, 1e-3, 1e-3),
    max |d| < 1."""
    n = 1 << 20
    z = np.zeros(n)
    _, d0 = gar.dither_quantize(z, 16, seed, 0, 0)
    _, d1 = gar.dither_quantize(z, 16, seed, 1, 0)
    assert np.abs(d0).max() < 1.0 and np.abs(d1).max() < 1.0
    assert abs(d0.mean()) <= 2.5e-3, d0.mean()
    assert abs(d0.var() - 1.0 / 6.0) <= 2e-3, d0.var()
    assert abs(np.corrcoef(d0[:-1], d0[1:])[0, 1]) <= 6e-3
    assert abs(np.corrcoef(d0, d1)[0, 1]) <= 6e-3


@pytest.mark.parametrize("frac", [0.0, 0.25, 0.5, 0.9])
def test_dc_linearity(gar, frac):
    """A constant (100 + f) / 32767 over 2^18 positions quantizes to mean 100 + f within 6e-3 LSB (standard error
    1e-3), and only values within +-2 of 100 occur."""
    y = np.full(1 << 18, (100.0 + frac) / 32767.0)
    q, _ = gar.dither_quantize(y, 16, 7, 0, 0)
    assert abs(q.mean() - (100.0 + frac)) <= 6e-3, q.mean() - 100.0
    assert q.min() >= 98 and q.max() <= 102


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_clamp(gar, bits):
    """y = +-1.0 over 2^16 positions never leaves +-maxVal and reaches it."""
    mv = int(D.MAXV[bits])
    n = 1 << 16
    hi, _ = gar.dither_quantize(np.full(n, 1.0), bits, 3, 0, 0)
    lo, _ = gar.dither_quantize(np.full(n, -1.0), bits, 3, 0, 0)
    assert hi.max() == mv and hi.min() >= mv - 1
    assert lo.min() == -mv and lo.max() <= -mv + 1


def _dry(gar, ch=2):
    return gar.New(gar.Config(44100, 48000, ch, gar.QualityHigh, DryRun=True))


def _device_step(gar, r, frames, ot):
    """One dry-run gar_process_device (the stream-length bookkeeping only); returns the frames produced."""
    L = gar.lib()
    got = C.c_int64(0)
    one = C.c_void_p(1)
    ch = r.Channels
    n = L.gar_device_output_size(r._h, frames)
    assert L.gar_process_device(r._h, one, gar.F32, ch, 1, frames, ch, one, ot, ch, 1, n, C.byref(got), None) == gar.GAR_OK
    return got.value


def test_setting_default_round_trip_and_refusals(gar):
    L = gar.lib()
    r = _dry(gar)
    assert r.get_dither() == (gar.DITHER_NONE, 0, 0)
    r.set_dither(gar.DITHER_TPDF, 0x123456789ABCDEF0)
    assert r.get_dither() == (gar.DITHER_TPDF, 0x123456789ABCDEF0, 0)
    r.set_dither(gar.DITHER_TPDF, 2 ** 64 - 1)
    assert r.get_dither()[:2] == (gar.DITHER_TPDF, 2 ** 64 - 1)
    r.set_dither(gar.DITHER_TPDF)
    assert r.get_dither()[:2] == (gar.DITHER_TPDF, 0)
    r.set_dither(gar.DITHER_TPDF, 9)
    for bad in (2, -1, 1 << 20):
        assert L.gar_set_dither(r._h, bad, 77) == gar.INVALID_ARGUMENT
        with pytest.raises(gar.ResamplerError):
            r.set_dither(bad, 77)
    assert r.get_dither()[:2] == (gar.DITHER_TPDF, 9)
    assert L.gar_set_dither(None, gar.DITHER_TPDF, 1) == gar.INVALID_ARGUMENT
    m = C.c_int32(-5)
    assert L.gar_get_dither(None, C.byref(m), None, None) == gar.INVALID_ARGUMENT and m.value == -5
    # each output of gar_get_dither may be NULL
    s, p = C.c_uint64(0), C.c_int64(-7)
    assert L.gar_get_dither(r._h, None, None, None) == gar.GAR_OK
    assert L.gar_get_dither(r._h, None, C.byref(s), None) == gar.GAR_OK and s.value == 9
    assert L.gar_get_dither(r._h, None, None, C.byref(p)) == gar.GAR_OK and p.value == 0
    r.set_dither(gar.DITHER_NONE, 0)
    assert r.get_dither() == (gar.DITHER_NONE, 0, 0)


def test_position_follows_samples_out_and_reset(gar):
    r = _dry(gar)
    r.set_dither(gar.DITHER_TPDF, 5)
    total = 0
    for frames, ot in ((4410, gar.PCM16), (1000, gar.F32), (3333, gar.PCM24_PACKED)):
        total += _device_step(gar, r, frames, ot)
        assert r.get_dither()[2] == total == r.GetStatistics()["samplesOut"]
    assert total > 0
    L = gar.lib()
    got = C.c_int64(0)
    m = L.gar_device_flush_size(r._h)
    assert L.gar_flush_device(r._h, 2, C.c_void_p(1), gar.PCM16, 2, 1, m, C.byref(got), None) == gar.GAR_OK
    assert r.get_dither()[2] == total + got.value == r.GetStatistics()["samplesOut"]
    r.Reset()
    assert r.get_dither() == (gar.DITHER_TPDF, 5, 0)


def test_position_is_minus_one_when_not_in_lockstep(gar):
    r = _dry(gar)
    r.Process(np.zeros(1000))  # the host Process advances channel 0 alone: the handle splits
    assert r.get_dither()[2] == -1


def test_setting_is_configuration_not_state(gar):
    """state_size and the blob bytes are identical with dither on and off; load_state keeps the handle's own
    setting and restores the position (the statistics)."""
    a, b = _dry(gar), _dry(gar)
    b.set_dither(gar.DITHER_TPDF, 0xDEADBEEF)
    for r in (a, b):
        _device_step(gar, r, 5000, gar.PCM16)
    assert a.state_size() == b.state_size()
    blob_a, blob_b = a.save_state(), b.save_state()
    assert blob_a == blob_b
    pos = b.get_dither()[2]
    assert pos > 0
    c = _dry(gar)
    c.set_dither(gar.DITHER_TPDF, 42)
    c.load_state(blob_a)
    assert c.get_dither() == (gar.DITHER_TPDF, 42, pos)
    b.load_state(blob_a)
    assert b.get_dither() == (gar.DITHER_TPDF, 0xDEADBEEF, pos)
    a.load_state(blob_b)
    assert a.get_dither() == (gar.DITHER_NONE, 0, pos)
