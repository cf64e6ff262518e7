"""CPU (dry-run handles and the host helper): the clip counter / peak meter of gar.h gar_set_meter.

  * gar_dev_meter_tally -- the kernels' tally function run on the host -- against the numpy restatement of the
    header's definition in meter_ref.py, exactly: all four PCM types, dither off and on, the edge values, positions
    crossing 2^32, and samples at exactly +-1.0 where only the dithered quantizer's second clamp can fire;
  * refusals that change nothing, the defaults, a dry-run handle reading zeros;
  * the setting is configuration: it survives Reset and load_state and is not in the blob.
"""
import ctypes as C

import numpy as np
import pytest

import dither_ref as D
import meter_ref as M

SEEDS = [0, 0x123456789ABCDEF0]
CHANNELS = [0, 1, 255]
STARTS = [0, 2 ** 32 - 100, 2 ** 40]


def _inputs(bits):
    mv = D.MAXV[bits]
    up = np.nextafter(1.0, 2.0)
    tiny = np.nextafter(0.0, 1.0)  # the smallest denormal
    edge = np.array([1.0, -1.0, up, -up, np.inf, -np.inf, np.nan, 0.0, -0.0, tiny, -tiny, 2.2e-308 / 4, 2.0, -3.5,
                     0.5 / mv, 1.0 - 0.25 / mv, -(1.0 - 0.25 / mv)])
    rng = np.random.default_rng(bits)
    return np.concatenate([edge, rng.uniform(-1.1, 1.1, 120), np.full(40, 1.0), np.full(40, -1.0), edge])


def _dry(gar, ch=2):
    return gar.New(gar.Config(44100, 48000, ch, gar.QualityHigh, DryRun=True))


@pytest.mark.parametrize("dither", [0, 1])
@pytest.mark.parametrize("bits", [16, 24, 32, 280])
def test_tally_equals_numpy_restatement(gar, bits, dither):
    y = _inputs(bits)
    assert y.size > 200
    for seed in SEEDS:
        for c in CHANNELS:
            for n0 in STARTS:
                want = M.tally(y, bits, dither, seed, c, n0)
                got = gar.meter_tally(y, bits, dither, seed, c, n0)
                assert got[0] == want[0], (hex(seed), c, n0, got, want)
                assert np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64)
    # without +-Inf the peak is the largest finite magnitude, NaN ignored; an empty run reads (0, 0)
    fin = y[np.isfinite(y) | np.isnan(y)]
    assert gar.meter_tally(fin, bits, dither, 1, 0, 0)[1] == 3.5
    assert gar.meter_tally(np.array([np.nan, np.nan]), bits, dither, 1, 0, 0) == (0, 0.0)
    assert gar.meter_tally(np.array([]), bits, dither, 1, 0, 0) == (0, 0.0)


@pytest.mark.parametrize("bits", [16, 24, 32, 280])
def test_second_clamp_counts_at_exact_full_scale(gar, bits):
    """Samples of exactly +-1.0 and just inside: the first clamp changes none of them, so every clip is the dithered
    quantizer's second clamp -- and the numpy side alone shows that it fires."""
    mv = D.MAXV[bits]
    y = np.concatenate([np.full(300, 1.0), np.full(300, -1.0), np.full(100, 1.0 - 0.25 / mv)])
    seed, c, n0 = 11, 3, 2 ** 32 - 350
    assert not M.first_clamp(y).any()
    second = M.second_clamp(y, bits, seed, c, n0)
    assert second[:300].any() and second[300:600].any(), "the inputs must make the second clamp fire on both sides"
    want = int(np.count_nonzero(second))
    assert gar.meter_tally(y, bits, 1, seed, c, n0) == (want, 1.0)
    assert gar.meter_tally(y, bits, 0, seed, c, n0) == (0, 1.0)


def test_tally_arguments(gar):
    L = gar.lib()
    y = np.array([0.25, -1.5])
    p = y.ctypes.data_as(C.c_void_p)
    cl, pk = C.c_uint64(77), C.c_double(-3.0)
    for bad in (gar.F32, gar.F64, gar.F16, gar.BF16, 0, 8, 23):
        assert L.gar_dev_meter_tally(bad, 0, 1, 0, 0, p, 2, C.byref(cl), C.byref(pk)) == gar.INVALID_ARGUMENT, bad
    for mode in (2, -1):
        assert L.gar_dev_meter_tally(gar.PCM16, mode, 1, 0, 0, p, 2, C.byref(cl), C.byref(pk)) == gar.INVALID_ARGUMENT
    assert L.gar_dev_meter_tally(gar.PCM16, 0, 1, -1, 0, p, 2, C.byref(cl), C.byref(pk)) == gar.INVALID_ARGUMENT
    assert (cl.value, pk.value) == (77, -3.0)
    assert L.gar_dev_meter_tally(gar.PCM16, 0, 1, 0, 0, p, 2, C.byref(cl), None) == gar.GAR_OK and cl.value == 1
    assert L.gar_dev_meter_tally(gar.PCM16, 0, 1, 0, 0, p, 2, None, C.byref(pk)) == gar.GAR_OK and pk.value == 1.5


def test_defaults_refusals_and_dry_run_reads_zeros(gar):
    L = gar.lib()
    r = _dry(gar, 3)
    assert r.get_meter() is False
    clips, peak = r.meter_read()
    assert clips.dtype == np.uint64 and clips.tolist() == [0, 0, 0] and peak.tolist() == [0.0, 0.0, 0.0]
    assert L.gar_set_meter(None, 1) == gar.INVALID_ARGUMENT
    assert L.gar_get_meter(None, None) == gar.INVALID_ARGUMENT
    assert L.gar_meter_read(None, 0, 1, None, None, 0) == gar.INVALID_ARGUMENT
    for bad in (2, -1, 1 << 20):
        assert L.gar_set_meter(r._h, bad) == gar.INVALID_ARGUMENT
        assert r.get_meter() is False
    r.set_meter(True)
    assert r.get_meter() is True
    for bad in (2, -1):
        with pytest.raises(gar.ResamplerError):
            r.set_meter(bad)
        assert r.get_meter() is True
    # a channel range outside the handle: refused, nothing read or reset
    c = np.full(4, 99, dtype=np.uint64)
    k = np.full(4, -1.0)
    pc, pk = c.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)
    for ch0, n in ((0, 4), (3, 1), (-1, 1), (2, 2), (0, -1), (1, 2 ** 31 - 1)):
        assert L.gar_meter_read(r._h, ch0, n, pc, pk, 1) == gar.INVALID_ARGUMENT, (ch0, n)
        assert c.tolist() == [99] * 4 and k.tolist() == [-1.0] * 4
    # in range: zeros on a dry-run handle, either pointer may be NULL, an empty range is fine
    assert L.gar_meter_read(r._h, 1, 2, pc, pk, 1) == gar.GAR_OK
    assert c.tolist() == [0, 0, 99, 99] and k.tolist() == [0.0, 0.0, -1.0, -1.0]
    assert L.gar_meter_read(r._h, 0, 3, None, None, 0) == gar.GAR_OK
    assert L.gar_meter_read(r._h, 3, 0, pc, pk, 0) == gar.GAR_OK
    r.set_meter(False)
    assert r.get_meter() is False


def _device_step(gar, r, frames, ot):
    L = gar.lib()
    got = C.c_int64(0)
    one = C.c_void_p(1)
    ch = r.Channels
    n = L.gar_device_output_size(r._h, frames)
    assert L.gar_process_device(r._h, one, gar.F32, ch, 1, frames, ch, one, ot, ch, 1, n, C.byref(got), None) == gar.GAR_OK
    return got.value


def test_setting_is_configuration_not_state(gar):
    """The setting survives Reset and load_state; state_size and the blob bytes are the same with the meter on and off."""
    a, b = _dry(gar), _dry(gar)
    b.set_meter(True)
    for r in (a, b):
        assert _device_step(gar, r, 5000, gar.PCM16) > 0
    assert a.state_size() == b.state_size()
    blob_a, blob_b = a.save_state(), b.save_state()
    assert blob_a == blob_b
    b.Reset()
    assert b.get_meter() is True
    b.load_state(blob_a)
    assert b.get_meter() is True
    a.load_state(blob_b)
    assert a.get_meter() is False
    assert b.save_state() == blob_a
    assert b.meter_read()[0].tolist() == [0, 0]
