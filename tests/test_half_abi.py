"""CPU (dry-run handles): the half-precision device sample types GAR_F16 / GAR_BF16 -- header and
Python constants agree, the device entry points take them as input and as output type (the stream-
length state machine runs), and they are refused as compute types."""
import ctypes as C
import os
import re

import pytest

HALF = ["F16", "BF16"]


def test_half_constants_match_header(gar):
    """gar.h GAR_F16 / GAR_BF16 equal the Python mirror's codes."""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gar.h")).read()
    m = re.search(r"GAR_F16 = (\d+), GAR_BF16 = (\d+)", hdr)
    assert m and tuple(int(v) for v in m.groups()) == (gar.F16, gar.BF16) == (4, 5)


@pytest.mark.parametrize("name", HALF)
def test_half_device_calls_on_dry_handle(gar, name):
    """A dry stereo 44.1k -> 48k handle: process and flush with the half code as input type, as
    output type and as both return GAR_OK with the exact lengths."""
    t = getattr(gar, name)
    L = gar.lib()
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, DryRun=True))
    got = C.c_int64(0)
    one = C.c_void_p(1)
    for it, ot in ((t, gar.F32), (gar.F32, t), (t, t), (gar.PCM16, t), (t, gar.F64)):
        r.Reset()
        n = L.gar_device_output_size(r._h, 4410)
        assert n > 0
        rc = L.gar_process_device(r._h, one, it, 2, 1, 4410, 2, one, ot, 2, 1, n, C.byref(got), None)
        assert rc == gar.GAR_OK and got.value == n, (it, ot)
        m = L.gar_device_flush_size(r._h)
        assert m > 0
        rc = L.gar_flush_device(r._h, 2, one, ot, 2, 1, m, C.byref(got), None)
        assert rc == gar.GAR_OK and got.value == m, (it, ot)


@pytest.mark.parametrize("name", HALF)
def test_half_is_not_a_compute_type(gar, name):
    """compute_dtype GAR_F16 / GAR_BF16: GAR_ERR_INVALID_CONFIG from gar_config_validate, gar_new
    and gar_new_batch (no handle returned)."""
    L = gar.lib()
    cfg = gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=getattr(gar, name), DryRun=True)
    assert L.gar_config_validate(C.byref(cfg)) == gar.INVALID_CONFIG
    h = C.c_void_p(0)
    assert L.gar_new(C.byref(cfg), C.byref(h)) == gar.INVALID_CONFIG and not h.value
    assert L.gar_new_batch(C.byref(cfg), 2, C.byref(h)) == gar.INVALID_CONFIG and not h.value
    with pytest.raises(gar.ErrInvalidConfig):
        gar.New(cfg)
    ok = gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.F32, DryRun=True)
    assert L.gar_config_validate(C.byref(ok)) == gar.GAR_OK


def test_half_io_type_of_torch_dtypes(gar):
    import torch
    assert gar._io_type(torch.float16) == gar.F16
    assert gar._io_type(torch.bfloat16) == gar.BF16
    assert gar._io_type(torch.float32) == gar.F32 and gar._io_type(torch.int16) == gar.PCM16


def _bf16_once(v):
    """float64 -> bfloat16 bits with ONE rounding, ties to even, in exact arithmetic: |v| scaled by the
    bf16 spacing of its binade (8 significant bits, subnormal spacing 2^-133), rounded by rint."""
    import numpy as np
    fin = np.isfinite(v) & (v != 0)
    _, e = np.frexp(np.where(fin, np.abs(v), 1.0))
    q = np.maximum(e - 8, -133)
    val = np.ldexp(np.rint(np.ldexp(np.abs(v), -q)), q)
    with np.errstate(over="ignore"):
        b = (np.where(fin, val, np.abs(v)).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return np.where(np.signbit(v), b | 0x8000, b).astype(np.uint16)


def _conversion_inputs(np):
    """Random values over every binade both types reach, every tie of f16 / bf16 (the midpoint of two
    neighbours) with its float64 and float32 neighbours on either side -- the values where rounding
    f64 -> f32 -> half to nearest twice differs from one rounding -- and the special values."""
    rng = np.random.default_rng(1)
    x = [rng.standard_normal(400000) * np.exp(rng.uniform(-25, 13, 400000))]
    for lo, hi in ((np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64),
                    np.arange(1, 0x7c01, dtype=np.uint16).view(np.float16).astype(np.float64)),
                   ((np.arange(0x3000, 0x4800, dtype=np.uint32) << 16).view(np.float32).astype(np.float64),
                    (np.arange(0x3001, 0x4801, dtype=np.uint32) << 16).view(np.float32).astype(np.float64))):
        with np.errstate(over="ignore", invalid="ignore"):
            mid = np.where(np.isfinite(hi), (lo + hi) / 2, 65520.0)
        m32 = mid.astype(np.float32)
        x += [mid, np.nextafter(mid, np.inf), np.nextafter(mid, -np.inf), mid * (1 + 2.0 ** -30), mid * (1 - 2.0 ** -30),
              np.nextafter(m32, np.float32(np.inf)).astype(np.float64), np.nextafter(m32, np.float32(-np.inf)).astype(np.float64)]
    x.append(np.array([0.0, np.inf, 65504.0, 65519.99, 65520.0, 65536.0, 1e-8, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -40),
                       2.0 ** -24, 1e300, 1e-300, 5e-324, 3.3895313892515355e38, 3.4e38]))
    x = np.concatenate(x)
    return np.concatenate([x, -x])


def test_half_conversions_on_host(gar):
    """The kernels' conversion functions, run on the host (gar_dev_half_convert): f64 -> f16 equals
    numpy's single rounding and f64 -> bf16 an exact-arithmetic single rounding on ~1.4 M values
    including every tie; float32 -> half equals torch's cast; NaN stays NaN; and every f16 / bf16
    bit pattern survives widening and rounding back (subnormals included)."""
    import numpy as np
    import torch
    x = _conversion_inputs(np)
    with np.errstate(over="ignore"):
        xf = torch.from_numpy(x.astype(np.float32))
    for t, td in ((gar.F16, torch.float16), (gar.BF16, torch.bfloat16)):
        a, b, w = gar.half_convert(x, t)
        with np.errstate(over="ignore"):
            once = x.astype(np.float16).view(np.uint16) if t == gar.F16 else _bf16_once(x)
        assert np.array_equal(a, once), (t, int(np.count_nonzero(a != once)))
        assert np.array_equal(b, xf.to(td).view(torch.int16).numpy().view(np.uint16)), t
        assert np.array_equal(w, torch.from_numpy(a.view(np.int16)).view(td).float().numpy()), t
        # one rounding differs from two nearest roundings on some of these inputs (the test has teeth)
        assert np.count_nonzero(a != b) > 0, t
        nan, _, wn = gar.half_convert(np.array([np.nan, -np.nan]), t)
        assert np.isnan(wn).all() and np.isnan(torch.from_numpy(nan.view(np.int16)).view(td).float().numpy()).all()
        # every non-NaN bit pattern: widen (exact), round back
        pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        val = torch.from_numpy(pat.view(np.int16)).view(td).double().numpy()
        keep = ~np.isnan(val)
        back, back32, wide = gar.half_convert(val[keep], t)
        assert np.array_equal(back, pat[keep]) and np.array_equal(back32, pat[keep]), t
        assert np.array_equal(wide.astype(np.float64), val[keep]), t
