"""CPU (dry-run handles): packed 24-bit PCM, GAR_PCM24_PACKED -- 3 bytes per sample, little-endian,
the layout of 24-bit WAV data (cmd/resample-wav/main.go:648-665).  Header and Python constants agree,
the device entry points take the type as input and as output type (the stream-length state machine
runs), it is refused as a compute type, and the kernels' conversion functions, run on the host, give
GAR_PCM24's values: int(clamp(y, -1, 1) * 8388607) truncating, NaN -> 0, low three bytes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

MAX24 = 8388607.0


def test_packed_constants_match_header(gar):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gar.h")).read()
    m = re.search(r"GAR_PCM24_PACKED = 0x100 \| 24", hdr)
    assert m and gar.PCM24_PACKED == (0x100 | 24) == 280


@pytest.mark.parametrize("it,ot", [("PCM24_PACKED", "F32"), ("F32", "PCM24_PACKED"), ("PCM24_PACKED", "PCM24_PACKED"),
                                   ("PCM16", "PCM24_PACKED"), ("PCM24_PACKED", "PCM16"), ("F16", "PCM24_PACKED"),
                                   ("PCM24_PACKED", "F16"), ("PCM24_PACKED", "F64"), ("F64", "PCM24_PACKED")])
def test_packed_device_calls_on_dry_handle(gar, it, ot):
    """A dry stereo 44.1k -> 48k handle: process and flush with the packed code as input type, as
    output type, as both and mixed with PCM16 / F16 / F64 return GAR_OK with the exact lengths."""
    it, ot = getattr(gar, it), getattr(gar, ot)
    L = gar.lib()
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, DryRun=True))
    got = C.c_int64(0)
    one = C.c_void_p(1)
    n = L.gar_device_output_size(r._h, 4410)
    assert n > 0
    rc = L.gar_process_device(r._h, one, it, 2, 1, 4410, 2, one, ot, 2, 1, n, C.byref(got), None)
    assert rc == gar.GAR_OK and got.value == n, (it, ot, L.gar_last_error())
    m = L.gar_device_flush_size(r._h)
    assert m > 0
    rc = L.gar_flush_device(r._h, 2, one, ot, 2, 1, m, C.byref(got), None)
    assert rc == gar.GAR_OK and got.value == m, (it, ot)


def test_packed_is_not_a_compute_type(gar):
    """compute_dtype GAR_PCM24_PACKED: GAR_ERR_INVALID_CONFIG from gar_config_validate, gar_new and
    gar_new_batch (no handle returned)."""
    L = gar.lib()
    cfg = gar.Config(44100, 48000, 2, gar.QualityHigh, ComputeDtype=gar.PCM24_PACKED, DryRun=True)
    assert L.gar_config_validate(C.byref(cfg)) == gar.INVALID_CONFIG
    h = C.c_void_p(0)
    assert L.gar_new(C.byref(cfg), C.byref(h)) == gar.INVALID_CONFIG and not h.value
    assert L.gar_new_batch(C.byref(cfg), 2, C.byref(h)) == gar.INVALID_CONFIG and not h.value
    with pytest.raises(gar.ErrInvalidConfig):
        gar.New(cfg)


def _boundary_values():
    u = 2.0 ** -23
    return np.array([1.0, -1.0, 1.0 - u, -(1.0 - u), 1.0 + 1e-9, -(1.0 + 1e-9), 1.5, -1.5, 1e300, -1e300, np.inf, -np.inf,
                     0.0, -0.0, 1e-12, -1e-12, 5e-324, -5e-324, 1.0 / MAX24, -1.0 / MAX24, 0.999999 / MAX24,
                     -0.999999 / MAX24, 0.5, -0.5, 8388606.5 / MAX24, -8388606.5 / MAX24])


def _want_int(v):
    """int(clamp(v, -1, 1) * 8388607), truncating; NaN -> 0."""
    with np.errstate(invalid="ignore"):
        s = np.clip(v, -1.0, 1.0) * MAX24
    return np.where(np.isnan(s), 0.0, np.trunc(s)).astype(np.int64)


def test_packed_conversions_on_host(gar):
    """gar_dev_pcm24_convert: the bytes are the low three, little-endian, of numpy's
    int(clip(v, -1, 1) * 8388607) on the boundary values, NaN and 10^4 random values; the bytes read
    back sign-extend to that integer (so -8388607 .. 8388607 all survive)."""
    rng = np.random.default_rng(24)
    x = np.concatenate([_boundary_values(), np.array([np.nan, -np.nan]), rng.uniform(-1.2, 1.2, 10000)])
    b, i = gar.pcm24_convert(x)
    want = _want_int(x)
    assert b.shape == (x.size, 3) and b.dtype == np.uint8
    u = want.astype(np.int64) & 0xFFFFFF
    wb = np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], axis=1).astype(np.uint8)
    assert np.array_equal(b, wb), int(np.count_nonzero(b != wb))
    assert np.array_equal(i.astype(np.int64), want)
    assert want.max() == 8388607 and want.min() == -8388607 and (want[26:28] == 0).all()
    # either output may be NULL
    L = gar.lib()
    xs = np.ascontiguousarray(x[:4])
    only = np.zeros(4, dtype=np.int32)
    assert L.gar_dev_pcm24_convert(xs.ctypes.data_as(C.c_void_p), 4, None, only.ctypes.data_as(C.c_void_p)) == gar.GAR_OK
    assert np.array_equal(only, want[:4])


def test_pack_unpack_helpers_round_trip(gar):
    """gar.pack_pcm24 / gar.unpack_pcm24: every boundary integer, 0x800000 and 0x7FFFFF included, keeps
    its value; the bytes are little-endian; shapes gain / lose the last dimension of 3."""
    v = np.array([0, 1, -1, 255, 256, -256, 65535, 65536, -65536, 0x7FFFFF, -0x800000, 0x7FFFFE, -0x7FFFFF, 0x123456,
                  -0x123456], dtype=np.int32)
    b = gar.pack_pcm24(v)
    assert b.shape == (v.size, 3) and b.dtype == np.uint8
    assert bytes(b[13]) == b"\x56\x34\x12" and bytes(b[9]) == b"\xff\xff\x7f" and bytes(b[10]) == b"\x00\x00\x80"
    back = gar.unpack_pcm24(b)
    assert back.dtype == np.int32 and np.array_equal(back, v)
    rng = np.random.default_rng(3)
    m = rng.integers(-0x800000, 0x800000, size=(37, 5), dtype=np.int32)
    pm = gar.pack_pcm24(m)
    assert pm.shape == (37, 5, 3) and np.array_equal(gar.unpack_pcm24(pm), m)
    import torch
    assert np.array_equal(gar.unpack_pcm24(torch.from_numpy(pm)), m)
    assert np.array_equal(gar.pack_pcm24(torch.from_numpy(m)), pm)
    # the device conversion's read-back equals the helper's
    _, i = gar.pcm24_convert(m.reshape(-1) / MAX24)
    bb, _ = gar.pcm24_convert(m.reshape(-1) / MAX24)
    assert np.array_equal(gar.unpack_pcm24(bb), i)


def test_packed_io_type_and_tensor_form(gar):
    """_io_type answers for uint8; process_device / flush_device refuse a uint8 tensor that is not
    [frames, channels, 3] with adjacent bytes and whole-sample strides."""
    import torch
    assert gar._io_type(torch.uint8) == gar.PCM24_PACKED
    assert gar._io_type(torch.int32, 24) == gar.PCM24 and gar._io_type(torch.float32) == gar.F32
    r = gar.New(gar.Config(44100, 48000, 2, gar.QualityHigh, DryRun=True))
    with pytest.raises(ValueError):
        r.process_device(torch.zeros((16, 2, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        r.process_device(torch.zeros((16, 2), dtype=torch.uint8))
    with pytest.raises(ValueError):
        r.process_device(torch.zeros((16, 2, 6), dtype=torch.uint8)[:, :, ::2])  # last stride 2
    with pytest.raises(ValueError):
        r.process_device(torch.zeros((16 * 8,), dtype=torch.uint8).as_strided((16, 2, 3), (8, 3, 1)))  # frame stride 8 B
    with pytest.raises(ValueError):
        r.flush_device(out=torch.zeros((16, 2, 2), dtype=torch.uint8))
