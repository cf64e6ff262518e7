"""The refusals of the process and flush entry points, CPU only (dry-run handles): status code and
exact gar_last_error text of every refusal that needs no GPU, for

    gar_process_multi_f64 / gar_flush_multi_f64, gar_process_device / gar_flush_device,
    gar_process_f64 / gar_flush_f64, gar_process_into_f64 and the f32 twin gar_process_f32.

The expected strings are the ones the library returned before the process and flush halves of each
pair were merged into one function; callers may match on them, so the pairs keep their differing
texts (channel mismatch of the multi-channel calls, lockstep of the device calls).

A refused call changes nothing: against a twin handle that never saw it, the statistics of every
channel and the length the next call returns are the same.

Channel 0 is the only channel the per-channel entry points address, so "channel out of range" is
reached through gar_get_statistics, which the comparison uses anyway.
"""
import ctypes as C

import numpy as np
import pytest

CH = 2
N = 4410
ONE = C.c_void_p(1)       # a non-NULL device pointer: a dry-run handle launches nothing


def handle(gar):
    return gar.New(gar.Config(44100, 48000, CH, gar.QualityHigh, DryRun=True))


def last_error(gar):
    return gar.lib().gar_last_error().decode()


def stats(r):
    return [r.GetStatistics(c) for c in range(CH)]


# -- the eight entry points, raw: (status, n_out as the call left it; the sentinel -1 = untouched) --
def mono(gar, name, r, n, cap, flush=False):
    f32 = name.endswith("f32")
    buf = np.zeros(max(n, cap, 1), dtype=np.float32 if f32 else np.float64)
    got = C.c_int64(-1)
    h = r._h if r is not None else None
    fn = getattr(gar.lib(), name)
    if flush:
        rc = fn(h, buf.ctypes.data, cap, C.byref(got))
    else:
        rc = fn(h, buf.ctypes.data, n, buf.ctypes.data, cap, C.byref(got))
    return rc, got.value


def multi(gar, r, nch, n, cap, flush=False):
    bufs = [np.zeros(max(n, cap, 1)) for _ in range(max(nch, 1))]
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
    counts = np.full(len(bufs), -1, dtype=np.int64)
    h = r._h if r is not None else None
    if flush:
        rc = gar.lib().gar_flush_multi_f64(h, ptrs, nch, cap, counts.ctypes.data)
    else:
        rc = gar.lib().gar_process_multi_f64(h, ptrs, nch, n, ptrs, cap, counts.ctypes.data)
    return rc, list(counts[:max(nch, 0)])


def device(gar, r, n, cap, flush=False, nch=CH, it=1, ot=1, inp=ONE):
    got = C.c_int64(-1)
    h = r._h if r is not None else None
    if flush:
        rc = gar.lib().gar_flush_device(h, nch, ONE, ot, CH, 1, cap, C.byref(got), None)
    else:
        rc = gar.lib().gar_process_device(h, inp, it, CH, 1, n, nch, ONE, ot, CH, 1, cap, C.byref(got), None)
    return rc, got.value


def check(gar, setup, refused, code, text, follow, untouched):
    """`refused(a)` on handle a is refused with (code, text) and leaves n_out as `untouched` says;
    afterwards a agrees with the twin b, which never saw the call, in statistics and in what
    `follow` (the next call) returns."""
    a, b = handle(gar), handle(gar)
    for r in (a, b):
        setup(r)
    rc, nout = refused(a)
    assert rc == code
    if text is not None:
        assert last_error(gar) == text
    assert nout == untouched
    assert stats(a) == stats(b)
    fa, fb = follow(a), follow(b)
    assert fa[0] == gar.GAR_OK and fa == fb
    assert stats(a) == stats(b)


def nothing(r):
    pass


def fed(r):
    r.ProcessMulti([np.zeros(N)] * CH)


def split(r):
    r.Process(np.zeros(100))       # a per-channel call: channel 0 leaves the lockstep group


def test_nil_handle(gar):
    INV = gar.INVALID_ARGUMENT
    for name in ("gar_process_f64", "gar_process_f32", "gar_process_into_f64"):
        assert mono(gar, name, None, 10, 100)[0] == INV and last_error(gar) == "nil resampler"
    assert mono(gar, "gar_flush_f64", None, 0, 100, flush=True)[0] == INV and last_error(gar) == "nil resampler"
    for flush in (False, True):
        assert multi(gar, None, CH, 10, 100, flush)[0] == INV and last_error(gar) == "nil resampler"
        assert device(gar, None, 10, 100, flush) == (INV, -1) and last_error(gar) == "nil resampler"


def test_channel_out_of_range(gar):
    r = handle(gar)
    a, b = C.c_int64(-1), C.c_int64(-1)
    for ch in (-1, CH):
        assert gar.lib().gar_get_statistics(r._h, ch, C.byref(a), C.byref(b)) == gar.INVALID_ARGUMENT
        assert last_error(gar) == "channel out of range"
        assert (a.value, b.value) == (0, 0)
        assert gar.lib().gar_output_size(r._h, ch, 100) == -1 and gar.lib().gar_flush_size(r._h, ch) == -1


@pytest.mark.parametrize("name", ["gar_process_f64", "gar_process_f32", "gar_process_into_f64"])
def test_mono_process(gar, name):
    L = gar.lib()
    fresh = handle(gar)
    est = fresh.EstimateOutput(N)

    def follow(r):
        return mono(gar, name, r, N, est)

    def short(r):
        need = L.gar_output_size(r._h, 0, N)
        assert 0 < need <= est
        return mono(gar, name, r, N, need - 1)

    for setup in (nothing, split):
        check(gar, setup, lambda r: mono(gar, name, r, -1, est), gar.INVALID_ARGUMENT, "negative length", follow, 0)
        check(gar, setup, short, gar.BUFFER_TOO_SMALL, "output buffer too small", follow, 0)
    if "into" in name:   # ProcessInto asks for EstimateOutput's room, whatever the call would return
        check(gar, nothing, lambda r: mono(gar, name, r, N, est - 1), gar.BUFFER_TOO_SMALL, "output buffer too small", follow, 0)
        assert fresh.EstimateOutput(0) == 64
        check(gar, nothing, lambda r: mono(gar, name, r, 0, 63), gar.BUFFER_TOO_SMALL, "output buffer too small", follow, 0)


def test_mono_flush(gar):
    L = gar.lib()

    def follow(r):
        return mono(gar, "gar_flush_f64", r, 0, L.gar_flush_size(r._h, 0), flush=True)

    def short(r):
        m = L.gar_flush_size(r._h, 0)
        assert m > 0
        return mono(gar, "gar_flush_f64", r, 0, m - 1, flush=True)

    for setup in (fed, lambda r: (fed(r), split(r))):
        check(gar, setup, short, gar.BUFFER_TOO_SMALL, "output buffer too small", follow, 0)


def test_multi_process(gar):
    L = gar.lib()

    def follow(r):
        return multi(gar, r, CH, N, N * 2)

    def short(r):
        need = max(L.gar_output_size(r._h, c, N) for c in range(CH))
        assert need > 0
        return multi(gar, r, CH, N, need - 1)

    for setup in (nothing, split):
        for nch in (CH - 1, CH + 1):
            check(gar, setup, lambda r: multi(gar, r, nch, N, N * 2), gar.CHANNEL_MISMATCH,
                  f"expected {CH} channels, got {nch}", follow, [-1] * nch)
        check(gar, setup, lambda r: multi(gar, r, CH, -1, N * 2), gar.INVALID_ARGUMENT, "negative length", follow, [-1] * CH)
        check(gar, setup, short, gar.BUFFER_TOO_SMALL, "output buffer too small", follow, [-1] * CH)


def test_multi_flush(gar):
    L = gar.lib()

    def follow(r):
        return multi(gar, r, CH, 0, 4096, flush=True)

    def short(r):
        need = max(L.gar_flush_size(r._h, c) for c in range(CH))
        assert need > 0
        return multi(gar, r, CH, 0, need - 1, flush=True)

    for setup in (fed, lambda r: (fed(r), split(r))):
        for nch in (CH - 1, CH + 1):
            check(gar, setup, lambda r: multi(gar, r, nch, 0, 4096, flush=True), gar.CHANNEL_MISMATCH,
                  "channel count mismatch", follow, [-1] * nch)
        check(gar, setup, short, gar.BUFFER_TOO_SMALL, "output buffer too small", follow, [-1] * CH)


BAD_TYPES = (3, 8, 17, 64, -1, 279, 281)


def test_device_process(gar):
    L = gar.lib()
    INV = gar.INVALID_ARGUMENT

    def follow(r):
        return device(gar, r, N, N * 2)

    for nch in (CH - 1, CH + 1):
        check(gar, nothing, lambda r: device(gar, r, N, N * 2, nch=nch), gar.CHANNEL_MISMATCH,
              f"expected {CH} channels, got {nch}", follow, 0)
    check(gar, nothing, lambda r: device(gar, r, -1, N * 2), INV, "negative length", follow, 0)
    check(gar, nothing, lambda r: device(gar, r, 1, N * 2, inp=None), INV, "input is NULL", follow, 0)
    assert device(gar, handle(gar), 0, N * 2, inp=None) == (gar.GAR_OK, 0)   # no frames: no input is read
    for bad in BAD_TYPES:
        check(gar, nothing, lambda r: device(gar, r, N, N * 2, it=bad), INV, "unknown sample type", follow, 0)
        check(gar, nothing, lambda r: device(gar, r, N, N * 2, ot=bad), INV, "unknown sample type", follow, 0)
    # the order of the argument checks: channels, length, input, sample types, lockstep
    r = handle(gar)
    split(r)
    assert device(gar, r, -1, N * 2, nch=CH + 1, it=3)[0] == gar.CHANNEL_MISMATCH
    assert device(gar, r, -1, N * 2, it=3, inp=None) == (INV, 0) and last_error(gar) == "negative length"
    assert device(gar, r, 1, N * 2, it=3, inp=None) == (INV, 0) and last_error(gar) == "input is NULL"
    assert device(gar, r, 1, N * 2, it=3) == (INV, 0) and last_error(gar) == "unknown sample type"

    def follow_split(r):
        return mono(gar, "gar_process_f64", r, N, N * 2)

    check(gar, split, lambda r: device(gar, r, N, N * 2), gar.NOT_SUPPORTED,
          "channels are not in lockstep (per-channel calls were made)", follow_split, 0)

    # capacity one short: the status alone (this refusal writes no text: the previous one stays)
    def short(r):
        need = L.gar_device_output_size(r._h, N)
        assert need > 0
        assert device(gar, r, -1, need)[0] == INV
        return device(gar, r, N, need - 1)

    check(gar, nothing, short, gar.BUFFER_TOO_SMALL, "negative length", follow, 0)
    for t in (gar.PCM16, gar.F16, gar.PCM24_PACKED, gar.F64):   # a converted output is sized the same way
        check(gar, nothing, lambda r: device(gar, r, N, L.gar_device_output_size(r._h, N) - 1, ot=t),
              gar.BUFFER_TOO_SMALL, None, follow, 0)


def test_device_flush(gar):
    L = gar.lib()
    INV = gar.INVALID_ARGUMENT

    def follow(r):
        return device(gar, r, 0, 4096, flush=True)

    for nch in (CH - 1, CH + 1):
        check(gar, fed, lambda r: device(gar, r, 0, 4096, flush=True, nch=nch), gar.CHANNEL_MISMATCH,
              f"expected {CH} channels, got {nch}", follow, 0)
    for bad in BAD_TYPES:
        check(gar, fed, lambda r: device(gar, r, 0, 4096, flush=True, ot=bad), INV, "unknown sample type", follow, 0)
    r = handle(gar)
    split(r)
    assert device(gar, r, 0, 4096, flush=True, nch=CH + 1, ot=3)[0] == gar.CHANNEL_MISMATCH
    assert device(gar, r, 0, 4096, flush=True, ot=3) == (INV, 0) and last_error(gar) == "unknown sample type"

    def follow_split(r):
        return mono(gar, "gar_flush_f64", r, 0, 4096, flush=True)

    check(gar, lambda r: (fed(r), split(r)), lambda r: device(gar, r, 0, 4096, flush=True), gar.NOT_SUPPORTED,
          "channels are not in lockstep", follow_split, 0)

    def short(r):
        need = L.gar_device_flush_size(r._h)
        assert need > 0
        assert device(gar, r, 0, need, flush=True, ot=3)[0] == INV
        return device(gar, r, 0, need - 1, flush=True)

    check(gar, fed, short, gar.BUFFER_TOO_SMALL, "unknown sample type", follow, 0)
    for t in (gar.PCM16, gar.F16, gar.PCM24_PACKED, gar.F64):
        check(gar, fed, lambda r: device(gar, r, 0, L.gar_device_flush_size(r._h) - 1, flush=True, ot=t),
              gar.BUFFER_TOO_SMALL, None, follow, 0)
