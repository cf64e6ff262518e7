"""State snapshots (gar.h gar_state_size / gar_state_save / gar_state_load), CPU only: dry-run
handles carry the whole host state machine, and their blobs hold counters and no rows.

  * sizes and the too-small answer; one state has one blob (save twice, save -> load -> save);
  * length continuation: a restored fresh handle returns the same output length and statistics as the
    original for every later call, for every engine kind, from snapshots taken before any input,
    inside the priming phase, mid-stream and after a Flush (Process after Flush);
  * refusals (GAR_ERR_INVALID_ARGUMENT, nothing changed): a blob of another design, truncation,
    flipped bytes, a wrong length, a real handle's flag on a dry-run handle, and fields changed
    together (checksum fixed up) into a state the design cannot reach;
  * a split handle comes back split.

The host Process of the ABI (gar_process_f64, Go's Process) advances channel 0; that is the
per-channel call that splits a multi-channel handle here.
"""
import ctypes as C
import struct

import numpy as np
import pytest

# (name, constructor kind, in rate, out rate, preset)
CASES = [
    ("44k1_48k_high", "new", 44100, 48000, 3),
    ("48k_44k1_veryhigh", "new", 48000, 44100, 4),
    ("16k_44k1_high", "new", 16000, 44100, 3),          # polyphase step with a fraction: stage-by-stage
    ("96k_44k1_veryhigh", "new", 96000, 44100, 4),      # decimator + second stage
    ("96k_16k_high", "new", 96000, 16000, 3),           # multi-stage
    ("24k_48k_high", "new", 24000, 48000, 3),           # DFT only
    ("44k1_48k_quick", "new", 44100, 48000, 0),         # cubic
    ("48k_48k", "new", 48000, 48000, 3),                # pass-through
    ("engine_16k_44k1_high", "engine", 16000, 44100, 3),
    ("engine_48k_200_high", "engine", 48000, 200, 3),   # extreme down: the polyphase no-trim quirk
    ("engine_48k_44k1_quick", "engine", 48000, 44100, 0),   # cubic, sequential phase walk
]
IDS = [c[0] for c in CASES]

HDR = 104          # DESIGN.md "State snapshots": header bytes
FLAGS_AT = 12      # u32 flags, bit 0 = dry-run
COUNTER_AT = HDR + 24 + 8   # x_count of group 0, stage 0


def make(gar, case, channels=1, **kw):
    _, kind, i, o, preset = case
    if kind == "engine":
        return gar.NewEngineDry(i, o, preset)
    return gar.New(gar.Config(i, o, channels, preset, DryRun=True, **kw))


def checksum(b):
    """The blob's checksum: h = mix((h ^ w) * K) over the little-endian 64-bit words."""
    h, mask = 0x6A09E667F3BCC908, (1 << 64) - 1
    for (w,) in struct.iter_unpack("<Q", b):
        h = ((h ^ w) * 0x9E3779B97F4A7C15) & mask
        h ^= h >> 32
    return h


def with_checksum(b):
    return bytes(b[:-8]) + struct.pack("<Q", checksum(bytes(b[:-8])))


def probe(r):
    ch = r.Channels
    return ([r.OutputSize(1000, c) for c in range(ch)], [r.FlushSize(c) for c in range(ch)],
            [r.GetStatistics(c) for c in range(ch)], r.state_size())


def step(r, op):
    """One call; returns what the continuation test compares."""
    if op == "f":
        want = r.FlushSize()
        got = len(r.Flush())
    else:
        want = r.OutputSize(op)
        got = len(r.Process(np.zeros(op)))
    assert got == want
    return got, r.GetStatistics(), [r.stage_state(s) for s in range(r.num_stages())]


def test_blob_checksum_is_the_documented_one(gar):
    blob = make(gar, CASES[0]).save_state()
    assert blob[:8] == b"GARSTATE" and struct.unpack_from("<I", blob, 8)[0] == 1
    assert struct.unpack_from("<q", blob, 16)[0] == len(blob)
    assert struct.unpack_from("<I", blob, FLAGS_AT)[0] == 1     # dry-run
    assert with_checksum(blob) == blob


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_size_and_too_small(gar, case):
    r = make(gar, case)
    r.Process(np.zeros(3000))
    n = r.state_size()
    blob = r.save_state()
    assert n == len(blob) and n > HDR
    before = probe(r)
    with pytest.raises(gar.ErrBufferTooSmall) as e:
        r.save_state(cap=n - 1)
    assert e.value.needed == n
    with pytest.raises(gar.ErrBufferTooSmall) as e:
        r.save_state(cap=0)
    assert e.value.needed == n
    assert probe(r) == before and r.save_state() == blob
    assert gar.lib().gar_state_size(None) == -1


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_state_one_blob(gar, case):
    r = make(gar, case)
    for op in [0, 1234, 4099, "f", 77]:
        if op:
            step(r, op)
        a = r.save_state()
        assert r.save_state() == a
        f = make(gar, case)
        f.load_state(a)
        assert f.save_state() == a
        assert probe(f) == probe(r)
    # a used handle takes a blob as well as a fresh one, and Reset gives the never-used state
    f.Process(np.zeros(999))
    f.load_state(a)
    assert f.save_state() == a
    f.Reset()
    assert f.save_state() == make(gar, case).save_state()


def first_taps(r):
    g = r.stage_geometry(0)[1] if r.num_stages() else None
    return max([g.dft_taps, g.decim_taps, g.poly_taps]) if g else 0


@pytest.mark.parametrize("where", ["fresh", "priming", "mid", "after_flush"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_length_continuation(gar, case, where):
    rng = np.random.default_rng(sum(map(ord, case[0] + where)))
    a = make(gar, case)
    if where == "fresh":
        head = []
    elif where == "priming":
        t = first_taps(a)
        head = [max(1, min(10, t - 1))]      # fewer frames than the first stage's taps
        assert t == 0 or head[0] < t
    elif where == "mid":
        head = [int(n) for n in rng.integers(1, 5000, size=int(rng.integers(1, 6)))]
    else:
        head = [int(rng.integers(1, 5000)), "f"]
    tail = [int(n) for n in rng.integers(0, 5000, size=6)] + ["f", int(rng.integers(1, 3000)), "f", "f"]
    for op in head:
        step(a, op)
    blob = a.save_state()
    b = make(gar, case)
    b.load_state(blob)
    assert b.GetStatistics() == a.GetStatistics()
    for op in tail:
        assert step(a, op) == step(b, op), op
    assert a.save_state() == b.save_state()


def refused(gar, r, blob, n=None):
    """load of `blob` (n bytes of it, default all) answers INVALID_ARGUMENT with a detail and changes nothing."""
    before, mine = probe(r), r.save_state()
    rc = gar.lib().gar_state_load(r._h, blob, len(blob) if n is None else n)
    assert rc == gar.INVALID_ARGUMENT, rc
    assert gar.lib().gar_last_error().startswith(b"state blob refused")
    assert probe(r) == before and r.save_state() == mine


def test_refuses_other_designs(gar):
    base = dict(InputRate=44100, OutputRate=48000, Channels=2, Quality=3, ComputeDtype=gar.F64, DryRun=True)
    r = gar.New(gar.Config(**base))
    r.ProcessMulti([np.zeros(700)] * 2)
    others = [dict(base, InputRate=48000), dict(base, OutputRate=44100), dict(base, Channels=3), dict(base, Quality=4),
              dict(base, Quality=2), dict(base, ComputeDtype=gar.F32), dict(base, ComputeDtype=gar.F32_EXACT)]
    for kw in others:
        o = gar.New(gar.Config(**kw))
        o.ProcessMulti([np.zeros(700)] * kw["Channels"])
        refused(gar, r, o.save_state())
        refused(gar, o, r.save_state())
    f32, exact = (gar.New(gar.Config(**dict(base, ComputeDtype=d))) for d in (gar.F32, gar.F32_EXACT))
    refused(gar, f32, exact.save_state())
    # New path vs engine path of the same rates, one channel
    n1 = gar.New(gar.Config(44100, 48000, 1, 3, DryRun=True))
    e1 = gar.NewEngineDry(44100, 48000, 3)
    refused(gar, n1, e1.save_state())
    refused(gar, e1, n1.save_state())
    # a batch of 2 x 1 channels against one stream of 2 channels
    refused(gar, r, gar.NewBatch(gar.Config(**dict(base, Channels=1)), 2).save_state())
    with pytest.raises(gar.ResamplerError) as e:
        r.load_state(e1.save_state())
    assert e.value.code == gar.INVALID_ARGUMENT and "fingerprint" in str(e.value)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[6]], ids=[IDS[0], IDS[3], IDS[6]])
def test_refuses_damaged_blobs(gar, case):
    src = make(gar, case)
    src.Process(np.zeros(2000))
    blob = src.save_state()
    r = make(gar, case)
    r.Process(np.zeros(555))
    for n in [0, 1, 8, HDR - 1, HDR, HDR + 8, len(blob) // 2, len(blob) - 8, len(blob) - 1]:
        refused(gar, r, blob[:n])                         # truncated
    for at in [0, 9, FLAGS_AT, 17, 30, HDR - 8, COUNTER_AT, COUNTER_AT + 7, len(blob) - 8, len(blob) - 1]:
        bad = bytearray(blob)
        bad[at] ^= 0x01                                   # header, counter, checksum
        refused(gar, r, bytes(bad))
    refused(gar, r, blob, len(blob) - 8)                  # wrong n against a whole blob
    refused(gar, r, blob + bytes(8))
    refused(gar, r, blob, -1)
    # past the checksum: the same flips with the checksum fixed up reach the record validation
    for at, bit in [(COUNTER_AT, 0x01), (COUNTER_AT + 7, 0x80), (HDR + 4, 0x02), (HDR, 0x01), (8, 0x02)]:
        bad = bytearray(blob)
        bad[at] ^= bit
        refused(gar, r, with_checksum(bad))
    # dry <-> real: a real handle's blob carries flag 0
    real = bytearray(blob)
    struct.pack_into("<I", real, FLAGS_AT, 0)
    refused(gar, r, with_checksum(real))
    assert b"dry-run" in gar.lib().gar_last_error()
    r.load_state(blob)                                     # and the undamaged blob still loads
    assert r.save_state() == blob


# offsets inside a stage record: counters, then xh and uh (base, len, zero, pad, offset)
POLY_HIST, U_BASE, U_COUNT, Y_COUNT, UH_BASE, UH_LEN = 24, 40, 48, 64, 112, 120


def bump(blob, at, delta):
    struct.pack_into("<q", blob, at, struct.unpack_from("<q", blob, at)[0] + delta)


@pytest.mark.parametrize("flushed", [True, False], ids=["zero_history", "live_counters"])
def test_refuses_consistent_but_unreachable_histories(gar, flushed):
    """Several fields changed together, checksum fixed up: a polyphase history longer than the design
    keeps passes every cross-check of its own fields (poly_hist = u_count - u_base = uh.len, the excess a
    multiple of poly.taps) and is still refused -- a zero history or a dry-run blob stores no rows, so
    only the design bounds its length.  Likewise a shifted u_base / y_count."""
    cfg = dict(InputRate=44100, OutputRate=48000, Channels=2, Quality=3, DryRun=True)
    src = gar.New(gar.Config(**cfg))
    src.ProcessMulti([np.zeros(1000)] * 2)
    if flushed:
        src.FlushMulti()
    assert src.stage_state(0)[1] != flushed
    blob = src.save_state()
    taps = src.stage_geometry(0)[1].poly_taps
    rec = HDR + 24
    r = gar.New(gar.Config(**cfg))
    r.ProcessMulti([np.zeros(321)] * 2)
    for k in ([1, 7, 1 << 20, 1 << 43] if flushed else []):
        bad = bytearray(blob)
        for f in (POLY_HIST, U_COUNT, UH_LEN):
            bump(bad, rec + f, k * taps)
        refused(gar, r, with_checksum(bad))
        assert b"polyphase history" in gar.lib().gar_last_error()
    for k in (1, 1 << 30):                      # u_base moved back: a longer history, same u_count
        bad = bytearray(blob)
        bump(bad, rec + POLY_HIST, k)
        bump(bad, rec + U_BASE, -k)
        if flushed:
            bump(bad, rec + UH_BASE, -k)
            bump(bad, rec + UH_LEN, k)
        refused(gar, r, with_checksum(bad))
    bad = bytearray(blob)
    bump(bad, rec + Y_COUNT, 1)                 # an output count the position does not give
    refused(gar, r, with_checksum(bad))
    r.load_state(blob)
    assert r.save_state() == blob


def test_split_handle_comes_back_split(gar):
    cfg = dict(InputRate=44100, OutputRate=48000, Channels=3, Quality=3, DryRun=True)
    a = gar.New(gar.Config(**cfg))
    a.ProcessMulti([np.zeros(1500)] * 3)
    a.Process(np.zeros(640))                               # channel 0 alone: the handle splits
    blob = a.save_state()
    b = gar.New(gar.Config(**cfg))
    assert gar.lib().gar_device_output_size(b._h, 100) >= 0
    b.load_state(blob)
    assert probe(b) == probe(a)
    assert a.GetStatistics(0) != a.GetStatistics(1) and b.GetStatistics(0) == a.GetStatistics(0)
    assert gar.lib().gar_device_output_size(a._h, 100) == -1
    assert gar.lib().gar_device_output_size(b._h, 100) == -1
    for op in [333, 4000]:
        assert [len(y) for y in a.ProcessMulti([np.zeros(op)] * 3)] == [len(y) for y in b.ProcessMulti([np.zeros(op)] * 3)]
    assert [len(y) for y in a.FlushMulti()] == [len(y) for y in b.FlushMulti()]
    assert a.save_state() == b.save_state()
    # a blob whose channel ranges leave a gap or overlap is refused
    c0_of_group1 = HDR + 24 + a.num_stages() * 144
    for delta in (1, -1):
        bad = bytearray(blob)
        struct.pack_into("<i", bad, c0_of_group1, struct.unpack_from("<i", blob, c0_of_group1)[0] + delta)
        refused(gar, b, with_checksum(bad))
