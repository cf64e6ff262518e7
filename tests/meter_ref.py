"""The clip counter / peak meter of gar.h gar_set_meter, restated in numpy from the header's definition
(nothing of the library runs here): the expected values of test_meter_abi.py and test_gpu_meter.py.

  y: the sample in the compute type, widened exactly to float64
  clipped: y > 1.0 or y < -1.0 (+-Inf count, NaN does not); with TPDF dither on also when
           q = floor(clamp(y, -1, 1) * maxVal + (0.5 + d(c, n))), before its clamp, lies outside +-maxVal
  peak:    max |y|, NaN ignored, starts at 0, +Inf legal
"""
import numpy as np

import dither_ref as D


def first_clamp(y):
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (y > 1.0) | (y < -1.0)


def second_clamp(y, bits, seed, c, n0):
    """Samples whose dithered floor(s + t) leaves [-maxVal, maxVal] (float64 samples of channel c from position n0)."""
    y = np.asarray(y, dtype=np.float64)
    mv = D.MAXV[bits]
    pos = np.uint64(n0) + np.arange(y.size, dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        q = np.floor(np.clip(y, -1.0, 1.0) * mv + (0.5 + D.noise(seed, c, pos)))
        return (q > mv) | (q < -mv)


def tally(y, bits, dither, seed=0, c=0, n0=0):
    """(clips, peak) of the float64 samples y of channel c stored from stream position n0."""
    y = np.asarray(y, dtype=np.float64)
    clip = first_clamp(y)
    if dither:
        clip = clip | second_clamp(y, bits, seed, c, n0)
    a = np.abs(y[~np.isnan(y)])
    return int(np.count_nonzero(clip)), float(a.max()) if a.size else 0.0


def tally_frames(y, bits, dither, seed=0, n0=0, c0=0):
    """y[frames, channels] -> (clips uint64 [channels], peak float64 [channels]); channel j is channel c0 + j."""
    y = np.asarray(y)
    t = [tally(y[:, j].astype(np.float64), bits, dither, seed, c0 + j, n0) for j in range(y.shape[1])]
    return np.array([c for c, _ in t], dtype=np.uint64), np.array([p for _, p in t], dtype=np.float64)
