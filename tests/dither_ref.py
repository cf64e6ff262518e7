"""The dithered PCM quantizer of gar.h gar_set_dither, restated in numpy from the header's definition
(nothing of the library runs here): the expected values of test_dither_abi.py and test_gpu_dither.py.

  h32(x):   x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (uint32)
  key(c)  = h32(lo32(seed) ^ h32(hi32(seed) ^ h32(c + 1)))
  r(c, n) = h32(h32(key(c) + hi32(n)) ^ lo32(n))
  d(c, n) = ((r & 0xffff) - (r >> 16)) / 65536
  q       = clamp(floor(clamp(y, -1, 1) * maxVal + (0.5 + d)), -maxVal, maxVal);  NaN -> 0
"""
import numpy as np

MAXV = {16: 32767.0, 24: 8388607.0, 32: 2147483647.0, 280: 8388607.0}
U32 = np.uint32


def h32(x):
    x = np.array(x, dtype=np.uint32, ndmin=1, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> U32(16)
        x *= U32(0x7FEB352D)
        x ^= x >> U32(15)
        x *= U32(0x846CA68B)
        x ^= x >> U32(16)
    return x


def key(seed, c):
    lo, hi = U32(seed & 0xFFFFFFFF), U32((seed >> 32) & 0xFFFFFFFF)
    return h32(lo ^ h32(hi ^ h32(U32(c + 1))))


def noise(seed, c, n):
    """d(c, n) for an array of uint64 positions n."""
    n = np.asarray(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        kh = h32(key(seed, c) + (n >> np.uint64(32)).astype(np.uint32))
    r = h32(kh ^ (n & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    return ((r & U32(0xFFFF)).astype(np.int64) - (r >> U32(16)).astype(np.int64)) / 65536.0


def quantize(y, bits, seed, c, n0):
    """The integers stored for the float64 samples y of channel c at positions n0, n0 + 1, ... (int64)."""
    y = np.asarray(y, dtype=np.float64)
    mv = MAXV[bits]
    pos = np.uint64(n0) + np.arange(y.size, dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        s = np.clip(y, -1.0, 1.0) * mv
        q = np.clip(np.floor(s + (0.5 + noise(seed, c, pos))), -mv, mv)
    return np.where(np.isnan(q), 0.0, q).astype(np.int64)


def quantize_frames(y, bits, seed, n0=0, c0=0):
    """y[frames, channels] (float) -> int64, channel j quantized as channel c0 + j from position n0."""
    y = np.asarray(y)
    return np.stack([quantize(y[:, j].astype(np.float64), bits, seed, c0 + j, n0) for j in range(y.shape[1])], axis=1)
