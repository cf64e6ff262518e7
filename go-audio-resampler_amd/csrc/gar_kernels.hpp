// gar_kernels.hpp -- device-side descriptors and launchers (gar_kernels.hip).
#pragma once
#include <string>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "gar_cubic_seg.hpp"

namespace gar {

// A channel group's input stream seen by a kernel: the retained history
// (compute dtype, interleaved [t][C] with row stride hist_ld) virtually
// concatenated with the caller's new input (any strides, f32 or f64), and
// zero beyond valid_end -- the zero padding that DFTStage/PolyphaseStage/
// DFTDecimationStage.Flush append (dft_stage.go:347, :582,
// polyphase_stage.go:342) never has to be materialised.
struct SrcDesc {
    const void* hist;
    int64_t hist_base, hist_len, hist_ld;
    const void* in;
    int64_t in_base, in_len, in_fs, in_cs;
    int in_f64;
    int in_pcm;            // 0 float input, else PCM bits (16: int16, 24/32: int32 storage), 280: packed 24-bit
                           // (3 bytes per sample; in_fs / in_cs count samples) or 4 / 5: f16 / bf16
    int64_t valid_end;
};

// Output view: element (o, c) -> out[(o - o0) * fs + c * cs]; only o in [o_lo, o_hi) written.
struct OutDesc {
    void* out;
    int64_t o0, fs, cs;
    int f64;
    int pcm;               // 0 float output, else PCM bits (int(clamp(y, -1, 1) * maxVal)), 280: packed 24-bit
                           // (3 bytes per sample; fs / cs count samples) or 4 / 5: f16 / bf16 (RNE)
    int64_t o_lo, o_hi;
    int* err;              // the calling handle's device status word (host-mapped), null if none
    // TPDF dither of an integer PCM store (gar.h gar_set_dither; ditherNoise below): mode 0 truncates as ever.
    // dpos0 = position in the handle's output stream of output o0 (the view's base), so output o has o - o0 + dpos0
    // whichever launch of a call writes it; channel c of the view is channel c of the handle.
    int dither;
    uint32_t dseedLo, dseedHi;
    int64_t dpos0;
};

// Integer PCM <-> float, after cmd/resample-wav/main.go:444-543 (maxInt16/24/32, main.go:54-56):
// in = float64(i) * (1 / maxVal); out = int(clamp(float64(y), -1, 1) * maxVal), truncating.
// Packed 24-bit PCM (gar.h GAR_PCM24_PACKED = 0x100 | 24) travels in the same fields under its ABI
// code: GAR_PCM24's values in 3 bytes per sample, little-endian two's complement, at any byte address.
constexpr int kSampPcm24P = 280;
__host__ __device__ inline double pcmMax(int bits) {
    return bits == 16 ? 32767.0 : ((bits == 24 || bits == kSampPcm24P) ? 8388607.0 : 2147483647.0);
}
// Half-precision samples (gar.h GAR_F16 / GAR_BF16) travel in the same fields as the PCM bits
// (SrcDesc::in_pcm, OutDesc::pcm, launchConvert's type codes) under their ABI codes 4 and 5, below
// every PCM width.  In: exact widening (f16 subnormals are values).  Out: ONE round-to-nearest-even
// from the compute type -- overflow gives +-Inf (no clamp), NaN stays NaN, subnormals are produced.
// From f64 that is f64 -> f32 rounded to odd, then f32 -> half to nearest-even: the odd last bit
// keeps the inexactness the second rounding must see, so the pair equals a single f64 -> half RNE.
constexpr int kSampF16 = 4, kSampBF16 = 5;
__host__ __device__ inline bool sampIsHalf(int t) { return t == kSampF16 || t == kSampBF16; }
__host__ __device__ inline float halfToF32(uint16_t b, int code) {
    if (code == kSampBF16) return __builtin_bit_cast(float, static_cast<uint32_t>(b) << 16);
    return static_cast<float>(__builtin_bit_cast(_Float16, b));
}
__host__ __device__ inline uint16_t halfOfF32(float v, int code) {
    if (code == kSampBF16) {
        uint32_t u = __builtin_bit_cast(uint32_t, v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40u);  // NaN stays NaN
        u += 0x7fffu + ((u >> 16) & 1u);  // nearest even; a carry out of the mantissa reaches Inf
        return static_cast<uint16_t>(u >> 16);
    }
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
}
__host__ __device__ inline float f32OddOfF64(double d) {
    const float f = static_cast<float>(d);
    if (d != d || static_cast<double>(f) == d) return f;
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if (u & 1u) return f;  // the nearest float is the odd neighbour already
    const double af = f < 0 ? -static_cast<double>(f) : static_cast<double>(f), ad = d < 0 ? -d : d;
    u += af > ad ? ~0u : 1u;  // the other neighbour (sign-magnitude: +-1 on the bits); Inf -> largest finite
    return __builtin_bit_cast(float, u);
}
__host__ __device__ inline uint16_t halfOfF64(double d, int code) { return halfOfF32(f32OddOfF64(d), code); }

__host__ __device__ inline int pcmBytes(int bits) { return bits == kSampPcm24P ? 3 : (bits <= 16 ? 2 : 4); }
__host__ __device__ inline double pcmToF64(int32_t i, int bits) { return static_cast<double>(i) * (1.0 / pcmMax(bits)); }
// int(clamp(y, -1, 1) * maxVal), truncating; NaN passes the clamp as in Go and converts to 0
__host__ __device__ inline int32_t pcmOfF64(double y, int bits) {
    const double v = y > 1.0 ? 1.0 : (y < -1.0 ? -1.0 : y);
    const double s = v * pcmMax(bits);
    return s == s ? static_cast<int32_t>(s) : 0;
}
// TPDF-dithered quantizer (gar.h gar_set_dither).  The noise of a sample is a function of
// (seed, channel, position in the output stream) alone, through a 32-bit integer hash (wrapping uint32):
//   key(c)  = h32(lo32(seed) ^ h32(hi32(seed) ^ h32(c + 1)))          per channel
//   kh      = h32(key(c) + hi32(n))                                   per 2^32 positions
//   r       = h32(kh ^ lo32(n));  d = ((r & 0xffff) - (r >> 16)) / 65536   in (-1, 1), triangular, exact
// so a store path hoists key and kh and pays one h32 (two 32-bit multiplies) per sample.
constexpr int kDitherNone = 0, kDitherTpdf = 1;
__host__ __device__ inline bool pcmIsInt(int t) { return t >= 16; }  // 16 / 24 / 32 / packed 24: not f32 / f64 / half
__host__ __device__ inline uint32_t ditherH32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t ditherKey(uint32_t seedLo, uint32_t seedHi, uint32_t c) {
    return ditherH32(seedLo ^ ditherH32(seedHi ^ ditherH32(c + 1u)));
}
__host__ __device__ inline uint32_t ditherKeyHi(uint32_t key, uint32_t nHi) { return ditherH32(key + nHi); }
__host__ __device__ inline double ditherNoise(uint32_t kh, uint32_t nLo) {
    const uint32_t r = ditherH32(kh ^ nLo);
    return static_cast<double>(static_cast<int32_t>(r & 0xffffu) - static_cast<int32_t>(r >> 16)) * (1.0 / 65536.0);
}
// floor(clamp(y, -1, 1) * maxVal + (0.5 + d)), clamped to +-maxVal; NaN -> 0: round to nearest with a +-1 LSB
// triangular dither d (one f64 addition, then floor)
__host__ __device__ inline int32_t pcmDitherOfF64(double y, int bits, double d) {
#pragma clang fp contract(off)  // the product rounds before the addition (an f64 sample's product is not exact)
    const double m = pcmMax(bits);
    const double v = y > 1.0 ? 1.0 : (y < -1.0 ? -1.0 : y);
    const double q = __builtin_floor(v * m + (0.5 + d));
    const double c = q > m ? m : (q < -m ? -m : q);
    return c == c ? static_cast<int32_t>(c) : 0;
}
// The quantizer of one sample from scratch (checked stores, the staged kernels, gar_dev_dither_quantize).
__host__ __device__ inline int32_t pcmDitherAt(double y, int bits, uint32_t seedLo, uint32_t seedHi, uint32_t c, uint64_t n) {
    const uint32_t kh = ditherKeyHi(ditherKey(seedLo, seedHi, c), static_cast<uint32_t>(n >> 32));
    return pcmDitherOfF64(y, bits, ditherNoise(kh, static_cast<uint32_t>(n)));
}
// Clip / peak meter of an integer PCM store (gar.h gar_set_meter): THE tally of one stored sample,
// called by every metered store path and by gar_dev_meter_tally.  y = the sample in the compute type, widened
// exactly; `dither` with d = the sample's noise (ditherNoise) when the dithered quantizer stores it.  clips counts
// y > 1 or y < -1 (+-Inf count, NaN does not) and, dithered, a floor(s + t) outside +-maxVal before its clamp
// (pcmDitherOfF64's q, the same operations); peak = the largest |y| as the bit pattern of the non-negative double,
// which orders like the value (NaN ignored, +Inf the largest).
__host__ __device__ inline void meterTally(double y, int bits, bool dither, double d, uint32_t& clips, uint64_t& peak) {
#pragma clang fp contract(off)
    bool c = y > 1.0 || y < -1.0;
    if (dither) {
        const double m = pcmMax(bits);
        const double v = y > 1.0 ? 1.0 : (y < -1.0 ? -1.0 : y);
        const double q = __builtin_floor(v * m + (0.5 + d));
        c = c || q > m || q < -m;
    }
    clips += c ? 1u : 0u;
    const uint64_t a = __builtin_bit_cast(uint64_t, y) & 0x7fffffffffffffffull;
    if (y == y && a > peak) peak = a;
}
// The tally of one sample from scratch: channel c at stream position n (the checked stores, the staged kernels).
__host__ __device__ inline void meterTallyAt(double y, int bits, int dither, uint32_t seedLo, uint32_t seedHi, uint32_t c, uint64_t n,
                                             uint32_t& clips, uint64_t& peak) {
    double d = 0.0;
    if (dither) d = ditherNoise(ditherKeyHi(ditherKey(seedLo, seedHi, c), static_cast<uint32_t>(n >> 32)), static_cast<uint32_t>(n));
    meterTally(y, bits, dither != 0, d, clips, peak);
}
// One packed 24-bit sample at byte address b (no alignment): byte-wise, so nothing outside its 3 bytes is touched.
__host__ __device__ inline int32_t pcm24Load(const uint8_t* b) {
    const uint32_t u = static_cast<uint32_t>(b[0]) | (static_cast<uint32_t>(b[1]) << 8) | (static_cast<uint32_t>(b[2]) << 16);
    return static_cast<int32_t>(u << 8) >> 8;  // sign-extend bit 23
}
__host__ __device__ inline void pcm24Store(uint8_t* b, int32_t i) {
    b[0] = static_cast<uint8_t>(i);
    b[1] = static_cast<uint8_t>(i >> 8);
    b[2] = static_cast<uint8_t>(i >> 16);
}
// Four packed samples <-> three little-endian dwords (the vector pack / unpack kernels);
// u32x3a: the three dwords as one 12-byte access from a 4-byte aligned address.
typedef uint32_t u32x3a __attribute__((ext_vector_type(3), aligned(4)));
__host__ __device__ inline void pcm24Pack4(const int32_t (&i)[4], uint32_t (&d)[3]) {
    const uint32_t a = static_cast<uint32_t>(i[0]) & 0xffffffu, b = static_cast<uint32_t>(i[1]) & 0xffffffu;
    const uint32_t c = static_cast<uint32_t>(i[2]) & 0xffffffu, e = static_cast<uint32_t>(i[3]) & 0xffffffu;
    d[0] = a | (b << 24);
    d[1] = (b >> 8) | (c << 16);
    d[2] = (c >> 16) | (e << 8);
}
__host__ __device__ inline void pcm24Unpack4(const uint32_t (&d)[3], int32_t (&i)[4]) {
    i[0] = static_cast<int32_t>(d[0] << 8) >> 8;
    i[1] = static_cast<int32_t>(((d[0] >> 24) | (d[1] << 8)) << 8) >> 8;
    i[2] = static_cast<int32_t>(((d[1] >> 16) | (d[2] << 16)) << 8) >> 8;
    i[3] = static_cast<int32_t>(d[2]) >> 8;
}
__host__ __device__ inline double pcmRead(const void* p, int64_t e, int bits) {
    if (sampIsHalf(bits)) return static_cast<double>(halfToF32(static_cast<const uint16_t*>(p)[e], bits));
    if (bits == kSampPcm24P) return pcmToF64(pcm24Load(static_cast<const uint8_t*>(p) + 3 * e), 24);
    return bits == 16 ? pcmToF64(static_cast<const int16_t*>(p)[e], 16) : pcmToF64(static_cast<const int32_t*>(p)[e], bits);
}
__host__ __device__ inline void pcmWrite(void* p, int64_t e, int bits, double y) {
    if (sampIsHalf(bits)) {
        static_cast<uint16_t*>(p)[e] = halfOfF64(y, bits);
        return;
    }
    if (bits == kSampPcm24P) {
        pcm24Store(static_cast<uint8_t*>(p) + 3 * e, pcmOfF64(y, 24));
        return;
    }
    const double v = y > 1.0 ? 1.0 : (y < -1.0 ? -1.0 : y);  // NaN passes through as in Go, then converts
    const double s = v * pcmMax(bits);
    if (bits == 16) static_cast<int16_t*>(p)[e] = static_cast<int16_t>(s == s ? static_cast<int32_t>(s) : 0);
    else static_cast<int32_t*>(p)[e] = s == s ? static_cast<int32_t>(s) : 0;
}
// pcmWrite of an integer PCM type with the dithered quantizer: sample of channel c at stream position n.
__host__ __device__ inline void pcmWriteDither(void* p, int64_t e, int bits, double y, uint32_t seedLo, uint32_t seedHi,
                                               uint32_t c, uint64_t n) {
    const int32_t i = pcmDitherAt(y, bits, seedLo, seedHi, c, n);
    if (bits == kSampPcm24P) pcm24Store(static_cast<uint8_t*>(p) + 3 * e, i);
    else if (bits == 16) static_cast<int16_t*>(p)[e] = static_cast<int16_t>(i);
    else static_cast<int32_t*>(p)[e] = i;
}

struct HxDev;

// Device status codes a kernel writes into the handle's status word (OutDesc::err):
// hxt_kernel (gar_hxt.hpp hxtWait) -- 1 a compute wave's load-progress wait expired, 2 a loader's
// ring-slot wait expired.
constexpr int kHxtErrLoadWait = 1, kHxtErrSlotWait = 2;

// A launch whose configuration the device cannot run (dynamic LDS above the kernel's limit): the
// launcher records what was exceeded here and returns hipErrorInvalidConfiguration; the C-ABI turns
// it into GAR_ERR_INVALID_ARGUMENT with this message (gar_engine.hpp wrap).
std::string& launchLimitMsg();
hipError_t ldsTooBig(const char* kernel, size_t need, size_t limit);

// Device copy of a plan's ExactRows (gar_plan.hpp; uploaded by gar_stage.cpp uploadExact), read by the one
// exact recompute, firExact (gar_bg.hpp).  A launch's argument block embeds it as it is.
struct ExactDev {
    const double* rows;   // [Pc][rowMax] FIR rows (f64)
    const int* rowOff;    // [Pc] window offset of row r within its macro period
    const int* rowLen;    // [Pc]
    int rowMax;
    int twoStage;         // rows are DFT x2 (*) polyphase composites: a non-finite window runs the two stages
    const int* rowPh;     // [Pc] polyphase phase of each composite row
    const int* rowPar;    // [Pc] DFT output parity of each composite row
    const double* polyA;  // [L][T2] polyphase bank a (polyphase_stage.go:121-154), one upload per stage
    const double* dftC;   // [2][T1] DFT x2 banks (dft_stage.go:88-101), one upload per stage
    int T1, T2;           // DFT taps per phase, polyphase taps per phase
};

// Device copy of a BgPlan (gar_plan.hpp).
struct BgDev {
    int f64;
    int Pc, Qc, Kc, Kread, NS, nrb;
    int nprog, kch, nw, ncg, nred, nslots;
    const void* A;      // [nprog][kch*NS][64]
    const int* progs;   // [nprog][kBgProgInts] (gar_plan.hpp BgPlan::progTable)
    const int* reds;    // [nred][kBgRedInts]
    const HxDev* hx;    // host pointer: split-f16 variant of this plan (f32 compute) or null
    int rbAligned;      // BgPlan::rbAligned: small launches may run bg_rb_kernel
    int maxPrb;         // most programs of one row block
    const int* rbStart; // [nrb + 1]
    const int* hRbStart; // host copies (bg_rb_kernel passes them by value): [nrb + 1]
    const int* hRbK0;    // first input row of each program [nprog]
    ExactDev ex;           // outputs whose real window holds a non-finite sample (gar_bg.hpp bgNfFixOne)
    int* nfList;          // bg_kernel's non-finite fix list (gar_bg.hpp kBgNfInts ints, zeroed)
};
constexpr size_t kBgNfListBytes = 4 * (2 + 256 * 129 + 1);  // gar_bg.hpp kBgNfInts (static_assert there)

// Device copy of an HxPlan (gar_plan.hpp): split-f16 MFMA FIR, f32 compute.
struct HxDev {
    int Pc, Qc, Kc, Kread, NS, nrb;
    int nw, kch, nred, nslots, ea;
    int rb;              // row-block mode (HxPlan::rbMode)
    const void* A;       // [nw][kch*NS][2][64][8] f16
    const int* progs;    // [nw][kBgProgInts] (HxPlan::progTable)
    const int* reds;     // [nred][kBgRedInts]
    ExactDev ex;         // outputs whose windows hold a loud element: !(|x| < kHxLoud = 16 - 2^-8), Inf, NaN
    int* fix;           // [1 + fixCap]: interior blocks holding loud elements (count first)
    int fixCap;
    int hxsOk;           // host: the plan fits hxs_kernel (hxsPlanFits), so fused PCM I/O can use it
    int hU0[16], hRbw[16];  // host copies of each row-block program's first row / row block (rb mode, nw <= 16)
};

// General polyphase stage with live cubic coefficient interpolation
// (polyphase_stage.go:257-293): output m uses at = at0 + m*step (local).
struct PolyDev {
    int f64;
    int L, T;
    int64_t step, at0, u_base;  // u_base = global stream index of local history index 0
    int64_t m0;                 // the stage's absolute output index of the launch's first output (tap rotation)
    const void *a, *b, *c, *d;  // [L][T] reversed, compute dtype
    const void* abcd;           // [L][T][4] the same four banks interleaved (poly_kernel's one-load tap)
};

// Launchers (all asynchronous on `stream`).  Return hipSuccess or the launch error.
// Optional history keep folded into a streaming FIR launch: dst[(t - t0) * C + c] = src(t, c) for
// t in [t0, t0 + n) (what launchGather does), written by the launch's workgroups after their
// blocks; `done` set when the launch took it (the launch plan's histFolded), else the caller gathers.
struct HistCopy {
    void* dst = nullptr;
    int64_t t0 = 0, n = 0;
    bool done = false;
};

// Every x == 0 FIR stage: plans the launch (gar_hx_launch.hpp firPlanLaunch: the bg kernels, the streaming
// split-f16 kernels or hx_kernel) and dispatches it.
// `meter` (gar_set_meter on, an integer PCM view): the handle's tallies, [C] x {clips, peak bits}; the launch runs the
// metered instantiations of the streaming kernels (gar_hxs_i5.hip), same plan, same stored bytes.
hipError_t launchBg(const BgDev& p, const SrcDesc& src, const OutDesc& out, int C, hipStream_t stream,
                    HistCopy* hc = nullptr, uint64_t* meter = nullptr);
// True when a row-block plan fits the streaming kernels' geometry at one period per group (its smallest
// ring), i.e. their planner never declines it (gar_hxs_launch.cpp).
bool hxsPlanFits(const HxDev& p);
// Compute units of the current device (256 when it cannot be queried).
int deviceCUs();
hipError_t launchPoly(const PolyDev& p, const SrcDesc& src, const OutDesc& out, int64_t nout, int C,
                      hipStream_t stream);
// CubicStage outputs of nseg checkpointed segments (segs readable by the device:
// pinned host or device memory); x_end = one past the last input; step = 1/ratio.
hipError_t launchCubic(int f64, const CubicSeg* segs, int64_t nseg, int64_t x_end, double step, const SrcDesc& src,
                       const OutDesc& od, int C, hipStream_t stream, int segLen = static_cast<int>(kCubicSegInputs));
// dst[(t - t0) * C + c] = src(t, c) for t in [t0, t0 + n): history compaction / materialisation.
hipError_t launchGather(int f64, const SrcDesc& src, void* dst, int64_t t0, int64_t n, int C, hipStream_t stream);
// Strided copy with dtype conversion (pass-through stages, group split).
hipError_t launchCopy(const void* src, int src_f64, int64_t s_fs, int64_t s_cs, void* dst, int dst_f64,
                      int64_t d_fs, int64_t d_cs, int64_t n, int C, hipStream_t stream);
// PCM / half staging of the non-fused paths: type codes 0 f32, 1 f64, 4 f16, 5 bf16, 16/24/32 PCM, 280 packed
// 24-bit (pcmRead / pcmWrite); not the ABI's codes for f32 / f64.  Packed 24-bit against a contiguous f32 / f64
// buffer runs the vector kernels (unpack24_kernel / pack24_kernel: 4 samples <-> 3 dwords per thread) when the
// packed side is interleaved-contiguous from a 4-byte aligned base; every other case the per-element kernel.
// `dz` (mode on, an integer PCM d_type): element (t, c) is stored by the dithered quantizer at stream position dz.pos0 + t.
struct Dither {
    int mode = kDitherNone;
    uint32_t seedLo = 0, seedHi = 0;
    int64_t pos0 = 0;
};
hipError_t launchConvert(const void* src, int s_type, int64_t s_fs, int64_t s_cs, void* dst, int d_type, int64_t d_fs,
                         int64_t d_cs, int64_t n, int C, hipStream_t stream, const Dither& dz = Dither(), uint64_t* meter = nullptr);
// `meter` (an integer PCM d_type): the metered kernels of gar_meter.hip store the same bytes by the same layout
// choice and tally every stored sample of channel c into meter[2 * c], meter[2 * c + 1] (clips, peak bits).
hipError_t launchConvertMeter(const void* src, int s_type, int64_t s_fs, int64_t s_cs, void* dst, int d_type, int64_t d_fs,
                              int64_t d_cs, int64_t n, int C, hipStream_t stream, const Dither& dz, uint64_t* meter, bool packV);

// One history of a state snapshot (gar_state_save / gar_state_load): `rows` rows of C elements of `es`
// bytes, contiguous at `ptr` (leading dimension C, the engine's Hist layout), stored tightly packed from
// byte `off` (a multiple of 16) of the snapshot's row image.  chunk0 = 16-byte chunks of the segments
// before this one in the table (each segment has ceil(rows * C * es / 16)); no segment is empty.
struct StateSeg {
    void* ptr;
    int64_t rows;
    int32_t C, es;
    int64_t off;
    int64_t chunk0;
};
// Every segment of a handle in ONE launch: pack gathers the histories into the contiguous device image
// `img` (then one device-to-host copy), unpack scatters an uploaded image into the histories.  `segs`
// is the table in device memory (nseg entries, nchunks chunks in all).  Work is spread over (segment,
// 16-byte chunk): one 16-byte load + store where the chunk is whole and both sides are 16-byte aligned,
// element by element otherwise (a segment's tail), so nothing past a segment's last row is touched.
// The pad bytes between segments of the image are neither read nor written.
hipError_t launchStatePack(const StateSeg* segs, int nseg, int64_t nchunks, void* img, hipStream_t stream);
hipError_t launchStateUnpack(const StateSeg* segs, int nseg, int64_t nchunks, const void* img, hipStream_t stream);

}  // namespace gar
