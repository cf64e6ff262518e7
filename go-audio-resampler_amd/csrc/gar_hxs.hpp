// gar_hxs.hpp -- streaming split-f16 FIR kernel (row-block plans, gfx950).
//
// Same arithmetic as hx_kernel (gar_hx.hpp: constant split scale, three f16
// MFMA products per 32-deep step, lo products in their own accumulator), so
// the two kernels produce identical bits; the difference is the data flow:
//
//  * Wave specialisation.  Waves [0, nprog) are compute waves: each owns one
//    row block (A in registers for the whole kernel), reads B fragments from
//    LDS with ds_read_b64_tr_b16, runs the MFMAs and stores its outputs.  They
//    issue no global loads, so no s_waitcnt on vector memory ever stalls an
//    MFMA stream (on gfx950 stores and loads share vmcnt).  The last
//    kHxsLoaders waves are loader waves: they load the input rows into VGPRs
//    kHxsD groups ahead (a fixed buffer-load pattern the compiler's vmcnt
//    tracking pipelines), convert them to the f16 hi/lo split (or from integer
//    PCM first), detect loud elements and write the LDS ring.
//  * Long columns.  A column is (channel, chunk of Np consecutive macro
//    periods); a workgroup owns 16 columns and walks them group by group (G
//    periods per group, one barrier per group).  Each column's window lives
//    in an LDS ring of R = n*G*Qc rows (+ a mirror of the first Kread - Qc
//    rows, so every group's window is contiguous), so each input row is staged
//    once per column instead of once per G-period window (round-1 kernel:
//    W/(G*Qc) = 1.34x; here (Np*Qc + Kread - Qc)/(Np*Qc) ~ 1.02x).
//  * Loud elements (!(|x| < kHxLoud): |x| >= 16 - 2^-8, Inf, NaN) are staged as zero and their
//    column-relative row range recorded; after the block, every output whose
//    window holds one is recomputed exactly (hxsFixup -> gar_bg.hpp firExact: f64, two stages
//    when non-finite) by the same workgroup.
#pragma once
#include <climits>

#include "gar_hx.hpp"
#include "gar_hxs_geo.hpp"
#include "gar_meter.hpp"

namespace gar {

#ifndef GAR_HXS_D
#define GAR_HXS_D 2
#endif
constexpr int kHxsD = GAR_HXS_D;                        // loads in flight per loader wave (register staging)
constexpr int kHxsItems = (4 * kHxsNP + kHxsLoaders - 1) / kHxsLoaders;  // (quad, piece) items per loader per load
#ifndef GAR_HXS_PRIO
#define GAR_HXS_PRIO 0
#endif
#ifndef GAR_HXS_PF2
#define GAR_HXS_PF2 0  // B fragments two steps ahead (A/B builds)
#endif

struct HxsArgs {
    const h8v* A;          // [nprog][NS][2][64] f16x8
    const int* progs;      // [nprog][kBgProgInts]
    int ea, Pc, Qc, Kc, Kread, G, C, nprog;
    int ncols, nblocks, Np, ngroups;
    int R, Rt, mirror;     // ring rows (n*G*Qc), rows incl. mirror, mirrored ring rows [0, mirror)
    int Wg;                // rows one group reads: (G-1)*Qc + Kread
    unsigned long long* prof;  // development: per-phase cycle sums (GAR_HXS_PROF), null in production
    int dbg;               // development attribution (GAR_HXS_DBG, wrong output): 1 no steady DMAs, 2 no stores,
                           // 4 no MFMA, 16 no steady conversion
    int small;             // one period per column, window staged in one pass (hxsSmallStage)
    int bigSmall;          // development (GAR_HXS_SMALLK=0): small launches on hxs_kernel instead of hxs_small_kernel
    int vst, fmt;          // epilogue layout (template VST), load layout 0 gathered / 1 STEREO / 2 ROW16 /
                           // 3, 4 STEREO PCM / 6 STEREO half / 7 ROW16 half (5: hxt_kernel's ROW32)
    int xcdPair;           // ROW16 blocks 2m, 2m+1 share every 128-B input/output line: run them on one XCD
    int nt;                // development: non-temporal output stores (GAR_HXS_NT)
    int64_t a_lo, a_hi;    // absolute macro periods of the launch
    int64_t o_lo, o_hi;    // outputs written
    const char* in;        // input element (t, c) at byte in + (t*in_fs + c*in_cs)*in_esz, t absolute, raw loads for t in [fastLo, fastHi)
    int64_t in_fs, in_cs, fastLo, fastHi;
    int in_esz, in_pcm;    // bytes per input element; PCM bits or 4 / 5 for f16 / bf16 (0: f32 / f64 input)
    int out_pcm;           // PCM output bits or 4 / 5 for f16 / bf16 (0: f32 / f64 output); stores go through
                           // the checked path unless VST is the type's frame-pair layout (4, 5)
    float* hdst;           // folded history keep (HistCopy): hdst[(t - ht0) * C + c] = src(t, c), t < ht0 + hn
    int64_t ht0, hn;
    char* out;             // output (o, c) at out + o*out_fs + c*out_cs (bytes), o absolute
    int64_t out_fs, out_cs;
    int out_f64;
    // cold fields: edge gathers and the exact fallback (hxsFixup)
    SrcDesc src;
    OutDesc od;
    ExactDev ex;           // HxDev::ex
    // hxt_kernel (gar_hxt.hpp): compute wave w runs row block role[w] & 0xff on the periods p with
    // p % stride == phase (phase = (role[w] >> 8) & 0xff, stride = role[w] >> 16)
    int ncomp;
    int role[12];
    int* err;               // the handle's device status word (host-mapped), written when a progress wait expires
    int pollMax;            // progress-wait bound in polls (2^24; development knob GAR_HXT_FAULT: 2^12)
    int faultNeed;          // development (GAR_HXT_FAULT=1): added to the compute waves' load count, unreachable
    int coop;               // hxt_kernel: compute waves stage each block's first window (GAR_HXT_COOP=0: loaders)
    // hxq_kernel (small f32 STEREO / ROW16 launches): workgroup = (block, qRbs row blocks), qGroups per block
    int qRbs, qGroups;
    int qU0[12], qRbw[12];  // first window row / row block of each row-block program (HxDev::hU0)
    int qOpt;               // hxq_kernel variants (GAR_HXQ_OPT): 1 barrier after the first load batch issues, 2 buffer-load history keep
    // TPDF dither of the integer PCM stores (OutDesc::dither), read by the DITHER instantiations only (which such a
    // launch runs: hxsLaunchDither); last, so no other field moves: output o sits at stream position o + dpos
    int dither;
    uint32_t dseedLo, dseedHi;
    int64_t dpos;
};
typedef const __attribute__((address_space(4))) HxsArgs* HxsArgsP;

// Workgroup barrier for LDS hand-offs only: LDS operations drained
// (lgkmcnt(0)), no vector-memory wait.  __syncthreads() is a release/acquire
// fence and waits vmcnt(0): the loader waves' prefetch loads and the compute
// waves' output stores would both drain at every group.
__device__ __forceinline__ void hxsBarrier() {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // vmcnt max, expcnt max, lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

__device__ __forceinline__ HxsArgsP hxsCold() {
    uint64_t v = reinterpret_cast<uint64_t>(__builtin_amdgcn_kernarg_segment_ptr());
    asm volatile("" : "+s"(v));
    return reinterpret_cast<HxsArgsP>(v);
}

// Logical block of launch slot i.  Workgroups are dispatched round-robin over the 8 XCDs (slot
// i on XCD i % 8); with xcdPair, blocks 2m and 2m+1 -- the two halves of every 128-B line of
// a ROW16 layout (16 channels x 4 B = 64 B per row) -- run as slots i and i + 8 on the same
// XCD, so the second reader / writer of each line meets it in that XCD's L2.
__device__ __forceinline__ int hxsBlock(const HxsArgs& x, int i) {
    if (!x.xcdPair) return i;
    const int s = i >> 3, xc = i & 7;
    return ((s >> 1) * 8 + xc) * 2 + (s & 1);
}

// outWrite of the fixups; DITHER (the kernels of a launch with dither on, integer PCM output): the sample goes
// through the dithered quantizer, at the position every other store of the launch gives it.
template <bool DITHER>
__device__ __forceinline__ void hxsOutWrite(const OutDesc& od, int64_t o, int c, float v) {
    if constexpr (DITHER) {
        if (o < od.o_lo || o >= od.o_hi) return;
        pcmWriteDither(od.out, (o - od.o0) * od.fs + static_cast<int64_t>(c) * od.cs, od.pcm, static_cast<double>(v), od.dseedLo,
                       od.dseedHi, static_cast<uint32_t>(c), static_cast<uint64_t>(o - od.o0 + od.dpos0));
        return;
    }
    outWrite<float>(od, o, c, v);
}


// ---- staging --------------------------------------------------------------------
// A load (rows [T0, T0 + nrow) of every column of the block) travels:
//   global --buffer loads (loader waves, kHxsD loads ahead)--> VGPRs --f16 hi/lo split--> ring.
// A load is 4 quads x kHxsNP pieces of 64 rows; loader wave l owns the (quad, piece) items
// l, l + kHxsLoaders, ... (item = 4 * piece + quad), lane = row of the piece.  Layouts:
//  * STEREO (fmt 1, C == 2, frames interleaved): quad q = chunks 2q, 2q+1 (two channels each),
//    one buffer_load_dwordx2 per chunk (64 lanes = 512 B contiguous);
//  * ROW16 (fmt 2, C % 16 == 0, 16-B aligned rows): quad q = channels 4q..4q+3 of the block's
//    chunk, one buffer_load_dwordx4;
//  * STEREO half (fmt 6, f16 / bf16 frames): as STEREO PCM16 (fmt 3), one buffer_load_dword per
//    chunk row (both channels), widened to two f32 at conversion time;
//  * ROW16 half (fmt 7, C % 16 == 0, 8-B aligned 2-byte rows): quad q = channels 4q..4q+3, one
//    buffer_load_dwordx2 (a 16-row piece is 16 whole 32-B block rows);
//  * every other layout, f64 input and the edges (rows before the input: history seam, stream
//    start; partial blocks): gathered at conversion time.
// Rows past the caller's input read zeros through the buffer records.
struct HxsStage {
    int T0, nrow;   // column-relative first row and row count
    bool fast;      // buffer loads: every column live, no row before the raw f32 input
};

// Buffer resource (raw, stride 0) over the raw input from absolute row `row0`
// of channel offset `cofs` (elements): records end at row fastHi, so loads past
// the caller's input (the tail of the last chunk) read zeros.
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
template <class XP>
__device__ __forceinline__ u32x4v hxsRsrc(XP x, int64_t row0, int64_t cofs, int elemBytes) {
    const uint64_t base = reinterpret_cast<uint64_t>(x->in + (row0 * x->in_fs + cofs) * x->in_esz);
    const int64_t nb = x->fastHi > row0 ? (x->fastHi - row0 - 1) * x->in_fs * x->in_esz + elemBytes : 0;
    const unsigned nrec = static_cast<unsigned>(nb < 0x7fffffff ? nb : 0x7fffffff);
    u32x4v r;
    r.x = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(base));
    r.y = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(base >> 32) & 0xffffu);
    r.z = __builtin_amdgcn_readfirstlane(nrec);
    r.w = 0x00020000u;
    return r;
}

// The same resource as a buffer-resource value (compiler-tracked raw_buffer_load builtins).
template <class XP>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t hxsRsrcT(XP x, int64_t row0, int64_t cofs, int elemBytes) {
    const u32x4v r = hxsRsrc(x, row0, cofs, elemBytes);
    const uint64_t base = static_cast<uint64_t>(r.x) | (static_cast<uint64_t>(r.y) << 32);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(base), 0, static_cast<int>(r.z), 0x00020000);
}

// Element (t, c) of the stream for edge stages: history | input (f32/f64) |
// zero.  Branch-free address selection (a dummy readable address for zeros)
// so a piece's gathers issue together instead of one dependent load each.
__device__ __forceinline__ float hxsGather(const SrcDesc& s, int64_t t, int c, const void* dummy) {
    const int64_t h = t - s.hist_base, i = t - s.in_base;
    const bool valid = t >= 0 && t < s.valid_end;
    const bool inH = valid && s.hist && h >= 0 && h < s.hist_len;
    const bool inI = valid && !inH && s.in && i >= 0 && i < s.in_len;
    const float* hp = static_cast<const float*>(s.hist) + (inH ? h * s.hist_ld + c : 0);
    if (s.in_pcm) {  // integer PCM input (main.go:444-472 scaling) or f16 / bf16 (exact widening)
        const int64_t e = inI ? i * s.in_fs + static_cast<int64_t>(c) * s.in_cs : 0;
        const float vh = *(inH ? hp : static_cast<const float*>(dummy));
        const float vi = inI ? static_cast<float>(pcmRead(s.in, e, s.in_pcm)) : 0.f;
        return inH ? vh : vi;
    }
    if (s.in_f64) {
        const double* ip = static_cast<const double*>(s.in) + (inI ? i * s.in_fs + static_cast<int64_t>(c) * s.in_cs : 0);
        const float vh = *(inH ? hp : static_cast<const float*>(dummy));
        const double vi = *(inI ? ip : static_cast<const double*>(dummy));
        return inH ? vh : (inI ? static_cast<float>(vi) : 0.f);
    }
    const float* ip = static_cast<const float*>(s.in) + (inI ? i * s.in_fs + static_cast<int64_t>(c) * s.in_cs : 0);
    const float v = *(inH ? hp : (inI ? ip : static_cast<const float*>(dummy)));
    return (inH || inI) ? v : 0.f;
}

template <class XP>
__device__ __forceinline__ int64_t hxsChunkRow(XP x, int k, int T0) {
    return (x->a_lo + static_cast<int64_t>(k) * x->Np) * x->Qc + T0;
}

// Stage k of a block: k = 0 rows [0, Wg) (in parts of at most G*Qc), k >= 1
// rows [Wg + (k-1)*G*Qc, Wg + k*G*Qc).
template <class XP>
__device__ __forceinline__ HxsStage hxsStage(XP x, int b, int T0, int nrow) {
    HxsStage s;
    s.T0 = T0;
    s.nrow = nrow;
    const int c0 = b * 16, c1 = c0 + 15;
    const int64_t tlo = (x->a_lo + static_cast<int64_t>(c0 / x->C) * x->Np) * x->Qc + T0;
    s.fast = ((x->fmt >= 1 && x->fmt <= 4) || x->fmt == 6 || x->fmt == 7) && c1 < x->ncols && tlo >= x->fastLo && x->fastHi > x->fastLo;
    return s;
}
// Load j of a block: j < P = ceil(Wg / GQ) the parts of stage 0 (rows [j*GQ, ...) up to Wg),
// then stage j - P + 1 (rows [Wg + (j-P)*GQ, + GQ)).
template <class XP>
__device__ __forceinline__ HxsStage hxsLoad(XP x, int b, int j, int P) {
    const int GQ = x->G * x->Qc;
    if (j < P) return hxsStage(x, b, j * GQ, min(GQ, x->Wg - j * GQ));
    return hxsStage(x, b, x->Wg + (j - P) * GQ, GQ);
}

// One item (row `row` of the stage, quad q) -> ring rows (hi/lo split, mirror, loud marking).
template <class XP>
__device__ __forceinline__ void hxsPutItem(XP x, const HxsStage& st, int p0, int q, int row, f32x4 e,
                                           char* ring, uint32_t QS, int* loudLo, int* loudHi, int* flag) {
    const int t = st.T0 + row;  // column-relative row
    int p = p0 + row;           // ring row (nrow <= R)
    if (p >= x->R) p -= x->R;
    const bool l0 = hxLoud(e[0]), l1 = hxLoud(e[1]), l2 = hxLoud(e[2]), l3 = hxLoud(e[3]);
    if (__builtin_expect(l0 | l1 | l2 | l3, 0)) {
        if (l0) { atomicMin(loudLo + 4 * q, t); atomicMax(loudHi + 4 * q, t); e[0] = 0.f; }
        if (l1) { atomicMin(loudLo + 4 * q + 1, t); atomicMax(loudHi + 4 * q + 1, t); e[1] = 0.f; }
        if (l2) { atomicMin(loudLo + 4 * q + 2, t); atomicMax(loudHi + 4 * q + 2, t); e[2] = 0.f; }
        if (l3) { atomicMin(loudLo + 4 * q + 3, t); atomicMax(loudHi + 4 * q + 3, t); e[3] = 0.f; }
        *flag = 1;
    }
    uint2 hv, lv;
    hxSplit2(e[0], e[1], hv.x, lv.x);
    hxSplit2(e[2], e[3], hv.y, lv.y);
    char* qb = ring + q * QS;
    *reinterpret_cast<uint2*>(qb + 8 * p) = hv;
    *reinterpret_cast<uint2*>(qb + 8 * x->Rt + 8 * p) = lv;
    if (p < x->mirror) {
        p += x->R;
        *reinterpret_cast<uint2*>(qb + 8 * p) = hv;
        *reinterpret_cast<uint2*>(qb + 8 * x->Rt + 8 * p) = lv;
    }
}

// Small launches (x.small: one macro period per column, one group): every wave gathers
// its share of the block's whole window [0, Wg) straight into the ring in one pass --
// one memory round trip instead of the pipeline's chain of DMA stages.
template <class XP>
__device__ __forceinline__ void hxsSmallStage(XP x, int b, int tid, int nth, char* ring, uint32_t QS,
                                              int* loudLo, int* loudHi, int* flag) {
    const HxsArgsP xc = hxsCold();
    const SrcDesc src = kload(&xc->src);
    HxsStage st;
    st.T0 = 0;
    st.nrow = x->Wg;
    st.fast = false;
    // batches of kB items per thread: every gather of a batch issues before the first conversion,
    // so the window costs one memory round trip per batch, not one per item
    constexpr int kB = 4;
    const int nit = 4 * x->Wg;
    for (int i0 = tid; i0 < nit; i0 += kB * nth) {
        f32x4 e[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int i = i0 + u * nth;
            const int q = i & 3, row = i >> 2;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = b * 16 + 4 * q + n;
                const int k = col / x->C, c = col - k * x->C;
                e[u][n] = (i < nit && col < x->ncols) ? hxsGather(src, hxsChunkRow(x, k, row), c, x->A) : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const int i = i0 + u * nth;
            if (i < nit) hxsPutItem(x, st, 0, i & 3, i >> 2, e[u], ring, QS, loudLo, loudHi, flag);
        }
    }
}

// ---- register staging -------------------------------------------------------------
// One load's registers per loader wave: STEREO two f2v per item, ROW16 one f32x4.  One loop per
// format (hxsRegLoadersT<FMT>), so a loaded register is never merged with another format's
// value (a merge is a copy, and a copy waits for the load).
template <int FMT>
struct HxsRegBuf {
    f2v a[kHxsItems], b[kHxsItems];
};
template <>
struct HxsRegBuf<2> {
    f32x4 v[kHxsItems];
};
template <>
struct HxsRegBuf<3> {  // STEREO PCM16: one dword (both channels) per chunk row
    uint32_t a[kHxsItems], b[kHxsItems];
};
template <>
struct HxsRegBuf<4> {  // STEREO int32 PCM24 / PCM32: both channels of a chunk row, kept as integers
    uint2 a[kHxsItems], b[kHxsItems];
};
template <>
struct HxsRegBuf<6> {  // STEREO f16 / bf16: one dword (both channels) per chunk row
    uint32_t a[kHxsItems], b[kHxsItems];
};
template <>
struct HxsRegBuf<7> {  // ROW16 f16 / bf16: four channels (8 B) per lane
    uint2 v[kHxsItems];
};

// Two half samples of one dword -> f32 (code: kSampF16 / kSampBF16, uniform).
__device__ __forceinline__ f2v hxsHalf2(uint32_t u, int code) {
    if (code == kSampBF16) return f2v{__uint_as_float(u << 16), __uint_as_float(u & 0xffff0000u)};
    typedef _Float16 h2v_ __attribute__((ext_vector_type(2)));
    const h2v_ h = __builtin_bit_cast(h2v_, u);
    return f2v{static_cast<float>(h.x), static_cast<float>(h.y)};
}

// Per-block load source: one resource from the block's first chunk row 0 (records end at the
// caller's input end: zeros past it), the byte stride of a row and of a chunk.
struct HxsRegSrc {
    __amdgpu_buffer_rsrc_t r;
    int rowB, chunkB, lane0;
};

template <int FMT, class XP>
__device__ __forceinline__ HxsRegSrc hxsRegSrc(XP x, int b, int lane) {
    HxsRegSrc r;
    const int col0 = b * (FMT == 5 ? 32 : 16), k = col0 / x->C, c0 = col0 - k * x->C;
    r.rowB = static_cast<int>(x->in_fs) * x->in_esz;
    r.chunkB = x->Np * x->Qc * r.rowB;
    r.r = hxsRsrcT(x, hxsChunkRow(x, k, 0), (FMT == 2 || FMT == 5 || FMT == 7) ? c0 : 0,
                   FMT == 5 ? 128 : FMT == 2 ? 64 : FMT == 7 ? 32 : ((FMT == 3 || FMT == 6) ? 4 : 8));
    // ROW16: lane = 16 q + r reads row r of a 16-row piece, channels 4q..4q+3 -- one instruction
    // covers 16 whole 64-B block rows (16 lines) instead of 16 B of 64 rows (64 lines); ROW32 (FMT 5,
    // hxt_kernel only): lane = 8 r + q, 8 whole 128-B rows per instruction
    r.lane0 = FMT == 5 ? (lane >> 3) * r.rowB + 16 * (lane & 7)
            : FMT == 2 ? (lane & 15) * r.rowB + 16 * (lane >> 4)
            : FMT == 7 ? (lane & 15) * r.rowB + 8 * (lane >> 4) : lane * r.rowB;
    return r;
}

// Issue load `st` (live: a real load; else nothing to fetch).  Always the same instruction
// pattern, kHxsItems x (2 STEREO | 1 ROW16) loads: items the load does not need (past its
// rows, dead loads, edge loads that are gathered later) get an offset past every record,
// which returns zeros without a memory access -- the compiler's vmcnt tracking then waits
// for exactly the oldest load (a conditional issue would make it wait for all).
template <int FMT>
__device__ __forceinline__ bool hxsRegIssue(const HxsStage& st, bool live, const HxsRegSrc& rs, int l, HxsRegBuf<FMT>& r) {
    const bool fast = FMT != 0 && live && st.fast;
    const int npc = fast ? (st.nrow + 63) >> 6 : 0;
    // loader index and strides opaque per call: otherwise every item's offset and mask is hoisted out
    // of the step loop into SGPRs, which spill (v_readlane per item and step)
    int lq = l;
    HxsRegSrc rq = rs;
    asm volatile("" : "+s"(lq), "+s"(rq.rowB), "+s"(rq.chunkB));
    const int base = st.T0 * rq.rowB + rq.lane0;
#pragma unroll
    for (int k = 0; k < kHxsItems; ++k) {
        const int it = lq + k * kHxsLoaders, q = it & 3, i = it >> 2;
        const bool on = it < 4 * kHxsNP && i < npc;
        if constexpr (FMT == 2) {  // item = 16-row piece (all four quads)
            const bool on16 = it < 4 * kHxsNP && 16 * it < (fast ? st.nrow : 0);
            const int o = on16 ? base + 16 * it * rq.rowB : static_cast<int>(0x80000000u);
            r.v[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs.r, o, 0, 0));
        } else if constexpr (FMT == 7) {  // item = 16-row piece of 32-B half rows
            const bool on16 = it < 4 * kHxsNP && 16 * it < (fast ? st.nrow : 0);
            const int o = on16 ? base + 16 * it * rq.rowB : static_cast<int>(0x80000000u);
            r.v[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o, 0, 0));
        } else if constexpr (FMT == 1) {  // f32 stereo frames
            const int o = on ? base + 64 * i * rq.rowB + 2 * q * rq.chunkB : static_cast<int>(0x80000000u);
            const int o2 = on ? o + rq.chunkB : o;
            r.a[k] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o, 0, 0));
            r.b[k] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o2, 0, 0));
        } else if constexpr (FMT == 4) {  // int32 stereo frames, in integer registers: carried through a float vector
            // the second channel's conversion was dropped (both channels came out as channel 0)
            const int o = on ? base + 64 * i * rq.rowB + 2 * q * rq.chunkB : static_cast<int>(0x80000000u);
            const int o2 = on ? o + rq.chunkB : o;
            r.a[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o, 0, 0));
            r.b[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o2, 0, 0));
        } else if constexpr (FMT == 3 || FMT == 6) {  // int16 / half stereo frames
            const int o = on ? base + 64 * i * rq.rowB + 2 * q * rq.chunkB : static_cast<int>(0x80000000u);
            const int o2 = on ? o + rq.chunkB : o;
            r.a[k] = __builtin_amdgcn_raw_buffer_load_b32(rs.r, o, 0, 0);
            r.b[k] = __builtin_amdgcn_raw_buffer_load_b32(rs.r, o2, 0, 0);
        }
    }
    return fast;
}

// Small launches, interior blocks of a STEREO (fmt 1) / ROW16 (fmt 2) f32 input: the window [0, Wg)
// of every column comes straight from the raw input through buffer loads -- one 8-B load (both
// channels of a chunk) or one 16-B load (four channels) per lane and row, rows past the input end
// read as zeros through the records -- instead of four branch-free scalar gathers per item, whose
// 64-bit address arithmetic dominated a short call's instruction stream.  Same image, same split.
template <class XP>
__device__ __forceinline__ bool hxsSmallFast(XP x, int b, int tid, int nth, char* ring, uint32_t QS, int* loudLo,
                                             int* loudHi, int* flag) {
    if (x->fmt != 1 && x->fmt != 2) return false;
    const HxsStage st = hxsStage(x, b, 0, x->Wg);  // fast: every column live, row 0 at or after the raw input
    if (!st.fast) return false;
    const int lane = tid & 63, w = tid >> 6, nw = nth >> 6;
    constexpr int kB = 4;  // items per wave in flight
    if (x->fmt == 1) {
        const HxsRegSrc rs = hxsRegSrc<1>(x, b, lane);
        const int nit = 4 * ((st.nrow + 63) >> 6);
        for (int it0 = w; it0 < nit; it0 += kB * nw) {
            f2v a[kB], c[kB];
#pragma unroll
            for (int u = 0; u < kB; ++u) {
                const int it = it0 + u * nw, q = it & 3, pc = it >> 2;
                const int o = it < nit ? rs.lane0 + 64 * pc * rs.rowB + 2 * q * rs.chunkB : static_cast<int>(0x80000000u);
                const int o2 = it < nit ? o + rs.chunkB : o;
                a[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o, 0, 0));
                c[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(rs.r, o2, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < kB; ++u) {
                const int it = it0 + u * nw, row = 64 * (it >> 2) + lane;
                if (it < nit && row < st.nrow)
                    hxsPutItem(x, st, 0, it & 3, row, f32x4{a[u].x, a[u].y, c[u].x, c[u].y}, ring, QS, loudLo, loudHi, flag);
            }
        }
    } else {
        const HxsRegSrc rs = hxsRegSrc<2>(x, b, lane);
        const int nit = (st.nrow + 15) >> 4;
        for (int it0 = w; it0 < nit; it0 += kB * nw) {
            f32x4 v[kB];
#pragma unroll
            for (int u = 0; u < kB; ++u) {
                const int it = it0 + u * nw;
                const int o = it < nit ? rs.lane0 + 16 * it * rs.rowB : static_cast<int>(0x80000000u);
                v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs.r, o, 0, 0));
            }
#pragma unroll
            for (int u = 0; u < kB; ++u) {
                const int it = it0 + u * nw, row = 16 * it + (lane & 15);
                if (it < nit && row < st.nrow) hxsPutItem(x, st, 0, lane >> 4, row, v[u], ring, QS, loudLo, loudHi, flag);
            }
        }
    }
    return true;
}

// int(clamp(float64(y), -1, 1) * 32767) with pcmWrite's semantics (f64 product: exact; NaN -> 0).
__device__ __forceinline__ int32_t pcm16Of(float y) {
    const double d = static_cast<double>(y);
    const double v = (d > 1.0 ? 1.0 : (d < -1.0 ? -1.0 : d)) * 32767.0;
    return v == v ? static_cast<int32_t>(v) : 0;
}

// Interior store of a lane's four rows.  VST (the launch's output layout, a template parameter so
// the epilogue carries no layout branches): 0 any f32 layout (4 stores), 1 channel-contiguous f32
// (one 16-B store), 2 stereo-interleaved f32 (lane pairs swap halves by DPP: one 16-B store of two
// frames each), 3 f64 (4 stores), 4 stereo-interleaved PCM16 (two int16 frames, 8 B), 5 stereo-
// interleaved f16 / bf16 (two frames, 8 B: the same lane-pair swap, packed f32 -> half conversion).
// DITHER (VST 4): the dithered quantizer, pos = the stream position of the first frame at p.
template <int VST, bool DITHER = false>
__device__ __forceinline__ void hxsStoreFast(const HxsArgs& x, char* p, f32x4 y, int lane, int64_t pos = 0) {
    const bool nt = kHxsDev && x.nt;
    if (VST == 2 || VST == 4 || VST == 5) {
        const bool even = (lane & 1) == 0;
        const float s0 = even ? y[2] : y[0], s1 = even ? y[3] : y[1];
        const float q0 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s0), 0xB1, 0xf, 0xf, false));
        const float q1 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s1), 0xB1, 0xf, 0xf, false));
        f32x4 w;
        if (even) { w[0] = y[0]; w[1] = q0; w[2] = y[1]; w[3] = q1; }
        else      { w[0] = q0; w[1] = y[2]; w[2] = q1; w[3] = y[3]; }
        if constexpr (VST == 4) {  // two int16 stereo frames (8 B): clamp, x32767, truncate (main.go:497-541)
            int32_t i0, i1, i2, i3;
            if constexpr (DITHER) {  // after the lane-pair swap: w[0], w[1] = channels 0, 1 of frame pos; w[2], w[3] of pos + 1
                const uint64_t n0 = static_cast<uint64_t>(pos), n1 = n0 + 1;
                const uint32_t key0 = ditherKey(x.dseedLo, x.dseedHi, 0), key1 = ditherKey(x.dseedLo, x.dseedHi, 1);  // uniform
                const uint32_t h0 = static_cast<uint32_t>(n0 >> 32), h1 = static_cast<uint32_t>(n1 >> 32);
                const uint32_t ka = ditherKeyHi(key0, h0), kb = ditherKeyHi(key1, h0);
                uint32_t kc = ka, kd = kb;
                if (h1 != h0) {  // the pair straddles a multiple of 2^32
                    kc = ditherKeyHi(key0, h1);
                    kd = ditherKeyHi(key1, h1);
                }
                const uint32_t l0 = static_cast<uint32_t>(n0), l1 = static_cast<uint32_t>(n1);
                i0 = pcmDitherOfF64(static_cast<double>(w[0]), 16, ditherNoise(ka, l0));
                i1 = pcmDitherOfF64(static_cast<double>(w[1]), 16, ditherNoise(kb, l0));
                i2 = pcmDitherOfF64(static_cast<double>(w[2]), 16, ditherNoise(kc, l1));
                i3 = pcmDitherOfF64(static_cast<double>(w[3]), 16, ditherNoise(kd, l1));
            } else {
                i0 = pcm16Of(w[0]); i1 = pcm16Of(w[1]); i2 = pcm16Of(w[2]); i3 = pcm16Of(w[3]);
            }
            uint2 v;
            v.x = (static_cast<uint32_t>(i0) & 0xffffu) | (static_cast<uint32_t>(i1) << 16);
            v.y = (static_cast<uint32_t>(i2) & 0xffffu) | (static_cast<uint32_t>(i3) << 16);
            *reinterpret_cast<uint2*>(p) = v;
        } else if constexpr (VST == 5) {  // two half stereo frames (8 B): one RNE each, no clamp
            uint2 v;
            if (x.out_pcm == kSampBF16) {
                v.x = static_cast<uint32_t>(halfOfF32(w[0], kSampBF16)) | (static_cast<uint32_t>(halfOfF32(w[1], kSampBF16)) << 16);
                v.y = static_cast<uint32_t>(halfOfF32(w[2], kSampBF16)) | (static_cast<uint32_t>(halfOfF32(w[3], kSampBF16)) << 16);
            } else {
                typedef _Float16 h2v_ __attribute__((ext_vector_type(2)));
                v.x = __builtin_bit_cast(uint32_t, h2v_{static_cast<_Float16>(w[0]), static_cast<_Float16>(w[1])});
                v.y = __builtin_bit_cast(uint32_t, h2v_{static_cast<_Float16>(w[2]), static_cast<_Float16>(w[3])});
            }
            *reinterpret_cast<uint2*>(p) = v;
        } else if (nt) {
            __builtin_nontemporal_store(w, reinterpret_cast<f32x4*>(p));
        } else {
            *reinterpret_cast<f32x4*>(p) = w;
        }
    } else if (VST == 1) {
        if (nt) __builtin_nontemporal_store(y, reinterpret_cast<f32x4*>(p));
        else *reinterpret_cast<f32x4*>(p) = y;
    } else if (VST == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float*>(p + i * x.out_fs) = y[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<double*>(p + i * x.out_fs) = static_cast<double>(y[i]);
    }
}

// The per-block protocol shared by both roles (identical barrier sequences).
// Loads j = 0 .. P + ngroups - 2 (hxsLoad: the P parts of stage 0, then stages 1 ..):
//   reset B | loaders issue loads 0 .. kHxsD-1 | B |
//   step j = 0 .. stepsPad - 1: loaders convert load j (registers -> ring) and issue load
//   j + kHxsD; compute waves run MFMA group j - P (when 0 <= j - P < ngroups: stage 0 and
//   stages 1 .. j - P are in the ring); B | [fixup]
// Steps of a block (P stage-0 parts + ngroups groups), padded to a multiple of kHxsD so the
// loaders' unrolled loop issues the same loads on every path.
__device__ __forceinline__ int hxsStepsPad(const HxsArgs& x) {
    const int GQ = x.G * x.Qc;
    const int n = (x.small ? 0 : (x.Wg + GQ - 1) / GQ) + x.ngroups;
    return (n + kHxsD - 1) / kHxsD * kHxsD;
}

struct HxsShared {
    unsigned long long* stamp;
    char* ring;
    uint32_t QS;
    int* loudLo;
    int* loudHi;
    int* flag;
};

// Register staging: loader l's items of load `st` -> ring rows, from the registers of its issue
// (fast) or gathered now (edge loads).
template <int FMT, class XP>
__device__ __forceinline__ void hxsRegConvert(XP x, const HxsStage& st, bool fast, const HxsRegBuf<FMT>& r,
                                              int b, int l, int lane, const HxsShared& sh) {
    const int p0 = uni(st.T0 % x->R);
    if (FMT != 0 && fast) {  // straight-line: registers -> ring
        int lq = l;  // opaque per call (hxsRegIssue)
        asm volatile("" : "+s"(lq));
#pragma unroll
        for (int k = 0; k < kHxsItems; ++k) {
            const int it = lq + k * kHxsLoaders, q = it & 3, i = it >> 2;
            if constexpr (FMT == 2) {
                const int row = 16 * it + (lane & 15);
                if (it < 4 * kHxsNP && 16 * it < st.nrow && row < st.nrow)
                    hxsPutItem(x, st, p0, lane >> 4, row, r.v[k], sh.ring, sh.QS, sh.loudLo, sh.loudHi, sh.flag);
            } else if constexpr (FMT == 7) {
                const int row = 16 * it + (lane & 15);
                if (it < 4 * kHxsNP && 16 * it < st.nrow && row < st.nrow) {
                    const f2v a = hxsHalf2(r.v[k].x, x->in_pcm), c = hxsHalf2(r.v[k].y, x->in_pcm);
                    hxsPutItem(x, st, p0, lane >> 4, row, f32x4{a.x, a.y, c.x, c.y}, sh.ring, sh.QS, sh.loudLo, sh.loudHi, sh.flag);
                }
            } else if (it < 4 * kHxsNP && 64 * i < st.nrow) {  // uniform
                f32x4 e;
                if constexpr (FMT == 1) {
                    e = f32x4{r.a[k].x, r.a[k].y, r.b[k].x, r.b[k].y};
                } else if constexpr (FMT == 3) {  // int16 pairs -> float64(i) * (1 / 32767) -> f32
                    const uint32_t ua = r.a[k], ub = r.b[k];
                    e = f32x4{static_cast<float>(pcmToF64(static_cast<int16_t>(ua & 0xffffu), 16)),
                              static_cast<float>(pcmToF64(static_cast<int16_t>(ua >> 16), 16)),
                              static_cast<float>(pcmToF64(static_cast<int16_t>(ub & 0xffffu), 16)),
                              static_cast<float>(pcmToF64(static_cast<int16_t>(ub >> 16), 16))};
                } else if constexpr (FMT == 6) {  // f16 / bf16 pairs: exact widening
                    const f2v a = hxsHalf2(r.a[k], x->in_pcm), c = hxsHalf2(r.b[k], x->in_pcm);
                    e = f32x4{a.x, a.y, c.x, c.y};
                } else {  // FMT 4: int32 pairs (PCM24 / PCM32)
                    const int bits = x->in_pcm;
                    e = f32x4{static_cast<float>(pcmToF64(static_cast<int32_t>(r.a[k].x), bits)),
                              static_cast<float>(pcmToF64(static_cast<int32_t>(r.a[k].y), bits)),
                              static_cast<float>(pcmToF64(static_cast<int32_t>(r.b[k].x), bits)),
                              static_cast<float>(pcmToF64(static_cast<int32_t>(r.b[k].y), bits))};
                }
                const int row = 64 * i + lane;
                if (row < st.nrow) hxsPutItem(x, st, p0, q, row, e, sh.ring, sh.QS, sh.loudLo, sh.loudHi, sh.flag);
            }
        }
        return;
    }
    const HxsArgsP xc = hxsCold();
    const SrcDesc src = kload(&xc->src);
#pragma unroll 1
    for (int k = 0; k < kHxsItems; ++k) {
        const int it = l + k * kHxsLoaders, q = it & 3, i = it >> 2;
        const int row = 64 * i + lane;
        if (it >= 4 * kHxsNP || 64 * i >= st.nrow) break;  // uniform (items ascend in i)
        if (row >= st.nrow) continue;
        f32x4 e;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int col = b * 16 + 4 * q + n;
            const int kk = col / x->C, c = col - kk * x->C;
            e[n] = col < x->ncols ? hxsGather(src, hxsChunkRow(x, kk, st.T0 + row), c, x->A) : 0.f;
        }
        hxsPutItem(x, st, p0, q, row, e, sh.ring, sh.QS, sh.loudLo, sh.loudHi, sh.flag);
    }
}

// History keep for the next call (launchGather's job, folded into this launch): hdst is the other
// buffer of the double-buffered history, so it never aliases what the launch reads.  Large launches:
// every thread after its role; small launches: the loader waves during the MFMA step (hxsRegLoadersT).
__device__ __forceinline__ void hxsHistKeep(const HxsArgs& x, int64_t me, int64_t nth) {
    const HxsArgsP xc = hxsCold();
    const SrcDesc src = kload(&xc->src);
    const int64_t total = x.hn * x.C;
    for (int64_t i = me; i < total; i += nth) {
        const int64_t t = i / x.C;
        x.hdst[i] = srcRead<float>(src, x.ht0 + t, static_cast<int>(i - t * x.C));
    }
}

// ---- hxq_kernel: small launches of f32 STEREO / ROW16 input over many workgroups ----------------
// A 4096-frame stereo call is 28 macro periods x 2 channels = 56 columns = 4 blocks: on
// hxs_small_kernel that is 4 workgroups, each gathering its whole window and running all row
// blocks.  Here workgroup (b, g) runs row blocks [g*qRbs, (g+1)*qRbs) of block b (qRbs = 1: 40
// workgroups for the stereo call): its waves load only the union of those row blocks' windows,
// every row -- history seam and flush tail included -- through buffer loads (input and history
// resources, per-lane selection, zeros past both), split it into the same f16 image and run the
// same MFMA order and epilogue (hxsSmallOut): identical bits to hxs_small_kernel / hxs_kernel.
constexpr int kHxqMaxWaves = 12;
constexpr int kHxqB = 6;  // items per wave in flight (4 waves: 24 items, a 5-6 piece window in one round trip)

struct HxqSrc {
    __amdgpu_buffer_rsrc_t in, hist;
    int64_t Tb;           // absolute row of the block's first chunk, row 0
    int64_t fastLo, fastHi, hb, hlen, vend;
    int rowB, hld;        // input row bytes, history row stride (elements)
    bool useH;            // the block's window reaches into the history
};

// Sources of absolute row T: the input (inI: row T - Tb of the input resource) or the history (inH:
// byte offset oh of element cH of its row); neither -> zeros.  Offsets past every record: 0x80000000.
constexpr int kHxqOob = static_cast<int>(0x80000000u);
__device__ __forceinline__ void hxqRow(const HxqSrc& q, int64_t T, int cH, bool& inI, bool& inH, int& oh) {
    const int64_t h = T - q.hb;
    inH = q.useH && T >= 0 && T < q.vend && h >= 0 && h < q.hlen;
    inI = !inH && T >= q.fastLo && T < q.fastHi;
    oh = inH ? (static_cast<int>(h) * q.hld + cH) * 4 : kHxqOob;
}

// Conversion of one item: row `row` of the image (column-relative row lo + row), quad q.
__device__ __forceinline__ void hxqPut(char* ring, uint32_t QS, uint32_t Rt, int q, int row, int t, f32x4 e, int* loudLo,
                                       int* loudHi, int* flag) {
    const bool l0 = hxLoud(e[0]), l1 = hxLoud(e[1]), l2 = hxLoud(e[2]), l3 = hxLoud(e[3]);
    if (__builtin_expect(l0 | l1 | l2 | l3, 0)) {
        if (l0) { atomicMin(loudLo + 4 * q, t); atomicMax(loudHi + 4 * q, t); e[0] = 0.f; }
        if (l1) { atomicMin(loudLo + 4 * q + 1, t); atomicMax(loudHi + 4 * q + 1, t); e[1] = 0.f; }
        if (l2) { atomicMin(loudLo + 4 * q + 2, t); atomicMax(loudHi + 4 * q + 2, t); e[2] = 0.f; }
        if (l3) { atomicMin(loudLo + 4 * q + 3, t); atomicMax(loudHi + 4 * q + 3, t); e[3] = 0.f; }
        *flag = 1;
    }
    uint2 hv, lv;
    hxSplit2(e[0], e[1], hv.x, lv.x);
    hxSplit2(e[2], e[3], hv.y, lv.y);
    char* qb = ring + q * QS + 8 * row;
    *reinterpret_cast<uint2*>(qb) = hv;
    *reinterpret_cast<uint2*>(qb + 8 * Rt) = lv;
}


// ---- clip / peak meter (gar.h gar_set_meter): what the metered inclusion of gar_hxs_body.inc adds ----------
// Argument block of the metered kernels: the plain block first -- hxsCold() reads it in place -- then the handle's
// tallies, so no kernel that exists without the meter sees a field move or its argument block grow.
struct HxsMeterArgs {
    HxsArgs x;
    uint64_t* meter;  // [C] x {clips, peak bits} (gar_meter.hpp)
};
__device__ __forceinline__ uint64_t* hxsMeterBuf() {
    return reinterpret_cast<const __attribute__((address_space(4))) HxsMeterArgs*>(hxsCold())->meter;
}
// A lane's tallies of the block it is storing: its own column's channel only (every lane tallies the rows of its
// own accumulator, before any lane-pair swap), published once per block by meterFlushWave.
struct HxsMeter {
    uint32_t clips = 0;
    uint64_t peak = 0;
    int lo = 0, hi = -1;  // the column's loud row range as of the last hxsMeterRange (hi < 0: none)
};
// The column's loud row range from the kernels' LDS (after the ring: smem + 4 * QS), read once per group, right
// after the barrier that released the group's MFMAs -- every row of the group's windows is marked by then, and
// later marks only widen the range -- so no LDS read (and no wait for one) sits among the MFMAs' fragment reads.
__device__ __forceinline__ void hxsMeterRange(const HxsArgs& x, HxsMeter& mt, int l16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int* loudLo = reinterpret_cast<const int*>(smem + 4 * (16 * static_cast<size_t>(x.Rt) + 64));
    mt.hi = loudLo[16 + l16];
    mt.lo = loudLo[l16];
}
// True when the fixup will rewrite output (period p of the column, row r; macro period a, channel c): its window
// meets the column's loud row range [lo, hi] as recorded so far AND really holds a loud element -- hxsFixup's own
// two tests.  Every row of the output's window was staged, and marked, before the barrier that released its MFMAs,
// and the range only grows during a block, so an output the fixup rewrites always passes here and one that passes
// here is rewritten: each sample is tallied once, with the value that stays in memory.
__device__ __forceinline__ bool hxsMeterLoud(HxsArgsP xp, int lo, int hi, int p, int r, int64_t a, int c) {
    const int w0 = p * xp->Qc + xp->ex.rowOff[r], w1 = w0 + xp->ex.rowLen[r];
    if (w1 <= lo || w0 > hi) return false;
    const SrcDesc src = kload(&xp->src);
    const int64_t t0 = a * xp->Qc + xp->ex.rowOff[r];
    bool loud = false;
    for (int kk = 0; kk < w1 - w0 && !loud; ++kk) loud = hxLoud(srcRead<float>(src, t0 + kk, c));
    return loud;
}
// The tally of the stored rows of a lane's accumulator (bit i of `rows`: y[i], row oRow0 + i of period p, macro
// period a), against the column's loud range of hxsMeterRange.
template <bool DITHER>
__device__ __forceinline__ void hxsMeterRows(const HxsArgs& x, HxsMeter& mt, const f32x4& y, int rows, int l16, int p, int64_t a,
                                             int64_t oRow0, int c) {
    const int hi = mt.hi, lo = mt.lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!((rows >> i) & 1)) continue;
        if (__builtin_expect(hi >= 0, 0) && hxsMeterLoud(hxsCold(), lo, hi, p, static_cast<int>(oRow0) + i, a, c)) continue;
        if constexpr (DITHER)
            meterTallyAt(static_cast<double>(y[i]), x.out_pcm, 1, x.dseedLo, x.dseedHi, static_cast<uint32_t>(c),
                         static_cast<uint64_t>(a * x.Pc + oRow0 + i + x.dpos), mt.clips, mt.peak);
        else
            meterTally(static_cast<double>(y[i]), x.out_pcm, false, 0.0, mt.clips, mt.peak);
    }
}
__device__ __forceinline__ void hxsMeterFlush(int ch, const HxsMeter& mt) {
    const int mCh[1] = {ch};
    const uint32_t mC[1] = {mt.clips};
    const uint64_t mP[1] = {mt.peak};
    meterFlushWave<1>(hxsMeterBuf(), mCh, mC, mP);
}
// The fixup's recomputed value, tallied on its way to hxsOutWrite (it is the value that stays in memory).
template <bool DITHER>
__device__ __forceinline__ float hxsMeterFixV(const OutDesc& od, int64_t o, int c, float v, HxsMeter& mt) {
    meterTallyAt(static_cast<double>(v), od.pcm, DITHER ? 1 : 0, od.dseedLo, od.dseedHi, static_cast<uint32_t>(c),
                 static_cast<uint64_t>(o - od.o0 + od.dpos0), mt.clips, mt.peak);
    return v;
}

// The storing half of the kernels: the meter's hooks empty (gar_hxs_body.inc)
#define GAR_HXS_M_KARG HxsArgs x
#define GAR_HXS_M_KPRO
#define GAR_HXS_M_DECL
#define GAR_HXS_M_STEP
#define GAR_HXS_M_ALSO_ROWS(p, a)
#define GAR_HXS_M_ROWS(p, a)
#define GAR_HXS_M_ROW(i, p, a)
#define GAR_HXS_M_FLUSH
#define GAR_HXS_M_FIX_BEGIN
#define GAR_HXS_M_FIXV(v) v
#define GAR_HXS_M_FIX_END
#include "gar_hxs_body.inc"
#undef GAR_HXS_M_KARG
#undef GAR_HXS_M_KPRO
#undef GAR_HXS_M_DECL
#undef GAR_HXS_M_STEP
#undef GAR_HXS_M_ALSO_ROWS
#undef GAR_HXS_M_ROWS
#undef GAR_HXS_M_ROW
#undef GAR_HXS_M_FLUSH
#undef GAR_HXS_M_FIX_BEGIN
#undef GAR_HXS_M_FIXV
#undef GAR_HXS_M_FIX_END

template <int NS, int VST, bool DITHER>
hipError_t hxsLaunchT(const HxsArgs& x, size_t lds, int64_t blocks, hipStream_t st, int qWaves) {
    if (x.small && x.qGroups > 0) {  // hxq_kernel: (block, row-block group) workgroups
        if (const size_t lim_ = setMaxLdsOnce(reinterpret_cast<const void*>(&hxq_kernel<NS, VST, DITHER>)); lim_ < lds) return ldsTooBig("hxq_kernel", lds, lim_);
        const int nw = std::min(kHxqMaxWaves, std::max(std::max(qWaves, 1), x.qRbs));  // waves per workgroup (HxsKnobs::hxqW)
        hipLaunchKernelGGL((hxq_kernel<NS, VST, DITHER>), dim3(static_cast<unsigned>(blocks * x.qGroups)), dim3(64 * nw), lds, st, x);
        return hipGetLastError();
    }
    if (x.small && !x.bigSmall) {
        if (const size_t lim_ = setMaxLdsOnce(reinterpret_cast<const void*>(&hxs_small_kernel<NS, VST, DITHER>)); lim_ < lds) return ldsTooBig("hxs_small_kernel", lds, lim_);
        hipLaunchKernelGGL((hxs_small_kernel<NS, VST, DITHER>), dim3(static_cast<unsigned>(blocks)), dim3(64 * x.nprog), lds, st, x);
        return hipGetLastError();
    }
    if (const size_t lim_ = setMaxLdsOnce(reinterpret_cast<const void*>(&hxs_kernel<NS, VST, DITHER>)); lim_ < lds) return ldsTooBig("hxs_kernel", lds, lim_);
    hipLaunchKernelGGL((hxs_kernel<NS, VST, DITHER>), dim3(static_cast<unsigned>(blocks)), dim3(64 * (x.nprog + kHxsLoaders)), lds, st, x);
    return hipGetLastError();
}
template <int NS, int VST>
hipError_t hxsLaunch(const HxsArgs& x, size_t lds, int64_t blocks, hipStream_t st, int qWaves) {
    return hxsLaunchT<NS, VST, false>(x, lds, blocks, st, qWaves);
}
// A launch with dither on (HxsArgs::dither; the store layouts that take integer PCM: VST 0 and 4): the DITHER
// instantiations of the three kernels, a build unit of their own (gar_hxs_i4.hip), so the others carry no dither code.
template <int NS, int VST>
hipError_t hxsLaunchDither(const HxsArgs& x, size_t lds, int64_t blocks, hipStream_t st, int qWaves) {
    return hxsLaunchT<NS, VST, true>(x, lds, blocks, st, qWaves);
}

// A launch with the meter on (integer PCM output: VST 0 and 4): the metered kernels, defined in their own build units
// only (gar_hxs_i5.hip / gar_hxs_i6.hip define GAR_HXS_METER_BUILD), so every other unit compiles what it always did.
// Same geometry as hxsLaunchT; the DITHER instantiation by x.dither.
template <int NS, int VST>
hipError_t hxsLaunchMeter(const HxsArgs& x, uint64_t* meter, size_t lds, int64_t blocks, hipStream_t st, int qWaves);
#ifdef GAR_HXS_METER_BUILD
// the second inclusion's functions and kernels under names of their own
#define hxsFixup hxsFixupM
#define hxsGroups hxsGroupsM
#define hxsCompute hxsComputeM
#define hxsRegLoadersT hxsRegLoadersTM
#define hxsRegLoaders hxsRegLoadersM
#define hxs_kernel hxs_meter_kernel
#define hxsSmallOut hxsSmallOutM
#define hxs_small_kernel hxs_small_meter_kernel
#define hxq_kernel hxq_meter_kernel
// in the hooks: x, y, lane, oRow0, ccol, colOk are the enclosing function's; mt its lane tallies
#define GAR_HXS_M_KARG HxsMeterArgs xm
#define GAR_HXS_M_KPRO const HxsArgs& x = xm.x;
#define GAR_HXS_M_DECL HxsMeter mt;
#define GAR_HXS_M_STEP hxsMeterRange(x, mt, lane & 15);
#define GAR_HXS_M_ALSO_ROWS(p, a) , hxsMeterRows<DITHER>(x, mt, y, 15, lane & 15, p, a, oRow0, ccol)
#define GAR_HXS_M_ROWS(p, a) hxsMeterRows<DITHER>(x, mt, y, 15, lane & 15, p, a, oRow0, ccol);
#define GAR_HXS_M_ROW(i, p, a) hxsMeterRows<DITHER>(x, mt, y, 1 << (i), lane & 15, p, a, oRow0, ccol);
#define GAR_HXS_M_FLUSH hxsMeterFlush(colOk ? ccol : -1, mt);
#define GAR_HXS_M_FIX_BEGIN HxsMeter mt;
#define GAR_HXS_M_FIXV(v) hxsMeterFixV<DITHER>(od, o, c, v, mt)
#define GAR_HXS_M_FIX_END hxsMeterFlush(c, mt);
#include "gar_hxs_body.inc"
#undef GAR_HXS_M_KARG
#undef GAR_HXS_M_KPRO
#undef GAR_HXS_M_DECL
#undef GAR_HXS_M_STEP
#undef GAR_HXS_M_ALSO_ROWS
#undef GAR_HXS_M_ROWS
#undef GAR_HXS_M_ROW
#undef GAR_HXS_M_FLUSH
#undef GAR_HXS_M_FIX_BEGIN
#undef GAR_HXS_M_FIXV
#undef hxsFixup
#undef hxsGroups
#undef hxsCompute
#undef hxsRegLoadersT
#undef hxsRegLoaders
#undef hxs_kernel
#undef hxsSmallOut
#undef hxs_small_kernel
#undef hxq_kernel
#undef GAR_HXS_M_FIX_END
template <int NS, int VST, bool DITHER>
hipError_t hxsLaunchMeterT(const HxsMeterArgs& a, size_t lds, int64_t blocks, hipStream_t st, int qWaves) {
    const HxsArgs& x = a.x;
    if (x.small && x.qGroups > 0) {
        if (const size_t lim_ = setMaxLdsOnce(reinterpret_cast<const void*>(&hxq_meter_kernel<NS, VST, DITHER>)); lim_ < lds) return ldsTooBig("hxq_meter_kernel", lds, lim_);
        const int nw = std::min(kHxqMaxWaves, std::max(std::max(qWaves, 1), x.qRbs));
        hipLaunchKernelGGL((hxq_meter_kernel<NS, VST, DITHER>), dim3(static_cast<unsigned>(blocks * x.qGroups)), dim3(64 * nw), lds, st, a);
        return hipGetLastError();
    }
    if (x.small && !x.bigSmall) {
        if (const size_t lim_ = setMaxLdsOnce(reinterpret_cast<const void*>(&hxs_small_meter_kernel<NS, VST, DITHER>)); lim_ < lds) return ldsTooBig("hxs_small_meter_kernel", lds, lim_);
        hipLaunchKernelGGL((hxs_small_meter_kernel<NS, VST, DITHER>), dim3(static_cast<unsigned>(blocks)), dim3(64 * x.nprog), lds, st, a);
        return hipGetLastError();
    }
    if (const size_t lim_ = setMaxLdsOnce(reinterpret_cast<const void*>(&hxs_meter_kernel<NS, VST, DITHER>)); lim_ < lds) return ldsTooBig("hxs_meter_kernel", lds, lim_);
    hipLaunchKernelGGL((hxs_meter_kernel<NS, VST, DITHER>), dim3(static_cast<unsigned>(blocks)), dim3(64 * (x.nprog + kHxsLoaders)), lds, st, a);
    return hipGetLastError();
}
template <int NS, int VST>
hipError_t hxsLaunchMeter(const HxsArgs& x, uint64_t* meter, size_t lds, int64_t blocks, hipStream_t st, int qWaves) {
    const HxsMeterArgs a{x, meter};
    return x.dither ? hxsLaunchMeterT<NS, VST, true>(a, lds, blocks, st, qWaves)
                    : hxsLaunchMeterT<NS, VST, false>(a, lds, blocks, st, qWaves);
}
#endif

#define GAR_HXS_FOR4(M, NS) M(NS, 0) M(NS, 1) M(NS, 2) M(NS, 3) M(NS, 4)
#if GAR_HXS_QUICK  // development A/B builds (tools/hxs_variant.sh): only the BASELINE plans' NS = 9, 10
#define GAR_HXS_FOR_LO(M) GAR_HXS_FOR4(M, 9)
#define GAR_HXS_FOR_HI(M) GAR_HXS_FOR4(M, 10)
#else
#define GAR_HXS_FOR_LO(M) GAR_HXS_FOR4(M, 1) GAR_HXS_FOR4(M, 2) GAR_HXS_FOR4(M, 3) GAR_HXS_FOR4(M, 4) GAR_HXS_FOR4(M, 5)
#define GAR_HXS_FOR_HI(M) GAR_HXS_FOR4(M, 6) GAR_HXS_FOR4(M, 7) GAR_HXS_FOR4(M, 8) GAR_HXS_FOR4(M, 9) GAR_HXS_FOR4(M, 10)
#endif
// VST 5 (half frame pairs): a build unit of its own (gar_hxs_i3.hip)
#if GAR_HXS_QUICK
#define GAR_HXS_FOR_HALF(M) M(9, 5) M(10, 5)
#else
#define GAR_HXS_FOR_HALF(M) M(1, 5) M(2, 5) M(3, 5) M(4, 5) M(5, 5) M(6, 5) M(7, 5) M(8, 5) M(9, 5) M(10, 5)
#endif
#define GAR_HXS_FOR_ALL(M) GAR_HXS_FOR_LO(M) GAR_HXS_FOR_HI(M) GAR_HXS_FOR_HALF(M)
#define GAR_HXS_INST(NS, V) template hipError_t hxsLaunch<NS, V>(const HxsArgs&, size_t, int64_t, hipStream_t, int);
#if GAR_HXS_QUICK
#define GAR_HXS_FOR_DITHER(M) M(9, 0) M(9, 4) M(10, 0) M(10, 4)
#else
#define GAR_HXS_FOR_DITHER(M) M(1, 0) M(1, 4) M(2, 0) M(2, 4) M(3, 0) M(3, 4) M(4, 0) M(4, 4) M(5, 0) M(5, 4) \
                              M(6, 0) M(6, 4) M(7, 0) M(7, 4) M(8, 0) M(8, 4) M(9, 0) M(9, 4) M(10, 0) M(10, 4)
#endif
// the metered instantiations, two build units: NS 1 .. 5 (gar_hxs_i5.hip) and 6 .. 10 (gar_hxs_i6.hip)
#if GAR_HXS_QUICK
#define GAR_HXS_FOR_METER_LO(M) M(9, 0) M(9, 4)
#define GAR_HXS_FOR_METER_HI(M) M(10, 0) M(10, 4)
#else
#define GAR_HXS_FOR_METER_LO(M) M(1, 0) M(1, 4) M(2, 0) M(2, 4) M(3, 0) M(3, 4) M(4, 0) M(4, 4) M(5, 0) M(5, 4)
#define GAR_HXS_FOR_METER_HI(M) M(6, 0) M(6, 4) M(7, 0) M(7, 4) M(8, 0) M(8, 4) M(9, 0) M(9, 4) M(10, 0) M(10, 4)
#endif
#define GAR_HXS_INST_METER(NS, V) template hipError_t hxsLaunchMeter<NS, V>(const HxsArgs&, uint64_t*, size_t, int64_t, hipStream_t, int);
#define GAR_HXS_INST_DITHER(NS, V) template hipError_t hxsLaunchDither<NS, V>(const HxsArgs&, size_t, int64_t, hipStream_t, int);

}  // namespace gar
