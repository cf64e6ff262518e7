// gar_hxs_geo.hpp -- the constants the streaming FIR kernels (gar_hxs.hpp, gar_hxt.hpp) share with
// their host-only launch planner (gar_hxs_launch.cpp): layout codes, wave and ring limits, LDS sizes.
// constexpr only: no device code, no HIP call, so host sources compiled as plain C++ include it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "gar_plan.hpp"

namespace gar {

// ---- load layouts (HxsArgs::fmt, template parameter FMT) ----------------------------------------
constexpr int kFmtGather = 0;       // any layout: per-column element gathers at conversion time
constexpr int kFmtStereo = 1;       // STEREO: interleaved f32 stereo frames, two chunks per quad (dwordx2)
constexpr int kFmtRow16 = 2;        // ROW16: rows of 16 contiguous f32 channels, four per quad (dwordx4)
constexpr int kFmtStereoPcm16 = 3;  // STEREO PCM16: interleaved int16 stereo frames (one dword each)
constexpr int kFmtStereoPcm32 = 4;  // STEREO PCM24 / PCM32: interleaved int32 stereo frames
constexpr int kFmtRow32 = 5;        // ROW32: hxt_kernel's 32-channel blocks of f32 rows (whole 128-B lines)
constexpr int kFmtStereoHalf = 6;   // STEREO half: interleaved f16 / bf16 stereo frames (one dword each)
constexpr int kFmtRow16Half = 7;    // ROW16 half: rows of 16 contiguous f16 / bf16 channels (32 B)
// ---- store layouts (HxsArgs::vst, template parameter VST; hxsStoreFast) --------------------------
constexpr int kVstAny = 0;          // any layout or type: the epilogue's checked per-element path
constexpr int kVstRows = 1;         // channel-contiguous f32 rows: four channels per 16-B store
constexpr int kVstStereo = 2;       // interleaved f32 stereo: frame pairs per 16-B store
constexpr int kVstF64 = 3;          // f64 output
constexpr int kVstStereoPcm16 = 4;  // interleaved int16 stereo: frame pairs per 8-B store
constexpr int kVstStereoHalf = 5;   // interleaved f16 / bf16 stereo: frame pairs per 8-B store

// ---- hxs_kernel ---------------------------------------------------------------------------------
#ifndef GAR_HXS_L
#define GAR_HXS_L 6
#endif
constexpr int kHxsLoaders = GAR_HXS_L;                  // loader waves per workgroup
constexpr int kHxsWaves = kHxRbMaxWaves + kHxsLoaders;  // __launch_bounds__ (4 waves per SIMD, 128 VGPRs)
#ifndef GAR_HXS_NP
#define GAR_HXS_NP 12
#endif
constexpr int kHxsNP = GAR_HXS_NP;                      // 64-row pieces per load (G*Qc <= 768: cfg2 G = 5)
constexpr int kHxsMaxG = 6;                             // periods per group (launcher: largest that fits)
// Development instrumentation (GAR_HXS_DBG attribution modes, GAR_HXS_PROF phase cycles): compiled
// in only with -DGAR_HXS_DEV=1 (tools/hxs_variant.sh); the production kernel carries none of it.
#ifndef GAR_HXS_DEV
#define GAR_HXS_DEV 0
#endif
constexpr bool kHxsDev = GAR_HXS_DEV != 0;
#ifndef GAR_HXS_QUICK
#define GAR_HXS_QUICK 0
#endif
// NS values with an instantiated kernel (GAR_HXS_QUICK development builds: only 9 and 10).
constexpr bool hxsNsBuilt(int ns) { return GAR_HXS_QUICK ? (ns == 9 || ns == 10) : (ns >= 1 && ns <= 10); }

// ---- hxt_kernel ---------------------------------------------------------------------------------
// NL loader waves (template parameter, 4 or 6) + up to 16 - NL compute waves, 16 waves at most.
constexpr int kHxtMaxComp = 12;                         // compute waves (3 per SIMD)
constexpr int kHxtWaves = 16;                           // __launch_bounds__: 16 waves, 128 VGPRs
constexpr int kHxtD = 2;                                // loads in flight per loader (register staging)
// 64-row pieces of one load (G*Qc <= 64 * pieces): 10 with 4 loaders, 12 with 6 (the registers
// of a loader's two loads in flight stay at 80 / 64 VGPRs)
constexpr int hxtPieces(int NL) { return NL >= 6 ? 12 : 10; }
// rows of one load: 64-row pieces, or the 8-row pieces of a 32-channel block dealt over NL loaders
constexpr int hxtMaxRowsF(int FMT, int NL) {
    return FMT == kFmtRow32 ? 8 * NL * ((4 * hxtPieces(NL) + NL - 1) / NL) : 64 * hxtPieces(NL);
}
// loader waves beside ncomp compute waves: six where they fit the 16-wave workgroup, else four
constexpr int hxtLoadersFor(int ncomp) { return ncomp + 6 <= kHxtWaves ? 6 : 4; }
constexpr int kHxtSlots = 16;                           // arrival slots per direction (progress counters)
// LDS bytes past loudLo (hxsLds reserves them): loudLo[16], loudHi[16], flag, then the counters
// (FMT 5: loudLo[32], loudHi[32], flag)
constexpr int kHxtSyncOff = 160;
constexpr int kHxtSyncOffWide = 288;
constexpr int kHxtSyncBytes = 4 * (2 * kHxtSlots + 1);

// hxsRingFor's geometry as constants: the lean loaders (gar_hxt.hpp) are compiled for one of these,
// and the planner dispatches them on an exact match.
template <int QC, int G_, int KREAD>
struct HxtGeo {
    static constexpr int Qc = QC, G = G_, Kread = KREAD, GQ = G_ * QC, Wg = (G_ - 1) * QC + KREAD;
    static constexpr int nslot = (Wg + GQ + GQ - 1) / GQ, R = nslot * GQ;
    static constexpr int mirror = Wg > GQ ? Wg - GQ : 0;
    static constexpr int Rt = (R + mirror + 15) / 16 * 16;
    static constexpr int P = (Wg + GQ - 1) / GQ;
    static constexpr uint32_t QS = 16u * Rt + 64u, dL = 8u * Rt;
    // first step (j - P) whose ring rows had an occupant, hxtFreeNeed: step i waits for group i - i0
    static constexpr int i0 = (R + 1 - Wg + GQ - 1) / GQ - 1;
    static_assert(Wg > GQ && mirror < GQ && P % kHxtD == 0 && i0 >= 0, "lean loaders: ring shape");
};
// Q24 44.1k -> 48k (Pc 160, Qc 147, Kread 420, ten row blocks of NS = 9 steps): G = 5 beside six
// loaders, G = 4 beside four (balanced roles)
template <int NL>
using HxtLeanGeo = HxtGeo<147, NL >= 6 ? 5 : 4, 420>;
constexpr int kHxtLeanPc = 160, kHxtLeanNS = 9, kHxtLeanNw = 10;

// ---- LDS and ring -------------------------------------------------------------------------------
constexpr size_t kHxsLdsMax = 160 * 1024;
// LDS bytes of an hxs launch: ring (four quads of hi + lo rows), loud ranges + flag, hxt_kernel's
// progress counters (kHxtSyncOff + kHxtSyncBytes, rounded up).
static_assert(kHxtSyncOff + kHxtSyncBytes <= 320, "hxt progress counters past the reserved LDS");
constexpr size_t hxsLds(int Rt) { return 4 * (16 * static_cast<size_t>(Rt) + 64) + 320; }
// hxt_kernel FMT 5 (32-channel blocks): eight quads, loudLo/Hi[32] + flag + the progress counters
static_assert(kHxtSyncOffWide + kHxtSyncBytes <= 448, "hxt FMT 5 progress counters past the reserved LDS");
constexpr size_t hxtLdsWide(int Rt) { return 8 * (16 * static_cast<size_t>(Rt) + 64) + 448; }

// Ring geometry of G periods per group: R ring rows, Rt rows incl. the mirror (rounded to 16 so
// the quad stride 16*Rt + 64 is 64 mod 256 B: the four quads of a transposed read land on
// distinct banks), Wg rows one group reads.
struct HxsRing { int R, Rt, Wg; };
constexpr HxsRing hxsRingFor(int Qc, int Kread, int G) {
    const int GQ = G * Qc, Wg = (G - 1) * Qc + Kread;
    const int R = (Wg + GQ + GQ - 1) / GQ * GQ;
    return {R, (R + std::max(0, Wg - GQ) + 15) / 16 * 16, Wg};
}
// Static LDS of hxs_kernel next to the dynamic ring: the development build's per-wave stamps.
constexpr size_t kHxsStaticLds = kHxsDev ? sizeof(unsigned long long) * kHxsWaves : 0;
constexpr bool hxsRingFits(int Qc, int G, int Rt) {
    return hxsLds(Rt) + kHxsStaticLds <= kHxsLdsMax && (G * Qc + 63) / 64 <= kHxsNP;
}

}  // namespace gar
