// gar_bg_geo.hpp -- what the banded-GEMM FIR kernels (gar_bg.hpp) share with their host-only launch
// planner (gar_bg_launch.cpp): the launch geometry a kernel receives, LDS sizes, the grid of the small
// launches.  POD and constexpr only: no device code, no HIP call, so host sources include it.
#pragma once
#include <cstddef>
#include <cstdint>

#include "gar_plan.hpp"

namespace gar {

constexpr size_t kBgStaticLds = 64;  // bg_kernel's static LDS (nfFlag), rounded up
constexpr int kBgProfWords = 64;

struct BgGrid {
    int Pc, Qc, Kc, W, Wl, Ws, G;
    int64_t a_lo;
    int nchunk, ncols, nblocks;
    int C, nprog, kch, nwt, ncg, nred, nslots, parity;
    int dbg;  // development timing knob (GAR_BG_DBG): 1 skip tile DMA after the first, 2 skip stores
    int vst;  // f32 epilogue: 0 scalar, 1 channel-contiguous (fs == 1), 2 stereo interleaved (C == 2, fs == 2, cs == 1)
    int rbMode;  // small launch of a row-block-aligned plan: 1 bg_rb_kernel, 2 bg_rt_kernel (G = 1)
    // bg_rb_kernel: program ranges and first input rows passed by value (kernarg), so a wave issues
    // its A and B loads without first loading its program from the tables
    int rbStart[kBgRbKMaxRb + 1];
    int rbK0[kBgRbKMaxProg];
    void* hdst;       // folded history keep (HistCopy): hdst[(t - ht0) * C + c] = src(t, c), t < ht0 + hn
    int64_t ht0, hn;
    unsigned long long* prof;  // development stamps (kBgDev), else null
};

// XCD-grouped item order of the small launches: workgroup slot bb runs item (group, member) with
// group = 8 (bb / 8 / M) + bb % 8 and member = (bb / 8) % M, so the M items that read the same
// input lines (the row blocks of one column block; the row blocks x channels of one time block) run
// on workgroup slots of one residue mod 8, i.e. on one XCD under the round-robin dispatch, and share
// its L2 (cfg5 decimator: each 64-B line of the 8-channel stream was fetched by 8 XCDs).  The grid
// is 8 M ceil(ngroups / 8) slots (a multiple of 8 also when capped); slots past the last group idle.
constexpr int64_t bgXcdSlots(int64_t ngroups, int64_t M) { return 8 * M * ((ngroups + 7) / 8); }

// bg_rt_kernel: LDS rows are padded by kRtPad(Qc) every Qc rows so the 16 columns of a B read (Qc
// rows apart) fall on distinct bank pairs; bgRtLds: the union window of 16 macro periods + the
// programs' partial slots.
constexpr int kRtPad(int Qc) { return ((2 - Qc) % 32 + 32) % 32; }  // (Qc + pad) % 32 == 2
constexpr size_t bgRtLds(int Qc, int Kread, int nprog, size_t esz) {
    const int nrow = 15 * Qc + Kread;
    const size_t win = (static_cast<size_t>(nrow) + static_cast<size_t>(kRtPad(Qc)) * (nrow / Qc + 1)) * esz;
    return (win + 15) / 16 * 16 + static_cast<size_t>(nprog) * 64 * 4 * esz;
}

}  // namespace gar
