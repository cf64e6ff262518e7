// gar_meter.hpp -- device side of the clip / peak meter (gar.h gar_set_meter): publishing a wave's tallies.
// The tally of one sample is meterTally (gar_kernels.hpp); a store path keeps (clips, peak bits) per lane in
// registers and publishes them here, once per block (the streaming kernels) or per launch (the staged kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "gar_kernels.hpp"

namespace gar {

// The handle's tallies: meter[2 * c] = clips of channel c, meter[2 * c + 1] = bits of its peak.
// Every lane of the wave calls this (converged) with K slots: slot k holds the tallies of channel ch[k] (-1: none).
// Slots of equal channel, in any lane, are reduced by __shfl_xor; the first lane holding a channel then issues
// at most one atomicAdd (clips != 0) and one atomicMax (peak above what memory holds: the word only grows
// between resets, so a smaller or equal peak has nothing to publish) -- per channel the wave stored.
template <int K>
__device__ inline void meterFlushWave(uint64_t* meter, const int (&ch)[K], const uint32_t (&clips)[K], const uint64_t (&peak)[K]) {
    const int lane = static_cast<int>(__lane_id());
    bool any[K];
    bool anyL = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        any[k] = ch[k] >= 0 && (clips[k] != 0 || peak[k] != 0);
        anyL = anyL || any[k];
    }
    unsigned long long todo = __ballot(anyL);
    while (todo) {  // uniform: one round per distinct channel
        const int leader = __ffsll(todo) - 1;
        int mine = -1;
#pragma unroll
        for (int k = K - 1; k >= 0; --k) mine = any[k] ? ch[k] : mine;  // the leader's first live slot
        const int lc = __shfl(mine, leader);
        uint32_t c = 0;
        unsigned long long p = 0;
        bool left = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (any[k] && ch[k] == lc) {
                c += clips[k];
                p = peak[k] > p ? peak[k] : p;
                any[k] = false;
            }
            left = left || any[k];
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            c += __shfl_xor(c, off);
            const unsigned long long q = __shfl_xor(p, off);
            p = q > p ? q : p;
        }
        if (lane == leader) {
            unsigned long long* m = reinterpret_cast<unsigned long long*>(meter) + 2 * static_cast<size_t>(lc);
            if (c) atomicAdd(m, static_cast<unsigned long long>(c));
            if (p > m[1]) atomicMax(m + 1, p);
        }
        todo = __ballot(left);
    }
}

}  // namespace gar
