// gar_meter.hip -- the staged integer PCM stores with the clip / peak meter on (gar.h gar_set_meter): metered
// twins of convert_kernel and pack24_kernel (gar_kernels.hip), a build unit of their own so the unmetered kernels
// carry no meter code.  Same quantizers, same layout choice, same stored bytes; the dither mode is a run-time
// argument.  A thread's elements step by a multiple of C, so each of its tally slots stays on one channel for the
// whole launch and a wave publishes once, at the end (meterFlushWave: one atomic pair per channel at most).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gar_meter.hpp"

namespace gar {

__global__ __launch_bounds__(256) void convert_meter_kernel(const void* s, int st, int64_t sfs, int64_t scs, void* d, int dt,
                                                            int64_t dfs, int64_t dcs, int64_t n, int C, Dither dz, uint64_t* meter) {
    const int64_t total = n * C;
    const int64_t nth = static_cast<int64_t>(gridDim.x) * blockDim.x, step = nth - nth % C;  // launcher: nth >= C
    const int64_t me = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    const int ch[1] = {me < step ? static_cast<int>(me % C) : -1};
    uint32_t clips[1] = {0};
    uint64_t peak[1] = {0};
    if (me < step) {
        for (int64_t idx = me; idx < total; idx += step) {
            const int64_t t = idx / C;
            const int c = ch[0];  // idx = me (mod C)
            const int64_t se = t * sfs + c * scs, de = t * dfs + c * dcs;
            const double v = st >= kSampF16 ? pcmRead(s, se, st)
                                      : (st == 1 ? static_cast<const double*>(s)[se] : static_cast<double>(static_cast<const float*>(s)[se]));
            const uint64_t pos = static_cast<uint64_t>(dz.pos0 + t);
            if (dz.mode) pcmWriteDither(d, de, dt, v, dz.seedLo, dz.seedHi, static_cast<uint32_t>(c), pos);
            else pcmWrite(d, de, dt, v);
            meterTallyAt(v, dt, dz.mode, dz.seedLo, dz.seedHi, static_cast<uint32_t>(c), pos, clips[0], peak[0]);
        }
    }
    meterFlushWave<1>(meter, ch, clips, peak);
}

// pack24_kernel's quads and byte-wise tail: thread q0 takes quads q0, q0 + step, ... (step a multiple of C), so its
// slot k holds channel (4 q0 + k) % C throughout; the tail's samples 4 nq + k fall on the same slots.
template <class T>
__global__ __launch_bounds__(256) void pack24_meter_kernel(const T* s, uint8_t* d, int64_t total, int C, Dither dz, uint64_t* meter) {
    typedef T tx2 __attribute__((ext_vector_type(2)));
    typedef T tx4 __attribute__((ext_vector_type(4)));
    const int64_t nq = total >> 2;
    const int64_t nth = static_cast<int64_t>(gridDim.x) * blockDim.x, step = nth - nth % C;  // launcher: nth >= C
    const int64_t me = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
    int ch[4];
    uint32_t clips[4] = {0, 0, 0, 0};
    uint64_t peak[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) ch[k] = me < step ? static_cast<int>((4 * me + k) % C) : -1;
    if (me < step) {
        for (int64_t q = me; q <= nq; q += step) {
            if (q == nq) {  // checked tail
                for (int64_t e = 4 * nq; e < total; ++e) {
                    const int k = static_cast<int>(e - 4 * nq);
                    const int64_t t = e / C;
                    const double v = static_cast<double>(s[e]);
                    const uint64_t pos = static_cast<uint64_t>(dz.pos0 + t);
                    if (dz.mode) pcmWriteDither(d, e, kSampPcm24P, v, dz.seedLo, dz.seedHi, static_cast<uint32_t>(e - t * C), pos);
                    else pcmWrite(d, e, kSampPcm24P, v);
                    uint32_t cl = 0;
                    uint64_t pk = 0;
                    meterTallyAt(v, 24, dz.mode, dz.seedLo, dz.seedHi, static_cast<uint32_t>(e - t * C), pos, cl, pk);
#pragma unroll
                    for (int u = 0; u < 3; ++u)
                        if (u == k) { clips[u] += cl; peak[u] = pk > peak[u] ? pk : peak[u]; }
                }
                break;
            }
            T y[4];
            if constexpr (sizeof(T) == 4) {
                const tx4 v = *reinterpret_cast<const tx4*>(s + 4 * q);
                y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
            } else {
                const tx2 a = *reinterpret_cast<const tx2*>(s + 4 * q), b = *reinterpret_cast<const tx2*>(s + 4 * q + 2);
                y[0] = a.x; y[1] = a.y; y[2] = b.x; y[3] = b.y;
            }
            int32_t i[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t e = 4 * q + k, t = e / C;
                const double v = static_cast<double>(y[k]);
                const uint64_t pos = static_cast<uint64_t>(dz.pos0 + t);
                i[k] = dz.mode ? pcmDitherAt(v, 24, dz.seedLo, dz.seedHi, static_cast<uint32_t>(ch[k]), pos) : pcmOfF64(v, 24);
                meterTallyAt(v, 24, dz.mode, dz.seedLo, dz.seedHi, static_cast<uint32_t>(ch[k]), pos, clips[k], peak[k]);
            }
            uint32_t w[3];
            pcm24Pack4(i, w);
            *reinterpret_cast<u32x3a*>(d + 12 * q) = u32x3a{w[0], w[1], w[2]};
        }
    }
    meterFlushWave<4>(meter, ch, clips, peak);
}

hipError_t launchConvertMeter(const void* src, int s_type, int64_t s_fs, int64_t s_cs, void* dst, int d_type, int64_t d_fs,
                              int64_t d_cs, int64_t n, int C, hipStream_t stream, const Dither& dz, uint64_t* meter, bool packV) {
    if (n <= 0) return hipSuccess;
    const int64_t total = n * C;
    const int64_t minBlocks = (static_cast<int64_t>(C) + 255) / 256;  // at least C threads: a step that is a multiple of C
    if (packV) {  // launchConvert's test: contiguous packed 24-bit from a 4-byte aligned base, contiguous 16-B aligned f32 / f64
        int64_t vb = ((total >> 2) + 1 + 255) / 256;
        vb = std::max(std::min<int64_t>(vb, 65536), minBlocks);
        const dim3 g(static_cast<unsigned>(vb)), b(256);
        uint8_t* dp = static_cast<uint8_t*>(dst);
        if (s_type == 1) hipLaunchKernelGGL(pack24_meter_kernel<double>, g, b, 0, stream, static_cast<const double*>(src), dp, total, C, dz, meter);
        else hipLaunchKernelGGL(pack24_meter_kernel<float>, g, b, 0, stream, static_cast<const float*>(src), dp, total, C, dz, meter);
        return hipGetLastError();
    }
    int64_t blocks = (total + 255) / 256;
    blocks = std::max(std::min<int64_t>(blocks, 65536), minBlocks);
    hipLaunchKernelGGL(convert_meter_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, src, s_type, s_fs, s_cs, dst,
                       d_type, d_fs, d_cs, n, C, dz, meter);
    return hipGetLastError();
}

}  // namespace gar
