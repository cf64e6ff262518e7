// gar_hxs_body.inc -- the storing half of the streaming kernels (gar_hxs.hpp includes this text): the exact
// fallback, the compute and loader roles, and the three kernels hxs_kernel, hxs_small_kernel and hxq_kernel.
// Included once in namespace gar with the GAR_HXS_M_* hooks empty -- the kernels as they are without the meter,
// token for token -- and, in the metered build units only (GAR_HXS_METER_BUILD), a second time with the hooks defined
// and the names below renamed (hxs_meter_kernel, ...): the same kernels, tallying every integer PCM sample they store
// (gar.h gar_set_meter; the hooks and their functions are in gar_hxs.hpp).
//
// Rules for editing this text.  The hooks expand inside hxsFixup, hxsGroups (and its epilogue lambda), hxsSmallOut
// and the kernels, and use these locals of theirs by name: x, y, lane, oRow0, ccol, colOk (store paths); od, o, c
// (hxsFixup); xm (kernel argument).  Keep those names, keep every hook where its statement is (a hook after a store
// tallies exactly what that store wrote), and add no identifier that one of the second inclusion's renames
// (hxsFixup, hxsGroups, hxsCompute, hxsRegLoadersT, hxsRegLoaders, hxsSmallOut, hxs_kernel, hxs_small_kernel,
// hxq_kernel) would capture by accident.  GAR_HXS_M_ALSO_ROWS follows an expression statement without braces and
// expands to `, call`: the comma keeps the plain inclusion's tokens unchanged.

// After a block: recompute (gar_bg.hpp firExact) every output whose window intersects a column's loud
// row range and really holds a loud element (all threads).  hxq_kernel restricts it to the output rows
// [r0, r1) of each period, its workgroup's row blocks: another workgroup owns -- and stores -- the others.
template <bool DITHER = false>
__device__ __forceinline__ void hxsFixup(HxsArgsP xp, int b, const int* loudLo, const int* loudHi, int r0 = 0,
                                         int r1 = INT_MAX) {
    const SrcDesc src = kload(&xp->src);
    const OutDesc od = kload(&xp->od);
    const int Pc = xp->Pc, Qc = xp->Qc, Np = xp->Np, C = xp->C, ncols = xp->ncols;
    const int nr = min(r1, Pc) - r0;
    const bool ranged = r0 != 0 || r1 != INT_MAX;  // a constant where inlined; a ranged call may hold no row (nr <= 0)
    const int64_t a_lo = xp->a_lo, a_hi = xp->a_hi;
    for (int j = 0; j < 16; ++j) {
        const int lo = loudLo[j], hi = loudHi[j];
        const int col = b * 16 + j;
        if (hi < 0 || col >= ncols || (ranged && nr <= 0)) continue;
        const int k = col / C, c = col - k * C;
        const int p0 = max(0, (lo - xp->Kread) / Qc), p1 = min(Np - 1, hi / Qc);
        const int n = (p1 - p0 + 1) * nr;
        GAR_HXS_M_FIX_BEGIN
        for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
            const int p = p0 + idx / nr, r = r0 + (idx - (idx / nr) * nr);
            const int64_t a = a_lo + static_cast<int64_t>(k) * Np + p;
            if (a >= a_hi) continue;
            const int64_t o = a * Pc + r;
            if (o < od.o_lo || o >= od.o_hi) continue;
            const int w0 = p * Qc + xp->ex.rowOff[r], w1 = w0 + xp->ex.rowLen[r];
            if (w1 <= lo || w0 > hi) continue;
            const int64_t t0 = a * Qc + xp->ex.rowOff[r];
            bool loud = false;
            for (int kk = 0; kk < w1 - w0 && !loud; ++kk) loud = hxLoud(srcRead<float>(src, t0 + kk, c));
            if (loud)
                hxsOutWrite<DITHER>(od, o, c, GAR_HXS_M_FIXV(static_cast<float>(firExact<float>(&xp->ex, kload(&xp->src), xp->Qc, a, r, c).y)));
        }
        GAR_HXS_M_FIX_END
    }
}

// Compute waves (one row block each).
// Per block a wave decides once whether every period of its 16 columns is an interior, fully
// stored row block ("fast": the common case -- all but the launch's edge blocks); then the
// epilogue of a period is scale + (stereo) lane swap + one 16-B store at a pointer advanced by a
// constant per period, with no per-period range checks or 64-bit index arithmetic.
template <int NS, int VST, bool FAST, bool DITHER>
__device__ __forceinline__ void hxsGroups(const HxsArgs& x, const HxsShared& sh_, int lane, const h8v (&Ah)[NS],
                                          const h8v (&Al)[NS], uint32_t laneOff, int u0, int P, int nslot,
                                          char* obase, int64_t pstride, int64_t aCol, int64_t oRow0, bool colOk,
                                          int ccol, bool fullRb, unsigned long long& tm, unsigned long long& tw) {
    const int sh = -(x.ea + kHxXs);
    const int GQ = x.G * x.Qc;
    const uint32_t dL = 8u * static_cast<uint32_t>(x.Rt);
    const uint32_t pstep = 8u * static_cast<uint32_t>(x.Qc);
    const int dbg = kHxsDev ? x.dbg : 0;
    GAR_HXS_M_DECL
    auto epilogue = [&](const f32x4& oA, const f32x4& oL, int p) {
        const f32x4 y = hxScale(oA, oL, sh);
        if (dbg & 2) return;
        if constexpr (FAST) {
            // periods past the chunk (ngroups * G > Np) belong to the next chunk's column, whose
            // fixup owns their loud outputs: storing them here raced with it (r05 loud sweep, C=3)
            if (p < x.Np) hxsStoreFast<VST, DITHER>(x, obase + static_cast<int64_t>(p) * pstride, y, lane, (aCol + p) * x.Pc + oRow0 + ((lane & 1) ? 2 : 0) + x.dpos) GAR_HXS_M_ALSO_ROWS(p, aCol + p);
        } else {
            const int64_t a = aCol + p;
            const int64_t o0 = a * x.Pc + oRow0;
            const bool live = colOk && p < x.Np && a < x.a_hi;
            if (fullRb && live && (!x.out_pcm || VST == 4 || VST == 5) && a * x.Pc >= x.o_lo && (a + 1) * x.Pc <= x.o_hi) {
                char* pp = x.out + (o0 + (((VST == 2 || VST == 4 || VST == 5) && (lane & 1)) ? 2 : 0)) * x.out_fs + ((VST == 2 || VST == 4 || VST == 5) ? 0 : ccol * x.out_cs);
                hxsStoreFast<VST, DITHER>(x, pp, y, lane, o0 + ((lane & 1) ? 2 : 0) + x.dpos);
                GAR_HXS_M_ROWS(p, a)
            } else if (live) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t o = o0 + i;
                    if (oRow0 + i < x.Pc && o >= x.o_lo && o < x.o_hi) {
                        char* pp = x.out + o * x.out_fs + ccol * x.out_cs;
                        if constexpr (DITHER)  // integer PCM (hxsArgsOf)
                            pcmWriteDither(pp, 0, x.out_pcm, static_cast<double>(y[i]), x.dseedLo, x.dseedHi, static_cast<uint32_t>(ccol),
                                           static_cast<uint64_t>(o + x.dpos));
                        else if (x.out_pcm) pcmWrite(pp, 0, x.out_pcm, static_cast<double>(y[i]));
                        else if (x.out_f64) *reinterpret_cast<double*>(pp) = static_cast<double>(y[i]);
                        else *reinterpret_cast<float*>(pp) = y[i];
                        GAR_HXS_M_ROW(i, p, a)
                    }
                }
            }
        }
    };
    const int nstepsPad = hxsStepsPad(x);
    for (int j = 0; j < nstepsPad; ++j) {
        // load j -> ring (the loaders' share), then the MFMA periods of group j - P
        const unsigned long long t0 = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memtime() : 0;
        const int g = j - P;
        if (g < 0 || g >= x.ngroups) {
            hxsBarrier();
            continue;
        }
        const int slot = g % nslot;
        GAR_HXS_M_STEP
        uint32_t aH = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_s4p)(sh_.ring + laneOff))) +
                      8u * static_cast<uint32_t>(slot * GQ + u0);
        // B fragments read kPF steps ahead of their MFMAs (across period boundaries)
        constexpr int kPF = (NS >= 2 && GAR_HXS_PF2) ? 2 : 1;
        h8v bh0 = bFragA(aH), bl0 = bFragA(aH + dL);
        h8v bh1 = bh0, bl1 = bl0;
        if constexpr (kPF == 2) { bh1 = bFragA(aH + 256); bl1 = bFragA(aH + dL + 256); }
        // one period's MFMA program into nA (hi-x products) and nL (lo-x products); the
        // epilogue of period ep (oA, oL) issues after its second step when epi
        auto period = [&](f32x4& nA, f32x4& nL, const f32x4& oA, const f32x4& oL, bool epi, int ep, bool last) {
            asm volatile("" : "+v"(aH));  // opaque per-period base: reads use base + offset:imm
            uint32_t aL = aH + dL;
            asm volatile("" : "+v"(aL));  // lo reads: aL + offset:imm (hxt_kernel r05: -3 .. -6 %)
            const uint32_t aN = aH + pstep, aNL = aN + dL;
            nA = f32x4{0, 0, 0, 0};
            nL = nA;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int ug = (s + kPF) / NS, us = (s + kPF) % NS;
                h8v bhn = kPF == 2 ? bh1 : bh0, bln = kPF == 2 ? bl1 : bl0;
                if (!(ug == 1 && last)) {
                    bhn = bFragA((ug == 0 ? aH : aN) + 256 * us);
                    bln = bFragA((ug == 0 ? aL : aNL) + 256 * us);
                }
                nA = mfma16(Ah[s], bh0, nA);
                nA = mfma16(Al[s], bh0, nA);
                nL = mfma16(Ah[s], bl0, nL);
                if constexpr (kPF == 2) {
                    bh0 = bh1; bl0 = bl1; bh1 = bhn; bl1 = bln;
                } else {
                    bh0 = bhn; bl0 = bln;
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (s == (NS > 1 ? 1 : 0) && epi) epilogue(oA, oL, ep);
            }
            aH = aN;
        };
        const int p0 = g * x.G;
        f32x4 a0, a1 = {0, 0, 0, 0}, l0, l1 = a1;
        if (dbg & 4) {
            epilogue(a1, l1, p0);
            if (x.G > 1) epilogue(a1, l1, p0 + 1);
            if (x.G > 2) epilogue(a1, l1, p0 + 2);
        } else {
            // periods in pairs (alternating accumulators): period i's stores issue from
            // inside period i+1's MFMA stream
            period(a0, l0, a1, l1, false, 0, x.G == 1);
            int i = 1;
            for (; i + 1 < x.G; i += 2) {
                period(a1, l1, a0, l0, true, p0 + i - 1, false);
                period(a0, l0, a1, l1, true, p0 + i, i + 1 == x.G - 1);
            }
            if (i < x.G) {
                period(a1, l1, a0, l0, true, p0 + i - 1, true);
                epilogue(a1, l1, p0 + i);
            } else {
                epilogue(a0, l0, p0 + i - 1);
            }
        }
        const unsigned long long t1 = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memtime() : 0;
        hxsBarrier();  // step done: load j in the ring, load j + 1 landed
        if (kHxsDev && x.prof) { tm += t1 - t0; tw += __builtin_amdgcn_s_memtime() - t1; }
    }
    GAR_HXS_M_FLUSH
}

template <int NS, int VST, bool DITHER>
__device__ __forceinline__ void hxsCompute(const HxsArgs& x, const HxsShared& sh_, int wt, int lane) {
    const uint32_t QS = sh_.QS;
    const int GQ = x.G * x.Qc;
    const int grp = lane >> 4, l16 = lane & 15;
    const uint32_t laneOff = (l16 & 3) * QS + 8u * (4 * grp + (l16 >> 2));
    const int* pt = x.progs + kBgProgInts * wt;
    const int u0 = uni(pt[4]), rbw = uni(pt[3]);
    const int tid = wt * 64 + lane, nth = 64 * (x.nprog + kHxsLoaders);
    const unsigned long long tEntry = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memtime() : 0;
    unsigned long long tGath = 0, tSteps = 0;
    if constexpr (GAR_HXS_PRIO > 0) __builtin_amdgcn_s_setprio(GAR_HXS_PRIO);  // A/B: MFMA waves win VALU arbitration
    h8v Ah[NS], Al[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        Ah[s] = x.A[((static_cast<size_t>(wt) * NS + s) * 2 + 0) * 64 + lane];
        Al[s] = x.A[((static_cast<size_t>(wt) * NS + s) * 2 + 1) * 64 + lane];
    }
    unsigned long long tA = 0, tB1 = 0;
    if (kHxsDev && x.prof && wt == 0) {  // development: A landed (an extra wait, stamp only)
        __builtin_amdgcn_s_waitcnt(0);
        tA = __builtin_amdgcn_s_memtime();
    }
    const bool fullRb = (rbw + 1) * 16 <= x.Pc;
    const int nslot = x.R / GQ;
    unsigned long long tm = 0, tw = 0;
    const int P = x.small ? 0 : (x.Wg + GQ - 1) / GQ;
    const int64_t pstride = static_cast<int64_t>(x.Pc) * x.out_fs;

    for (int bi = blockIdx.x; bi < x.nblocks; bi += gridDim.x) {
        const int b = hxsBlock(x, bi);
        hxsBarrier();  // loud state reset; the previous block's ring reads done
        if (kHxsDev && x.prof && bi == static_cast<int>(blockIdx.x)) tB1 = __builtin_amdgcn_s_memtime();
        if (x.small) hxsSmallStage(&x, b, tid, nth, sh_.ring, QS, sh_.loudLo, sh_.loudHi, sh_.flag);
        hxsBarrier();  // load 0 landed (small: the whole window in the ring)
        if (kHxsDev && x.prof && bi == static_cast<int>(blockIdx.x)) tGath = __builtin_amdgcn_s_memtime();
        const int col = b * 16 + l16;
        const bool colOk = col < x.ncols;
        const int kcol = col / x.C, ccol = col - kcol * x.C;
        const int64_t aCol = x.a_lo + static_cast<int64_t>(kcol) * x.Np;
        const int64_t oRow0 = static_cast<int64_t>(rbw) * 16 + 4 * grp;  // first row of this lane's accumulator
        const bool laneFast = fullRb && colOk && (!x.out_pcm || VST == 4 || VST == 5) && aCol + x.Np <= x.a_hi &&
                              aCol * x.Pc >= x.o_lo && (aCol + x.Np) * x.Pc <= x.o_hi;
        char* obase = x.out + (aCol * x.Pc + oRow0 + (((VST == 2 || VST == 4 || VST == 5) && (lane & 1)) ? 2 : 0)) * x.out_fs +
                      ((VST == 2 || VST == 4 || VST == 5) ? 0 : ccol * x.out_cs);
        if (__builtin_amdgcn_ballot_w64(!laneFast) == 0)
            hxsGroups<NS, VST, true, DITHER>(x, sh_, lane, Ah, Al, laneOff, u0, P, nslot, obase, pstride, aCol, oRow0, colOk,
                                     ccol, fullRb, tm, tw);
        else
            hxsGroups<NS, VST, false, DITHER>(x, sh_, lane, Ah, Al, laneOff, u0, P, nslot, obase, pstride, aCol, oRow0, colOk,
                                      ccol, fullRb, tm, tw);
        if (kHxsDev && x.prof && bi == static_cast<int>(blockIdx.x)) tSteps = __builtin_amdgcn_s_memtime();
        if (*sh_.flag) {  // uniform (LDS after the barrier; reset only after the barrier below)
            __builtin_amdgcn_s_waitcnt(0);  // this wave's output stores landed
            __syncthreads();
            hxsFixup<DITHER>(hxsCold(), b, sh_.loudLo, sh_.loudHi);
            __syncthreads();  // every wave's fixup read loudLo/loudHi before the next block resets them
        }
    }
    if (kHxsDev && x.prof && wt == 0 && lane == 0) {  // development: first-block phase stamps of wave 0
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long tExit = __builtin_amdgcn_s_memtime();
        atomicAdd(x.prof + 20, tGath - tEntry);
        atomicAdd(x.prof + 21, tSteps - tGath);
        atomicAdd(x.prof + 22, tExit - tSteps);
        atomicAdd(x.prof + 23, 1ull);
        atomicAdd(x.prof + 24, tA - tEntry);
        atomicAdd(x.prof + 25, tB1 - tEntry);
        unsigned long long lo = ~0ull, hi = 0;
        for (int w = 0; w < x.nprog + kHxsLoaders; ++w) { lo = min(lo, sh_.stamp[w]); hi = max(hi, sh_.stamp[w]); }
        atomicAdd(x.prof + 26, hi - lo);
        atomicAdd(x.prof + 27, tEntry - lo);
    }
    if (kHxsDev && x.prof && lane == 0) {
        atomicAdd(x.prof + 4, tm);
        atomicAdd(x.prof + 5, tw);
        atomicAdd(x.prof + 6, 1ull);
    }
}

// Loader wave l: same barrier sequence as the compute
// waves; in step j it converts load j (issued kHxsD steps earlier) into the ring
// and issues load j + kHxsD into the registers just freed.
template <int FMT, bool DITHER>
__device__ __forceinline__ void hxsRegLoadersT(const HxsArgs& x, const HxsShared& sh_, int l, int lane) {
    // Every argument is read through an opaque kernarg pointer renewed per step (hxsCold), so
    // the scalar loads sit next to their uses instead of pinning ~70 SGPRs for the whole
    // kernel (spilled SGPRs cost a v_readlane per use inside the conversion).
    HxsArgsP xp = hxsCold();
    const int GQ = xp->G * xp->Qc;
    const int P = xp->small ? 0 : (xp->Wg + GQ - 1) / GQ, nL = xp->small ? 0 : P + xp->ngroups - 1;
    const int nstepsPad = hxsStepsPad(x);
    const int tid = (x.nprog + l) * 64 + lane, nth = 64 * (x.nprog + kHxsLoaders);
    for (int bi = blockIdx.x; bi < xp->nblocks; bi += gridDim.x) {
        const int b = hxsBlock(x, bi);
        if (l == 0 && lane < 16) { sh_.loudLo[lane] = INT_MAX; sh_.loudHi[lane] = -1; }
        if (l == 0 && lane == 0) *sh_.flag = 0;
        hxsBarrier();  // loud state reset; the previous block's ring reads done
        HxsRegBuf<FMT> buf[kHxsD];
        bool fastL[kHxsD];
        const HxsRegSrc rs = hxsRegSrc<FMT>(xp, b, lane);
#pragma unroll
        for (int d = 0; d < kHxsD; ++d) fastL[d] = hxsRegIssue<FMT>(hxsLoad(xp, b, d, P), d < nL, rs, l, buf[d]);
        if (xp->small) hxsSmallStage(xp, b, tid, nth, sh_.ring, sh_.QS, sh_.loudLo, sh_.loudHi, sh_.flag);
        hxsBarrier();  // (small: the whole window in the ring)
        for (int j0 = 0; j0 < nstepsPad; j0 += kHxsD) {
#pragma unroll
            for (int d = 0; d < kHxsD; ++d) {
                const int j = j0 + d;
                xp = hxsCold();
                const int dbg = kHxsDev ? xp->dbg : 0;
                if (xp->small && j == 0 && x.hn > 0 && bi == static_cast<int>(blockIdx.x))  // beside the MFMA group
                    hxsHistKeep(x, static_cast<int64_t>(blockIdx.x) * 64 * kHxsLoaders + 64 * l + lane,
                                static_cast<int64_t>(gridDim.x) * 64 * kHxsLoaders);
                if ((dbg & 64) && j >= P) {  // development: consume the registers, no conversion
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < kHxsItems; ++k) {
                        if constexpr (FMT == 2) s += buf[d].v[k][0] + buf[d].v[k][3];
                        else if constexpr (FMT == 1) s += buf[d].a[k].x + buf[d].b[k].y;
                        else if constexpr (FMT == 4) s += static_cast<float>(buf[d].a[k].x ^ buf[d].b[k].y);
                        else if constexpr (FMT == 3 || FMT == 6) s += static_cast<float>(buf[d].a[k] ^ buf[d].b[k]);
                        else if constexpr (FMT == 7) s += static_cast<float>(buf[d].v[k].x ^ buf[d].v[k].y);
                    }
                    if (s == 1234.5f) sh_.loudLo[0] = 0;
                } else if (j < nL && !((dbg & 16) && j >= P)) {
                    hxsRegConvert<FMT>(xp, hxsLoad(xp, b, j, P), fastL[d], buf[d], b, l, lane, sh_);
                }
                if (!(dbg & 128))  // development: no issue at all (the skeleton's cost without dummy loads)
                    fastL[d] = hxsRegIssue<FMT>(hxsLoad(xp, b, j + kHxsD, P), j + kHxsD < nL && !((dbg & 1) && j >= P), rs,
                                                l, buf[d]);
                hxsBarrier();  // step done: load j in the ring
            }
        }
        if (*sh_.flag) {  // same sequence as the compute waves
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            hxsFixup<DITHER>(hxsCold(), b, sh_.loudLo, sh_.loudHi);
            __syncthreads();
        }
    }
}

template <bool DITHER>
__device__ __forceinline__ void hxsRegLoaders(const HxsArgs& x, const HxsShared& sh_, int l, int lane) {
#ifdef GAR_HXS_ONLYFMT  // development: one loader format per build (register-allocation studies)
    hxsRegLoadersT<GAR_HXS_ONLYFMT, DITHER>(x, sh_, l, lane);
    return;
#endif
    if (x.fmt == 1) hxsRegLoadersT<1, DITHER>(x, sh_, l, lane);
    else if (x.fmt == 2) hxsRegLoadersT<2, DITHER>(x, sh_, l, lane);
    else if (x.fmt == 3) hxsRegLoadersT<3, DITHER>(x, sh_, l, lane);
    else if (x.fmt == 4) hxsRegLoadersT<4, DITHER>(x, sh_, l, lane);
    else if (x.fmt == 6) hxsRegLoadersT<6, DITHER>(x, sh_, l, lane);
    else if (x.fmt == 7) hxsRegLoadersT<7, DITHER>(x, sh_, l, lane);
    else hxsRegLoadersT<0, DITHER>(x, sh_, l, lane);
}

template <int NS, int VST, bool DITHER = false>
__global__ __launch_bounds__(64 * kHxsWaves) void hxs_kernel(GAR_HXS_M_KARG) {
    GAR_HXS_M_KPRO
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    HxsShared s;
#if GAR_HXS_DEV
    __shared__ unsigned long long hxsStamp[kHxsWaves];  // development (GAR_HXS_PROF): wave entry times
    if (x.prof && (threadIdx.x & 63) == 0) hxsStamp[threadIdx.x >> 6] = __builtin_amdgcn_s_memtime();
    s.stamp = hxsStamp;
#else
    s.stamp = nullptr;
#endif
    s.QS = 16u * static_cast<uint32_t>(x.Rt) + 64u;  // quad: hi rows, lo rows, +64 B skew
    s.ring = reinterpret_cast<char*>(smem);
    s.loudLo = reinterpret_cast<int*>(smem + 4 * static_cast<size_t>(s.QS));
    s.loudHi = s.loudLo + 16;
    s.flag = s.loudHi + 16;
    const int lane = threadIdx.x & 63;
    const int wt = uni(threadIdx.x >> 6);
    // History keep for the next call (launchGather's job, folded into this launch; hdst is the other
    // buffer of the double-buffered history, so it never aliases what this launch reads).  Small
    // launches: the loader waves copy it while the compute waves run their MFMAs (the loaders' only
    // other work is the one-pass window gather); otherwise every thread after its role.
    if (wt < x.nprog) hxsCompute<NS, VST, DITHER>(x, s, wt, lane);
    else hxsRegLoaders<DITHER>(x, s, wt - x.nprog, lane);
    if (x.hn > 0 && !x.small) hxsHistKeep(x, static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x,
                                          static_cast<int64_t>(gridDim.x) * blockDim.x);
}

// One compute wave of a small launch (one macro period per column): NS steps of 3 MFMAs over the
// window image from LDS address aH (hi plane; lo plane at + dL), scale, store row block rbw of
// block b's 16 columns.  Shared by hxs_small_kernel and hxq_kernel: identical bits.
template <int NS, int VST, bool DITHER>
__device__ __forceinline__ void hxsSmallOut(const HxsArgs& x, uint32_t aH, uint32_t dL, const h8v* Ah, const h8v* Al, int b,
                                            int rbw, int lane, int sh) {
    const int grp = lane >> 4, l16 = lane & 15;
    GAR_HXS_M_DECL
    GAR_HXS_M_STEP
    f32x4 nA = {0, 0, 0, 0}, nL = nA;
    uint32_t aL = aH + dL;
    asm volatile("" : "+v"(aL));  // lo reads: aL + offset:imm
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const h8v bh = bFragA(aH + 256 * s), bl = bFragA(aL + 256 * s);
        nA = mfma16(Ah[s], bh, nA);
        nA = mfma16(Al[s], bh, nA);
        nL = mfma16(Ah[s], bl, nL);
    }
    const f32x4 y = hxScale(nA, nL, sh);
    const int col = b * 16 + l16;
    const bool colOk = col < x.ncols;
    const int kcol = col / x.C, ccol = col - kcol * x.C;
    const int64_t a = x.a_lo + static_cast<int64_t>(kcol) * x.Np;  // Np == 1: the column's one period
    const int64_t oRow0 = static_cast<int64_t>(rbw) * 16 + 4 * grp;
    const int64_t o0 = a * x.Pc + oRow0;
    const bool fullRb = (rbw + 1) * 16 <= x.Pc;
    const bool live = colOk && a < x.a_hi;
    // whole-period stores need both lanes of a stereo pair (same chunk: same condition)
    if (fullRb && live && (!x.out_pcm || VST == 4 || VST == 5) && a * x.Pc >= x.o_lo && (a + 1) * x.Pc <= x.o_hi) {
        char* pp = x.out + (o0 + (((VST == 2 || VST == 4 || VST == 5) && (lane & 1)) ? 2 : 0)) * x.out_fs +
                   ((VST == 2 || VST == 4 || VST == 5) ? 0 : ccol * x.out_cs);
        hxsStoreFast<VST, DITHER>(x, pp, y, lane, o0 + ((lane & 1) ? 2 : 0) + x.dpos);
        GAR_HXS_M_ROWS(0, a)
    } else if (live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t o = o0 + i;
            if (oRow0 + i < x.Pc && o >= x.o_lo && o < x.o_hi) {
                char* pp = x.out + o * x.out_fs + ccol * x.out_cs;
                if constexpr (DITHER)  // integer PCM (hxsArgsOf)
                    pcmWriteDither(pp, 0, x.out_pcm, static_cast<double>(y[i]), x.dseedLo, x.dseedHi, static_cast<uint32_t>(ccol),
                                   static_cast<uint64_t>(o + x.dpos));
                else if (x.out_pcm) pcmWrite(pp, 0, x.out_pcm, static_cast<double>(y[i]));
                else if (x.out_f64) *reinterpret_cast<double*>(pp) = static_cast<double>(y[i]);
                else *reinterpret_cast<float*>(pp) = y[i];
                GAR_HXS_M_ROW(i, 0, a)
            }
        }
    }
    GAR_HXS_M_FLUSH
}

// Launch (explicitly instantiated in gar_hxs_i*.hip).
// Small launches (x.small: stream chunks, flush tails -- one macro period per column): a compact
// kernel of compute waves only, so the launch runs a short, warm instruction stream instead of the
// streaming kernel's loader / ring / format machinery (whose cold code dominated a 4096-frame call).
// Same window image, same A fragments, same MFMA order and epilogue as hxs_kernel: identical bits.
//   all waves: gather the block's window [0, Wg) into the image (hxsSmallStage) | barrier |
//   wave w < nprog: row block w, NS steps of 3 MFMAs, scale, store | loud fixup | history keep.
template <int NS, int VST, bool DITHER = false>
__global__ __launch_bounds__(64 * kHxRbMaxWaves) void hxs_small_kernel(GAR_HXS_M_KARG) {
    GAR_HXS_M_KPRO
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t QS = 16u * static_cast<uint32_t>(x.Rt) + 64u;
    char* ring = reinterpret_cast<char*>(smem);
    int* loudLo = reinterpret_cast<int*>(smem + 4 * static_cast<size_t>(QS));
    int* loudHi = loudLo + 16;
    int* flag = loudHi + 16;
    const int lane = threadIdx.x & 63;
    const int wt = uni(threadIdx.x >> 6);
    const int grp = lane >> 4, l16 = lane & 15;
    const bool comp = wt < x.nprog;
    h8v Ah[NS], Al[NS];
    int u0 = 0, rbw = 0;
    if (comp) {  // A lands while the window is gathered
        const int* pt = x.progs + kBgProgInts * wt;
        u0 = uni(pt[4]);
        rbw = uni(pt[3]);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            Ah[s] = x.A[((static_cast<size_t>(wt) * NS + s) * 2 + 0) * 64 + lane];
            Al[s] = x.A[((static_cast<size_t>(wt) * NS + s) * 2 + 1) * 64 + lane];
        }
    }
    const uint32_t laneOff = (l16 & 3) * QS + 8u * (4 * grp + (l16 >> 2));
    const uint32_t dL = 8u * static_cast<uint32_t>(x.Rt);
    const int sh = -(x.ea + kHxXs);
    // history keep for the next call: the first kHk elements of this thread are read up front, so
    // their round trip overlaps the window gather's instead of following the MFMAs
    constexpr int kHk = 2;
    const int64_t hme = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t hnth = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t htot = x.hn * x.C;
    float hk[kHk];
    if (x.hn > 0) {
        const HxsArgsP xc = hxsCold();
        const SrcDesc src = kload(&xc->src);
#pragma unroll
        for (int u = 0; u < kHk; ++u) {
            const int64_t i = hme + u * hnth;
            const int64_t t = i / x.C;
            hk[u] = i < htot ? hxsGather(src, x.ht0 + t, static_cast<int>(i - t * x.C), x.A) : 0.f;
        }
    }
    for (int b = blockIdx.x; b < x.nblocks; b += gridDim.x) {
        if (threadIdx.x < 16) { loudLo[threadIdx.x] = INT_MAX; loudHi[threadIdx.x] = -1; }
        if (threadIdx.x == 0) *flag = 0;
        __syncthreads();  // loud state reset; the previous block's image reads done
        if (!hxsSmallFast(&x, b, static_cast<int>(threadIdx.x), static_cast<int>(blockDim.x), ring, QS, loudLo, loudHi, flag))
            hxsSmallStage(&x, b, static_cast<int>(threadIdx.x), static_cast<int>(blockDim.x), ring, QS, loudLo, loudHi, flag);
        __syncthreads();  // the whole window in the image
        if (comp)
            hxsSmallOut<NS, VST, DITHER>(x, static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_s4p)(ring + laneOff))) + 8u * static_cast<uint32_t>(u0),
                                 dL, Ah, Al, b, rbw, lane, sh);
        if (*flag) {  // uniform (LDS after the barrier)
            __builtin_amdgcn_s_waitcnt(0);
            __syncthreads();
            hxsFixup<DITHER>(hxsCold(), b, loudLo, loudHi);
        }
        __syncthreads();  // every wave done with the image / loud state before the next block
    }
    if (x.hn > 0) {
#pragma unroll
        for (int u = 0; u < kHk; ++u)
            if (hme + u * hnth < htot) x.hdst[hme + u * hnth] = hk[u];
        if (htot > kHk * hnth) hxsHistKeep(x, hme + kHk * hnth, hnth);  // the rest (long histories)
    }
}

template <int NS, int VST, bool DITHER = false>
__global__ __launch_bounds__(64 * kHxqMaxWaves) void hxq_kernel(GAR_HXS_M_KARG) {
    GAR_HXS_M_KPRO
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t Rt = static_cast<uint32_t>(x.Rt), QS = 16u * Rt + 64u;
    char* ring = reinterpret_cast<char*>(smem);
    int* loudLo = reinterpret_cast<int*>(smem + 4 * static_cast<size_t>(QS));
    int* loudHi = loudLo + 16;
    int* flag = loudHi + 16;
    const int lane = threadIdx.x & 63;
    const int w = uni(threadIdx.x >> 6), nw = uni(blockDim.x >> 6);
    const unsigned long long tEntry = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memtime() : 0;
    const unsigned long long rEntry = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memrealtime() : 0;
    const int b = uni(blockIdx.x / x.qGroups);
    const int r0 = uni((blockIdx.x - b * x.qGroups) * x.qRbs);
    const int nrw = min(x.qRbs, x.nprog - r0);
    // union window [lo, lo + nrow) of the workgroup's row blocks (column-relative rows)
    int lo = INT_MAX, hi = 0;
    for (int i = 0; i < nrw; ++i) {
        const int u = x.qU0[r0 + i];
        lo = min(lo, u);
        hi = max(hi, u);
    }
    const int nrow = hi + 32 * NS - lo;
    const bool comp = w < nrw;
    h8v Ah[NS], Al[NS];
    int u0 = 0, rbw = 0;
    if (comp) {  // A lands while the window loads
        const int wt = r0 + w;
        u0 = x.qU0[wt];
        rbw = x.qRbw[wt];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            Ah[s] = x.A[((static_cast<size_t>(wt) * NS + s) * 2 + 0) * 64 + lane];
            Al[s] = x.A[((static_cast<size_t>(wt) * NS + s) * 2 + 1) * 64 + lane];
        }
    }
    const HxsArgsP xc = hxsCold();
    const SrcDesc src = kload(&xc->src);
    // load sources
    HxqSrc q;
    const int col0 = b * 16, kb = col0 / x.C, c0 = col0 - kb * x.C;
    const int chunkRows = x.Np * x.Qc;
    q.Tb = hxsChunkRow(&x, kb, 0);
    q.fastLo = x.fastLo;
    q.fastHi = x.fastHi;
    q.hb = src.hist_base;
    q.hlen = src.hist ? src.hist_len : 0;
    q.vend = src.valid_end;
    q.rowB = static_cast<int>(x.in_fs) * 4;
    q.hld = static_cast<int>(src.hist_ld);
    if (x.fmt == 0)  // per-lane checks guard every load (host: every offset < 2^31)
        q.in = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(x.in + q.Tb * x.in_fs * x.in_esz), 0, 0x7fffffff, 0x00020000);
    else
        q.in = hxsRsrcT(&x, q.Tb, x.fmt == 2 ? c0 : 0, x.fmt == 2 ? 64 : 8);
    {
        const int64_t hrows = min(q.hlen, q.vend - q.hb);
        const int64_t nb = hrows > 0 ? hrows * q.hld * 4 : 0;
        q.hist = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(src.hist), 0, static_cast<int>(nb < 0x7fffffff ? nb : 0x7fffffff),
                                                   0x00020000);
    }
    q.useH = q.hlen > 0 && q.Tb + lo < q.hb + q.hlen;  // uniform: some row of the block's window is history
    // history keep for the next call (rows [ht0, ht0 + hn) of the stream): the first kHk elements of
    // this thread up front, through buffer loads (vector-memory counter only: a flat load would also
    // hold every LDS wait and barrier of the window staging until it lands)
    constexpr int kHk = 2;
    const int64_t hme = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t hnth = static_cast<int64_t>(gridDim.x) * blockDim.x;
    const int64_t htot = x.hn * x.C;
    float hk[kHk];
    if (x.hn > 0 && !(x.qOpt & 2)) {  // variant: flat gathers
#pragma unroll
        for (int u = 0; u < kHk; ++u) {
            const int64_t i = hme + u * hnth;
            const int64_t t = i / x.C;
            hk[u] = i < htot ? hxsGather(src, x.ht0 + t, static_cast<int>(i - t * x.C), x.A) : 0.f;
        }
    }
    if (x.hn > 0 && (x.qOpt & 2)) {
        HxqSrc qk = q;
        qk.useH = q.hlen > 0;
        const __amdgpu_buffer_rsrc_t rk =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(x.in + x.ht0 * x.in_fs * x.in_esz), 0, 0x7fffffff, 0x00020000);
#pragma unroll
        for (int u = 0; u < kHk; ++u) {
            const int64_t i = hme + u * hnth;
            const int64_t t = i / x.C;
            const int c = static_cast<int>(i - t * x.C);
            bool inI, inH;
            int oh;
            hxqRow(qk, i < htot ? x.ht0 + t : -1, c, inI, inH, oh);
            const int oi = inI ? static_cast<int>((t * x.in_fs + static_cast<int64_t>(c) * x.in_cs) * x.in_esz) : kHxqOob;
            const float vi = x.in_esz == 8 ? static_cast<float>(__builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rk, oi, 0, 0)))
                                           : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rk, oi, 0, 0));
            const float vh = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(qk.hist, oh, 0, 0));
            hk[u] = inH ? vh : vi;
        }
    }
    // loud state reset, then a barrier before any conversion: placed after the first batch's loads
    // issue (every wave runs one batch at least), so the barrier overlaps their round trip
    auto loudReset = [&]() {
        if (threadIdx.x < 16) { loudLo[threadIdx.x] = INT_MAX; loudHi[threadIdx.x] = -1; }
        if (threadIdx.x == 0) *flag = 0;
        hxsBarrier();
    };
    unsigned long long tB1 = 0;
    const bool early = x.qOpt & 1;
    if (!early) { loudReset(); if (kHxsDev && x.prof) tB1 = __builtin_amdgcn_s_memtime(); }
    if (x.fmt == 1) {  // STEREO: item = (quad, 64-row piece), chunks 2q, 2q+1 of the block (both channels)
        const int nit = 4 * ((nrow + 63) >> 6);
        for (int it0 = w, first = 1; first || it0 < nit; it0 += kHxqB * nw) {
            f2v a[kHxqB], c[kHxqB], ah[kHxqB], ch[kHxqB];
            bool hA[kHxqB], hC[kHxqB];
#pragma unroll
            for (int u = 0; u < kHxqB; ++u) {
                const int it = it0 + u * nw, qd = it & 3, pc = it >> 2;
                const int t = lo + 64 * pc + lane;
                const bool on = it < nit && 64 * pc + lane < nrow;
                const int64_t T0 = q.Tb + static_cast<int64_t>(2 * qd) * chunkRows + t;
                int oh0, oh1;
                bool i0, i1;
                hxqRow(q, on ? T0 : -1, 0, i0, hA[u], oh0);
                hxqRow(q, on ? T0 + chunkRows : -1, 0, i1, hC[u], oh1);
                const int oi0 = i0 ? static_cast<int>(T0 - q.Tb) * q.rowB : kHxqOob;
                const int oi1 = i1 ? static_cast<int>(T0 + chunkRows - q.Tb) * q.rowB : kHxqOob;
                a[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(q.in, oi0, 0, 0));
                c[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(q.in, oi1, 0, 0));
                if (q.useH) {
                    ah[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(q.hist, oh0, 0, 0));
                    ch[u] = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(q.hist, oh1, 0, 0));
                }
            }
            if (first && early) { loudReset(); if (kHxsDev && x.prof) tB1 = __builtin_amdgcn_s_memtime(); }
            first = 0;
#pragma unroll
            for (int u = 0; u < kHxqB; ++u) {
                const int it = it0 + u * nw, pc = it >> 2, row = 64 * pc + lane;
                if (it < nit && row < nrow) {
                    const f2v va = (q.useH && hA[u]) ? ah[u] : a[u];
                    const f2v vc = (q.useH && hC[u]) ? ch[u] : c[u];
                    hxqPut(ring, QS, Rt, it & 3, row, lo + row, f32x4{va.x, va.y, vc.x, vc.y}, loudLo, loudHi, flag);
                }
            }
        }
    } else if (x.fmt == 0) {  // any other f32 / f64 layout: item = (quad, 64-row piece), one element load per column
        const int nit = 4 * ((nrow + 63) >> 6);
        const int esz = x.in_esz;
        for (int it0 = w, first = 1; first || it0 < nit; it0 += kHxqB * nw) {
            f32x4 v[kHxqB], vh[kHxqB];
            bool hV[kHxqB][4];
#pragma unroll
            for (int u = 0; u < kHxqB; ++u) {
                const int it = it0 + u * nw, qd = it & 3, pc = it >> 2;
                const int row = 64 * pc + lane;
                const bool on = it < nit && row < nrow;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int col = col0 + 4 * qd + n, k = col / x.C, c = col - k * x.C;  // wave-uniform
                    const int64_t dT = static_cast<int64_t>(k - kb) * chunkRows + lo + row;  // T - Tb
                    int oh;
                    bool inI;
                    hxqRow(q, on ? q.Tb + dT : -1, c, inI, hV[u][n], oh);
                    const int oi = inI ? static_cast<int>((dT * x.in_fs + static_cast<int64_t>(c) * x.in_cs) * esz) : kHxqOob;
                    if (esz == 8) v[u][n] = static_cast<float>(__builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(q.in, oi, 0, 0)));
                    else v[u][n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(q.in, oi, 0, 0));
                    if (q.useH) vh[u][n] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(q.hist, oh, 0, 0));
                }
            }
            if (first && early) { loudReset(); if (kHxsDev && x.prof) tB1 = __builtin_amdgcn_s_memtime(); }
            first = 0;
#pragma unroll
            for (int u = 0; u < kHxqB; ++u) {
                const int it = it0 + u * nw, row = 64 * (it >> 2) + lane;
                if (it < nit && row < nrow) {
                    f32x4 e = v[u];
                    if (q.useH) {
#pragma unroll
                        for (int n = 0; n < 4; ++n) e[n] = hV[u][n] ? vh[u][n] : e[n];
                    }
                    hxqPut(ring, QS, Rt, it & 3, row, lo + row, e, loudLo, loudHi, flag);
                }
            }
        }
    } else {  // ROW16: item = 16-row piece, lane = 16 quad + row: channels c0 + 4 quad .. + 3 of chunk kb
        const int nit = (nrow + 15) >> 4;
        const int qd = lane >> 4;
        for (int it0 = w, first = 1; first || it0 < nit; it0 += kHxqB * nw) {
            f32x4 v[kHxqB], vh[kHxqB];
            bool hV[kHxqB];
#pragma unroll
            for (int u = 0; u < kHxqB; ++u) {
                const int it = it0 + u * nw;
                const int row = 16 * it + (lane & 15);
                const bool on = it < nit && row < nrow;
                int oh;
                bool inI;
                hxqRow(q, on ? q.Tb + lo + row : -1, c0 + 4 * qd, inI, hV[u], oh);
                const int oi = inI ? (lo + row) * q.rowB + 16 * qd : kHxqOob;
                v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(q.in, oi, 0, 0));
                if (q.useH) vh[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(q.hist, oh, 0, 0));
            }
            if (first && early) { loudReset(); if (kHxsDev && x.prof) tB1 = __builtin_amdgcn_s_memtime(); }
            first = 0;
#pragma unroll
            for (int u = 0; u < kHxqB; ++u) {
                const int it = it0 + u * nw, row = 16 * it + (lane & 15);
                if (it < nit && row < nrow) hxqPut(ring, QS, Rt, qd, row, lo + row, (q.useH && hV[u]) ? vh[u] : v[u], loudLo, loudHi, flag);
            }
        }
    }
    hxsBarrier();  // the window image complete
    const unsigned long long tImg = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memtime() : 0;
    if (comp) {
        const int grp = lane >> 4, l16 = lane & 15;
        const uint32_t laneOff = (l16 & 3) * QS + 8u * (4 * grp + (l16 >> 2));
        hxsSmallOut<NS, VST, DITHER>(x, static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_s4p)(ring + laneOff))) + 8u * static_cast<uint32_t>(u0 - lo),
                             8u * Rt, Ah, Al, b, rbw, lane, -(x.ea + kHxXs));
    }
    if (*flag) {  // uniform (LDS after the barrier)
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        hxsFixup<DITHER>(hxsCold(), b, loudLo, loudHi, 16 * r0, 16 * (r0 + nrw));
    }
    const unsigned long long tOut = (kHxsDev && x.prof) ? __builtin_amdgcn_s_memtime() : 0;
    if (x.hn > 0) {
#pragma unroll
        for (int u = 0; u < kHk; ++u)
            if (hme + u * hnth < htot) x.hdst[hme + u * hnth] = hk[u];
        if (htot > kHk * hnth) hxsHistKeep(x, hme + kHk * hnth, hnth);
    }
    if (kHxsDev && x.prof && threadIdx.x == 0) {  // development: wave 0's phases, workgroup life, launch span
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long tEnd = __builtin_amdgcn_s_memtime(), rEnd = __builtin_amdgcn_s_memrealtime();
        atomicAdd(x.prof + 40, tB1 - tEntry);
        atomicAdd(x.prof + 41, tImg - tB1);
        atomicAdd(x.prof + 42, tOut - tImg);
        atomicAdd(x.prof + 43, tEnd - tOut);
        atomicAdd(x.prof + 44, 1ull);
        atomicMin(x.prof + 10, rEntry);
        atomicMax(x.prof + 11, rEnd);
        if (blockIdx.x < 4096) { x.prof[64 + 2 * blockIdx.x] = rEntry; x.prof[65 + 2 * blockIdx.x] = rEnd - rEntry; }
    }
}

