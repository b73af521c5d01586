// The balanced many-row GEMM (gemm_bf16_rows, rows_kernels.h) on 4-bit group-quantised weight records (q4.h), 1..80 rows:
//
//     part[sb][m][n] = sum_{k in slab sb} X[m][k] * w[n][k]        (or the fused QKV / activation epilogue when SB == 1)
//
// with w = bf16(s * (q - z)) decoded in registers.  The records kernels for <= 8 rows pay the decode (21 VALU operations
// per eight weights) once per MFMA; here a k-step's operand is decoded ONCE and meets MT m-tiles back to back, so the
// decode is paid per weight and the launch streams 4.25 bits where the bf16 kernel streams 16.
//
// What is gemm_bf16_rows': one workgroup of 16 waves per CU, n-tiles dealt to NG n-groups as evenly as integers allow, SB
// k-slabs; loader waves move the activation panel - already in MFMA fragment order - into a double-buffered LDS panel by
// LDS-DMA one chunk ahead; one workgroup barrier per chunk; the k-groups' accumulators folded through LDS in front of
// gemm_epilogue_fold.
//
// What is new is the weight side.  A record is four k-steps and is never split: the plan (q4_rows_plan, engine.hip) cuts
// slabs in whole records, the kernel cuts a slab's k-groups in whole records, and a chunk is CH = 4 or 8 k-steps, so every
// wave's k-range starts and ends on a record.  A compute wave owns one n-tile over one k-group and requests its records in
// bursts of Q4R_BURST: per record one 16-byte request and the 4-byte (s, z) dword per lane, at fixed addresses - 5 dwords
// where four bf16 tiles are 16, so a burst of 16 k-steps sits in the 20 registers in which the bf16 kernel holds 5.  The
// burst is multiplied when it has landed (the CU's other compute waves cover the wait); its first is requested in front
// of the first barrier.  A record past the wave's range is not requested: its registers are set to zero codes with a zero
// scale, which decode to a zero operand, and meet the panel tile the loader clamped (finite values).
#pragma once
#include "q4.h"
#include "rows_kernels.h"

#define Q4R_BURST 4                                          // records a compute wave requests together (16 k-steps)
#define Q4R_MAX_MT 5                                         // m-tiles of the widest instance (80 rows)

template <int MT, int EPI>
__global__ __launch_bounds__(GR_THREADS) void gemm_q4_rows(const unsigned *__restrict__ Wr, const u32x4 *__restrict__ Xp,
                                                          float *__restrict__ part, int M, int Mpad, int N, int K, int NG,
                                                          int ks_per_blk, int nwn, int nwk, int nld, GemmEpiT<bf16_t> e) {
    typedef bf16_t H;
    constexpr int CH = MT <= 2 ? 8 : 4;                           // k-steps per panel chunk: 2 x nwk x CH x MT KiB of LDS
    constexpr int RC = CH / 4;                                    // records per chunk
    constexpr int WBM = Q4R_BURST / RC;                           // chunks per burst
    extern __shared__ __attribute__((aligned(16))) char gr_smem[];
    // activation panel [2][kg][ck][mt][lane]; after the k-loop the same bytes hold the fold buffer [tile][kg][mt][lane]
    u32x4 (*xs)[CH][MT][64] = reinterpret_cast<u32x4 (*)[CH][MT][64]>(gr_smem);      // xs[buf * nwk + kg]
    f32x4 (*red)[MT][64] = reinterpret_cast<f32x4 (*)[MT][64]>(gr_smem);             // red[tile * nwk + kg]
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int NT = N >> 4, KS = K >> 5, KR = K >> 7;
    const int g = blockIdx.x % NG, sb = blockIdx.x / NG;
    const int t0 = (int)((long long)g * NT / NG), t1 = (int)((long long)(g + 1) * NT / NG);
    const int kb0 = sb * ks_per_blk, kb1 = min(KS, kb0 + ks_per_blk);               // both multiples of 4
    const int per = ((((kb1 - kb0) >> 2) + nwk - 1) / nwk) << 2;  // k-steps per k-group: whole records
    const int nch = (per + CH - 1) / CH;                          // chunks: the same count for every wave (barriers)
    const int ncomp = nwn * nwk;
    const int mt_valid = Mpad >> 4;                               // m-tiles the activation buffer really holds (<= MT)

    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ni = wv % nwn, kg = wv / nwn;                       // (meaningful for compute waves)
    const bool comp = wv < ncomp && t0 + ni < t1;
    const int ks0 = min(kb1, kb0 + kg * per), ks1 = min(kb1, ks0 + per);           // the k-group's range

    if (wv >= ncomp && wv < ncomp + nld) {
        // ---------------- loader: k-groups ld, ld + nld, ... (gemm_bf16_rows' loader) ----------------
        const int ld = wv - ncomp;
        auto dma = [&](int c, int buf) {
            for (int k2 = ld; k2 < nwk; k2 += nld) {
                const int ks0 = min(kb1, kb0 + k2 * per), ks1 = min(kb1, ks0 + per);
                if (ks0 >= ks1) continue;                         // (an empty k-group: its compute waves multiply nothing)
                const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane(
                    (int)(unsigned)(uintptr_t)&xs[buf * nwk + k2][0][0][0]);               // LDS byte address (wave-uniform)
#pragma unroll
                for (int ck = 0; ck < CH; ++ck) {
                    // a k-step past the range re-reads the last valid tile: finite values that meet a zero weight operand
                    const int ks = min(ks0 + c * CH + ck, ks1 - 1);
#pragma unroll
                    for (int t = 0; t < MT; ++t)                  // (an m-tile past the buffer re-reads its last one: rows >= M,
                        gr_glds16(Xp + ((size_t)min(t, mt_valid - 1) * KS + ks) * 64 + lane,     //  dropped by the epilogue)
                                  base + (unsigned)((ck * MT + t) * 1024));
                }
            }
        };
        dma(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (int c = 0; c < nch; ++c) {
            __syncthreads();                                      // compute(c - 1) is over: panel (c + 1) & 1 is free
            if (c + 1 < nch) {
                dma(c + 1, (c + 1) & 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // landed before this wave arrives at the next barrier
            }
        }
    } else if (comp && ks0 < ks1) {
        // ---------------- compute: tile t0 + ni, k-group kg (an EMPTY k-group has no panel: its waves idle below and
        // fold their zero accumulators) ----------------
        const int nr = (ks1 - ks0) >> 2;                          // records of this wave
        const unsigned *rp = Wr + ((size_t)(t0 + ni) * KR + min(ks0 >> 2, KR - 1)) * Q4_REC_DWORDS;
        Q4Rec w[Q4R_BURST];
        auto burst = [&](int r0) {
            if (r0 + Q4R_BURST <= nr) {                           // a whole burst: back-to-back requests, no branch between
#pragma unroll
                for (int u = 0; u < Q4R_BURST; ++u) w[u] = q4_fetch(rp + (size_t)(r0 + u) * Q4_REC_DWORDS, lane);
            } else {
#pragma unroll
                for (int u = 0; u < Q4R_BURST; ++u) {
                    w[u].c = u32x4{0u, 0u, 0u, 0u};               // zero codes, s = 0, z = 0: a zero operand
                    w[u].sz = 0u;
                    if (r0 + u < nr) w[u] = q4_fetch(rp + (size_t)(r0 + u) * Q4_REC_DWORDS, lane);
                }
            }
        };
        // the FIRST burst does not wait for the panel: records do not depend on the activations, so they are requested in
        // front of the first barrier and travel while the loader's first chunk lands
        burst(0);
        for (int cb = 0; cb < nch; cb += WBM) {
#pragma unroll
            for (int j = 0; j < WBM; ++j) {
                const int c = cb + j;
                if (c >= nch) break;                              // (wave-uniform, and the same for every wave: barriers)
                __syncthreads();                                  // chunk c's panel is in LDS
                if (j == 0 && c > 0) burst(c * RC);
                const int pbuf = (c & 1) * nwk + kg;
#pragma unroll
                for (int r = 0; r < RC; ++r) {
                    const Q4Rec &rec = w[j * RC + r];
                    const Q4Lane gc = q4_lane(rec.sz);            // once per record
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        u32x4 xf[MT];
#pragma unroll
                        for (int t = 0; t < MT; ++t) xf[t] = xs[pbuf][r * 4 + u][t][lane];
                        const u32x4 wk = q4_decode(rec.c[u], gc); // once per k-step, for MT MFMAs
#pragma unroll
                        for (int t = 0; t < MT; ++t) acc[t] = mfma16<H>(wk, xf[t], acc[t]);
                    }
                }
            }
        }
    } else {
        for (int c = 0; c < nch; ++c) __syncthreads();            // idle wave: keeps the barrier count
    }
    // ---- fold the k-groups' accumulators through LDS, then the epilogue (gemm_bf16_rows' tail): the workgroup's threads
    // are dealt (tile, m-tile, lane) items - EL per tile; a tile's nwk partial sums are added as ((k0 + k1) + (k2 + k3))
    __syncthreads();
    if (comp) {
#pragma unroll
        for (int t = 0; t < MT; ++t) red[ni * nwk + kg][t][lane] = acc[t];
    }
    __syncthreads();
    constexpr int EL = (EPI == EPI_ACT_SILU ? 32 : 64) * MT;      // threads one tile's epilogue takes (SiLU pairs gate / up lanes)
    for (int i = (int)threadIdx.x; i < nwn * EL; i += GR_THREADS) {
        const int g4 = i / EL, tile = t0 + g4;
        if (tile >= t1) continue;
        f32x4 (*rt)[MT][64] = red + (size_t)g4 * nwk;
        auto folded = [&](int pp, int l) -> f32x4 {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 s0 = rt[0][pp][l], s1 = nwk > 1 ? rt[1][pp][l] : z, s2 = nwk > 2 ? rt[2][pp][l] : z,
                        s3 = nwk > 3 ? rt[3][pp][l] : z;
            return (s0 + s1) + (s2 + s3);
        };
        gemm_epilogue_fold<MT, EPI, 1, MT, H>(folded, 0, part, M, Mpad, N, sb, tile, e, i - g4 * EL);
    }
}
