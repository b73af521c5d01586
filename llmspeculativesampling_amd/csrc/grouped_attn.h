// Grouped-query decode attention (decode, verify and stream-batched passes of a GQA model): one workgroup per (KV head, row
// group, key split) serves ALL G = Hq / Hkv query heads of its KV head, both products on the matrix cores, softmax online.
//
// attn_kernel (model_kernels.h) launches one workgroup per QUERY head: the G heads of a KV head stream the same K / V rows G
// times, its score MFMA runs with <= 8 of 16 query columns in use, P.V runs on the vector ALUs, and a chunk's score rows
// live in LDS, which bounds the context.  Here:
//   * Query tile.  The G heads x grp_n rows of the group are the rows of one tile: tile row r = h * grp_n + t is head
//     kvh * G + h, group row t (G <= 8, grp_n <= 8: <= 64 rows = NQT <= 4 MFMA column tiles; rows past G * grp_n are zero).
//     The causal limit of row r is the position of row t, so rows of one tile have different limits: the mask is per lane.
//   * Key split.  Workgroup z takes keys [z * chunk, (z + 1) * chunk) (chunk a multiple of 64, the same for every group of
//     the pass: sd_grouped_attn_plan), cut into 64-key blocks.  Wave w owns blocks w, w + 4, .. of the chunk and keeps its
//     own online-softmax state (running maximum, denominator, accumulators), so the key loop has no workgroup barrier; the
//     four waves merge once at the end.  Every K and V element of the chunk is read from memory once, by one wave.
//   * Scores.  S^T = K Q^T: A = 16 keys x 32 dims straight from the arena (attn_body's operand), B = Q^T held in registers
//     for the whole loop.  Lane l ends with score[key 16 kt + 4 (l >> 4) + j][row 16 qt + (l & 15)], j = 0..3.  Roundings
//     are attn_body's: rnd(acc [* k_scale]), Llama: rnd(. / sqrt(D)); masked entries -inf.
//   * Softmax.  Per block and row: the lane's maximum over its 16 scores, two cross-lane steps (lanes l, l ^ 16, l ^ 32
//     share a row), then m' = max(m, .), alpha = exp(m - m'), p = exp(s - m'), l = l * alpha + sum p (per lane; folded across
//     the four lanes once, after the loop), acc *= alpha.  All fp32; p is rounded to T for the product.
//   * P.V.  O^T = V^T P^T: the k-slot order of an MFMA is free while A and B agree, so the lane's p of key tiles 2 s, 2 s + 1
//     ARE the B operand of 32-key step s (slot 4 h + j of lane group g = key 32 s + 16 h + 4 g + j) - no cross-lane move.
//     A = V^T: the wave stages its block's V rows [key][dim] in its own LDS image and reads them back transposed with
//     ds_read_b64_tr_b16, in prefill_attn.h's slot order and row pitch (PA_VST: conflict-free).  The image is per wave, and
//     a wave's LDS operations execute in order, so a wave-level fence is all the loop needs.  fp8 values are widened to T
//     while staged (exact); v_scale multiplies the output.
//   * Loads.  None sits inside a branch (attn_body's comment on hipcc's waitcnt insertion): key indices are clamped to the
//     group's last visible key and tested at use.  A block's V rows are requested in front of its score MFMAs and land during the
//     softmax; the next block's K rows are requested in front of the P.V MFMAs.
//   * LDS does not grow with the context: 4 x 64 x PA_VST(D) bytes of V images + 2 KiB of merge state (+ 16 KiB of Q
//     operands at D = 128).  The merge reuses the
//     images: waves 2, 3 leave their accumulators for waves 0, 1, then wave 1 for wave 0, which stores.
//   * nsplit > 1: un-normalised sums, row maximum and denominator go to the partial buffer in attn_combine_kernel's layout
//     [(group, head)][split][ATT_TQ][D + 2]; that kernel merges and stores.  nsplit == 1 stores the output rows directly, in
//     the operand layout (xoff<T>).
// The transposed read needs EXEC all ones: every loop bound around it is per wave.
#pragma once
#include "prefill_attn.h"

#define GA_BLK 64                                   // keys per block (one wave's unit of work)
#define GA_MAX_QT 4                                 // 16-row tiles of the query tile (G * grp_n <= 64)
// dynamic LDS: the four V images, the merge state [2][4 waves][64 rows], and at D = 128 the Q operands of up to four tiles
static constexpr size_t ga_lds_bytes(int D) {
    return (size_t)4 * GA_BLK * PA_VST(D) + 2 * 4 * 64 * sizeof(float) + (D == 128 ? (size_t)GA_MAX_QT * 16 * D * 2 : 0);
}

__device__ __forceinline__ void ga_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float ga_xor_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}

template <typename T, int D, bool KV8, int NQT>
__device__ __forceinline__ void attn_grouped_body(const T *__restrict__ qbuf, const RowTab &tab, int layer, T *__restrict__ out, int Hq,
                                                  int Hkv, int arch, float inv_sqrt_d, int chunk, int nsplit,
                                                  float *__restrict__ partial, char *smem) {
    static_assert(D == 64 || D == 128, "output tiles of 16 dims, PA_VST's pitch");
    static_assert(sizeof(T) == 2, "16-bit models");
    using E = typename std::conditional<KV8, unsigned char, T>::type;      // arena element
    using E8 = typename std::conditional<KV8, uint2, u32x4>::type;         // 8 consecutive arena elements
    constexpr int VST = PA_VST(D), NDT = D / 16, NDK = D / 32, PPR = D / 8;
    const int kvh = blockIdx.x, bg = blockIdx.y, bz = blockIdx.z;
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = tid & 63;
    const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
    const int G = Hq / Hkv;
    const int r0 = tab.grp_row0[bg], nr = tab.grp_n[bg], strm = tab.grp_stream[bg], max_seq = tab.max_seq[strm];
    const int p0 = tab.grp_pos[bg];                               // position of the group's first row
    const int s_all = p0 + nr, s_last = s_all - 1;                // keys the group's last row sees; the last of them
    const int k_lo = bz * chunk, k_hi = min(s_all, k_lo + chunk); // this workgroup's keys (none: k_hi <= k_lo)
    const E *karena = (const E *)tab.kv_base[strm] + (size_t)layer * 2 * Hkv * max_seq * D;
    const E *K = karena + (size_t)kvh * max_seq * D, *V = karena + (size_t)(Hkv + kvh) * max_seq * D;
    float k_scale = 1.f, v_scale = 1.f;
    if constexpr (KV8) {
        k_scale = tab.kv_scale[strm][(size_t)layer * 2 * Hkv + kvh];
        v_scale = tab.kv_scale[strm][(size_t)layer * 2 * Hkv + Hkv + kvh];
    }
    char *vb = smem + (size_t)w * GA_BLK * VST;                    // this wave's V image [GA_BLK][VST]
    float *ms = reinterpret_cast<float *>(smem + (size_t)4 * GA_BLK * VST), *ls = ms + 4 * 64;    // [4 waves][64 rows]

    // ---- the lane's query rows: tile row 16 qt + i16 = head h, group row t; its last visible key; its operand
    int hrow[NQT], trow[NQT], lim[NQT];
    bool real[NQT];
    u32x4 qf[NQT][NDK];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        const int r = 16 * qt + i16;
        real[qt] = r < G * nr;
        hrow[qt] = real[qt] ? r / nr : 0;
        trow[qt] = real[qt] ? r - hrow[qt] * nr : 0;
        lim[qt] = p0 + trow[qt];
        const T *qr = qbuf + (size_t)(r0 + trow[qt]) * Hq * D + (size_t)(kvh * G + hrow[qt]) * D + g4 * 8;
#pragma unroll
        for (int dk = 0; dk < NDK; ++dk) {
            qf[qt][dk] = *reinterpret_cast<const u32x4 *>(qr + dk * 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) qf[qt][dk][i] = real[qt] ? qf[qt][dk][i] : 0u;   // rows past the tile are zero
        }
    }
    // 3 - 4 tiles of D = 128 with a 16-bit arena: Q (64 registers), K and V (64 each) and the accumulators do not all fit the
    // registers, so the Q operands live in LDS in operand order [tile][dk][lane]: wave 0 writes them, lane l of every wave reads
    // what wave 0's lane l wrote - right because qf depends on the lane alone, not on the wave
    constexpr bool Q_LDS = D == 128 && !KV8 && NQT > 2;
    u32x4 *qs = reinterpret_cast<u32x4 *>(ls + 4 * 64);
    if constexpr (Q_LDS) {
        if (w == 0) {
#pragma unroll
            for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
                for (int dk = 0; dk < NDK; ++dk) qs[(qt * NDK + dk) * 64 + lane] = qf[qt][dk];
        }
        __syncthreads();
    }
    auto q_op = [&](int qt, int dk) -> u32x4 {
        if constexpr (Q_LDS) return qs[(qt * NDK + dk) * 64 + lane];
        else return qf[qt][dk];
    };
    float m[NQT], l[NQT];
    f32x4 acc[NQT][NDT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        m[qt] = -INFINITY, l[qt] = 0.f;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) acc[qt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    E8 kf[4][NDK], vr[PPR];
    auto load_k = [&](int b0) {                                   // A operands of the block's four key tiles
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const E *kr = K + (size_t)min(b0 + 16 * kt + i16, s_last) * D + g4 * 8;
#pragma unroll
            for (int dk = 0; dk < NDK; ++dk) kf[kt][dk] = *reinterpret_cast<const E8 *>(kr + dk * 32);
        }
    };
    auto load_v = [&](int b0) {                                   // the block's V rows: piece = 8 elements, PPR pieces per key
#pragma unroll
        for (int i = 0; i < PPR; ++i) {
            const int piece = lane + 64 * i;
            vr[i] = *reinterpret_cast<const E8 *>(V + (size_t)min(b0 + piece / PPR, s_last) * D + (piece % PPR) * 8);
        }
    };

    const int b_first = k_lo + w * GA_BLK;
    load_k(b_first);
    for (int b0 = b_first; b0 < k_hi; b0 += 4 * GA_BLK) {         // (a per-wave bound)
        // ---- the block's A operands (fp8: widened once, exact), then per query tile: scores, online softmax - the MFMAs of
        // tile qt + 1 run under the softmax of tile qt.  The probabilities become the B operands of the two 32-key steps
        u32x4 ka[4][NDK];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int dk = 0; dk < NDK; ++dk) {
                if constexpr (KV8) ka[kt][dk] = fp8x8_to_16<T>(kf[kt][dk]);
                else ka[kt][dk] = kf[kt][dk];
            }
        asm volatile("" ::: "memory");                            // program order = queue order
        load_v(b0);                                               // lands during the softmax
        asm volatile("" ::: "memory");
        u32x4 pf[NQT][2];
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt) {
            f32x4 sc[4];
            u32x4 qo[NDK];
#pragma unroll
            for (int dk = 0; dk < NDK; ++dk) qo[dk] = q_op(qt, dk);
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dk = 0; dk < NDK; ++dk) sc[kt] = mfma16<T>(ka[kt][dk], qo[dk], sc[kt]);
            }
            float bm = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = b0 + 16 * kt + 4 * g4 + j;
                    float v = rnd<T>(KV8 ? sc[kt][j] * k_scale : sc[kt][j]);
                    if (arch == SD_ARCH_LLAMA) v = rnd<T>(v * inv_sqrt_d);
                    v = key <= lim[qt] && key < k_hi ? v : -INFINITY;
                    sc[kt][j] = v;
                    bm = fmaxf(bm, v);
                }
            const float mn = fmaxf(m[qt], ga_xor_max(bm));
            const float mz = mn == -INFINITY ? 0.f : mn;          // no visible key yet: exp(-inf - 0) = 0, not exp(-inf + inf)
            const float alpha = expf(m[qt] - mz);
            m[qt] = mn;
            float ps = 0.f;
            T ph[16];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = expf(sc[kt][j] - mz);
                    ps += p;
                    ph[4 * kt + j] = (T)p;
                }
            l[qt] = l[qt] * alpha + ps;
            pf[qt][0] = *reinterpret_cast<const u32x4 *>(ph);
            pf[qt][1] = *reinterpret_cast<const u32x4 *>(ph + 8);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) acc[qt][dt] *= alpha;
        }
        // ---- the block's V rows into the wave's image (the previous block's reads are behind: a wave's LDS operations
        // execute in order), then O^T += V^T P^T
        ga_wave_fence();
#pragma unroll
        for (int i = 0; i < PPR; ++i) {
            const int piece = lane + 64 * i;
            u32x4 vw;
            if constexpr (KV8) vw = fp8x8_to_16<T>(vr[i]);        // exact; from here on the 16-bit path's image
            else vw = vr[i];
            *reinterpret_cast<u32x4 *>(vb + (piece / PPR) * VST + (piece % PPR) * 16) = vw;
        }
        ga_wave_fence();
        load_k(b0 + 4 * GA_BLK);                                  // lands during P.V (past the chunk: clamped, never used)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                // lane 4 q4 + p4 of its 16-lane group addresses key row 16 h + 4 g4 + q4 of the step, dims 16 dt + 4 p4 .. + 3
                const char *va = vb + (size_t)(st * 32 + 4 * g4 + q4) * VST + (dt * 16 + 4 * p4) * 2;
                const pa_v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_v4s __attribute__((address_space(3))) *)(va));
                const pa_v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_v4s __attribute__((address_space(3))) *)(va + 16 * VST));
                u32x4 af;
                af[0] = ((const unsigned *)&a0)[0]; af[1] = ((const unsigned *)&a0)[1];
                af[2] = ((const unsigned *)&a1)[0]; af[3] = ((const unsigned *)&a1)[1];
#pragma unroll
                for (int qt = 0; qt < NQT; ++qt) acc[qt][dt] = mfma16<T>(af, pf[qt][st], acc[qt][dt]);
            }
    }

    // ---- merge the four waves: common maximum, rescale, then a two-level sum through the (now idle) V images
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        l[qt] += __shfl_xor(l[qt], 16);
        l[qt] += __shfl_xor(l[qt], 32);
        if (g4 == 0) { ms[w * 64 + 16 * qt + i16] = m[qt]; ls[w * 64 + 16 * qt + i16] = l[qt]; }
    }
    __syncthreads();
    float M[NQT], L[NQT];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        const int r = 16 * qt + i16;
        M[qt] = fmaxf(fmaxf(ms[r], ms[64 + r]), fmaxf(ms[128 + r], ms[192 + r]));
        const float mz = M[qt] == -INFINITY ? 0.f : M[qt];
        L[qt] = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) L[qt] += ls[u * 64 + r] * expf(ms[u * 64 + r] - mz);
        const float mine = expf(m[qt] - mz);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) acc[qt][dt] *= mine;
    }
    f32x4 *slot = reinterpret_cast<f32x4 *>(smem);                // [2][NQT * NDT][64 lanes]: <= 64 KiB of the 4 x 64 x VST
    auto put = [&](int s) {
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) slot[((size_t)s * NQT * NDT + qt * NDT + dt) * 64 + lane] = acc[qt][dt];
    };
    auto add = [&](int s) {
#pragma unroll
        for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) acc[qt][dt] += slot[((size_t)s * NQT * NDT + qt * NDT + dt) * 64 + lane];
    };
    if (w >= 2) put(w - 2);
    __syncthreads();
    if (w < 2) add(w);
    __syncthreads();
    if (w == 1) put(0);
    __syncthreads();
    if (w != 0) return;
    add(0);

    // ---- lane l holds out[row 16 qt + i16][dims 16 dt + 4 g4 .. + 3]
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        if (!real[qt]) continue;
        const int head = kvh * G + hrow[qt], t = trow[qt];
        if (nsplit > 1) {
            float *pz = partial + ((((size_t)bg * Hq + head) * nsplit + bz) * ATT_TQ + t) * (D + 2);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const f32x4 a = KV8 ? acc[qt][dt] * v_scale : acc[qt][dt];
                float2 *dst = reinterpret_cast<float2 *>(pz + dt * 16 + 4 * g4);      // ((D + 2) t is even: 8-byte aligned)
                dst[0] = float2{a[0], a[1]};
                dst[1] = float2{a[2], a[3]};
            }
            if (g4 == 0) { pz[D] = M[qt]; pz[D + 1] = L[qt]; }
        } else {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const f32x4 a = KV8 ? acc[qt][dt] * v_scale : acc[qt][dt];
                store4_maybe_wt<false>(out + xoff<T>(r0 + t, head * D + dt * 16 + 4 * g4, Hq * D), a[0] / L[qt], a[1] / L[qt],
                                       a[2] / L[qt], a[3] / L[qt]);
            }
        }
    }
}

// grid (Hkv, row groups, nsplit) x 256 threads, ga_lds_bytes(D) of dynamic LDS; chunk: keys per split (a multiple of GA_BLK)
template <typename T, int D, bool KV8>
__global__ __launch_bounds__(256) void attn_grouped_kernel(const T *__restrict__ qbuf, RowTab tab, int layer, T *__restrict__ out,
                                                          int Hq, int Hkv, int arch, float inv_sqrt_d, int chunk, int nsplit,
                                                          float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char ga_smem[];
    const int rows = (Hq / Hkv) * tab.grp_n[blockIdx.y];          // per workgroup: the tile count is uniform
    if (rows <= 16) attn_grouped_body<T, D, KV8, 1>(qbuf, tab, layer, out, Hq, Hkv, arch, inv_sqrt_d, chunk, nsplit, partial, ga_smem);
    else if (rows <= 32) attn_grouped_body<T, D, KV8, 2>(qbuf, tab, layer, out, Hq, Hkv, arch, inv_sqrt_d, chunk, nsplit, partial, ga_smem);
    else if (rows <= 48) attn_grouped_body<T, D, KV8, 3>(qbuf, tab, layer, out, Hq, Hkv, arch, inv_sqrt_d, chunk, nsplit, partial, ga_smem);
    else attn_grouped_body<T, D, KV8, 4>(qbuf, tab, layer, out, Hq, Hkv, arch, inv_sqrt_d, chunk, nsplit, partial, ga_smem);
}
