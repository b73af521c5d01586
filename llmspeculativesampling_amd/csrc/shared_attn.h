// Shared-prefix attention (stream-batched decode and verify passes whose streams all hold copies of one prompt prefix): the
// first cross-stream attention launch.  The prefix's K / V rows are read from ONE arena - the donor's, which every stream's
// rows [0, P) were copied from - once per 64-row query tile of the whole pass instead of once per stream.
//
// attn_kernel and attn_grouped_kernel serve one stream's rows against one stream's arena: a pass over n streams streams the
// same P prefix rows n times, and on an MHA model a stream's <= 8 rows fill 8 of an MFMA's 16 query columns.  Here one
// launch holds workgroups of two roles, uniform per workgroup (a 1-D grid, prefix workgroups first: they are the long ones):
//   * Prefix workgroup = (prefix split z, KV head, query tile), the tile fastest in launch order so that the tiles of one
//     (KV head, split) - which read the same K / V rows - start next to each other.  The pass's G * n_rows rows of the KV head
//     (G = Hq / Hkv in 1..8, n_rows <= 80: <= 640 rows, <= 10 tiles) are numbered R = m * G + h (pass row m, head kvh * G + h);
//     tile i takes R in [64 i, 64 i + 64), rows past the end are zero.  Keys [z * chunk_p, min(P, (z + 1) * chunk_p)) of the
//     donor arena.  Every row of the pass sits at a position >= P, so the loop has NO causal mask: only the range end bounds
//     the keys, and the lane keeps no per-row limit.
//   * Suffix workgroup = (suffix split z, row group, KV head).  The group's G * nr <= 64 rows, tile row r = h * nr + t as in
//     grouped_attn.h; keys [P + z * chunk_s, ..) cut at pos + nr, of the stream's OWN arena, causal limit pos + t per row (the
//     rows this pass wrote are among them).
//   * Keys over waves (both roles): the chunk is cut into 64-key blocks, wave w owns blocks w, w + 4, .. and keeps its own
//     online-softmax state; no workgroup barrier in the key loop, one merge of the four waves at the end.  A query tile is
//     not cut over waves: every wave holds all NQT column tiles, so each K / V element of the chunk is read by one wave, once.
//   * Products.  S^T = K Q^T on mfma 16x16x32 with Q^T in registers (LDS for 3 - 4 tiles of D = 128 over a 16-bit arena); the
//     lane's p of key tiles 2 s, 2 s + 1 are the B operand of O^T = V^T P^T; V^T comes back from the wave's own LDS image
//     through ds_read_b64_tr_b16 in PA_VST pitch (grouped_attn.h's layout, which this file includes for its helpers).
//     Roundings are attn_body's: rnd(acc [* k_scale]), Llama: rnd(. / sqrt(D)), p rounded to T; fp8 rows are widened exactly
//     and v_scale multiplies the output.
//   * Loads.  None sits inside a branch: key indices are clamped to the role's last key and tested at use.
//   * LDS = ga_lds_bytes(D), fixed: it depends on neither P nor the context.
//   * Output.  Always partial: un-normalised sums, row maximum, denominator in attn_combine_kernel's layout
//     [(group, head)][split][ATT_TQ][D + 2], split = z for the prefix and prefix_splits + z for the suffix; a prefix tile's
//     rows scatter to the groups they came from.  A chunk with no key of a row leaves m = -inf, which the combine skips.
// The transposed read needs EXEC all ones: every loop bound around it is per wave.
#pragma once
#include "grouped_attn.h"

template <typename T, int D, bool KV8, int NQT, bool PREFIX>
__device__ __forceinline__ void attn_shared_body(const T *__restrict__ qbuf, const RowTab &tab, int layer, int Hq, int Hkv, int arch,
                                                 float inv_sqrt_d, int kvh, int unit, int bz, int chunk, int split, int nsplit,
                                                 float *__restrict__ partial, char *smem) {
    static_assert(D == 64 || D == 128, "output tiles of 16 dims, PA_VST's pitch");
    static_assert(sizeof(T) == 2, "16-bit models");
    using E = typename std::conditional<KV8, unsigned char, T>::type;      // arena element
    using E8 = typename std::conditional<KV8, uint2, u32x4>::type;         // 8 consecutive arena elements
    constexpr int VST = PA_VST(D), NDT = D / 16, NDK = D / 32, PPR = D / 8;
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = tid & 63;
    const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
    const int G = Hq / Hkv, P = tab.shared_keys;

    // ---- the role's keys [k_lo, k_hi), the last key a load may touch, the arena and its scales (all uniform)
    int k_lo, k_hi, s_last, max_seq, r0 = 0, nr = 0, p0 = 0;
    const void *arena;
    const float *scales = nullptr;
    if constexpr (PREFIX) {
        k_lo = bz * chunk; k_hi = min(P, k_lo + chunk); s_last = P - 1;
        arena = tab.shared_kv; max_seq = tab.shared_max_seq;
        if constexpr (KV8) scales = tab.shared_scale;
    } else {
        const int strm = tab.grp_stream[unit];
        r0 = tab.grp_row0[unit]; nr = tab.grp_n[unit]; p0 = tab.grp_pos[unit];
        k_lo = P + bz * chunk; k_hi = min(p0 + nr, k_lo + chunk); s_last = p0 + nr - 1;
        arena = tab.kv_base[strm]; max_seq = tab.max_seq[strm];
        if constexpr (KV8) scales = tab.kv_scale[strm];
    }
    const E *karena = (const E *)arena + (size_t)layer * 2 * Hkv * max_seq * D;
    const E *K = karena + (size_t)kvh * max_seq * D, *V = karena + (size_t)(Hkv + kvh) * max_seq * D;
    float k_scale = 1.f, v_scale = 1.f;
    if constexpr (KV8) {
        k_scale = scales[(size_t)layer * 2 * Hkv + kvh];
        v_scale = scales[(size_t)layer * 2 * Hkv + Hkv + kvh];
    }
    char *vb = smem + (size_t)w * GA_BLK * VST;                    // this wave's V image [GA_BLK][VST]
    float *ms = reinterpret_cast<float *>(smem + (size_t)4 * GA_BLK * VST), *ls = ms + 4 * 64;    // [4 waves][64 rows]

    // ---- the lane's query rows: where tile row 16 qt + i16 comes from (pass row, head), where its partial sums go, and - the
    // suffix role alone - its last visible key
    int poff[NQT], lim[NQT];
    bool real[NQT];
    u32x4 qf[NQT][NDK];
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        int m, h, bg, t;
        if constexpr (PREFIX) {
            const int R = 64 * unit + 16 * qt + i16;
            real[qt] = R < G * tab.n_rows;
            m = real[qt] ? R / G : 0;
            h = real[qt] ? R - m * G : 0;
            bg = 0; t = m;
            for (int g = 1; g < tab.n_groups; ++g) {              // (a uniform index: the table stays in scalar registers)
                const int gr0 = tab.grp_row0[g];
                if (m >= gr0) { bg = g; t = m - gr0; }
            }
            lim[qt] = 0;
        } else {
            const int r = 16 * qt + i16;
            real[qt] = r < G * nr;
            h = real[qt] ? r / nr : 0;
            t = real[qt] ? r - h * nr : 0;
            m = r0 + t; bg = unit;
            lim[qt] = p0 + t;
        }
        const int head = kvh * G + h;
        poff[qt] = ((((bg * Hq + head) * nsplit + split) * ATT_TQ) + t) * (D + 2);
        const T *qr = qbuf + (size_t)m * Hq * D + (size_t)head * D + g4 * 8;
#pragma unroll
        for (int dk = 0; dk < NDK; ++dk) {
            qf[qt][dk] = *reinterpret_cast<const u32x4 *>(qr + dk * 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) qf[qt][dk][i] = real[qt] ? qf[qt][dk][i] : 0u;   // rows past the tile are zero
        }
    }
    // 3 - 4 tiles of D = 128 with a 16-bit arena: Q, K, V and the accumulators do not all fit the registers, so the Q operands
    // live in LDS in operand order [tile][dk][lane] (qf depends on the lane alone, not on the wave: wave 0 writes, all read)
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
                    bool seen = key < k_hi;                       // the prefix role: the range end alone
                    if constexpr (!PREFIX) seen = seen && key <= lim[qt];
                    v = seen ? v : -INFINITY;
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
        // ---- the block's V rows into the wave's image (a wave's LDS operations execute in order), then O^T += V^T P^T
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

    // ---- lane l holds the sums of row 16 qt + i16, dims 16 dt + 4 g4 .. + 3
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
        if (!real[qt]) continue;
        float *pz = partial + poff[qt];
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const f32x4 a = KV8 ? acc[qt][dt] * v_scale : acc[qt][dt];
            float2 *dst = reinterpret_cast<float2 *>(pz + dt * 16 + 4 * g4);          // ((D + 2) t is even: 8-byte aligned)
            dst[0] = float2{a[0], a[1]};
            dst[1] = float2{a[2], a[3]};
        }
        if (g4 == 0) { pz[D] = M[qt]; pz[D + 1] = L[qt]; }
    }
}

template <typename T, int D, bool KV8, bool PREFIX>
__device__ __forceinline__ void attn_shared_role(int rows, const T *__restrict__ qbuf, const RowTab &tab, int layer, int Hq, int Hkv,
                                                 int arch, float inv_sqrt_d, int kvh, int unit, int bz, int chunk, int split, int nsplit,
                                                 float *__restrict__ partial, char *smem) {
#define SA_BODY(N) attn_shared_body<T, D, KV8, N, PREFIX>(qbuf, tab, layer, Hq, Hkv, arch, inv_sqrt_d, kvh, unit, bz, chunk, split, nsplit, partial, smem)
    if (rows <= 16) SA_BODY(1);
    else if (rows <= 32) SA_BODY(2);
    else if (rows <= 48) SA_BODY(3);
    else SA_BODY(4);
#undef SA_BODY
}

// grid (Hkv * tiles * psplits + Hkv * groups * ssplits) x 256 threads, ga_lds_bytes(D) of dynamic LDS; pchunk / schunk: keys per
// prefix / suffix split (multiples of GA_BLK); the partial buffer holds psplits + ssplits splits per (group, head)
template <typename T, int D, bool KV8>
__global__ __launch_bounds__(256) void attn_shared_kernel(const T *__restrict__ qbuf, RowTab tab, int layer, int Hq, int Hkv, int arch,
                                                         float inv_sqrt_d, int tiles, int psplits, int pchunk, int ssplits, int schunk,
                                                         float *__restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) char sa_smem[];
    const int G = Hq / Hkv, nsplit = psplits + ssplits, n_prefix = Hkv * tiles * psplits;
    int id = blockIdx.x;                                          // per workgroup: the role and the tile count are uniform
    if (id < n_prefix) {
        const int tile = id % tiles, kvh = (id / tiles) % Hkv, z = id / (tiles * Hkv);
        attn_shared_role<T, D, KV8, true>(min(64, G * tab.n_rows - 64 * tile), qbuf, tab, layer, Hq, Hkv, arch, inv_sqrt_d, kvh, tile, z,
                                          pchunk, z, nsplit, partial, sa_smem);
    } else {
        id -= n_prefix;
        const int kvh = id % Hkv, bg = (id / Hkv) % tab.n_groups, z = id / (Hkv * tab.n_groups);
        attn_shared_role<T, D, KV8, false>(G * tab.grp_n[bg], qbuf, tab, layer, Hq, Hkv, arch, inv_sqrt_d, kvh, bg, z, schunk,
                                           psplits + z, nsplit, partial, sa_smem);
    }
}
