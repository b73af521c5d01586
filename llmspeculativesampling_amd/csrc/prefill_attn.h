// Causal attention of a prefill pass (rows that are consecutive positions of a stream; reference modeling_llama.py:346-372,
// modeling_opt.py:210-256): 16 rows of one head per workgroup, P.V on the matrix cores.
//
// attn_kernel (model_kernels.h) is built for a decode / verify step: <= 8 rows per workgroup, the scores by MFMA, P.V on the
// vector ALUs (each thread 8 head dims of 8 rows per key).  A 256-row prefill pass runs 32 of its row groups per head -
// 2.7 ms of a 12.4 ms pass at the 13b shape, every group re-reading the head's keys and values.  Here a workgroup takes 16
// rows (one full MFMA row tile), and both products run on the matrix cores:
//   * scores: A = 16 keys x 32 dims straight from the arena, B = q^T - attn_kernel's code, the same roundings
//     (rnd(q.k), Llama: rnd(. / sqrt(D)); masked entries -inf);
//   * softmax in fp32 over the visible keys, P rounded to the model type (modeling_llama.py:371) - attn_kernel's half-wave
//     reduction, step for step, so a row's probabilities do not depend on which kernel ran;
//   * out^T[dim][row] = sum_key V^T[dim][key] P[row][key]: B = P (8 consecutive-ish keys of a row per lane, from the score
//     tile in LDS), A = V^T - V lies [key][dim] in the arena, so its 64-key chunks are staged in LDS as they are and read
//     back TRANSPOSED by ds_read_b64_tr_b16 (per 16 lanes a block of 4 keys x 16 dims, delivered dim-major).  The k index of
//     the two operands only has to AGREE: element j = 4h + q of lane group g stands for key 16h + 4g + q of the 32-key step,
//     which makes the two groups of a 32-lane half read 8 consecutive key rows (288-byte row pitch: conflict-free).
// fp32 accumulation inside the MFMA, one rounding of the output - the reference's bf16 matmul; the order of the sum differs
// from attn_kernel's (and from torch's), as any two correct evaluations do.
//
// Instances: head_dim D in {64, 128}, the arena in the model type T or in fp8 e4m3 (KV8).
//   * KV8: a lane's score operand is 8 consecutive BYTES of the key row, widened to T by fp8x8_to_16 (exact), and the scores
//     are rounded as attn_body rounds them - rnd(acc * k_scale), then Llama's rnd(. / sqrt(D)) - so a row's probabilities
//     still do not depend on which kernel ran.  Values are widened to T while their chunk is staged, so the LDS holds the
//     same [key][pitch] image of T as on the 16-bit path (the global reads halve, the transposed-read / MFMA loop is the
//     same code), P stays in T, and the fp32 accumulators are multiplied by v_scale in front of the single rounding of the
//     store (attn_body: `a * v_scale` in the same place).  The scales travel per group in PaGroups.
//   * D = 64: D / 32 = 2 score MFMAs per key tile; four 16-dim output tiles, so wave w owns dims 16 w .. 16 w + 15 (ONE
//     accumulator where D = 128 has two); a V chunk is 64 keys x 128 B of T.
//   * Row pitch of the V image, 2 D + 32 bytes.  ds_read_b64_tr_b16 is served in two groups of 32 lanes, a lane's bank is
//     (addr / 4) mod 64, i.e. its offset inside a 256-byte bank row.  A 32-lane half is the lane groups g4 = 2 a, 2 a + 1:
//     their lanes 4 q4 + p4 address key rows 8 a + 4 (g4 & 1) + q4 = 8 consecutive rows r = 0..7 of the image, 32
//     contiguous bytes (4 p4 x 8 B: 8 banks) at the same column offset in each.  8 rows x 8 banks fill the 64 banks exactly
//     once iff the row starts r * pitch mod 256 are the 8 distinct multiples of 32, i.e. iff pitch = 32 x (an odd number)
//     mod 256.  D = 128 (256-byte rows): 288 = 32 x 9, r * 288 mod 256 = 0, 32, 64, .., 224.  D = 64 (128-byte rows): the
//     bare 128 = 32 x 4 would put rows r and r + 2 on the same banks (4-way); 160 = 32 x 5 gives r * 160 mod 256 = 0, 160,
//     64, 224, 128, 32, 192, 96 - conflict-free, and a multiple of 16 for the staging writes.  The second read of a step
//     (+ 16 rows = 16 x pitch, a multiple of 256) is an instruction of its own on the same banks.
//   * The transposed read needs EXEC all ones: no divergent flow surrounds it (chunk and step counts are per workgroup).
#pragma once
#include "model_kernels.h"

#define PA_ROWS 16
#define PA_VCH 64                                   // keys per staged V chunk
#define PA_VST(D) (2 * (D) + 32)                    // bytes per key row of the LDS V image (derivation above): 288 / 160
#define PA_SPAD 4                                   // floats of padding per score row (16 rows x ds_read_b128: no bank shared)

// row groups of a prefill pass: <= 16 consecutive rows of one stream each (built on the host from the table's 8-row groups)
struct PaGroups {
    int n;
    int row0[SD_MAX_GROUPS], nrows[SD_MAX_GROUPS], pos[SD_MAX_GROUPS], max_seq[SD_MAX_GROUPS];
    const void *kv[SD_MAX_GROUPS];
    const float *kv_scale[SD_MAX_GROUPS];           // fp8 arena: the group's stream's scales [L][2][Hkv] (NULL otherwise)
};
static_assert(sizeof(PaGroups) <= 1536, "PaGroups travels by value in the kernel arguments (4 KiB in all)");

typedef short pa_v4s __attribute__((ext_vector_type(4)));

// What one workgroup of either kernel holds and does: the two kernels differ in their softmax alone, and every other passage
// is this code - which is why their outputs are bit-identical.  LDS: [16][ss] floats of scores / probabilities (ss = the
// kernel's key capacity + PA_SPAD), then the V image [PA_VCH][PA_VST(D)].
template <typename T, int D, bool KV8>
struct PaWorkgroup {
    static_assert(D == 64 || D == 128, "four waves x (D / 64) output tiles of 16 dims");
    static_assert(sizeof(T) == 2, "16-bit models");
    using E = typename std::conditional<KV8, unsigned char, T>::type;      // arena element
    using E8 = typename std::conditional<KV8, uint2, u32x4>::type;         // 8 consecutive arena elements
    // P.V: wave w owns head dims (D / 4) w .. + D / 4 - 1 (NT tiles of 16 dims).  A V chunk = 64 keys x D elements = 64 PPR
    // pieces of 8 elements (16 B of T in the image; 8 B in an fp8 arena); thread tid moves the NP pieces tid, tid + 256, ...:
    // key piece / PPR, 16-byte column piece % PPR
    static constexpr int VST = PA_VST(D), NT = D / 64, PPR = D / 8, NP = PA_VCH * PPR / 256;
    float *sc;                                                    // [16][ss]
    char *vb;                                                     // [PA_VCH][VST]
    int ss;                                                       // score row pitch (floats)
    int head, tid, w, lane, r0, nr, p0, arch;
    const E *K, *V;
    float k_scale = 1.f, v_scale = 1.f, inv_sqrt_d;
    int s_hi, s_last, s_pad, nch;                                 // keys, the last one, keys in whole 32-key steps; V chunks
    u32x4 qf[D / 32];                                             // the q operand of the score MFMAs
    E8 vr[NP];                                                    // the V chunk in flight
    f32x4 acc[NT];                                                // out^T

    __device__ __forceinline__ PaWorkgroup(char *smem, int s_cap, const T *__restrict__ qbuf, const PaGroups &pg, int layer, int Hq,
                                           int Hkv, int arch_, float inv_sqrt_d_)
        : arch(arch_), inv_sqrt_d(inv_sqrt_d_) {
        ss = s_cap + PA_SPAD;
        sc = reinterpret_cast<float *>(smem);
        vb = smem + (size_t)PA_ROWS * ss * sizeof(float);
        head = blockIdx.x;
        const int g = blockIdx.y;
        tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = tid & 63;
        r0 = pg.row0[g], nr = pg.nrows[g], p0 = pg.pos[g];
        const int max_seq = pg.max_seq[g], kvh = head / (Hq / Hkv);
        const E *karena = (const E *)pg.kv[g] + (size_t)layer * 2 * Hkv * max_seq * D;
        K = karena + (size_t)kvh * max_seq * D;
        V = karena + (size_t)(Hkv + kvh) * max_seq * D;
        if constexpr (KV8) {
            const float *scl = pg.kv_scale[g] + (size_t)layer * 2 * Hkv;
            k_scale = scl[kvh];
            v_scale = scl[Hkv + kvh];
        }
        s_hi = p0 + nr, s_last = s_hi - 1;                        // row t of the group sees keys 0 .. p0 + t
        s_pad = (s_hi + 31) & ~31;
        nch = (s_hi + PA_VCH - 1) / PA_VCH;
        const int mrow = lane & 15, kq = (lane >> 4) * 8;
#pragma unroll
        for (int dk = 0; dk < D / 32; ++dk) {
            qf[dk] = *reinterpret_cast<const u32x4 *>(qbuf + (size_t)(r0 + min(mrow, nr - 1)) * Hq * D + head * D + dk * 32 + kq);
#pragma unroll
            for (int i = 0; i < 4; ++i) qf[dk][i] = mrow < nr ? qf[dk][i] : 0u;       // rows >= nr of the q operand are zero
        }
#pragma unroll
        for (int d2 = 0; d2 < NT; ++d2) acc[d2] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // ---- scores of keys b0 .. b_hi - 1 (b0 a multiple of 64, b_hi <= s_hi) into sc[row][key - b0], -inf past the causal
    // limit (attn_kernel's MFMA path): lane l ends up with score[key = 16 kt + 4 (l >> 4) + j][row = l & 15]
    __device__ __forceinline__ void scores(int b0, int b_hi) {
        const int mrow = lane & 15, kq = (lane >> 4) * 8;
        for (int kt0 = b0 / 16 + w; kt0 * 16 < b_hi; kt0 += 16) { // four key tiles per wave and round, all K loads up front
            E8 kf[4][D / 32];                                     // (fp8: 8 bytes per operand, widened at the MFMA)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const E *kr = K + (size_t)min((kt0 + 4 * u) * 16 + mrow, s_last) * D + kq;
#pragma unroll
                for (int dk = 0; dk < D / 32; ++dk) kf[u][dk] = *reinterpret_cast<const E8 *>(kr + dk * 32);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kt = kt0 + 4 * u;
                if (kt * 16 >= b_hi) continue;
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int dk = 0; dk < D / 32; ++dk) {
                    if constexpr (KV8) a = mfma16<T>(fp8x8_to_16<T>(kf[u][dk]), qf[dk], a);
                    else a = mfma16<T>(kf[u][dk], qf[dk], a);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s = kt * 16 + (lane >> 4) * 4 + j;
                    if (s < b_hi) {
                        float v = rnd<T>(KV8 ? a[j] * k_scale : a[j]);
                        if (arch == SD_ARCH_LLAMA) v = rnd<T>(v * inv_sqrt_d);
                        sc[(size_t)mrow * ss + s - b0] = s <= p0 + mrow ? v : -INFINITY;
                    }
                }
            }
        }
    }

    // V chunk c from the arena into vr (a key past the range re-reads the last one: its probabilities are zero)
    __device__ __forceinline__ void vload(int c) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int piece = tid + 256 * i, key = min(c * PA_VCH + piece / PPR, s_last);
            vr[i] = *reinterpret_cast<const E8 *>(V + (size_t)key * D + (piece % PPR) * 8);
        }
    }

    // ---- acc += V^T P over the chunks c0 .. c1 - 1, the probabilities of key b0 + s in sc[row][s]; vload(c0) has been issued
    __device__ __forceinline__ void pv(int c0, int c1, int b0) {
        const int g4 = lane >> 4, i16 = lane & 15, q4 = i16 >> 2, p4 = i16 & 3;
        for (int c = c0; c < c1; ++c) {
            __syncthreads();                                      // the previous chunk is no longer read (c = c0: P is complete)
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                const int piece = tid + 256 * i;
                u32x4 vw;
                if constexpr (KV8) vw = fp8x8_to_16<T>(vr[i]);    // exact; from here on the 16-bit path's image
                else vw = vr[i];
                *reinterpret_cast<u32x4 *>(vb + (piece / PPR) * VST + (piece % PPR) * 16) = vw;
            }
            __syncthreads();
            if (c + 1 < c1) vload(c + 1);
            const int nsteps = min(PA_VCH / 32, (s_hi - c * PA_VCH + 31) / 32);
            for (int st = 0; st < nsteps; ++st) {
                // B: P[row i16][k0 + 16 h + 4 g4 + (0..3)], h = 0, 1 - already values of T: the conversion is exact
                const float *pr = sc + (size_t)i16 * ss + (c * PA_VCH - b0) + st * 32 + 4 * g4;
                const f32x4 pa = *reinterpret_cast<const f32x4 *>(pr), pb = *reinterpret_cast<const f32x4 *>(pr + 16);
                const T ph[8] = {(T)pa[0], (T)pa[1], (T)pa[2], (T)pa[3], (T)pb[0], (T)pb[1], (T)pb[2], (T)pb[3]};
                const u32x4 pf = *reinterpret_cast<const u32x4 *>(ph);
#pragma unroll
                for (int d2 = 0; d2 < NT; ++d2) {
                    // A: lane 4 q4 + p4 of its 16-lane group supplies the address of key row 16 h + 4 g4 + q4 of the step,
                    // dims 16 dt + 4 p4 .. + 3; lane i16 receives dim 16 dt + i16 of the group's four keys
                    const char *va = vb + (size_t)(st * 32 + 4 * g4 + q4) * VST + ((NT * w + d2) * 16 + 4 * p4) * 2;
                    const pa_v4s a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_v4s __attribute__((address_space(3))) *)(va));
                    const pa_v4s a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_v4s __attribute__((address_space(3))) *)(va + 16 * VST));
                    u32x4 af;
                    af[0] = ((const unsigned *)&a0)[0]; af[1] = ((const unsigned *)&a0)[1];
                    af[2] = ((const unsigned *)&a1)[0]; af[3] = ((const unsigned *)&a1)[1];
                    acc[d2] = mfma16<T>(af, pf, acc[d2]);
                }
            }
        }
    }

    // lane l holds out[row l & 15][dims 16 dt + 4 (l >> 4) .. + 3]: one 8-byte store inside an 8-element operand group
    __device__ __forceinline__ void store(T *__restrict__ out, int Hq) {
        const int g4 = lane >> 4, i16 = lane & 15;
        if (i16 < nr) {
#pragma unroll
            for (int d2 = 0; d2 < NT; ++d2) {
                if constexpr (KV8) acc[d2] *= v_scale;
                store4_maybe_wt<false>(out + xoff<T>(r0 + i16, head * D + (NT * w + d2) * 16 + 4 * g4, Hq * D), acc[d2][0], acc[d2][1],
                                       acc[d2][2], acc[d2][3]);
            }
        }
    }
};

template <typename T, int D, bool KV8>
__global__ __launch_bounds__(256) void attn_prefill_kernel(const T *__restrict__ qbuf, PaGroups pg, int layer, T *__restrict__ out,
                                                          int Hq, int Hkv, int arch, float inv_sqrt_d, int s_cap) {
    extern __shared__ __attribute__((aligned(16))) char pa_smem[];
    PaWorkgroup<T, D, KV8> wg(pa_smem, s_cap, qbuf, pg, layer, Hq, Hkv, arch, inv_sqrt_d);
    const int tid = wg.tid, nr = wg.nr, p0 = wg.p0, s_hi = wg.s_hi, s_pad = wg.s_pad, ss = wg.ss;
    float *sc = wg.sc;
    wg.scores(0, s_hi);
    __syncthreads();

    {   // ---- softmax: one half-wave per row, the partial sums a full wave's lower and upper lanes would hold
        const int hl = tid & 31, grp = tid >> 5;
        const bool upper = (tid & 32) != 0;
        for (int t = grp; t < nr; t += 8) {
            float *row = sc + (size_t)t * ss;
            const int len = min(s_hi, p0 + t + 1);
            float lo, hi, lo1, hi1;
            float m0 = -INFINITY;
            for (int s = hl; s < len; s += 32) m0 = fmaxf(m0, row[s]);
            half_maxes(m0, lo, hi);
            const float m = upper ? hi : lo;
            float s0 = 0.f, s1 = 0.f;                             // what lanes l and l + 32 of a full wave accumulate
            for (int s = hl; s < len; s += 64) {
                const float e = expf(row[s] - m);
                row[s] = e;
                s0 += e;
            }
            for (int s = hl + 32; s < len; s += 64) {
                const float e = expf(row[s] - m);
                row[s] = e;
                s1 += e;
            }
            half_sums(s0, lo, hi);
            half_sums(s1, lo1, hi1);
            const float sum = upper ? hi + hi1 : lo + lo1;
            for (int s = hl; s < s_pad; s += 32) row[s] = s < len ? rnd<T>(row[s] / sum) : 0.f;
        }
        for (int i = tid; i < (PA_ROWS - nr) * s_pad; i += 256) {  // rows past the group: zero probabilities (never stored)
            const int t = nr + i / s_pad, s = i - (i / s_pad) * s_pad;
            sc[(size_t)t * ss + s] = 0.f;
        }
    }

    wg.vload(0);
    wg.pv(0, wg.nch, 0);
    wg.store(out, Hq);
}

// The same attention with the score tile cut into blocks of kb keys (a multiple of 64), for contexts whose whole tile does
// not fit the LDS: the footprint is 16 x (kb + 4) floats + the V chunk, whatever the context.  The rounding points do not
// move (no online-softmax rescaling: that would round P in front of the normalisation), so the blocks are swept three
// times and the scores recomputed each time (PaWorkgroup::scores) - the same MFMA inputs in the same order, hence the same bits:
//   1. row maxima: a lane of a row's half-wave keeps a running max over its keys hl, hl + 32, ... (the single-tile
//      kernel's sequence, cut at block edges), half_maxes once at the end;
//   2. denominators: e = expf(score - m) with the final m; the lane's two partial sums s0 (keys hl + 64 k) and s1 (keys
//      hl + 32 + 64 k) are carried across blocks - kb is a multiple of 64, so each receives the identical sequence of
//      additions - and one half_sums at the end gives the single-tile kernel's denominator bit for bit;
//   3. P.V: p = rnd(expf(score - m) / sum), zero past the causal limit and for rows past nr, then the single-tile kernel's
//      chunk loop (PaWorkgroup::pv) over the block's 64-key V chunks in ascending order, the accumulators living across blocks.
// The output is therefore bit-identical to attn_prefill_kernel's wherever both can run.  A half-wave owns rows grp and
// grp + 8 of the group and keeps their (max, s0, s1) in registers between blocks.  Blocks wholly past the group's last key
// are not visited; every loop bound is per workgroup (the transposed read needs EXEC all ones).
// Small forced blocks: a wave requests the K rows of four key tiles (64 keys) per round whether or not they lie inside the block
// (rows past b_hi are clamped to s_last and their scores dropped), so with kb = 64 and four waves three quarters of the
// requests of every sweep are discarded - harmless, and nothing at the default kb = 256 (one round of 4 x 4 tiles per
// block), but times taken under SD_PREFILL_ATTN_BLOCK=64 / 128 overstate the cost of a small block.
template <typename T, int D, bool KV8>
__global__ __launch_bounds__(256) void attn_prefill_blocked_kernel(const T *__restrict__ qbuf, PaGroups pg, int layer,
                                                                  T *__restrict__ out, int Hq, int Hkv, int arch, float inv_sqrt_d,
                                                                  int kb) {
    extern __shared__ __attribute__((aligned(16))) char pa_smem[];
    PaWorkgroup<T, D, KV8> wg(pa_smem, kb, qbuf, pg, layer, Hq, Hkv, arch, inv_sqrt_d);   // sc: the scores, then the probabilities, of ONE block
    const int tid = wg.tid, nr = wg.nr, p0 = wg.p0, s_hi = wg.s_hi, s_pad = wg.s_pad, ss = wg.ss;
    float *sc = wg.sc;

    // ---- softmax state: half-wave grp owns rows grp and grp + 8 (a row past nr: len 0, never read)
    const int hl = tid & 31, grp = tid >> 5;
    const bool upper = (tid & 32) != 0;
    int len[2];
    float m[2], sum[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) len[i] = grp + 8 * i < nr ? min(s_hi, p0 + grp + 8 * i + 1) : 0;
    {   // sweep 1: row maxima
        float mx[2] = {-INFINITY, -INFINITY};
        for (int b0 = 0; b0 < s_hi; b0 += kb) {
            const int b_hi = min(b0 + kb, s_hi);
            wg.scores(b0, b_hi);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float *row = sc + (size_t)(grp + 8 * i) * ss;
                const int lim = min(len[i], b_hi) - b0;
                for (int s = hl; s < lim; s += 32) mx[i] = fmaxf(mx[i], row[s]);
            }
            __syncthreads();                                      // the next block's scores overwrite these
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float lo, hi;
            half_maxes(mx[i], lo, hi);
            m[i] = upper ? hi : lo;
        }
    }
    {   // sweep 2: denominators - the partial sums a full wave's lower and upper lanes would hold, carried across blocks
        float s0[2] = {0.f, 0.f}, s1[2] = {0.f, 0.f};
        for (int b0 = 0; b0 < s_hi; b0 += kb) {
            const int b_hi = min(b0 + kb, s_hi);
            wg.scores(b0, b_hi);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float *row = sc + (size_t)(grp + 8 * i) * ss;
                const int lim = min(len[i], b_hi) - b0;
                for (int s = hl; s < lim; s += 64) s0[i] += expf(row[s] - m[i]);
                for (int s = hl + 32; s < lim; s += 64) s1[i] += expf(row[s] - m[i]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float lo, hi, lo1, hi1;
            half_sums(s0[i], lo, hi);
            half_sums(s1[i], lo1, hi1);
            sum[i] = upper ? hi + hi1 : lo + lo1;
        }
    }
    // sweep 3: probabilities of a block, then P.V over its V chunks
    for (int b0 = 0; b0 < s_hi; b0 += kb) {
        const int b_hi = min(b0 + kb, s_hi);
        wg.scores(b0, b_hi);
        __syncthreads();
        const int c0 = b0 / PA_VCH, c1 = min(wg.nch, (b0 + kb) / PA_VCH);
        wg.vload(c0);
        const int b_pad = min(b0 + kb, s_pad) - b0;               // the P.V steps read whole 32-key steps: zeros past the keys
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float *row = sc + (size_t)(grp + 8 * i) * ss;
            for (int s = hl; s < b_pad; s += 32) row[s] = b0 + s < len[i] ? rnd<T>(expf(row[s] - m[i]) / sum[i]) : 0.f;
        }
        wg.pv(c0, c1, b0);
        __syncthreads();                                          // the next block's scores overwrite P
    }
    wg.store(out, Hq);
}
