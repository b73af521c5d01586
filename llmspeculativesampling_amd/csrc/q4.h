// 4-bit group-quantised records of a bf16 weight matrix in the streaming tile order ("4-bit records").
// Quantisation groups are 128 consecutive k of one output row, each with a bf16 scale s and a zero point z in 0..15; codes
// q are in 0..15 and the weight is DEFINED as
//     w = bf16_rne(float(s) * float(q - z))
// (the product is exact in fp32: 8 significant bits times at most 5, so this is one rounding).  The model keeps the tiled
// bf16 matrix of exactly these w for every route that does not stream records; the records are a second image of the same
// numbers at 4.25 bits per weight.
//
// One record covers a 16-row n-tile times one group: four k-steps of the 16 x 32 fragment order, 1088 bytes, record
// (n-tile nt, group g) at byte ((nt * K / 128) + g) * 1088:
//   dwords 0 .. 255: lane l owns dwords 4l .. 4l + 3 (ONE 16-byte request feeds four MFMAs); dword u holds the eight codes of
//     W[n = 16 nt + l % 16][k = 128 g + 32 u + 8 (l / 16) + e], code e in bits 4e .. 4e + 3
//   dwords 256 .. 271: row r of the tile: s (bf16 bits) | z << 16.  A lane's row is fixed, so its 32 codes share one dword.
// Every record has a fixed size and address and no load depends on another load.
//
// Decode, in registers right before the MFMA.  A code never moves to bit 0: `(x & 0xF << 4i) | 0x4B000000` is the float
// 2^23 + 16^i q for i = 0..3 (one v_and_or_b32; the upper four codes after ONE shift by 16), from which 2^23 + 16^i z is
// subtracted - exact - and the difference multiplied by s / 16^i - a power-of-two rescaling of s, exact (*) - so the
// product is s (q - z) itself, exact in fp32, and the conversion to bf16 is the definition's single rounding.  Subtract and
// multiply pair up as packed fp32 operations and the conversion is one v_cvt_pk_bf16_f32 per output dword: 21 VALU
// operations per eight weights.  ((*) down to s / 4096 >= 2^-145 for the smallest bf16 denormal: fp32 denormals are on.)
#pragma once
#include "normload_kernels.h"

#define Q4_REC_DWORDS 272                                    // 64 lanes x 4 dwords of codes + 16 (s, z) dwords
#define Q4_MAGIC 0x4B000000u                                 // 2^23 as a float: an integer < 2^23 in its mantissa adds exactly

using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

struct Q4Rec { u32x4 c; unsigned sz; };                      // what a lane requests of a record
// a lane's group constants: scale and offset of the code at bits 4i of a half-dword, as the pairs the packed operations take
struct Q4Lane { f32x2 s01, s23, o01, o23; };

__device__ __forceinline__ Q4Rec q4_fetch(const unsigned *rec, int lane) {
    Q4Rec r;
    r.c = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(rec) + lane);
    r.sz = __builtin_nontemporal_load(rec + 256 + (lane & 15));
    return r;
}
__device__ __forceinline__ Q4Lane q4_lane(unsigned sz) {
    const float s = __uint_as_float(sz << 16);
    const unsigned z = (sz >> 16) & 15u;
    Q4Lane g;
    g.s01 = f32x2{s, s * 0.0625f};
    g.s23 = f32x2{s * 0.00390625f, s * 0.000244140625f};
    g.o01 = f32x2{__uint_as_float(Q4_MAGIC | z), __uint_as_float(Q4_MAGIC | z << 4)};
    g.o23 = f32x2{__uint_as_float(Q4_MAGIC | z << 8), __uint_as_float(Q4_MAGIC | z << 12)};
    return g;
}
// four codes of a half-dword -> two dwords of bf16 pairs
__device__ __forceinline__ uint2 q4_half(unsigned h, const Q4Lane &g) {
    const f32x2 a = f32x2{__uint_as_float((h & 0x000Fu) | Q4_MAGIC), __uint_as_float((h & 0x00F0u) | Q4_MAGIC)};
    const f32x2 b = f32x2{__uint_as_float((h & 0x0F00u) | Q4_MAGIC), __uint_as_float((h & 0xF000u) | Q4_MAGIC)};
    return uint2{__builtin_bit_cast(unsigned, __builtin_convertvector((a - g.o01) * g.s01, bf16x2)),
                 __builtin_bit_cast(unsigned, __builtin_convertvector((b - g.o23) * g.s23, bf16x2))};
}
// one code dword (a k-step of the lane's row) -> the u32x4 MFMA operand of the bf16 tile
__device__ __forceinline__ u32x4 q4_decode(unsigned x, const Q4Lane &g) {
    const uint2 lo = q4_half(x, g), hi = q4_half(x >> 16, g);
    return u32x4{lo.x, lo.y, hi.x, hi.y};
}

// ---- packer: one wave per record, from plain row-major q [N][K] (uint8), s [N][K / 128] (bf16), z [N][K / 128] (uint8).
// Writes the record and the four tiles of the bf16 copy, the latter by the definition in plain arithmetic (not by the
// decoder above: the expander below runs that one, and the two must agree).  Codes and zero points are taken mod 16.
template <int = 0>
__global__ __launch_bounds__(64) void q4_pack_kernel(const uint8_t *__restrict__ q, const uint16_t *__restrict__ sc,
                                                     const uint8_t *__restrict__ zp, unsigned *__restrict__ rec,
                                                     u32x4 *__restrict__ tiles, int K) {
    const int lane = threadIdx.x, KG = K >> 7;
    const int nt = blockIdx.x / KG, g = blockIdx.x - nt * KG;
    const size_t row = (size_t)nt * 16 + (lane & 15);
    const unsigned sb = sc[row * KG + g], z = zp[row * KG + g] & 15u;
    const float s = __uint_as_float(sb << 16);
    unsigned *r = rec + (size_t)blockIdx.x * Q4_REC_DWORDS;
    u32x4 codes;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const uint2 b8 = *reinterpret_cast<const uint2 *>(q + row * K + (size_t)g * 128 + u * 32 + (lane >> 4) * 8);
        unsigned x = 0u;
        bf16_t w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned c = ((e < 4 ? b8.x : b8.y) >> (8 * (e & 3))) & 15u;
            x |= c << (4 * e);
            w[e] = (bf16_t)(s * (float)((int)c - (int)z));
        }
        codes[u] = x;
        tiles[((size_t)nt * (K >> 5) + g * 4 + u) * 64 + lane] = *reinterpret_cast<const u32x4 *>(w);
    }
    reinterpret_cast<u32x4 *>(r)[lane] = codes;
    if (lane < 16) r[256 + lane] = sb | z << 16;
}

// ---- expander (the format's executable definition and the tests' hook): records -> the tiled bf16 layout
template <int = 0>
__global__ __launch_bounds__(64) void q4_unpack_kernel(const unsigned *__restrict__ rec, u32x4 *__restrict__ tiles, int K) {
    const int lane = threadIdx.x, KG = K >> 7;
    const int nt = blockIdx.x / KG, g = blockIdx.x - nt * KG;
    const Q4Rec r = q4_fetch(rec + (size_t)blockIdx.x * Q4_REC_DWORDS, lane);
    const Q4Lane c = q4_lane(r.sz);
#pragma unroll
    for (int u = 0; u < 4; ++u) tiles[((size_t)nt * (K >> 5) + g * 4 + u) * 64 + lane] = q4_decode(r.c[u], c);
}

// ---- the norm-on-load GEMM (gemm_bf16_stream_xn, normload_kernels.h) on 4-bit records.  One workgroup per n-tile runs the
// whole k-range (SB == 1) and K % 1024 == 0, so a wave's K / 128 k-steps start and end on a record: group j of the bf16
// loop IS record j of the wave, the k-steps run in the bf16 instance's order and the sums are its sums bit for bit.  The
// prologue and the compact conversion of the rows are that kernel's; what differs is the weight side: a record is 5 dwords
// per lane where a group of bf16 tiles is 16, so the NEXT record is requested before the current one is decoded (two in
// flight per wave), and a k-step's operand is decoded right before its MFMA, one at a time, to stay inside 64 VGPRs.
template <int EPI, int C>
__global__ __launch_bounds__(256, 8) void gemm_q4_stream_xn(const unsigned *__restrict__ Wr, const bf16_t *__restrict__ X,
                                                           int M, int N, int K, GemmEpiT<bf16_t> e) {
    typedef bf16_t H;
    constexpr int G = 4, NCV = (G + C - 1) / C;
    __shared__ f32x4 red[4][1][64];
    __shared__ float ssq_sh[4][16];
    extern __shared__ __attribute__((aligned(16))) char xn_smem[];           // the norm weight, K elements
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int KS = K >> 5, ntg = blockIdx.x;
    const int ng = KS >> 4, ks0 = wv * ng * G;                   // groups per wave (K % 1024 == 0), the wave's first k-step
    const unsigned *rp = Wr + ((size_t)ntg * (KS >> 2) + (size_t)wv * ng) * Q4_REC_DWORDS;
    // ---- prologue requests: norm weight -> LDS by DMA (no registers), the row's partials, then the first record
    const unsigned gs_base = (unsigned)(uintptr_t)xn_smem;
    const u32x4 *gsrc = reinterpret_cast<const u32x4 *>(e.nrm_w);
    for (int j = wv; j < (K >> 9); j += 4) gr_glds16(gsrc + (size_t)j * 64 + lane, gs_base + (unsigned)j * 1024u);
    const int mrow = (lane & 15) < M ? (lane & 15) : 0;
    const int nt = e.nrm_nt, tper = nt >> 4, n4 = tper >> 2;     // nt % 64 == 0
    const float4 *sp = reinterpret_cast<const float4 *>(e.nrm_ssq + (size_t)mrow * nt + (wv * 4 + (lane >> 4)) * tper);
    float4 sv[XN_MAX4];
#pragma unroll
    for (int j = 0; j < XN_MAX4; ++j) sv[j] = sp[min(j, n4 - 1)];
    asm volatile("" ::: "memory");
    Q4Rec cur = q4_fetch(rp, lane);
    asm volatile("" ::: "memory");
    // ---- row totals
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < XN_MAX4; ++j) {
        const bool on = j < n4;
        sum += on ? sv[j].x : 0.f; sum += on ? sv[j].y : 0.f; sum += on ? sv[j].z : 0.f; sum += on ? sv[j].w : 0.f;
    }
    for (int j0 = XN_MAX4; j0 < n4; j0 += XN_MAX4) {             // (hidden > 5120: further passes)
#pragma unroll
        for (int j = 0; j < XN_MAX4; ++j) sv[j] = sp[min(j0 + j, n4 - 1)];
#pragma unroll
        for (int j = 0; j < XN_MAX4; ++j) {
            const bool on = j0 + j < n4;
            sum += on ? sv[j].x : 0.f; sum += on ? sv[j].y : 0.f; sum += on ? sv[j].z : 0.f; sum += on ? sv[j].w : 0.f;
        }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (lane < 16) ssq_sh[wv][lane] = sum;
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");             // the DMA pieces (older than the record's two requests) have landed
    __syncthreads();
    // ---- compact lane (s, quad, m) = lane cj of a conversion register; lanes past C * 4 * M repeat lane 0
    const int cj = lane < C * 4 * M ? lane : 0;
    const int cm = cj % M, ct = cj / M, cq = ct & 3, cs = ct >> 2;
    const float tot = (ssq_sh[0][cm] + ssq_sh[1][cm]) + (ssq_sh[2][cm] + ssq_sh[3][cm]);
    const float r = rsqrtf(tot / (float)K + e.nrm_eps);
    const H *xp = X + (size_t)ks0 * 512 + (cq * 16 + cm) * 8;
    const H *gp = reinterpret_cast<const H *>(xn_smem) + (size_t)ks0 * 32 + cq * 8;
    const int bsrc = (((lane >> 4) * M) + min(lane & 15, M - 1)) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // this lane's k-step of conversion v inside a group: lanes past the conversion's range repeat its first k-step
    auto kof = [&](int v) { return v * C + ((cs < C && v * C + cs < G) ? cs : 0); };
    for (int j = 0; j < ng; ++j) {
        u32x4 xc[NCV];
#pragma unroll
        for (int v = 0; v < NCV; ++v) xc[v] = *reinterpret_cast<const u32x4 *>(xp + (size_t)(j * G + kof(v)) * 512);
        asm volatile("" ::: "memory");
        const Q4Rec nxt = q4_fetch(rp + (size_t)min(j + 1, ng - 1) * Q4_REC_DWORDS, lane);   // (the last one again: in bounds)
#pragma unroll
        for (int v = 0; v < NCV; ++v) {
            xc[v] = norm_frag<H>(xc[v], *reinterpret_cast<const u32x4 *>(gp + (size_t)(j * G + kof(v)) * 32), r);
            __builtin_amdgcn_sched_barrier(0);                    // one conversion's temporaries at a time
        }
        const Q4Lane gc = q4_lane(cur.sz);
#pragma unroll
        for (int u = 0; u < G; ++u) {
            u32x4 x;
            const u32x4 wz = q4_decode(cur.c[u], gc);
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = (unsigned)__builtin_amdgcn_ds_bpermute(bsrc + (u % C) * 16 * M, (int)xc[u / C][i]);
            acc = mfma16<H>(wz, x, acc);
        }
        cur = nxt;
    }
    red[wv][0][lane] = acc;
    __syncthreads();
    gemm_epilogue_step<1, EPI, 1, 1, H>(red, 0, (float *)nullptr, M, 16, N, 0, ntg, e);
}

// ---- the finishing k-split GEMM (gemm_bf16_stream_fin) on 4-bit records.  A wave's k-range [ks0, ks1) is cut in k-steps
// and starts anywhere; records sit at absolute multiples of four k-steps.  The wave walks the records that overlap its
// range, the next one requested before the current one is decoded, and runs one MFMA per k-step of its OWN range, in
// ascending order: the bf16 instance's k-steps in its order on the same fragments, so the same fp32 sums.  The k-steps of
// a boundary record that belong to a neighbour are skipped behind wave-uniform branches (the rows of all four are loaded:
// a record never reaches past K).  Everything behind the k-loop - slabs, counters, finisher - is the bf16 instance's.
__device__ __forceinline__ f32x4 fin_q4_group(const Q4Rec &w, const bf16_t *xg, int lo, int hi, f32x4 acc) {
    u32x4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const u32x4 *>(xg + u * 512);
    const Q4Lane gc = q4_lane(w.sz);
    if (lo <= 0 && hi >= 4) {                                     // a whole record: decode all four, MFMAs back to back
        u32x4 wz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) wz[u] = q4_decode(w.c[u], gc);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = mfma16<bf16_t>(wz[u], x[u], acc);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u >= lo && u < hi) acc = mfma16<bf16_t>(q4_decode(w.c[u], gc), x[u], acc);
    }
    return acc;
}
template <int = 0>
__global__ __launch_bounds__(256) void gemm_q4_stream_fin(const unsigned *__restrict__ Wr, const bf16_t *__restrict__ X,
                                                         float *__restrict__ part, int M, int N, int K, int SB,
                                                         int ks_per_blk, GemmEpiT<bf16_t> e, unsigned *__restrict__ ctr,
                                                         unsigned want, unsigned *__restrict__ wait_status) {
    typedef bf16_t H;
    __shared__ f32x4 red[4][1][64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int NTG = N >> 4, KS = K >> 5;
    const int sb = blockIdx.x / NTG, ntg = blockIdx.x - sb * NTG;
    const bool fin = sb == SB - 1;
    const int kb0 = sb * ks_per_blk, kb1 = min(KS, kb0 + ks_per_blk);
    const int per = (kb1 - kb0 + 3) >> 2;
    const int ks0 = min(kb1, kb0 + wv * per), ks1 = min(kb1, ks0 + per);
    const uint2 xpre = fin ? resid_prefetch<H>(e.res_x, M, N, ntg, (int)threadIdx.x) : uint2{0u, 0u};
    const int mrow = (lane & 15) < M ? (lane & 15) : 0;           // rows >= M read row 0 (their output columns are dropped)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (ks0 < ks1) {
        const int ga = ks0 >> 2, gb = (ks1 + 3) >> 2;             // records ga .. gb - 1, all inside K / 128
        const unsigned *rp = Wr + (size_t)ntg * (KS >> 2) * Q4_REC_DWORDS;
        const H *xl = X + ((lane >> 4) * 16 + mrow) * 8;
        Q4Rec cur = q4_fetch(rp + (size_t)ga * Q4_REC_DWORDS, lane);
        for (int g = ga; g < gb; ++g) {
            const Q4Rec nxt = q4_fetch(rp + (size_t)min(g + 1, gb - 1) * Q4_REC_DWORDS, lane);
            acc = fin_q4_group(cur, xl + (size_t)g * 4 * 512, ks0 - g * 4, ks1 - g * 4, acc);
            cur = nxt;
        }
    }
    red[wv][0][lane] = acc;
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int l = lane, m = l & 15;
    float *slab = part + ((size_t)ntg * 16 + m) * 16 + (l >> 4) * 4;             // + s * 16 * N for slab s (tile-major)
    const f32x4 own = (red[0][0][l] + red[1][0][l]) + (red[2][0][l] + red[3][0][l]);
    if (!fin) {
        if (m < M) store_f32x4<true>(slab + (size_t)sb * 16 * N, own);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the slab has left this wave
        if (l == 0) (void)__hip_atomic_fetch_add(ctr + ntg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    bool timed_out = false;
    if (SB > 1) {
        const long long t0 = wall_clock64();
        for (;;) {
            const unsigned got = __hip_atomic_load(ctr + ntg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)(got - want) >= 0) break;
            __builtin_amdgcn_s_sleep(2);
            if (wall_clock64() - t0 > FIN_TIMEOUT_TICKS) { timed_out = true; break; }
        }
    }
    asm volatile("" ::: "memory");
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int s2 = 0; s2 + 1 < SB; ++s2)
        if (m < M) a += load_f32x4_sc1(slab + (size_t)s2 * 16 * N);
    a += own;
    if (timed_out) {
        a = f32x4{__uint_as_float(0x7fc00000u), 0.f, 0.f, 0.f};
        if (l == 0) (void)__hip_atomic_fetch_or(wait_status, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    red[0][0][l] = a;
    red[1][0][l] = red[2][0][l] = red[3][0][l] = f32x4{0.f, 0.f, 0.f, 0.f};
    resid_epilogue_step<H>(red, M, N, ntg, e, l, xpre);
}
