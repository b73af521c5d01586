// Lossless 12-bit records of a bf16 weight matrix in the streaming tile order ("12-bit records").
// A 16 x 32 tile (64 lanes x 8 bf16, 1 KiB) becomes 64 lanes x 3 dwords of codes (768 B) plus one 16-byte side record:
// per element the sign, the 7 mantissa bits and a 4-bit exponent code E - base, where base = max(E_max(tile) - 14, 0).
// An element whose exponent lies below the window ("escape": zeros and denormals under a large tile maximum) stores code 0
// and gets one of the side record's six entries (position, true exponent); the decoder repairs it in the register, so the
// fragment that reaches the MFMA is the bf16 tile bit for bit.  A matrix with a tile of more than six escapes is not
// packable (the packer says so and the matrix stays bf16).  Every record has a fixed size and a fixed address and no load
// depends on another load.
//
//   codes, lane l of a tile (l holds W[n = l % 16][k = (l / 16) * 8 .. + 8) as four dwords o0..o3 of two bf16 each):
//     p0 = (o0 & SM) | rotl32(o1 & SM, 8)     SM = 0x807f807f: sign and mantissa of both halves
//     p1 = (o2 & SM) | rotl32(o3 & SM, 8)
//     p2 = sum_i code(2i) << 4i | code(2i + 1) << (16 + 4i)
//   side record of a tile (four dwords):
//     m0 = base | c << 8 | E_0 << 16 | E_1 << 24          c = number of escapes (0..6)
//     m1 = E_2 | E_3 << 8 | E_4 << 16 | E_5 << 24         E_j = true exponent field of escape j
//     m2 = pos_0 | pos_1 << 9 | pos_2 << 18               pos_j = lane * 8 + element, ascending
//     m3 = pos_3 | pos_4 << 9 | pos_5 << 18               (unused entries are zero)
//   decode: o_i = ((sm_i & SM) | (shift(p2, 7 - 4i) & 0x07800780)) + base * 0x00800080, then for every escape the
//   exponent field of its element, which holds `base`, is lowered by base - E_j.
#pragma once
#include "model_kernels.h"

using u32x3 = __attribute__((ext_vector_type(3))) unsigned int;
typedef u32x3 u32x3_a4 __attribute__((aligned(4)));             // (a 12-byte record: the vector type itself is 16-aligned)
#define W12_CONST __attribute__((address_space(4)))          // uniform loads from it are scalar loads
#define W12_SM 0x807f807fu
#define W12_CM 0x07800780u
#define W12_MAX_ESC 6
#define W12_TILE_DWORDS 192                                  // 64 lanes x 3

struct W12Arg { const unsigned *codes; const u32x4 *meta; };

// The decode comes in two parts, so that a kernel can decode a whole burst of tiles straight-line and settle the escapes of
// the burst behind ONE uniform branch (gemm_bf16_stream_fin, normload_kernels.h): the codes under the tile's base, no
// branch, and the repair of the decoded fragment from the side record.  w12_escapes is the burst's predicate: OR the m[0]
// words of the burst's side records (scalar registers) and pass the result.
__device__ __forceinline__ u32x4 w12_decode(u32x3 p, unsigned base) {
    const unsigned bb = base * 0x00800080u;
    u32x4 o;
    o[0] = ((p[0] & W12_SM) | ((p[2] << 7) & W12_CM)) + bb;
    o[1] = ((__builtin_amdgcn_alignbit(p[0], p[0], 8) & W12_SM) | ((p[2] << 3) & W12_CM)) + bb;
    o[2] = ((p[1] & W12_SM) | ((p[2] >> 1) & W12_CM)) + bb;
    o[3] = ((__builtin_amdgcn_alignbit(p[1], p[1], 8) & W12_SM) | ((p[2] >> 5) & W12_CM)) + bb;
    return o;
}
__device__ __forceinline__ unsigned w12_escapes(unsigned m0) { return (m0 >> 8) & 7u; }
__device__ __forceinline__ void w12_repair(u32x4 &o, u32x4 m, int lane) {
    const unsigned base = m[0] & 0xffu;
    const int c = (int)w12_escapes(m[0]);
    if (c != 0) {                                             // (uniform where m is: ~5 % of the tiles of N(0, 1/sqrt(K)) weights)
#pragma unroll
        for (int j = 0; j < W12_MAX_ESC; ++j) {
            if (j < c) {
                const unsigned E = j < 2 ? (m[0] >> (16 + 8 * j)) & 0xffu : (m[1] >> (8 * (j - 2))) & 0xffu;
                const unsigned pos = (m[2 + j / 3] >> (9 * (j % 3))) & 0x1ffu;
                const unsigned d = (base - E) << (7u + 16u * (pos & 1u)), dw = (pos >> 1) & 3u;
                const bool mine = lane == (int)(pos >> 3);
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] -= (mine && dw == (unsigned)i) ? d : 0u;
            }
        }
    }
}

// ---- the two weight fetches of the norm-on-load / finishing GEMMs (normload_kernels.h): what a lane requests for one
// k-step, and the u32x4 MFMA operand it becomes.  `tile` is the workgroup's (n-tile, first k-step) index, k a k-step
// offset from it.
struct WFetchBf16 {
    typedef const u32x4 *__restrict__ Arg;
    typedef u32x4 Frag;
    const u32x4 *p;
    __device__ __forceinline__ WFetchBf16(Arg W, size_t tile, int lane) : p(W + tile * 64 + lane) {}
    __device__ __forceinline__ Frag fetch(size_t k) const { return __builtin_nontemporal_load(p + k * 64); }
    __device__ __forceinline__ void advance(int n) { p += (size_t)n * 64; }
    static __device__ __forceinline__ u32x4 frag(const Frag &f, int) { return f; }
    static constexpr bool kRecords = false;
};
struct WFetchW12 {
    typedef W12Arg Arg;
    struct Frag { u32x3 v; u32x4 m; };
    const unsigned *p;
    const W12_CONST u32x4 *mp;
    __device__ __forceinline__ WFetchW12(Arg W, size_t tile, int lane)
        : p(W.codes + (tile * 64 + lane) * 3),
          mp((const W12_CONST u32x4 *)(uintptr_t)(W.meta + __builtin_amdgcn_readfirstlane((int)tile))) {}
    __device__ __forceinline__ Frag fetch(size_t k) const {
        return Frag{__builtin_nontemporal_load(reinterpret_cast<const u32x3_a4 *>(p + k * W12_TILE_DWORDS)), mp[k]};
    }
    __device__ __forceinline__ void advance(int n) { p += (size_t)n * W12_TILE_DWORDS; mp += n; }
    static __device__ __forceinline__ u32x4 decode(const Frag &f) { return w12_decode(f.v, f.m[0] & 0xffu); }
    static __device__ __forceinline__ void repair(u32x4 &o, const Frag &f, int lane) { w12_repair(o, f.m, lane); }
    static __device__ __forceinline__ u32x4 frag(const Frag &f, int lane) {
        u32x4 o = decode(f);
        repair(o, f, lane);
        return o;
    }
    static constexpr bool kRecords = true;
};

// ---- packer: one wave per tile.  *status |= 1 when a tile has more than W12_MAX_ESC escapes (its records are still
// written, in bounds, and mean nothing).  (A template, like the expander: a kernel takes its place in the code object where it
// is first instantiated, and these two are instantiated after every kernel of the forward - engine.hip.)
template <int = 0>
__global__ __launch_bounds__(64) void w12_pack_kernel(const u32x4 *__restrict__ src, unsigned *__restrict__ codes,
                                                      u32x4 *__restrict__ meta, int *__restrict__ status) {
    __shared__ unsigned ent[W12_MAX_ESC];
    const int lane = threadIdx.x;
    const size_t tile = blockIdx.x;
    const u32x4 o = src[tile * 64 + lane];
    unsigned E[8], emax = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        E[e] = (o[e >> 1] >> (7 + 16 * (e & 1))) & 0xffu;
        emax = max(emax, E[e]);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) emax = max(emax, (unsigned)__shfl_xor((int)emax, d, 64));
    const unsigned base = emax > 14u ? emax - 14u : 0u;
    unsigned p2 = 0, n_esc = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bool esc = E[e] < base;
        n_esc += esc ? 1u : 0u;
        p2 |= (esc ? 0u : E[e] - base) << (4 * (e >> 1) + 16 * (e & 1));
    }
    unsigned incl = n_esc;                                       // escapes of lanes <= this one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)incl, d, 64);
        incl += lane >= d ? t : 0u;
    }
    const unsigned total = (unsigned)__shfl((int)incl, 63, 64);
    if (lane < W12_MAX_ESC) ent[lane] = 0u;
    __syncthreads();
    unsigned at = incl - n_esc;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (E[e] < base) {
            if (at < W12_MAX_ESC) ent[at] = (unsigned)(lane * 8 + e) | E[e] << 9;
            ++at;
        }
    __syncthreads();
    unsigned *cp = codes + (tile * 64 + lane) * 3;
    cp[0] = (o[0] & W12_SM) | __builtin_amdgcn_alignbit(o[1] & W12_SM, o[1] & W12_SM, 24);
    cp[1] = (o[2] & W12_SM) | __builtin_amdgcn_alignbit(o[3] & W12_SM, o[3] & W12_SM, 24);
    cp[2] = p2;
    if (lane == 0) {
        const unsigned c = min(total, (unsigned)W12_MAX_ESC);
        u32x4 m;
        m[0] = base | c << 8 | (ent[0] >> 9) << 16 | (ent[1] >> 9) << 24;
        m[1] = (ent[2] >> 9) | (ent[3] >> 9) << 8 | (ent[4] >> 9) << 16 | (ent[5] >> 9) << 24;
        m[2] = (ent[0] & 0x1ffu) | (ent[1] & 0x1ffu) << 9 | (ent[2] & 0x1ffu) << 18;
        m[3] = (ent[3] & 0x1ffu) | (ent[4] & 0x1ffu) << 9 | (ent[5] & 0x1ffu) << 18;
        meta[tile] = m;
        if (total > W12_MAX_ESC) atomicOr(status, 1);
    }
}

// ---- expander (the format's executable definition and the tests' hook): records -> the tiled bf16 layout
template <int = 0>
__global__ __launch_bounds__(64) void w12_unpack_kernel(W12Arg W, u32x4 *__restrict__ dst) {
    const int lane = threadIdx.x;
    WFetchW12 wf(W, blockIdx.x, lane);
    dst[(size_t)blockIdx.x * 64 + lane] = WFetchW12::frag(wf.fetch(0), lane);
}
