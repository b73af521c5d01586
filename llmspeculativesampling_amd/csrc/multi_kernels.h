// multi_kernels.h - device code of the native width-w loop (sd_spec_multi_generate, reference
// speculative_sampling.py:1379-1716 with strategy "iid") that is not sampling: the winner broadcast.
#pragma once
#include "common.h"

// Per-replica pointers of the broadcast, passed by value (width <= 16).
struct AdoptTab {
    char *d_kv[16], *t_kv[16];       // draft / target KV arenas [L][2][Hkv][max_seq][D]
    int32_t *seq[16];                // token buffers
};
// One arena family: `planes` = L * 2 * Hkv planes of max_seq rows of row_bytes bytes; positions [lo, hi) are adopted.
struct AdoptArena { int planes, max_seq, row_bytes, lo; };

// Block-cooperative byte copy, dst and src of any alignment: 16-byte vector accesses over the common aligned body when
// the two pointers are congruent mod 16, plain bytes for the unaligned head, the tail and the incongruent case.
__device__ __forceinline__ void adopt_copy_bytes(char *__restrict__ dst, const char *__restrict__ src, int nbytes) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const uintptr_t ds = (uintptr_t)dst, ss = (uintptr_t)src;
    if (((ds ^ ss) & 15) != 0) {
        for (int i = tid; i < nbytes; i += nt) dst[i] = src[i];
        return;
    }
    int head = (int)((16 - (ss & 15)) & 15);
    if (head > nbytes) head = nbytes;
    const int nvec = (nbytes - head) >> 4, tail0 = head + (nvec << 4);
    if (tid < head) dst[tid] = src[tid];
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + head);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
    for (int i = tid; i < nvec; i += nt) d4[i] = s4[i];
    if (tail0 + tid < nbytes) dst[tail0 + tid] = src[tail0 + tid];        // head, tail < 16 <= blockDim.x
}

// The winner broadcast of one width-w iteration, both models and the tokens in ONE launch, ordered behind the fused
// accept / resample launch by the stream alone.  The ranges come from the DEVICE result block (multi.py computes them on
// the host after a synchronisation):
//     new_draft  = min(L + gamma - 1, n + 1)         draft  KV positions [d.lo, new_draft)
//     new_target = all_accept ? L + gamma : n + 1    target KV positions [t.lo, new_target)
//     tokens seq[L .. n + 2)
// of the winner `choice` go to every other replica.  Grid (x, y): x = one workgroup per draft plane, per target plane, and
// one for the tokens; y = the destination replica.  The launch does not depend on the result: the workgroups of row
// y == choice and those whose range is empty exit.  A plane's positions are contiguous ([max_seq][D]), so each range is one
// byte run of (hi - lo) * row_bytes bytes whatever the element type (fp32, 16-bit, fp8) - at most (gamma + 1) rows, a few
// KiB, which 128 lanes move in one to five 16-byte accesses each.  A result block that does not describe this iteration
// (choice / n out of range) copies nothing.
__global__ __launch_bounds__(128) void multi_adopt_kernel(AdoptTab t, int width, const sd_multi_result *__restrict__ res,
                                                         int L, int gamma, AdoptArena d, AdoptArena tg, int seq_cap) {
    const int choice = res->choice, n = res->chosen.n;
    const bool all_accept = (res->chosen.flags & 4) != 0;
    const int w = blockIdx.y;
    if (choice < 0 || choice >= width || n < L - 1 || n > L + gamma - 1 || w == choice || w >= width) return;
    int b = blockIdx.x, kind = 2;                                 // 0 draft plane, 1 target plane, 2 the tokens
    size_t off;
    int nbytes;
    if (b < d.planes + tg.planes) {
        const bool draft = b < d.planes;
        const AdoptArena a = draft ? d : tg;
        kind = draft ? 0 : 1;
        if (!draft) b -= d.planes;
        int hi = draft ? min(L + gamma - 1, n + 1) : (all_accept ? L + gamma : n + 1);
        hi = min(hi, a.max_seq);
        if (a.lo < 0 || hi <= a.lo) return;
        off = ((size_t)b * a.max_seq + a.lo) * a.row_bytes;
        nbytes = (hi - a.lo) * a.row_bytes;
    } else {
        const int hi = min(n + 2, seq_cap);
        if (hi <= L) return;
        off = (size_t)L * sizeof(int32_t);
        nbytes = (hi - L) * (int)sizeof(int32_t);
    }
    auto arena = [&](int r) -> char * {
        return kind == 0 ? t.d_kv[r] : (kind == 1 ? t.t_kv[r] : reinterpret_cast<char *>(t.seq[r]));
    };
    adopt_copy_bytes(arena(w) + off, arena(choice) + off, nbytes);
}
