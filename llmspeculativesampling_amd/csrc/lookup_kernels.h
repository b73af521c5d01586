// lookup_kernels.h - prompt-lookup (n-gram) drafting without a draft model (sd_lookup_propose): the most recent earlier
// occurrence of a sequence's last few tokens is found in its device-resident token buffer, the tokens that followed it become
// the gamma drafted tokens, and the gamma draft rows of q_hist become their one-hot rows, so that the accept / residual kernels
// read them like a draft model's.  Up to 16 streams in ONE launch.  include/specdec.h has the definition and the contract.
#pragma once
#include "common.h"

// LOOKUP_WINDOW: floats of a row one workgroup fills (4 x 16 bytes per lane)
enum { LOOKUP_THREADS = 256, LOOKUP_MAX_ITEMS = 16, LOOKUP_MAX_GAMMA = 16, LOOKUP_VEC = 4,
       LOOKUP_WINDOW = LOOKUP_THREADS * LOOKUP_VEC * 4 };

// The items of one launch, passed by value (as PenaltyTab is).
struct LookupTab {
    int32_t *seq[LOOKUP_MAX_ITEMS];                    // tokens [0, L) are read, [L, L + gamma) written
    float *q_hist[LOOKUP_MAX_ITEMS];                   // rows L-1 .. L+gamma-2 (row stride ld) become one-hot
    int32_t *info[LOOKUP_MAX_ITEMS];                   // {match length, c}
    int L[LOOKUP_MAX_ITEMS];
};

// Grid (x, y) = (row * windows + window, item), 256 threads.  EVERY workgroup of an item repeats the item's match - L ints
// that sit in L2 after the first workgroup read them - so no workgroup waits for another and the result does not depend on
// which one ran first: the key (the last n_max tokens) in registers, one candidate continuation index c per lane and stride
// (c = 1 + tid, + 256, ...; lane-consecutive c read consecutive tokens), the match length k(c) by comparing backwards from
// c - 1 against the key, and the maximum of the packed (k, c) over the workgroup - 64 bits, so any c of an int32 sequence
// fits - through one LDS word (a maximum is the same in any order).  A candidate below n_min counts as none; with none the
// continuation is c = L - 1 at length 0.  The workgroup then fills its own window of its own row: zeros, 1.0f at the drafted
// token when that lies in the window (an id outside [0, V) lights nothing and is never used as an index).  Rows start anywhere:
// a scalar head up to the first 16-byte boundary (window 0 takes it), 16 bytes per lane, a scalar tail.  Workgroup 0 of an
// item also writes the gamma tokens and the two info ints; it reads seq[c + i mod (L - c)], which lies inside [0, L), so the
// tokens it writes at [L, L + gamma) are never read by this launch.
__global__ __launch_bounds__(LOOKUP_THREADS) void lookup_propose_kernel(LookupTab t, int V, long ld, int gamma, int n_max,
                                                                         int n_min, int windows) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int row = blockIdx.x / windows, w = blockIdx.x - row * windows;
    const int32_t *seq = t.seq[b];
    const int L = t.L[b];
    __shared__ unsigned long long s_best;
    if (tid == 0) s_best = 0ull;
    int key[SD_LOOKUP_MAX_NGRAM];                                 // key[j] = seq[L - 1 - j]
#pragma unroll
    for (int j = 0; j < SD_LOOKUP_MAX_NGRAM; ++j) key[j] = j < n_max && j < L ? seq[L - 1 - j] : -1;
    __syncthreads();
    unsigned long long best = 0ull;
    for (int c = 1 + tid; c <= L - 1; c += LOOKUP_THREADS) {
        const int lim = min(n_max, c);
        int k = 0;
#pragma unroll
        for (int j = 0; j < SD_LOOKUP_MAX_NGRAM; ++j) {
            if (j >= lim || k != j) break;
            if (seq[c - 1 - j] == key[j]) k = j + 1;
        }
        // packed (k, c): the longer match wins, among equal lengths the larger c; 0 = nothing that counts
        const unsigned long long cand = k >= n_min ? ((unsigned long long)k << 32) | (unsigned)c : 0ull;
        best = cand > best ? cand : best;
    }
    if (best) atomicMax(&s_best, best);
    __syncthreads();
    const unsigned long long m = s_best;
    const int k_best = (int)(m >> 32), c_best = m ? (int)(m & 0xffffffffu) : L - 1;
    const int period = L - c_best;                                // >= 1
    const int tok = seq[c_best + row % period];                   // the row's drafted token
    if (blockIdx.x == 0) {
        if (tid < gamma) t.seq[b][L + tid] = seq[c_best + tid % period];
        if (tid == 64) t.info[b][0] = k_best;
        if (tid == 65) t.info[b][1] = c_best;
    }
    // ---- this workgroup's window of row `row`: columns [lo, hi)
    float *o = t.q_hist[b] + (size_t)(L - 1 + row) * ld;
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)o & 15u)) & 15u) >> 2));
    const int lo = w == 0 ? 0 : head + w * LOOKUP_WINDOW;
    if (lo >= V) return;
    const int hi = min(V, head + (w + 1) * LOOKUP_WINDOW);
    const int a = max(lo, head);                                  // the 16-byte body is [a, a + 4 * n4)
    const int n4 = (hi - a) >> 2, tail0 = a + 4 * n4;
    for (int i = lo + tid; i < a; i += LOOKUP_THREADS) o[i] = i == tok ? 1.0f : 0.0f;
    float4 *o4 = reinterpret_cast<float4 *>(o + a);
#pragma unroll
    for (int u = 0; u < LOOKUP_VEC; ++u) {
        const int i = tid + u * LOOKUP_THREADS, id = a + 4 * i;
        if (i >= n4) continue;
        o4[i] = make_float4(id == tok ? 1.0f : 0.0f, id + 1 == tok ? 1.0f : 0.0f, id + 2 == tok ? 1.0f : 0.0f,
                            id + 3 == tok ? 1.0f : 0.0f);
    }
    for (int i = tail0 + tid; i < hi; i += LOOKUP_THREADS) o[i] = i == tok ? 1.0f : 0.0f;
}

static int launch_lookup_propose(const LookupTab &t, int n_items, int V, long ld, int gamma, int n_max, int n_min, hipStream_t st) {
    const int windows = (V + LOOKUP_WINDOW - 1) / LOOKUP_WINDOW;
    hipLaunchKernelGGL(lookup_propose_kernel, dim3(gamma * windows, n_items), dim3(LOOKUP_THREADS), 0, st, t, V, ld, gamma, n_max,
                       n_min, windows);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
