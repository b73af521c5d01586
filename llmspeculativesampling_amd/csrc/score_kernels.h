// score_kernels.h - token scoring of logit rows (sd_score_rows): per row the log-probability and the rank of one token and
// the top_n ids of the row with their log-probabilities, for up to 16 items x 80 rows in ONE launch.  include/specdec.h has
// the definition; the (m, s) pair is lse_row's (logprob_kernels.h), so the log-probabilities are sd_token_logprobs' bits.
#pragma once
#include "logprob_kernels.h"

enum {
    SCORE_THREADS = LOGPROB_THREADS,
    SCORE_MAX_ITEMS = 16,
    SCORE_CAND = 12288,      // ids the gather pass can hold (48 KiB of LDS)
    SCORE_CAND2 = 1024,      // the second list of the thinning rounds: >= SD_SCORE_MAX_TOP * SCORE_CAND / SCORE_THREADS
};
static_assert(SD_SCORE_MAX_TOP * (SCORE_CAND / SCORE_THREADS) <= SCORE_CAND2 && SD_SCORE_MAX_TOP * (SCORE_CAND2 / SCORE_THREADS) <= SCORE_CAND2,
              "a thinning round must fit the list it writes");
static_assert(SD_SCORE_MAX_TOP <= 64, "the last survivors are ordered by one wave");

// The items of one launch, passed by value (as LogprobTab is).
struct ScoreTab {
    const float *logits[SCORE_MAX_ITEMS];              // `rows` consecutive rows, row stride ld >= V
    const int32_t *tokens[SCORE_MAX_ITEMS];            // row r is scored at tokens[r]
    float *logprob[SCORE_MAX_ITEMS];                   // `rows` floats
    int32_t *rank[SCORE_MAX_ITEMS];                    // `rows` ranks, or NULL
    int32_t *top_ids[SCORE_MAX_ITEMS];                 // rows x top_n (unread when top_n == 0)
    float *top_logprobs[SCORE_MAX_ITEMS];
    long ld[SCORE_MAX_ITEMS];
    int rows[SCORE_MAX_ITEMS];
};

typedef unsigned long long score_word;

// Order-preserving key of a float: a < b <=> key(a) < key(b), -0.0 folded onto +0.0 as a float compare has it (the sampler's
// fkey lives in the other translation unit).  With the id below it the key becomes the row's order in ONE word: value
// descending, ties to the lower id, is the word descending - and no two entries of a row share a word.  0 is no entry's word.
__device__ __forceinline__ uint32_t score_key(float f) {
    const uint32_t u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ score_word score_order(float f, int id) {
    return ((score_word)score_key(f) << 32) | (uint32_t)~(uint32_t)id;
}

// Every entry of the row, rounded, with its id: lse_row's traversal (scalar head, 16-byte loads, scalar tail) without the sum.
template <int DT, class F>
__device__ __forceinline__ void score_for_each(const float *x, int V, int tid, F &&f) {
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2));
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    if (tid < head) f(rnd_dt(x[tid], DT), tid);
    const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
#pragma unroll 4
    for (int i = tid; i < n4; i += SCORE_THREADS) {
        const float4 v = x4[i];
        const int id = head + 4 * i;
        f(rnd_dt(v.x, DT), id); f(rnd_dt(v.y, DT), id + 1); f(rnd_dt(v.z, DT), id + 2); f(rnd_dt(v.w, DT), id + 3);
    }
    if (tail0 + tid < V) f(rnd_dt(x[tail0 + tid], DT), tail0 + tid);
}

// The k-th largest (1 <= k <= 256) of the workgroup's 256 words, one per thread.  A thread without an entry (word 0) takes part
// with a word of its own below every entry's (an entry's key is at least -inf's, 0x007fffff), so that no two words are equal
// and a thread's place is a count of one compare; such a result keeps every entry.  Every thread gets it.  sh: 257 words.
__device__ __forceinline__ score_word score_kth_of_threads(score_word mine, int k, score_word *sh, int tid) {
    if (mine == 0) mine = (score_word)(SCORE_THREADS - 1 - tid);
    __syncthreads();                                              // (the last call's result has been read)
    sh[tid] = mine;
    __syncthreads();
    int above = 0;
#pragma unroll 8
    for (int j = 0; j < SCORE_THREADS; ++j) above += sh[j] > mine;
    if (above == k - 1) sh[SCORE_THREADS] = mine;
    __syncthreads();
    return sh[SCORE_THREADS];
}

// Grid (x, y) = (row, item), one workgroup of 256 threads per row.
//   1. lse_row: (m, s), and each thread's first word of the row's order among the entries it read.  The top_n-th largest of
//      those 256 words is a threshold `thr` that at least top_n entries reach and that the row's top_n all reach; the entries
//      that reach it lie in the stripes of exactly top_n threads.
//   2. One more pass (L2): the ids of the entries that reach thr go to an LDS list, and the entries ahead of the token are
//      counted - its rank.
//   3. The list is thinned by the same threshold step (each thread the best of its share of the list) until one wave holds
//      it; that wave orders it and writes the first top_n.
// A list that outgrows its 12288 ids (more than top_n * (4 * ceil(V / 1024) + 2) entries cannot reach thr, so no row of
// V <= 156672 does) is replaced by the exact cut: the top_n-th largest word by bisection over its 64 bits, one counting pass per bit.
template <int DT>
__global__ __launch_bounds__(SCORE_THREADS) void score_rows_kernel(ScoreTab t, int V, int top_n) {
    const int b = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    if (r >= t.rows[b]) return;
    const float *x = t.logits[b] + (size_t)r * t.ld[b];
    __shared__ float sh_m[SCORE_THREADS / 64], sh_s[SCORE_THREADS / 64];
    __shared__ score_word sh_word[SCORE_THREADS + 1];
    __shared__ int sh_n, sh_ahead;
    __shared__ int cand[SCORE_CAND + SCORE_CAND2];

    score_word best = 0;
    lse_row<DT>(x, V, tid, sh_m, sh_s, [&](float v, int id) {
        const score_word w = score_order(v, id);
        best = w > best ? w : best;
    });
    float m, s;
    lse_fold(sh_m, sh_s, m, s);
    const float log_s = logf(s);
    const int tok = t.tokens[b][r];
    const bool tok_ok = tok >= 0 && tok < V;
    const float xt = tok_ok ? rnd_dt(x[tok], DT) : __builtin_nanf("");
    if (tid == 0) t.logprob[b][r] = (xt - m) - log_s;            // (token_logprob_kernel's expression: NaN on a void row)
    int32_t *const rank_out = t.rank[b];
    int32_t *const ids_out = top_n ? t.top_ids[b] + (size_t)r * top_n : nullptr;
    float *const lps_out = top_n ? t.top_logprobs[b] + (size_t)r * top_n : nullptr;
    if (!(s > 0.f && s < __builtin_inff())) {                     // void: a NaN or +inf entry, or nothing but -inf
        if (tid == 0 && rank_out) rank_out[r] = 0;
        if (tid < top_n) { ids_out[tid] = -1; lps_out[tid] = __builtin_nanf(""); }
        return;
    }
    if (top_n == 0 && !(rank_out && tok_ok)) {                    // nothing is left to read the row for
        if (tid == 0 && rank_out) rank_out[r] = 0;
        return;
    }

    // ---- 2. gather and count
    const score_word none = ~(score_word)0;                       // (above every entry's word: key 0xffffffff is a NaN's)
    score_word thr = top_n ? score_kth_of_threads(best, top_n, sh_word, tid) : none;
    const score_word wt = tok_ok ? score_order(xt, tok) : none;
    if (tid == 0) { sh_n = 0; sh_ahead = 0; }
    __syncthreads();
    int ahead = 0;
    score_for_each<DT>(x, V, tid, [&](float v, int id) {
        const score_word w = score_order(v, id);
        ahead += w > wt;
        if (w >= thr) {
            const int slot = atomicAdd(&sh_n, 1);
            if (slot < SCORE_CAND) cand[slot] = id;
        }
    });
    if (ahead) atomicAdd(&sh_ahead, ahead);
    __syncthreads();
    if (tid == 0 && rank_out) rank_out[r] = tok_ok ? 1 + sh_ahead : 0;
    if (top_n == 0) return;
    int n = sh_n;

    if (n > SCORE_CAND) {                                         // the exact cut instead: count(word >= cut) == top_n
        score_word cut = 0;
        for (int bit = 63; bit >= 0; --bit) {
            const score_word trial = cut | ((score_word)1 << bit);
            __syncthreads();
            if (tid == 0) sh_n = 0;
            __syncthreads();
            int c = 0;
            score_for_each<DT>(x, V, tid, [&](float v, int id) { c += score_order(v, id) >= trial; });
            if (c) atomicAdd(&sh_n, c);
            __syncthreads();
            if (sh_n >= top_n) cut = trial;
        }
        __syncthreads();
        if (tid == 0) sh_n = 0;
        __syncthreads();
        score_for_each<DT>(x, V, tid, [&](float v, int id) {
            if (score_order(v, id) >= cut) {
                const int slot = atomicAdd(&sh_n, 1);
                if (slot < SCORE_CAND) cand[slot] = id;
            }
        });
        __syncthreads();
        n = min(sh_n, (int)SCORE_CAND);
    }

    // ---- 3. thin the list until one wave holds it: a round leaves at most top_n * ceil(n / 256) ids
    int src = 0, dst = SCORE_CAND, dst_cap = SCORE_CAND2;
    while (n > 64) {
        score_word mine = 0;
        for (int j = tid; j < n; j += SCORE_THREADS) {
            const int id = cand[src + j];
            const score_word w = score_order(rnd_dt(x[id], DT), id);
            mine = w > mine ? w : mine;
        }
        thr = score_kth_of_threads(mine, top_n, sh_word, tid);
        if (tid == 0) sh_n = 0;
        __syncthreads();
        for (int j = tid; j < n; j += SCORE_THREADS) {
            const int id = cand[src + j];
            if (score_order(rnd_dt(x[id], DT), id) >= thr) {
                const int slot = atomicAdd(&sh_n, 1);
                if (slot < dst_cap) cand[dst + slot] = id;
            }
        }
        __syncthreads();
        n = min(sh_n, dst_cap);
        const int was = src;
        src = dst; dst = was; dst_cap = was == 0 ? (int)SCORE_CAND : (int)SCORE_CAND2;
    }

    // ---- the last <= 64 survivors, one per lane of wave 0: a lane's place is the number of words above its own
    if (tid >= 64) return;
    int id = -1;
    float v = 0.f;
    score_word w = 0;
    if (tid < n) {
        id = cand[src + tid];
        v = rnd_dt(x[id], DT);
        w = score_order(v, id);
    }
    int place = 0;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(w >> 32), j);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)w, j);
        place += (((score_word)hi << 32) | lo) > w;
    }
    if (w != 0 && place < top_n) { ids_out[place] = id; lps_out[place] = (v - m) - log_s; }
    if (tid >= n && tid < top_n) { ids_out[tid] = -1; lps_out[tid] = __builtin_nanf(""); }   // (n < top_n only when V < top_n)
}

static int launch_score_rows(const ScoreTab &t, int n_items, int max_rows, int V, int top_n, int dt, hipStream_t st) {
    const dim3 grid(max_rows, n_items), block(SCORE_THREADS);
    if (dt == 1) hipLaunchKernelGGL(score_rows_kernel<1>, grid, block, 0, st, t, V, top_n);
    else if (dt == 2) hipLaunchKernelGGL(score_rows_kernel<2>, grid, block, 0, st, t, V, top_n);
    else hipLaunchKernelGGL(score_rows_kernel<0>, grid, block, 0, st, t, V, top_n);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
