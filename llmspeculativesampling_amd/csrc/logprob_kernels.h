// logprob_kernels.h - per-token target log-probabilities (sd_token_logprobs): logprob = x[t] - log sum_v exp(x[v]) in fp32 of
// the raw logit rows a verify pass (or an autoregressive step) left on the device, for up to 16 items x 17 rows in ONE launch.
// The decode loops run it behind their accept / resample launch, which decides how many of a stream's rows count.
#pragma once
#include "common.h"

enum { LOGPROB_THREADS = 256, LOGPROB_MAX_ITEMS = 16, LOGPROB_MAX_ROWS = 17 };

// The items of one launch, passed by value (as AcceptTab is).
struct LogprobTab {
    const float *logits[LOGPROB_MAX_ITEMS];            // `rows` consecutive rows, row stride ld >= V
    const int32_t *tokens[LOGPROB_MAX_ITEMS];          // row r is scored at tokens[r]
    const sd_accept_result *res[LOGPROB_MAX_ITEMS];    // or NULL; with it only rows r <= res->n_accepted are scored
    float *out[LOGPROB_MAX_ITEMS];                     // `rows` floats
    long ld[LOGPROB_MAX_ITEMS];
    int rows[LOGPROB_MAX_ITEMS];
};

// A running (max, sum of exp(x - max)) pair.  m starts at -FLT_MAX, not -inf, so that exp(x - m) of a -inf entry is
// exp(-inf) = 0 and never exp(-inf + inf); a row of nothing but -inf ends with s == 0 and scores NaN.  fmaxf drops a NaN
// entry from m, exp(NaN - m) carries it into s.
struct LseAcc {
    float m, s;
    // the rescale runs only where the maximum rises (a few times per lane), so it can afford the exact expf
    __device__ __forceinline__ void lift(float mx) {
        if (mx > m) { s *= expf(m - mx); m = mx; }
    }
    __device__ __forceinline__ void add(float x) {
        lift(x);
        s += __expf(x - m);
    }
    __device__ __forceinline__ void add4(float a, float b, float c, float d) {
        lift(fmaxf(fmaxf(a, b), fmaxf(c, d)));
        s += (__expf(a - m) + __expf(b - m)) + (__expf(c - m) + __expf(d - m));
    }
};

// The row traversal sd_token_logprobs and sd_score_rows share (score_kernels.h), so that the two give the same (m, s) bit for
// bit: one pass over the row by a 256-thread workgroup - a scalar head up to the first 16-byte boundary (rows of an arena, or
// of a slab whose ld is no multiple of 4, start anywhere), 16 bytes per lane, a scalar tail - then the wave's pairs by
// cross-lane moves; the four waves' pairs are left in sh_m / sh_s (behind a barrier) for lse_fold.  DT: the rows still have
// to be rounded to a 16-bit type (rnd_dt's codes).  visit(x, id) sees every entry this thread reads, rounded, its ids ascending.
struct LseNoVisit {
    __device__ __forceinline__ void operator()(float, int) const {}
};
template <int DT, class Visit>
__device__ __forceinline__ void lse_row(const float *x, int V, int tid, float *sh_m, float *sh_s, Visit &&visit) {
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2));
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    LseAcc a = {-3.402823466e+38f, 0.f};
    if (tid < head) {
        const float v = rnd_dt(x[tid], DT);
        a.add(v);
        visit(v, tid);
    }
    const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
#pragma unroll 4
    for (int i = tid; i < n4; i += LOGPROB_THREADS) {
        const float4 v = x4[i];
        const float v0 = rnd_dt(v.x, DT), v1 = rnd_dt(v.y, DT), v2 = rnd_dt(v.z, DT), v3 = rnd_dt(v.w, DT);
        a.add4(v0, v1, v2, v3);
        const int id = head + 4 * i;
        visit(v0, id); visit(v1, id + 1); visit(v2, id + 2); visit(v3, id + 3);
    }
    if (tail0 + tid < V) {
        const float v = rnd_dt(x[tail0 + tid], DT);
        a.add(v);
        visit(v, tail0 + tid);
    }
    // the wave's pairs by cross-lane moves, the four waves' through LDS
    const float wm = wave_max(a.m);
    const float ws = wave_sum(a.s * expf(a.m - wm));
    if ((tid & 63) == 0) { sh_m[tid >> 6] = wm; sh_s[tid >> 6] = ws; }
    __syncthreads();
}
// ... and the fold of the four waves' pairs into the row's (m, s): log sum_v exp(x[v]) = m + log s.  Any thread may call it
// behind lse_row; every caller gets the same bits.
__device__ __forceinline__ void lse_fold(const float *sh_m, const float *sh_s, float &m, float &s) {
    m = sh_m[0]; s = 0.f;
    for (int w = 1; w < LOGPROB_THREADS / 64; ++w) m = fmaxf(m, sh_m[w]);
    for (int w = 0; w < LOGPROB_THREADS / 64; ++w) s += sh_s[w] * expf(sh_m[w] - m);
}

// Grid (x, y) = (row, item), one workgroup of 256 threads per scored row, one pass over the row (lse_row).  DT: the rows
// still have to be rounded to a 16-bit type (rnd_dt's codes) - every logit, the picked one too.
template <int DT>
__global__ __launch_bounds__(LOGPROB_THREADS) void token_logprob_kernel(LogprobTab t, int V) {
    const int b = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    if (r >= t.rows[b]) return;
    const sd_accept_result *res = t.res[b];
    if (res && r > res->n_accepted) return;                       // not emitted: the output float stays as it is
    const float *x = t.logits[b] + (size_t)r * t.ld[b];
    __shared__ float sh_m[LOGPROB_THREADS / 64], sh_s[LOGPROB_THREADS / 64];
    lse_row<DT>(x, V, tid, sh_m, sh_s, LseNoVisit());
    if (tid != 0) return;
    float m, s;
    lse_fold(sh_m, sh_s, m, s);
    const int tok = t.tokens[b][r];
    const float xt = tok >= 0 && tok < V ? rnd_dt(x[tok], DT) : __builtin_nanf("");
    t.out[b][r] = (xt - m) - logf(s);
}

static int launch_token_logprobs(const LogprobTab &t, int n_items, int max_rows, int V, int dt, hipStream_t st) {
    const dim3 grid(max_rows, n_items), block(LOGPROB_THREADS);
    if (dt == 1) hipLaunchKernelGGL(token_logprob_kernel<1>, grid, block, 0, st, t, V);
    else if (dt == 2) hipLaunchKernelGGL(token_logprob_kernel<2>, grid, block, 0, st, t, V);
    else hipLaunchKernelGGL(token_logprob_kernel<0>, grid, block, 0, st, t, V);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
