// penalty_kernels.h - per-request repetition / frequency / presence penalties (sd_penalize_rows): a raw logit row is
// rounded as the sampler would read it, edited by how often each token id occurs in the row's own history, and written into a
// second slab the norm launch then reads.  Up to 16 items x 17 rows in ONE launch; the decode loops run it between the
// lm_head and the norm launch of a pass that holds a penalised stream.  include/specdec.h has the contract.
#pragma once
#include "common.h"

// PEN_WINDOW: token ids per sweep of the count table (a multiple of 4); the table holds 3 more for an unaligned row's head
enum { PEN_THREADS = 256, PEN_MAX_ITEMS = 16, PEN_MAX_ROWS = 17, PEN_WINDOW = 4096, PEN_TABLE = PEN_WINDOW + 4,
       PEN_VEC = PEN_WINDOW / (4 * PEN_THREADS),     // 16-byte loads per lane and window
       PEN_HREG = 4 };                               // history entries a lane keeps in registers (PEN_HREG * PEN_THREADS in all)

// The items of one launch, passed by value (as LogprobTab is).
struct PenaltyTab {
    const float *in[PEN_MAX_ITEMS];                    // `rows` consecutive raw rows, row stride ld_in >= V
    float *out[PEN_MAX_ITEMS];                         // ... and where their edited copies go, row stride ld_out >= V
    const int32_t *seq[PEN_MAX_ITEMS];                 // the stream's tokens: row r's history is seq[0 .. hist0 + r)
    long ld_in[PEN_MAX_ITEMS], ld_out[PEN_MAX_ITEMS];
    int rows[PEN_MAX_ITEMS], hist0[PEN_MAX_ITEMS], prompt_len[PEN_MAX_ITEMS];
    float repetition[PEN_MAX_ITEMS], frequency[PEN_MAX_ITEMS], presence[PEN_MAX_ITEMS];
};

// One logit under its counts: y is the logit as the sampler reads it (pending rounding applied), c_all / c_out how often its
// token occurs in the whole history / behind the prompt.  Every result is one IEEE fp32 operation - no contraction of the
// product into the subtraction - and is rounded to the rows' 16-bit type where they live in one (dt: rnd_dt's codes).
__device__ __forceinline__ float penalized_logit(float y, int c_all, int c_out, float theta, float freq, float pres, int dt) {
#pragma clang fp contract(off)
    if (c_all > 0 && theta != 1.0f) y = rnd_dt(y > 0.0f ? __fdiv_rn(y, theta) : y * theta, dt);
    if (c_out > 0) {
        const float scaled = rnd_dt(freq * (float)c_out, dt);
        y = rnd_dt(y - scaled, dt);
        y = rnd_dt(y - pres, dt);
    }
    return y;
}

// Grid (x, y, z) = (row, item, window): a row is cut into windows of PEN_WINDOW token ids, one workgroup of 256 threads each
// (one workgroup per row leaves a single wave per SIMD to do a row's 32000 correctly rounded divisions: 40 us measured; the
// windows are independent, so they run side by side - every workgroup reads the row's whole history, which is small).  The
// window's two count tables (one int per id, in LDS) are cleared, filled from the history with integer LDS atomics - no
// scatter to memory, any order gives the same counts - and the window of the row is streamed through them, every output
// element written exactly once, by the one workgroup that owns its window.  A neutral item (1, 0, 0) counts nothing: it is rounded and copied.  Rows start anywhere: a
// scalar head up to the first 16-byte boundary, 16 bytes per lane, a scalar tail - when the input and the output row share
// their offset from a 16-byte boundary, else scalar throughout.  mode: the word the norm launch would get (bits 0-1 the
// pending rounding, bits 4-5 the rows' dtype).  What a window waits for is memory latency, so the loads that do not depend
// on the counts are issued ahead of them: the first PEN_HREG * PEN_THREADS history entries and the window's 16-byte loads of the
// row are issued before the tables are cleared and filled.
__global__ __launch_bounds__(PEN_THREADS) void penalize_rows_kernel(PenaltyTab t, int V, int mode) {
    const int b = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    if (r >= t.rows[b]) return;                                   // (whole workgroups leave: no barrier is skipped by a part of one)
    __shared__ int s_all[PEN_TABLE], s_out[PEN_TABLE];
    const float *x = t.in[b] + (size_t)r * t.ld_in[b];
    float *o = t.out[b] + (size_t)r * t.ld_out[b];
    const int rd = mode & 3, dt = (mode >> 4) & 3;
    const float theta = t.repetition[b], freq = t.frequency[b], pres = t.presence[b];
    const bool neutral = theta == 1.0f && freq == 0.0f && pres == 0.0f;
    const int32_t *seq = t.seq[b];
    const int n_hist = t.hist0[b] + r, prompt = t.prompt_len[b];
    const bool vec = (((uintptr_t)x ^ (uintptr_t)o) & 15u) == 0;
    const int head = vec ? min(V, (int)(((16u - (unsigned)((uintptr_t)x & 15u)) & 15u) >> 2)) : 0;
    const int w = blockIdx.z, lo = w == 0 ? 0 : head + w * PEN_WINDOW;
    if (lo >= V) return;
    int hreg[PEN_HREG];                                           // history entry tid + u * PEN_THREADS, -1 (in no window) past the end
#pragma unroll
    for (int u = 0; u < PEN_HREG; ++u) {
        const int i = tid + u * PEN_THREADS;
        hreg[u] = !neutral && i < n_hist ? seq[i] : -1;
    }
    {
        // ids [lo, hi): the first window takes the head with it, so every later one starts on a 16-byte boundary
        const int hi = min(V, head + (w + 1) * PEN_WINDOW);
        const int a = vec ? max(lo, head) : hi;                   // the 16-byte body is [a, a + 4 * n4), n4 <= PEN_VEC * PEN_THREADS
        const int n4 = (hi - a) >> 2, tail0 = a + 4 * n4;
        const float4 *x4 = reinterpret_cast<const float4 *>(x + a);
        float4 *o4 = reinterpret_cast<float4 *>(o + a);
        float4 v[PEN_VEC];
#pragma unroll
        for (int u = 0; u < PEN_VEC; ++u)
            if (tid + u * PEN_THREADS < n4) v[u] = x4[tid + u * PEN_THREADS];
        if (!neutral) {
            for (int i = tid; i < hi - lo; i += PEN_THREADS) { s_all[i] = 0; s_out[i] = 0; }
            __syncthreads();
            auto count = [&](int tok, int i) {
                if (tok >= lo && tok < hi) {                      // (an id outside [0, V) is in no window)
                    atomicAdd(&s_all[tok - lo], 1);
                    if (i >= prompt) atomicAdd(&s_out[tok - lo], 1);
                }
            };
#pragma unroll
            for (int u = 0; u < PEN_HREG; ++u) count(hreg[u], tid + u * PEN_THREADS);
            for (int i = tid + PEN_HREG * PEN_THREADS; i < n_hist; i += PEN_THREADS) count(seq[i], i);
            __syncthreads();
        }
        auto edit = [&](float v, int id) {
            const float y = rnd_dt(v, rd);
            return neutral ? y : penalized_logit(y, s_all[id - lo], s_out[id - lo], theta, freq, pres, dt);
        };
        for (int i = lo + tid; i < a; i += PEN_THREADS) o[i] = edit(x[i], i);
#pragma unroll
        for (int u = 0; u < PEN_VEC; ++u) {
            const int i = tid + u * PEN_THREADS, id = a + 4 * i;
            if (i >= n4) continue;
            float4 e = v[u];
            e.x = edit(e.x, id); e.y = edit(e.y, id + 1); e.z = edit(e.z, id + 2); e.w = edit(e.w, id + 3);
            o4[i] = e;
        }
        for (int i = tail0 + tid; i < hi; i += PEN_THREADS) o[i] = edit(x[i], i);
    }
}

static int launch_penalize_rows(const PenaltyTab &t, int n_items, int max_rows, int V, int mode, hipStream_t st) {
    const int windows = (V + PEN_WINDOW - 1) / PEN_WINDOW;
    hipLaunchKernelGGL(penalize_rows_kernel, dim3(max_rows, n_items, windows), dim3(PEN_THREADS), 0, st, t, V, mode);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
