// logit_edit_kernels.h - per-request logit bias, allowed-token mask and min_tokens (sd_edit_rows), on top of the penalties: a
// raw logit row is rounded as the sampler would read it, penalised by its history (penalty_kernels.h's penalized_logit,
// unchanged), biased by the request's sparse list, and masked to -inf outside the allowed set and - while the request has
// produced fewer than min_tokens tokens - at EOS.  Up to 16 items x 17 rows in ONE launch; the decode loops run it in
// penalize_rows_kernel's place when a call carries an edit block.  include/specdec.h has the contract.
#pragma once
#include "penalty_kernels.h"

// EDIT_MASK_WORDS: the mask words one window can touch - PEN_WINDOW / 32, one more for a window that starts inside a word
// (the unaligned head shifts every window start by 0..3 ids), and the first window's head
enum { EDIT_MASK_WORDS = PEN_WINDOW / 32 + 2 };

// The items of one launch, passed by value: PenaltyTab's fields and the edits' (1.6 KB of kernel arguments).
struct EditTab {
    PenaltyTab pen;
    const int32_t *bias_ids[PEN_MAX_ITEMS];            // n_bias strictly ascending ids ...
    const float *bias_vals[PEN_MAX_ITEMS];             // ... and their additive biases
    const uint32_t *allowed[PEN_MAX_ITEMS];            // bit t & 31 of word t >> 5 set = allowed; NULL = every id
    int n_bias[PEN_MAX_ITEMS], min_tokens[PEN_MAX_ITEMS], eos[PEN_MAX_ITEMS];
};

// penalize_rows_kernel's grid, windows, loads and stores (see there); what is new sits between the counts and the store:
//   bias   a third per-window table, of floats, cleared to -0 and filled by plain LDS stores, one lane per entry of the list,
//          only entries inside the window (ids are unique: no atomics; an id outside [0, V) is in no window; of duplicate ids
//          one value wins).  -0 marks "no entry": y + (-0) has y's bits for every y, and such an id skips the addition
//          altogether, so it keeps its bits (a signalling NaN included); a listed bias of -0 changes nothing either way.
//   mask   the window's words of the allowed mask, copied to LDS once (indexed by absolute id: a word may straddle two
//          windows, both read it); a cleared bit writes -inf whatever the logit holds.
//   EOS    row r predicts output token number j = hist0 + r - prompt_len; while j < min_tokens the EOS id is written as -inf.
// Any part may be absent in an item (no bias entries, NULL mask, min_tokens 0, neutral triple): its table is then neither
// cleared nor read, and an item with no part at all is rounded and copied without a barrier.  Static LDS: 3 x 16400 + 520 =
// 49720 bytes, three workgroups per CU - the grid of a decode pass (rows x streams x windows, a few hundred workgroups at
// most over 256 CUs) never stacks more, so the tables are not packed.
__global__ __launch_bounds__(PEN_THREADS) void edit_rows_kernel(EditTab e, int V, int mode) {
    const PenaltyTab &t = e.pen;
    const int b = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    if (r >= t.rows[b]) return;                                   // (whole workgroups leave: no barrier is skipped by a part of one)
    __shared__ int s_all[PEN_TABLE], s_out[PEN_TABLE];
    __shared__ float s_bias[PEN_TABLE];
    __shared__ uint32_t s_mask[EDIT_MASK_WORDS];
    const float *x = t.in[b] + (size_t)r * t.ld_in[b];
    float *o = t.out[b] + (size_t)r * t.ld_out[b];
    const int rd = mode & 3, dt = (mode >> 4) & 3;
    const float theta = t.repetition[b], freq = t.frequency[b], pres = t.presence[b];
    const bool neutral = theta == 1.0f && freq == 0.0f && pres == 0.0f;
    const int32_t *seq = t.seq[b];
    const int n_hist = t.hist0[b] + r, prompt = t.prompt_len[b];
    const int nb = e.n_bias[b];
    const int32_t *bias_ids = e.bias_ids[b];
    const float *bias_vals = e.bias_vals[b];
    const uint32_t *allowed = e.allowed[b];
    // the id this row may not emit, or none (min_tokens 0 floors nothing, also in a row that lies inside the prompt)
    const int eos = e.eos[b] >= 0 && e.min_tokens[b] > 0 && n_hist - prompt < e.min_tokens[b] ? e.eos[b] : -1;
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
    // ids [lo, hi): the first window takes the head with it, so every later one starts on a 16-byte boundary
    const int hi = min(V, head + (w + 1) * PEN_WINDOW);
    const int a = vec ? max(lo, head) : hi;                       // the 16-byte body is [a, a + 4 * n4), n4 <= PEN_VEC * PEN_THREADS
    const int n4 = (hi - a) >> 2, tail0 = a + 4 * n4;
    const float4 *x4 = reinterpret_cast<const float4 *>(x + a);
    float4 *o4 = reinterpret_cast<float4 *>(o + a);
    float4 v[PEN_VEC];
#pragma unroll
    for (int u = 0; u < PEN_VEC; ++u)
        if (tid + u * PEN_THREADS < n4) v[u] = x4[tid + u * PEN_THREADS];
    const int word0 = lo >> 5, n_words = ((hi - 1) >> 5) - word0 + 1;     // <= EDIT_MASK_WORDS: hi - lo <= PEN_TABLE - 1
    if (!neutral || nb > 0 || allowed) {                          // (uniform over the workgroup)
        if (!neutral)
            for (int i = tid; i < hi - lo; i += PEN_THREADS) { s_all[i] = 0; s_out[i] = 0; }
        if (nb > 0)
            for (int i = tid; i < hi - lo; i += PEN_THREADS) s_bias[i] = -0.0f;
        if (allowed)
            for (int i = tid; i < n_words; i += PEN_THREADS) s_mask[i] = allowed[word0 + i];
        __syncthreads();
        if (!neutral) {
            auto count = [&](int tok, int i) {
                if (tok >= lo && tok < hi) {                      // (an id outside [0, V) is in no window)
                    atomicAdd(&s_all[tok - lo], 1);
                    if (i >= prompt) atomicAdd(&s_out[tok - lo], 1);
                }
            };
#pragma unroll
            for (int u = 0; u < PEN_HREG; ++u) count(hreg[u], tid + u * PEN_THREADS);
            for (int i = tid + PEN_HREG * PEN_THREADS; i < n_hist; i += PEN_THREADS) count(seq[i], i);
        }
        for (int i = tid; i < nb; i += PEN_THREADS) {
            const int id = bias_ids[i];
            if (id >= lo && id < hi) s_bias[id - lo] = bias_vals[i];
        }
        __syncthreads();
    }
    auto edit = [&](float val, int id) {
#pragma clang fp contract(off)
        float y = rnd_dt(val, rd);
        if (!neutral) y = penalized_logit(y, s_all[id - lo], s_out[id - lo], theta, freq, pres, dt);
        if (nb > 0) {
            const float bias = s_bias[id - lo];
            if (__float_as_uint(bias) != 0x80000000u) y = rnd_dt(y + bias, dt);
        }
        if (allowed && !((s_mask[(id >> 5) - word0] >> (id & 31)) & 1u)) y = -INFINITY;
        if (id == eos) y = -INFINITY;
        return y;
    };
    for (int i = lo + tid; i < a; i += PEN_THREADS) o[i] = edit(x[i], i);
#pragma unroll
    for (int u = 0; u < PEN_VEC; ++u) {
        const int i = tid + u * PEN_THREADS, id = a + 4 * i;
        if (i >= n4) continue;
        float4 q = v[u];
        q.x = edit(q.x, id); q.y = edit(q.y, id + 1); q.z = edit(q.z, id + 2); q.w = edit(q.w, id + 3);
        o4[i] = q;
    }
    for (int i = tail0 + tid; i < hi; i += PEN_THREADS) o[i] = edit(x[i], i);
}

static int launch_edit_rows(const EditTab &e, int n_items, int max_rows, int V, int mode, hipStream_t st) {
    const int windows = (V + PEN_WINDOW - 1) / PEN_WINDOW;
    hipLaunchKernelGGL(edit_rows_kernel, dim3(max_rows, n_items, windows), dim3(PEN_THREADS), 0, st, e, V, mode);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
