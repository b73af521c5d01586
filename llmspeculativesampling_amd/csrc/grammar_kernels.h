// grammar_kernels.h - grammar-constrained decoding (sd_grammar_rows): sd_edit_rows' launch with one more mask, the allowed set
// of the automaton state the row's own output prefix leads to.  The state is not an input: every workgroup of a row walks the
// row's transitions itself, from the stream's state cache or from the start state, along the tokens in seq[] - drafted tokens
// included - so a pass needs no launch in front of this one and no workgroup waits for another.  edit_rows_kernel and
// penalize_rows_kernel keep their text and their code objects; a call without a grammar never gets here.
// include/specdec.h has the contract.
#pragma once
#include "logit_edit_kernels.h"

// The items of one launch, passed by value: EditTab's fields and the grammars' (2.3 KB of kernel arguments).
struct GrammarTab {
    EditTab edit;
    const uint32_t *masks[PEN_MAX_ITEMS];              // n_states x (V + 31) / 32 words; NULL = the item has no grammar
    const int32_t *next[PEN_MAX_ITEMS];                // n_states x n_classes
    const int32_t *cls[PEN_MAX_ITEMS];                 // V entries, or NULL: identity
    int32_t *states[PEN_MAX_ITEMS];                    // the stream's state cache, states[j] = s_j
    int n_states[PEN_MAX_ITEMS], n_classes[PEN_MAX_ITEMS], start[PEN_MAX_ITEMS];
};

// The state that masks row r of item b, s_j with j = hist0 + r - prompt_len, or -1 for a dead row; called by whole waves.
// The walk starts at s_base, base = max(j0 - 1, 0): the cached states[j0 - 1] when the item's first row has j0 >= 1, else
// s_0 = start, and takes j - base <= r + 1 transitions over seq[prompt_len + base ..], all inside the row's own history.
// Only the loads of `next` depend on one another: lane i of the wave fetches token i of the walk and its class up front
// (an id outside [0, V) or a class outside [0, n_classes) is class -1, which no state survives), and the chain then is one
// load per transition with the class handed over by a shuffle.  Every wave of every workgroup of the row repeats the walk -
// the inputs sit in L2 behind the first reader - as lookup_propose_kernel repeats its match.
__device__ __forceinline__ int grammar_row_state(const GrammarTab &g, int b, int j0, int j, int prompt, int V) {
    const int lane = threadIdx.x & 63;
    const int n_states = g.n_states[b], n_classes = g.n_classes[b];
    const int base = max(j0 - 1, 0);
    const int n_walk = min(max(j - base, 0), PEN_MAX_ROWS);       // <= r + 1 by construction; the clamp bounds the loop anyway
    int c = -1;
    if (lane < n_walk) {
        const int tok = g.edit.pen.seq[b][prompt + base + lane];
        if (tok >= 0 && tok < V) {
            c = g.cls[b] ? g.cls[b][tok] : tok;
            if (c < 0 || c >= n_classes) c = -1;
        }
    }
    int s = j0 >= 1 ? g.states[b][j0 - 1] : g.start[b];
    if (s < 0 || s >= n_states) s = -1;
    const int32_t *next = g.next[b];
    for (int i = 0; i < n_walk; ++i) {
        const int ci = __shfl(c, i);
        int to = -1;
        if (s >= 0 && ci >= 0) to = next[(size_t)s * n_classes + ci];
        s = to >= 0 && to < n_states ? to : -1;
    }
    return __builtin_amdgcn_readfirstlane(s);                     // (the same in every lane: the branches on it are uniform)
}

// edit_rows_kernel (see there for the grid, the windows, the tables and the loads) with the grammar between the allowed mask
// and the EOS floor.  What is new:
//   state  grammar_row_state above, per wave, in front of the tables; the row's first workgroup (window 0) writes
//          states[j0 + r] with one lane's plain store when j0 + r >= 0.  No workgroup reads an index a launch writes.
//   mask   a live row (j >= 0, state >= 0) copies the state's mask words for the window into s_mask, ANDed with the request's
//          `allowed` words when it has them; a dead row or a row inside the prompt keeps the request's words alone.  The edit
//          body is edit_rows_kernel's: one bit test per id.
// An item without a grammar (masks NULL) takes edit_rows_kernel's path statement for statement.  Static LDS is
// edit_rows_kernel's 49720 bytes: the walk lives in registers.
__global__ __launch_bounds__(PEN_THREADS) void grammar_rows_kernel(GrammarTab g, int V, int mode) {
    const EditTab &e = g.edit;
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
    const int hi = min(V, head + (w + 1) * PEN_WINDOW);
    const int a = vec ? max(lo, head) : hi;                       // the 16-byte body is [a, a + 4 * n4), n4 <= PEN_VEC * PEN_THREADS
    const int n4 = (hi - a) >> 2, tail0 = a + 4 * n4;
    const float4 *x4 = reinterpret_cast<const float4 *>(x + a);
    float4 *o4 = reinterpret_cast<float4 *>(o + a);
    float4 v[PEN_VEC];
#pragma unroll
    for (int u = 0; u < PEN_VEC; ++u)
        if (tid + u * PEN_THREADS < n4) v[u] = x4[tid + u * PEN_THREADS];
    // the row's automaton state; the row loads above are in flight meanwhile
    const uint32_t *gmask = nullptr;                              // the live state's mask words, or NULL
    if (g.masks[b]) {                                             // (uniform over the workgroup, as every branch below)
        const int j0 = t.hist0[b] - prompt, j = j0 + r;
        const int s = grammar_row_state(g, b, j0, j, prompt, V);
        if (w == 0 && tid == 0 && j >= 0) g.states[b][j] = s;
        if (j >= 0 && s >= 0) gmask = g.masks[b] + (size_t)s * ((V + 31) >> 5);
    }
    const bool masked = allowed || gmask;
    const int word0 = lo >> 5, n_words = ((hi - 1) >> 5) - word0 + 1;     // <= EDIT_MASK_WORDS: hi - lo <= PEN_TABLE - 1
    if (!neutral || nb > 0 || masked) {
        if (!neutral)
            for (int i = tid; i < hi - lo; i += PEN_THREADS) { s_all[i] = 0; s_out[i] = 0; }
        if (nb > 0)
            for (int i = tid; i < hi - lo; i += PEN_THREADS) s_bias[i] = -0.0f;
        if (masked)
            for (int i = tid; i < n_words; i += PEN_THREADS)
                s_mask[i] = (allowed ? allowed[word0 + i] : 0xffffffffu) & (gmask ? gmask[word0 + i] : 0xffffffffu);
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
        if (masked && !((s_mask[(id >> 5) - word0] >> (id & 31)) & 1u)) y = -INFINITY;
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

static int launch_grammar_rows(const GrammarTab &g, int n_items, int max_rows, int V, int mode, hipStream_t st) {
    const int windows = (V + PEN_WINDOW - 1) / PEN_WINDOW;
    hipLaunchKernelGGL(grammar_rows_kernel, dim3(max_rows, n_items, windows), dim3(PEN_THREADS), 0, st, g, V, mode);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
