/*
 * specdec.h - C ABI of libspecdec.so, the MI355X (gfx950) speculative-sampling decode engine.
 *
 * The reference (ZongyueQin/LLMSpeculativeSampling) exposes this path as a Python API with no
 * FFI; the entry points below are what a binding for that path binds.
 * Each one names the reference code it replaces (file:line under the reference repo).
 *
 * Conventions
 *   - plain C, no torch types: raw device pointers, explicit sizes, a hipStream_t passed as void*.
 *   - every function returns 0 on success or a negative sd_status; sd_last_error() gives the text.
 *   - the library never owns caller memory: weights, KV arenas, probability arenas and scratch
 *     are allocated by the caller and handed over as pointers; handles own only host structs.
 *   - nothing here synchronises the stream unless its comment says so.
 */
#ifndef SPECDEC_H
#define SPECDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_ABI_VERSION 7

typedef enum {
    SD_OK = 0,
    SD_ERR_INVALID = -1,      /* bad argument / unsupported shape                                  */
    SD_ERR_NORM_LOGITS = -2,  /* RuntimeError('norm logits error')   reference utils.py:203-207    */
    SD_ERR_PROB = -3,         /* RuntimeError('prob error')          reference utils.py:220-224    */
    SD_ERR_HIP = -4,          /* a HIP runtime call failed                                         */
    SD_ERR_CAPACITY = -5      /* sequence / row count beyond what the session was sized for        */
} sd_status;

typedef enum { SD_F32 = 0, SD_BF16 = 1, SD_F16 = 2 } sd_dtype;   /* fp16: what the reference harness loads (evaluation.py:185) */

/* dtype_mode of the sampling entry points (the `bf16_round_logits` argument of the norm_* calls is this word too).
 * The reference's Llama returns fp32 logits (modeling_llama.py:870: a 16-bit head's output cast with .float()), its OPT
 * keeps them - and with them the whole norm_logits / sample / max_fn chain - in the weight dtype (modeling_opt.py:974).
 *   SD_NORM_ROUND_*: the logits handed over are fp32 accumulators that still have to be rounded to the head's dtype;
 *   SD_NORM_DT_*:    the row lives in that 16-bit dtype: every tensor the reference materialises on the way (logits /
 *                    temperature, softmax, cumsum prefixes, the row sum and its log, log_softmax, exp, p - q, max_fn's
 *                    sum and quotient, p / noise) is rounded to it, as torch's bf16 / fp16 CPU kernels do (fp32 math, one
 *                    rounding per op).  Probability rows stay fp32 arrays; their values are then exactly representable.
 * Ties: with 16-bit logits the top-p cut can fall inside a run of equal logits; the reference's order inside such a run
 * is that of an unstable std::sort (torch.sort without stable=True, utils.py:170) and is not reproduced - this build
 * keeps the lowest token ids. */
#define SD_NORM_ROUND_BF16 1
#define SD_NORM_ROUND_F16 2
#define SD_NORM_DT_BF16 16
#define SD_NORM_DT_F16 32
typedef enum { SD_ARCH_LLAMA = 0, SD_ARCH_OPT = 1 } sd_arch;

int sd_version(void);
const char *sd_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Sampling primitives                                            reference sampling/utils.py
 * ------------------------------------------------------------------------------------------ */

/* norm_logits + top_k_top_p_filter (utils.py:182-210, 152-179), one workgroup per row:
 * logits/temperature -> keep >= k-th largest (ties kept) -> stable descending order, drop
 * everything after the first token whose cumulative softmax mass exceeds top_p ->
 * exp(log_softmax).  rows are `ld_*` elements apart.  err_flag[row] (device int, may be NULL)
 * is set to 1 where the reference would raise 'norm logits error' (NaN/Inf result).
 * bf16_round_logits != 0 rounds each fp32 logit to bf16 first (a bf16 lm_head whose output the
 * reference then casts with .float(), modeling_llama.py:869-870). */
int sd_norm_probs(const float *logits, int rows, int V, long ld_in, float temperature, int top_k,
                  float top_p, int bf16_round_logits, float *probs_out, long ld_out, int *err_flag,
                  void *workspace, void *stream);
/* workspace (device, sd_norm_workspace_bytes(rows) bytes, may be NULL): with it and 1 <= top_k <= 64 each row is first
 * cut over 16 workgroups that extract the candidates above a safe threshold, so one 128 KiB row is not limited by what a
 * single CU can pull (~25 GB/s); without it one workgroup does everything.  Results are identical either way. */
size_t sd_norm_workspace_bytes(int rows);

/* top_k_top_p_filter by itself (utils.py:152-179; the reference mutates its argument and returns it): out[i] = logit
 * where the token is kept, -inf where it is dropped; top_k == 0 and top_p == 0 leave the row untouched.  `out` must
 * not alias `logits` (the Python drop-in copies the result back into its argument).  dtype_mode: 0, or SD_NORM_DT_BF16 /
 * SD_NORM_DT_F16 when the caller's tensor is 16-bit - the reference then sorts, softmaxes and cumsums in that dtype
 * (utils.py:170-172), so the kept set near the top-p cut is decided on 16-bit sums, exactly as sd_norm_probs decides it. */
int sd_topk_topp_filter(const float *logits, int rows, int V, long ld_in, int top_k, float top_p, int dtype_mode,
                        float *out, long ld_out, void *stream);

/* One draft / autoregressive step's tail fused: norm_logits of ONE row followed by sample() on it
 * (kvcache_model.py:235-236 + :283), a single launch.  Writes the probability row (the accept scan and
 * the residual need it later) and the sampled token.  exp_noise / Philox as in sd_sample; with device
 * Philox only the surviving tokens draw a variate.  sample_err as sd_sample's err_flag. */
int sd_norm_sample(const float *logits, int V, float temperature, int top_k, float top_p,
                   int bf16_round_logits, float *probs_out, int *err_flag, const float *exp_noise,
                   uint64_t philox_seed, uint64_t draw_index, int *tok_out, int *sample_err, void *workspace,
                   void *stream);

/* Batched form of sd_norm_probs / sd_norm_sample for stream-batched decode: row r of `logits` is normalised into
 * rows[r].probs_out (rows of different streams live in different arenas); with sample != 0 each row also draws its
 * token into rows[r].tok_out from its own exp_noise row or Philox (seed, draw).  `rows` is a host array. */
typedef struct {
    float *probs_out;
    int *err;                 /* device int or NULL */
    const float *exp_noise;   /* device row or NULL (Philox) */
    uint64_t philox_seed, draw_index;
    int *tok_out, *sample_err;
} sd_norm_row;
int sd_norm_batch(const float *logits, int n_rows, int V, long ld_in, float temperature, int top_k, float top_p,
                  int bf16_round_logits, const sd_norm_row *rows, int sample, void *workspace, void *stream);
/* sd_norm_batch with one (temperature, top_k, top_p) per row: row r is filtered with params[r] (a host array of n_rows
 * entries), and its result is exactly what sd_norm_batch gives for that row alone with those three values, whatever the
 * other rows of the call ask for.  The candidate workspace serves the rows with 1 <= top_k <= 64; the others take the path
 * they take without one.  Refused with SD_ERR_INVALID before anything is written or launched, the message naming the row: a
 * NULL params, a temperature of 0, a negative top_k. */
typedef struct { float temperature; int32_t top_k; float top_p; } sd_row_sampling;
int sd_norm_batch_rows(const float *logits, int n_rows, int V, long ld_in, const sd_row_sampling *params,
                       int bf16_round_logits, const sd_norm_row *rows, int sample, void *workspace, void *stream);

/* sample (utils.py:213-233) for num_samples == 1: argmax_i probs[i] / noise[i] (first index wins
 * ties), then the "< 1e-9 -> argmax(probs)" fix-up.  exp_noise is a device row of Exp(1) variates
 * in the reference's draw order (parity mode), or NULL to draw them on the device from Philox
 * (seed, draw_index).  tok_out: device int32.  err_flag (device, may be NULL): 1 = invalid
 * distribution (negative / NaN / Inf), 2 = all-zero row; both are 'prob error' in the reference. */
int sd_sample(const float *probs, int V, const float *exp_noise, uint64_t philox_seed,
              uint64_t draw_index, int *tok_out, int *err_flag, int dtype_mode, void *stream);

/* The device RNG of the throughput mode made observable, so that a test can replay the exact variates into the CPU
 * oracle (the reference draws from torch's generator, utils.py:221 / speculative_sampling.py:1978; this build's
 * device mode draws from counter-based Philox4x32-10 instead).  out[i] = the Exp(1) variate the sampling kernels use
 * for vocabulary element i of draw (seed, draw_index): -log(u), u = (23 random bits + 1/2) * 2^-23 in (0,1). */
int sd_philox_exp(uint64_t philox_seed, uint64_t draw_index, int V, float *out, void *stream);
/* out[i] = the uniform in [0,1) the accept scans use for draw (seed, draw_index + i), i < n. */
int sd_philox_uniform(uint64_t philox_seed, uint64_t draw_index, int n, float *out, void *stream);

/* max_fn (utils.py:236-245) materialised: out = max(p-q,0) / (sum(max(p-q,0)) + 1e-6).  q may be
 * NULL (then max_fn(p)).  Only the drop-in sampling.utils.max_fn uses this; the decode loop uses
 * the fused sd_resample below and never writes the residual row. */
int sd_max_fn(const float *p, const float *q, int V, float *out, int dtype_mode, void *stream);

/* Result block written by the accept / resample kernels (device or pinned-host memory). */
typedef struct {
    int32_t n_accepted;    /* l: drafted tokens accepted this iteration   (speculative_sampling.py:1974-1991) */
    int32_t n;             /* last kept position, L+l-1                    (:1964, :1983)                      */
    int32_t next_token;    /* t: residual resample or bonus sample         (:2005-2023)                        */
    int32_t flags;         /* bit0 residual was all-zero -> fallback sample(max_fn(p_n)) (:2009-2010);
                              bit1 'prob error'; bit2 all gamma accepted; bit3 an error word of the iteration was set */
    float p_at[16];        /* target prob of each drafted token (for the acc_rate statistic, :1966-1971)      */
    float q_at[16];        /* draft prob of each drafted token                                                */
    int32_t drafted[16];   /* the gamma drafted token ids seq[L .. L+gamma) (saves a second device->host copy)      */
} sd_accept_result;

/* Accept scan (speculative_sampling.py:1964-1991): for i < gamma, j = seq[L+i]; reject iff
 * r[i] > float32(double(p_hist[L+i-1][j]) / double(q_hist[L+i-1][j])); the first reject decides.
 * p_hist / q_hist are probability arenas indexed by absolute position (row stride ld).  r: gamma
 * device floats in the reference's draw order (parity mode; the caller re-aligns the host generator
 * to the min(l+1, gamma) uniforms the reference would have consumed), or NULL for device Philox
 * (seed, draw_index + i).  Writes n_accepted, n, p_at, q_at, flags bit2; next_token = -1. */
int sd_accept_scan(const float *p_hist, const float *q_hist, long ld, const int32_t *seq, int L,
                   int gamma, const float *r, uint64_t philox_seed, uint64_t draw_index,
                   sd_accept_result *out, void *stream);

/* Residual resample / bonus sample (speculative_sampling.py:2005-2023) at position res->n, read
 * from the device result block: rejected -> sample(max_fn(p_n - q_n)) with the all-zero fallback
 * sample(max_fn(p_n)); all accepted -> sample(p_last).  Writes next_token and flags, appends the
 * token at seq[n+1] and stores the new sequence length n+2 into *seq_len (device int, may be NULL). */
int sd_resample(const float *p_hist, const float *q_hist, long ld, int V, int32_t *seq, int L,
                int gamma, const float *exp_noise, uint64_t philox_seed, uint64_t draw_index,
                sd_accept_result *res, int32_t *seq_len, int dtype_mode, void *stream);

/* sd_accept_scan + sd_resample in ONE launch whose sample works on candidate lists instead of two passes over V.
 * sd_norm_probs_lists is sd_norm_probs that also leaves, per row, the row's non-zero entries (token ids + probabilities;
 * sd_cand_list_bytes(rows) device bytes; a row gets a list when its kept set was decided on a sorted list - 1 <= top_k <= 64, or
 * <= 1024 finite survivors of top-k in the general path - and holds <= 128 entries, else it is marked list-less).  sd_accept_resample takes the lists of the gamma + 1 TARGET rows of
 * the iteration (positions L-1 .. L+gamma-1, in order) or NULL; results are bit-identical to the two-kernel form, which
 * it falls back to for a list-less row.  Philox only (seed, draw_scan + i for the uniforms unless r is given; draw_resample). */
size_t sd_cand_list_bytes(int rows);
int sd_norm_probs_lists(const float *logits, int rows, int V, long ld_in, float temperature, int top_k, float top_p,
                        int bf16_round_logits, float *probs_out, long ld_out, int *err_flag, void *workspace,
                        void *cand_lists, void *stream);
int sd_accept_resample(const float *p_hist, const float *q_hist, long ld, int V, int32_t *seq, int L, int gamma,
                       const float *r, uint64_t philox_seed, uint64_t draw_scan, uint64_t draw_resample,
                       sd_accept_result *res, const int *err_flags, int n_err, int dtype_mode, const void *target_lists,
                       void *stream);

/* TEST HOOK, not for production callers: sd_norm_probs_lists with every internal argument of the norm launch passed
 * through, and the route each row took read back.  cand_lists may be NULL.  tile_max (or NULL): [rows][V / 16] maxima of
 * the rows' 16-column tiles (NaN where a tile holds one) - the contract the lm_head's epilogue meets; the caller must then
 * also hand in zero-filled output rows.  filter_only: sd_topk_topp_filter's output instead of probabilities (as that entry launches it:
 * without workspace, tile maxima or lists).  do_sample (rows == 1): the fused sample of sd_norm_sample.  route_out (device,
 * rows ints, required): per row an OR of SD_ROUTE_*.  The hook launches instantiations of the norm kernel of its own (the
 * ones that record the route; production launches carry no trace of it), same source, same results;
 * bits 16-31 hold the size of the kept set when it was decided on a sorted list. */
enum {
    SD_ROUTE_ENTRY_A = 0x1,         /* candidates from the 16-chunk workspace kernel */
    SD_ROUTE_ENTRY_B = 0x2,         /* candidates from tile maxima */
    SD_ROUTE_A_CHUNK_CAP = 0x4,     /* gave up: one chunk kept > 192 */
    SD_ROUTE_A_TOTAL_CAP = 0x8,     /* gave up: the chunks together kept > 1024 */
    SD_ROUTE_B_TILE_CAP = 0x10,     /* gave up: > 1024 qualifying tiles */
    SD_ROUTE_B_CAND_CAP = 0x20,     /* gave up: > 1024 candidates inside them */
    SD_ROUTE_A_SECOND = 0x40,       /* second-level prefilter ran on the gathered list */
    SD_ROUTE_PREFILTER = 0x80,      /* in-kernel prefilter ran (first entry, or after A / B gave up) */
    SD_ROUTE_PREFILTER_CAP = 0x100, /* gave up: it kept > 1024 */
    SD_ROUTE_TOPK_BISECT = 0x200,   /* general top-k by bitwise bisection */
    SD_ROUTE_TOPP_LIST = 0x400,     /* top-p on a sorted list */
    SD_ROUTE_TOPP_MASS = 0x800,     /* top-p by mass bisection */
    SD_ROUTE_CUT_IDX = 0x1000,      /* cut_idx bisection: equal logits straddle the top-p cut */
    SD_ROUTE_STAGED = 0x2000,       /* row staged in LDS */
    SD_ROUTE_ERROR = 0x4000,        /* error row */
    SD_ROUTE_LIST = 0x8000          /* a candidate list was written */
};
int sd_norm_probs_debug(const float *logits, int rows, int V, long ld_in, float temperature, int top_k, float top_p,
                        int bf16_round_logits, float *probs_out, long ld_out, int *err_flag, void *workspace,
                        void *cand_lists, void *stream, const float *tile_max, int filter_only, int do_sample,
                        const float *exp_noise, uint64_t philox_seed, uint64_t draw_index, int *tok_out, int *sample_err,
                        int *route_out);
/* TEST HOOK: sd_norm_batch_rows on the route-recording instantiations.  tile_max (or NULL): the rows' tile maxima as above
 * (the output rows zero-filled by the caller); the launch uses them only when every row of it has 1 <= top_k <= 64 and
 * temperature > 0, else it drops them and the eligible rows go through the workspace.  cand_lists (or NULL): n_rows lists.
 * route_out (device, n_rows ints, required): row r's SD_ROUTE_* word. */
int sd_norm_batch_rows_debug(const float *logits, int n_rows, int V, long ld_in, const sd_row_sampling *params,
                             int bf16_round_logits, const sd_norm_row *rows, int sample, void *workspace, void *stream,
                             const float *tile_max, void *cand_lists, int *route_out);

/* sd_accept_scan + sd_resample for up to 16 independent streams in two launches (stream-batched decode).
 * Per item: its probability arenas, token buffer, prefix length L, the gamma uniforms r (or NULL: Philox
 * (philox_seed, draw_scan + i)), the resample noise row (or NULL: Philox (philox_seed, draw_resample)), the
 * device result block, and optionally n_err device error words folded into res.flags bit3. `items` is a host array. */
typedef struct {
    const float *p_hist, *q_hist;
    int32_t *seq;
    int32_t L;
    const float *r, *exp_noise;
    uint64_t philox_seed, draw_scan, draw_resample;
    sd_accept_result *res;
    const int *err_flags;
    int32_t n_err;
} sd_accept_item;
int sd_accept_batch(const sd_accept_item *items, int n_items, long ld, int V, int gamma, int dtype_mode, void *stream);
/* Internal (the native lock-step loop; exported so that tests can hold it to the oracle): sd_accept_resample for up to 16
 * streams in ONE launch.  lists[i] = the candidate lists of item i's gamma + 1 target rows, or NULL (dense passes for that
 * stream).  Device Philox only: an item with exp_noise is refused. */
int sd_accept_resample_batch(const sd_accept_item *items, int n_items, long ld, int V, int gamma, int dtype_mode,
                             const void *const *lists, void *stream);

/* Width-w acceptance of multi_speculative_sampling(strategy="iid") (speculative_sampling.py:1592-1640, SURVEY.md 8(f)
 * rank 2): replica w drafted seq_w[L .. L+gamma); replicas are scanned in order, replica w accepts its i-th token iff
 * r < min(1, p_w[L+i-1][j] / q_w[L+i-1][j]) (fp32 division; a NaN ratio rejects) and stops at its first reject; the
 * replica with the longest accepted run wins (first one on ties; replica 0 when nothing was accepted) and the scan
 * ends early at the first replica that accepts all gamma.  r: width*gamma device floats consumed strictly in that
 * order (parity mode; n_uniform tells the caller how many the reference would have drawn), or NULL for device Philox
 * (seed, draw_index + k).  `chosen` is filled like sd_accept_scan's result for the winning replica and feeds
 * sd_multi_resample; p_at/q_at hold every replica's gathered probabilities ([w][i], 16 columns per replica) for the
 * acc_rate statistic (:1592-1601).  `items` is a host array of width <= 16 entries. */
typedef struct {
    sd_accept_result chosen;
    int32_t choice, n_uniform, width, gamma;
    float p_at[256], q_at[256];
} sd_multi_result;
typedef struct {
    const float *p_hist, *q_hist;     /* probability arenas of replica w, indexed by absolute position (row stride ld) */
    const int32_t *seq;               /* replica w's token buffer */
} sd_multi_item;
int sd_accept_multi(const sd_multi_item *items, int width, long ld, int L, int gamma, const float *r,
                    uint64_t philox_seed, uint64_t draw_index, sd_multi_result *out, void *stream);

/* sd_resample with multi_speculative_sampling's fallback (speculative_sampling.py:1662-1668): when the residual
 * sample raises, the token is drawn from p_n itself, not from max_fn(p_n).  Everything else as sd_resample. */
int sd_multi_resample(const float *p_hist, const float *q_hist, long ld, int V, int32_t *seq, int gamma,
                      const float *exp_noise, uint64_t philox_seed, uint64_t draw_index, sd_accept_result *res,
                      int dtype_mode, void *stream);

/* Internal (the native width-w loop; exported so that tests can hold it to the pair above): sd_accept_multi followed by
 * sd_multi_resample on the winner's rows in ONE launch - the workgroup that ran the scan picks the winner's arenas itself,
 * so the host does not read `choice` between the two.  Device Philox only: uniforms (seed, draw_scan + k) unless r is
 * given, sample noise (seed, draw_resample).  Writes the token at the winner's seq[n + 1] (the `seq` of sd_multi_item is
 * written through).  `out` and that token are bit-equal to what the two-launch pair leaves. */
int sd_multi_accept_resample(const sd_multi_item *items, int width, long ld, int V, int L, int gamma, const float *r,
                             uint64_t philox_seed, uint64_t draw_scan, uint64_t draw_resample, sd_multi_result *out,
                             int dtype_mode, void *stream);

/* Winner broadcast of one width-w iteration (what multi_speculative_sampling does with rollback(end, choice) and the next
 * forward's repeat(), kvcache_model.py:180-192, 390-396): ONE launch that reads choice, chosen.n and the all-accept flag
 * from the DEVICE result block `res` (stream order is the only synchronisation) and copies, from the winner to every other
 * replica, KV positions [draft_lo, min(L+gamma-1, n+1)) of the draft arenas, [target_lo, all_accept ? L+gamma : n+1) of
 * the target arenas and the tokens seq[L .. n+2).  Arenas are [planes][max_seq][row_bytes] bytes (planes = n_layers * 2 *
 * n_kv_heads, row_bytes = head_dim * element size), moved byte-wise, so any element type goes the same way.  Nothing is
 * copied when the block does not describe this iteration (choice outside [0, width), n outside [L-1, L+gamma-1]).
 * `items` is a host array of width <= 16 entries; seq_cap = ints each token buffer holds. */
typedef struct {
    void *draft_kv, *target_kv;
    int32_t *seq;
} sd_multi_adopt_item;
int sd_multi_adopt(const sd_multi_adopt_item *items, int width, const sd_multi_result *res, int L, int gamma,
                   int draft_lo, int target_lo, int draft_planes, int draft_max_seq, int draft_row_bytes,
                   int target_planes, int target_max_seq, int target_row_bytes, int seq_cap, void *stream);

/* ------------------------------------------------------------------------------------------
 * Decoder model + KV arena           reference sampling/models/modeling_{llama,opt}.py,
 *                                    sampling/kvcache_model.py:141-252 (forward), :359-436 (rollback)
 * ------------------------------------------------------------------------------------------ */

typedef struct {
    int32_t arch;                 /* sd_arch                                                    */
    int32_t dtype;                /* sd_dtype of weights and activations                        */
    int32_t vocab, hidden, inter, n_layers, n_heads, n_kv_heads, head_dim;
    int32_t max_pos;              /* rows of the rope table (llama) / learned positions (opt)   */
    int32_t opt_pre_ln;           /* OPT do_layer_norm_before (125m/13b: 1, 350m: 0)            */
    int32_t opt_proj_dim;         /* OPT word_embed_proj_dim (== hidden when no project_in/out) */
    float norm_eps;
    int32_t logits_bf16_round;    /* round logits to bf16 before use (bf16 lm_head semantics)   */
    int32_t fused_layout;         /* bf16 only: wqkv / w_gate_up rows are in the fused-epilogue order below      */
} sd_model_config;

/* Weight table.  Matrices are [out][in] as in nn.Linear.  For dtype SD_BF16 every GEMM matrix is
 * handed over in the tile-packed layout produced by sd_pack_weight_bf16 ("HBM
 * layout"); for SD_F32 they stay row-major.  Vectors / embeddings are row-major in `dtype`.
 * Per-layer arrays have n_layers entries.  Unused entries are NULL.
 * With cfg.fused_layout (bf16): the QKV and gate/up GEMMs keep the whole k-range in one workgroup and finish with
 * a fused epilogue (RoPE + in-place KV append; SiLU(gate)*up / ReLU), which needs two row orders prepared at load:
 *   llama wqkv: inside each q and k head the rows are pair-interleaved, d0, d0+D/2, d1, d1+D/2, ... (v heads natural);
 *   llama w_gate_up: 8 gate rows then the same 8 up rows, repeated: g0..g7,u0..u7,g8..g15,u8..u15,...
 * OPT keeps the natural order. */
typedef struct {
    const void *embed;            /* [vocab][embed_dim] row-major                               */
    const void *pos_embed;        /* OPT: [max_pos+2][hidden]                                   */
    const void *project_in;       /* OPT 350m: [hidden][proj]   (GEMM matrix)                   */
    const void *project_out;      /* OPT 350m: [proj][hidden]   (GEMM matrix)                   */
    const void *final_norm_w, *final_norm_b;
    const void *lm_head;          /* [vocab][embed_dim]         (GEMM matrix)                   */
    const void *rope_cos, *rope_sin; /* llama: [max_pos][head_dim/2] in `dtype`                 */
    const void *const *wqkv;      /* [(n_heads+2*n_kv_heads)*head_dim][hidden], q rows then k then v */
    const void *const *bqkv;      /* OPT biases, same order                                     */
    const void *const *wo;        /* [hidden][hidden]                                           */
    const void *const *bo;
    const void *const *w_gate_up; /* llama: [2*inter][hidden], gate rows then up rows; OPT fc1: [inter][hidden] */
    const void *const *b_fc1;
    const void *const *w_down;    /* [hidden][inter] (OPT fc2)                                  */
    const void *const *b_fc2;
    const void *const *norm1_w, *const *norm1_b;  /* input_layernorm / self_attn_layer_norm      */
    const void *const *norm2_w, *const *norm2_b;  /* post_attention_layernorm / final_layer_norm */
} sd_model_weights;

typedef struct sd_model sd_model;

/* Copies the config and the pointer table into a host handle (weights stay where they are). */
int sd_model_create(const sd_model_config *cfg, const sd_model_weights *w, sd_model **out);
int sd_model_destroy(sd_model *m);
/* Rows one sd_session_forward call may carry for this model: 256 (prefill chunks; the many-row GEMM kernel needs every
 * per-layer weight matrix to have N % 128 == 0 and K % 64 == 0, K >= 512) or 64.  sd_session_create and
 * sd_session_scratch_bytes clamp their max_rows to it. */
int sd_model_max_rows(const sd_model *m);
/* Rows of one call whose rows are all logit rows (a stream-batched verify pass; sd_session_forward with n_logits == n_new):
 * at most 80 and at most sd_model_max_rows, and past 64 only when the lm_head (vocab % 128 == 0) has a many-row kernel too.
 * Calls with fewer logit rows than rows carry at most 64 logit rows. */
int sd_model_max_pass_rows(const sd_model *m);

/* Repack a row-major bf16 [N][K] matrix (N % 16 == 0, K % 32 == 0) into the streaming layout the
 * GEMM kernels read: 1 KiB tiles [N/16][K/32][lane 0..63][8 bf16], lane = 16*(k/8 % 4) + n % 16. */
int sd_pack_weight_bf16(const void *w_rowmajor, void *w_packed, int N, int K, void *stream);

/* Lossless 12-bit records of a bf16 matrix that is already in sd_pack_weight_bf16's layout: per
 * 1 KiB tile 768 bytes of codes (sign, mantissa, a 4-bit exponent code relative to the tile's window of 15 binades) and a
 * 16-byte side record (the window's base and up to six "escapes", elements below the window, with their true exponents).
 * The single-stream decode / verify passes of a bf16 Llama model (<= 8 rows, the norm-on-load route) stream them instead
 * of the bf16 tiles, 23.4 % fewer bytes, and decode them in registers to the same bits.
 * sd_w12_bytes: sizes of the two arrays.  codes must be 128-byte aligned, meta 16-byte aligned.
 * sd_pack_weight_w12: packs; *status_dev (a DEVICE int, cleared and written on `stream`) becomes 1 when some tile has more
 *   than six escapes - the matrix is then not packable, the two arrays mean nothing and the caller keeps bf16 - else 0.
 * sd_unpack_weight_w12: records -> the tiled bf16 layout (the format's executable definition; tests).
 * sd_model_set_w12: registers the records of layer `layer`'s matrix `which` with a bf16 model (NULL, NULL: unregisters).
 *   The bf16 copy stays in use for every other pass; the caller keeps both alive.  Not while a forward is in flight.
 * sd_session_w12_launches: GEMM launches of this session so far that streamed records (a host integer, for tests). */
enum { SD_W12_QKV = 0, SD_W12_GATE_UP = 1, SD_W12_DOWN = 2 };
int sd_w12_bytes(int N, int K, size_t *codes_bytes, size_t *meta_bytes);
int sd_pack_weight_w12(const void *w_tiled, void *codes, void *meta, int N, int K, int *status_dev, void *stream);
int sd_unpack_weight_w12(const void *codes, const void *meta, void *w_tiled, int N, int K, void *stream);
int sd_model_set_w12(sd_model *m, int which, int layer, const void *codes, const void *meta);

/* Row-major bf16 activations [M][K] (K % 32 == 0) -> the GEMM operand layout the engine keeps them in between
 * kernels: 16-row tiles [ceil(M/16)][K/32][lane 0..63][8 bf16], lane = 16*(k/8 % 4) + m % 16, so that a wave's MFMA
 * fragment is one contiguous 1 KiB read.  x_tiled must hold roundup(M,16) * K elements. */
int sd_pack_activation_bf16(const void *x_rowmajor, void *x_tiled, int M, int K, void *stream);

/* The weight-streaming GEMM on its own (unit tests, kernel-level roofline runs):
 * part[s][m][n] = sum over k-slice s of x[m][k] * W[n][k] for a tile-packed bf16 W, then (if out != NULL)
 * out[m][n] = sum_s part[s][m][n] in fp32.  M <= 64 (<= 256 with x_tiled and N % 128 == 0: past 64 rows the balanced
 * many-row kernel or gemm_bf16_mm runs, as in the forward).  x: plain rows (x_tiled == 0) or sd_pack_activation_bf16's
 * layout (x_tiled != 0, what the forward uses).  part must hold splits * roundup(M,16) * N floats; the split count the
 * policy chose comes back in *splits_out. */
int sd_gemm_bf16(const void *w_packed, const void *x, int x_tiled, int M, int N, int K, float *part,
                 size_t part_floats, float *out, int *splits_out, void *stream);

/* What the GEMM planner needs to know about a call besides (N, K, M): a set of these bits. */
enum {
    SD_GN_GATHER = 1,    /* X rows are gathered through a row table (the lm_head of some rows of a pass) */
    SD_GN_ROWMAJOR = 2,  /* X is plain row-major (sd_gemm_bf16 with x_tiled == 0) */
    SD_GN_FUSED = 4,     /* an epilogue runs in the launch: every workgroup keeps its whole k-range (one slab, X tiled) */
    SD_GN_QKV = 8,       /* ... and it is the QKV epilogue */
    SD_GN_ONE_SLAB = 16  /* one k-slab where the shape allows it (a tensor-parallel shard's O / down projection) */
};
/* The kernel a route names. */
enum { SD_GEMM_NONE = 0, SD_GEMM_STREAM = 1, SD_GEMM_STREAM_W16 = 2, SD_GEMM_ROWS = 3, SD_GEMM_MM = 4 };
/* The planner's answer for one 16-bit GEMM of M rows on an [N][K] weight, and the kernel instance its launch takes. */
typedef struct sd_gemm_route_info {
    int32_t kind;                       /* SD_GEMM_*; SD_GEMM_NONE: no kernel (the row limits keep such calls out) */
    int32_t S, ksp;                     /* k-slabs and k-steps (of 32) per slab: (S-1)*ksp < K/32 <= S*ksp */
    int32_t mtw;                        /* gemm_bf16_mm: m-tiles per wave (2: 128-row blocks, 4: 256-row blocks) */
    int32_t NG, grid, nwn, nwk, nld;    /* gemm_bf16_rows: n-groups, workgroups (NG * S) and the wave grid of a workgroup:
                                           nwn compute waves per k-group x nwk k-groups + nld loader waves */
    int32_t inst_mt;                    /* the instance's m-tiles (mm: of a row block); 0: the launch has no instance */
    int32_t inst_ntw, inst_unroll;      /* gemm_bf16_stream: n-tiles per wave, k-steps per burst (8: the one-burst form) */
    int32_t inst_ch, inst_wbm;          /* gemm_bf16_rows: k-steps per chunk, chunks per weight burst */
    int32_t inst_nt;                    /* gemm_bf16_mm: non-temporal weight loads */
    int32_t lds_bytes;                  /* dynamic LDS of the launch (rows, mm) */
    uint64_t part_floats;               /* S * roundup(M,16) * N: the floats an unfused launch leaves in `part` */
} sd_gemm_route_info;
/* The route of such a GEMM (host only: no device, no session; the launch helpers take their kernel instance by the
 * functions this query calls).  Reads the SD_GEMM_* / SD_MM_* tunables of the environment at the call.  SD_ERR_INVALID for
 * M outside 1..256, N % 16, K % 32 or need outside the SD_GN_* bits; a shape without a kernel is SD_OK with SD_GEMM_NONE. */
int sd_gemm_route(int N, int K, int M, int need, sd_gemm_route_info *out);
/* sd_gemm_bf16 on the route `need` selects: need = 0 is x_tiled, SD_GN_ROWMAJOR plain rows; SD_GN_FUSED and SD_GN_ONE_SLAB
 * (X tiled) run the one-slab plans the forward pass uses with its fused epilogues / on a shard as plain slab GEMMs.
 * SD_GN_GATHER and SD_GN_QKV need a row table / the QKV epilogue: SD_ERR_INVALID here. */
int sd_gemm_bf16_need(const void *w_packed, const void *x, int M, int N, int K, int need, float *part, size_t part_floats,
                      float *out, int *splits_out, void *stream);

/* A session =one KV arena + scratch for one sequence (one KVCacheModel of the reference).
 * kv_arena: [n_layers][2][n_kv_heads][max_seq][head_dim] in `dtype`, caller-allocated.
 * scratch: sd_session_scratch_bytes() bytes, caller-allocated. */
typedef struct sd_session sd_session;
size_t sd_session_kv_bytes(const sd_model *m, int max_seq);
size_t sd_session_scratch_bytes(const sd_model *m, int max_rows);
/* Floats of the scratch that hold the GEMMs' k-slabs (host only): no route of a pass of <= max_rows rows may leave more. */
size_t sd_session_part_floats(const sd_model *m, int max_rows);
int sd_session_create(sd_model *m, int max_seq, int max_rows, void *kv_arena, void *scratch,
                      sd_session **out);
int sd_session_destroy(sd_session *s);
/* fp8 KV arena (BASELINE config 5): the arena then holds OCP e4m3 bytes, [n_layers][2][n_kv_heads][max_seq][head_dim],
 * half the bytes of a 16-bit arena; `scales` = device floats [n_layers][2][n_kv_heads], an element x is stored as
 * fp8(x * (1 / scale)), reciprocal and product both in fp32, clamped to +-448, to nearest even; NaN stays NaN.  K / V rows
 * are quantised where they are appended (the fused QKV epilogue, after RoPE), the attention kernel widens them back in
 * registers.  16-bit models in the fused layout with head_dim >= 32; call before the first forward. */
int sd_session_set_kv_fp8(sd_session *s, const float *scales);
/* How many times this session has launched a matrix-core prefill attention kernel (attn_prefill_kernel or, past its context
 * limit, attn_prefill_blocked_kernel) so far: once
 * per layer of every pass that qualifies (16-bit model, head_dim 64 or 128, 16-bit or fp8 arena; a call of more than 80
 * rows or a batched prefill of >= 32 rows; no tree; SD_PREFILL_ATTN != 0); every other pass runs attn_kernel and leaves
 * the count alone.  A batched pass counts on its first session.  A host integer: no device work, no
 * synchronisation. */
int sd_session_prefill_attn_launches(const sd_session *s);
int sd_session_w12_launches(const sd_session *s);
/* The matrix-core prefill attention has two kernels: attn_prefill_kernel keeps a row group's whole score tile in LDS and
 * runs while that fits (2048 keys at head_dim 128, 2176 at 64); past it - by default where sd_prefill_attn_route says so, and
 * at any context when SD_PREFILL_ATTN_BLOCK=K (K > 0, rounded up to a multiple of 64) is set - attn_prefill_blocked_kernel
 * sweeps the keys in blocks and computes the same bits at any context length.  sd_session_prefill_attn_launches counts both, this one the blocked kernel's launches
 * alone. */
int sd_session_prefill_attn_blocked_launches(const sd_session *s);
/* The plan such a pass gets (host only: no device, no session): for a model of `head_dim`, a pass whose last row sees s_max
 * keys and block_keys = the value of SD_PREFILL_ATTN_BLOCK (0: the default policy), *kernel = 0 (no matrix-core kernel for
 * this head_dim), 1 (single tile) or 2 (blocked), *block = keys per score tile, *lds_bytes = the launch's dynamic LDS.
 * The launch path calls the same function.  Any out pointer may be NULL. */
int sd_prefill_attn_plan(int head_dim, int s_max, int block_keys, int *kernel, int *block, long *lds_bytes);
/* The route of a contiguous pass of n_rows rows (one stream) on a model of n_heads heads whose last row sees s_max keys (host
 * only; the function the launch path calls): *kernel = 0 (attn_kernel), 1 (single tile) or 2 (blocked).  Past the tile limit
 * the blocked kernel is the default where the launch has at least 2 workgroups (heads x 16-row groups) per CU - below that its
 * three sweeps are slower than attn_kernel's split keys - and where attn_kernel's splits cannot hold the pass at all; a forced
 * block always takes it.  cus = 0: the device's CU count (256 without a device). */
int sd_prefill_attn_route(int head_dim, int n_heads, int n_rows, int s_max, int block_keys, int cus, int *kernel);

/* One model forward over n_new tokens at absolute positions pos0 .. pos0+n_new-1, appending their
 * K/V rows into the arena in-kernel (replaces the per-layer torch.cat of modeling_llama.py:337-338 /
 * modeling_opt.py:192-193 and kvcache_model.py:214).  tokens: device int32, read at tokens[0..n_new).
 * Logits (fp32) are produced for the LAST n_logits of the new rows into logits_out[n_logits][vocab]
 * (row stride ld_logits); n_logits == 0 skips the head.  Rollback is O(1): the caller just passes a
 * smaller pos0 next time (kvcache_model.py:359-436).  n_new <= max_rows, pos0+n_new <= max_seq. */
int sd_session_forward(sd_session *s, const int32_t *tokens, int n_new, int pos0, int n_logits,
                       float *logits_out, long ld_logits, void *stream);

/* Tree verify (reference kvcache_model.py:38-136 forward_tree_attention with the extra attention
 * mask of modeling_llama.py:684-689 / modeling_opt.py:660-667): ONE target forward over the n <= 64 nodes of a draft token
 * tree.  tokens / positions / masks are DEVICE-side for tokens (int32[n]) and HOST-side for positions and masks:
 * node i sits at position positions[i] (its depth; RoPE / learned position), attends to all `base_len` cached positions and
 * to the nodes j with bit j of masks[i] set (its ancestors and itself, j <= i), and its K / V rows are appended at arena
 * slot base_len + i.  Logits of all n nodes go to logits_out[n][vocab].  sd_session_compact_kv afterwards moves the kept
 * path's rows together (reference kvcache_model.py:326-353 rollback_tree_attention): slot base_len + idx[j] -> base_len + j
 * (idx: device int32[k], ascending) in every layer and head. */
int sd_session_forward_tree(sd_session *s, const int32_t *tokens, const int32_t *positions, const uint64_t *masks, int n,
                            int base_len, float *logits_out, long ld_logits, void *stream);
int sd_session_compact_kv(sd_session *s, int base_len, const int32_t *idx_dev, int k, void *stream);

/* Single-stream decode / verify forwards of a 16-bit model run two kinds of launches whose workgroups wait for each other
 * on device-side counters: attention + O projection (csrc/fused_kernels.h) and the k-split down projection with the
 * residual epilogue (csrc/normload_kernels.h).  Every such wait is bounded (20 ms); one that runs into its limit poisons
 * its output rows with NaN - the sampler then reports the reference's 'norm logits error' (utils.py:186-188), never
 * finite numbers - and sets a sticky bit in the session's status word: bit 0 attention + O, bit 1 down projection.
 * sd_session_fused_status reads and clears the word (blocking copy; the session's stream must be idle); 0 = no wait has
 * timed out since the last read.  After a non-zero read, and after any forward that returned an error, the next forward
 * first re-zeroes the counters (stream-ordered), so one failed launch cannot leave every later wait short. */
int sd_session_fused_status(sd_session *s, unsigned *status_out);
/* TEST HOOK: the fused launches of the NEXT forward of this session expect `extra` (0..1024) arrivals more than will come,
 * i.e. every one of their waits times out.  Exists so that the timeout branch is covered by a test (tests/); the forward
 * after that one is back in step. */
int sd_session_test_skew_wait(sd_session *s, int extra);
/* Debugging aid: the per-workgroup records the last fused attention + O-projection launch left when the session was
 * created under SD_AO_STAMPS=1 (fused_kernels.h, AO_STAMP_WGS): out[w][8] long long for workgroups w < n_wgs <= 512 -
 * wall_clock64 (100 MHz) at the workgroup's milestones, XCC_ID / HW_ID, and role / head / row group. */
int sd_session_ao_stamps(sd_session *s, long long *out, int n_wgs);

/* Stream-batched forward: the new rows of up to 16 independent sequences share ONE pass over the
 * weights (same bytes streamed, n_items times the tokens).  Each item names its own session (KV arena), its token
 * buffer `seq` (device int32 indexed by ABSOLUTE position: the rows read seq[pos0 .. pos0+n_new)), its cache length
 * pos0, its number of new rows and how many of its last rows need logits.  Activations use items[0].session's
 * scratch (total rows <= its max_rows, <= 64); all sessions must belong to the same model.  Logit rows come out packed
 * in item order into logits_out.  sd_session_forward is the one-item case of this call. */
typedef struct {
    sd_session *session;
    const int32_t *seq;
    int32_t pos0, n_new, n_logits;
} sd_batch_item;
int sd_batch_forward(const sd_batch_item *items, int n_items, float *logits_out, long ld_logits, void *stream);
/* Batched prefill: the items' rows (each stream's n_new rows at positions pos0.. , a contiguous run; n_logits must be 0) go
 * through ONE pass over the weights - up to 256 rows and 32 attention groups (8 consecutive rows of one stream) in all.
 * K / V rows are appended to every stream's own arena; nothing else comes back.  All sessions share one model. */
int sd_batch_prefill(const sd_batch_item *items, int n_items, void *stream);

/* ---- Argument blocks of the native loops below: caller-owned host structs, used during the call only.  An entry refuses a
 * NULL block with SD_ERR_INVALID before anything is written or launched.
 * sd_sampling: what every loop samples with and stops on; ld = row stride of the probability arenas.
 * sd_head_scratch: one model's logit rows (scratch for its head) and the SD_NORM_* mode its rows are normalised in.
 * sd_spec_stream: the device side of ONE stream (the eight leading fields of sd_batch_stream): the two sessions, the device
 *   int32 token buffer, the probability arenas indexed by position (row stride sd_sampling.ld), 3*gamma+1 device error words
 *   (gamma draft norm words, gamma draft sample words, gamma+1 target norm words; folded into res.flags bit 3), the device
 *   result block and its pinned-host copy.
 * sd_spec_scratch: both heads; norm_workspace (device, may be NULL): sd_norm_workspace_bytes(max_rows_per_forward) bytes, the
 *   candidate rows of a pass and, behind them, one candidate list per row; the most rows a target pass may carry.
 * sd_lockstep_log: host arrays of max_iters_log entries (each may be NULL): time of an iteration's verify passes, streams in
 *   it, their mean context.  Out: n_iters, and err = 1 when a stream hit a sampling / normalisation error (the reference raises).
 * sd_seq_state: in/out state and logs of ONE sequence.  host_seq (host int32, capacity >= T + gamma + 1) holds the `len` tokens
 *   so far and receives the new ones; draft_len / target_len are the cache lengths, (seed, draw) the Philox position; the loop
 *   ends at T tokens, at a new EOS (more than ori_eos_cnt in all) or after max_iters iterations.  All written back on every way
 *   out, also after an error.  Per iteration i < n_iters: acc_len_out[i], p_at_out / q_at_out (the accept ratios' operands),
 *   draft_ms_out / target_ms_out[i]; any of the five may be NULL.  err: 0, 1 = 'prob error', 2 = 'norm logits error'.
 * sd_ar_log: host arrays of max_steps_log entries (may be NULL): HIP-event time of each step, streams in it.  Out: n_steps, err.
 * sd_loop_opts: what a call may carry per request, as the LAST argument of every loop entry: per-stream sampling parameters,
 *   per-token log-probabilities, penalties and logit edits.  32 bytes, defined below behind its members' types, each of which
 *   has its contract there.  Every member may be NULL, and a NULL `opts` is a block of four NULLs: the call is then, launch for
 *   launch, the loop without the feature.  A member is checked behind the entry's own refusals, in the members' order
 *   (row_params, logprobs, penalties, edits), with SD_ERR_INVALID before anything is written or launched; the text names the
 *   entry that was called, then the member. */
struct sd_loop_opts;
typedef struct { float temperature; int32_t top_k; float top_p; int32_t V; long ld; int32_t eos_token_id; } sd_sampling;
typedef struct { float *logits; long ld_logits; int32_t norm_mode; } sd_head_scratch;
typedef struct {
    sd_session *draft, *target; int32_t *seq; float *q_hist, *p_hist; int *err_words; sd_accept_result *res_dev, *res_host;
} sd_spec_stream;
typedef struct { sd_head_scratch draft, target; void *norm_workspace; int32_t max_rows_per_forward; } sd_spec_scratch;
typedef struct { float *verify_ms_out; int32_t *verify_streams_out; float *verify_ctx_out; int32_t max_iters_log, n_iters, err; } sd_lockstep_log;
typedef struct {
    int32_t *host_seq; int32_t len, T, ori_eos_cnt, draft_len, target_len; uint64_t seed, draw; int32_t max_iters;
    int32_t *acc_len_out; float *p_at_out, *q_at_out, *draft_ms_out, *target_ms_out;
    int32_t n_iters, err;
} sd_seq_state;
typedef struct { float *step_ms_out; int32_t *step_streams_out; int32_t max_steps_log; int32_t n_steps, err; } sd_ar_log;
/* The whole loop of speculative_sampling.py:1934-2046 for the device-RNG mode, no Python between iterations.  An iteration
 * (:1934-2031) is gamma x (draft forward over the uncached rows + sd_norm_sample straight into seq[]), one target forward over
 * its uncached rows + sd_norm_probs of the last gamma+1, sd_accept_scan and the residual / bonus sample (one launch on the
 * target rows' candidate lists when the workspace holds them), one async copy of the result block to dev->res_host and one
 * stream wait; iterations run until the sequence holds T tokens, a new EOS appears (more than ori_eos_cnt of
 * sampling->eos_token_id in total) or an error word is set.  The Philox position of `seq` is advanced exactly as the
 * iteration's draw order prescribes: gamma draft draws, the discarded target sample, gamma uniforms - or, with random_seed
 * != 0, the stream restarted at (random_seed, 0), the scan then reading r_const (gamma device floats) - and the resample.
 * gamma p_at / q_at values per iteration; the two phases are timed with HIP events exactly when seq->draft_ms_out or
 * seq->target_ms_out is set.  Norm modes: scratch->draft / target.norm_mode; the residual runs in the target's mode when both
 * are equal, else in fp32.  Refused with SD_ERR_INVALID before anything is written or launched, in this order: a NULL block or
 * a NULL pointer in dev, seq->host_seq or either scratch->*.logits; gamma outside 1..16; random_seed without r_const;
 * temperature 0; a norm_workspace with max_rows_per_forward < gamma + 1; then sampling->V differing from a model's vocabulary;
 * then opts: the loop samples with sampling's own triple, so a non-NULL opts->row_params is refused. */
int sd_spec_generate(const sd_spec_stream *dev, int gamma, const sd_sampling *sampling, const sd_spec_scratch *scratch,
                     sd_seq_state *seq, uint64_t random_seed, const float *r_const, void *stream,
                     const struct sd_loop_opts *opts);
/* The stream-batched loop (throughput mode) without the interpreter between iterations: up to 16
 * independent streams decode in lock-step - every draft step one sd_batch_forward + sd_norm_batch over the active
 * streams, every verify one target pass per max_rows_per_forward / (gamma + 1) streams, then sd_accept_batch, one copy of
 * the result blocks and one wait - until every stream holds T tokens or has produced a new EOS.  Per stream: the two
 * sessions, the device token buffer / probability arenas / error words, its device and pinned-host result block (the
 * streams' blocks must be consecutive: one copy moves them all), the host token buffer and the in/out loop state
 * (lengths, cache lengths, Philox position); per-iteration statistics as in sd_spec_generate.  Each stream runs exactly
 * the algorithm of sd_spec_generate with its own Philox stream.  Sampling parameters, scratch and log: the blocks above.
 * With a norm_workspace the loop runs the single-stream loop's sampling tail (since round 4):
 * the draft head leaves tile maxima and clears the streams' probability rows, the target rows come back with candidate
 * lists, accept scan + residual / bonus sample are one launch on them - bit-equal to the dense kernels named above, which
 * remain the path without a workspace, with more streams than one verify pass holds, and under SD_BATCH_FUSED_TAIL=0. */
typedef struct {
    sd_session *draft, *target;
    int32_t *seq;
    float *q_hist, *p_hist;
    int *err_words;
    sd_accept_result *res_dev, *res_host;
    int32_t *host_seq;
    int32_t len, T, ori_eos_cnt, draft_len, target_len;
    uint64_t seed, draw;
    int32_t done, calls;
    int32_t *acc_len_out;
    float *p_at_out, *q_at_out;
} sd_batch_stream;
int sd_spec_batch_generate(sd_batch_stream *streams, int n_streams, int gamma, const sd_sampling *sampling,
                           uint64_t random_seed, const float *r_const, const sd_spec_scratch *scratch, sd_lockstep_log *log,
                           void *stream, const struct sd_loop_opts *opts);
/* Continuous batching for the lock-step loop: any number of prompts share `n_slots` (1..16) slots.  A slot is an
 * sd_batch_stream of which the caller fills the device side only - the two sessions, the token buffer (slot_cap ints), the
 * probability arenas, the error words and the consecutive result blocks; the arenas and sessions hold slot_cap positions,
 * slot_cap >= max over the prompts of max(L, T) + gamma + 2.  The loop owns the other fields.  Prompts are admitted in array
 * order: whenever a slot's stream is done (it holds T tokens or produced a new EOS - sd_spec_batch_generate's rule) the next
 * waiting prompt takes the slot at the next iteration boundary as a JOINER: its tokens are copied to the slot's token buffer
 * (asynchronously, on `stream`), both cache lengths start at 0, the error words and the result block are cleared.  Its rows
 * [0, L-1) then ride the passes the loop runs anyway - the draft rows the gamma draft steps, the target rows the verify
 * passes - as extra items with n_logits = 0 behind the active streams' items, as many per pass as sd_spec_queue_plan gives;
 * it decodes from the first boundary at which both models hold L-1 positions (L = 1: at once), on Philox stream (seed, 0).
 * A prompt with L >= T is finished at admission.  While no stream is active (the start of the call, or every stream ending
 * at once) the joiners of all slots are prefilled by sd_batch_prefill passes instead.  Each prompt runs exactly the algorithm
 * of sd_spec_generate; everything else - the blocks, statistics, log->err, the sampling tail - is sd_spec_batch_generate's.
 * Per prompt: its tokens (pinned host, L ints), L, the length T to reach, the EOS count of the prompt, the seed, the host
 * token buffer (>= T + gamma + 1 ints, holding the prompt) and the per-iteration logs; out: len, calls, admit_iter (the
 * first iteration it decodes in) and finish_iter (its last; both the boundary's iteration number for a prompt that never
 * decodes).
 * Prompts that start with the same tokens: the donors are sessions of the draft and the target model that hold positions
 * [0, shared_rows) of those tokens - prefilled by the caller on `stream` - and stay untouched.  A prompt that takes a slot then
 * starts with both cache lengths at c = min(shared_rows, L - 1), not at 0: those rows reach the slot's arenas through one
 * sd_session_copy_kv launch (below) per model for all prompts admitted at that iteration boundary, on `stream`, ahead of the
 * iteration's forwards; its rows [c, L-1) then ride the passes as described (c == L-1: it decodes from that boundary on).
 * Without a shared prefix the donors are NULL and shared_rows is 0.
 * passes_out (6 ints, may be NULL): passes over the target weights, passes over the draft weights, target passes that carried
 * prompt rows only, how many of those were sd_batch_prefill passes, the target rows forwarded for prompts inside the call, and
 * the KV rows copied per model, summed over the prompts. */
typedef struct {
    const int32_t *tokens;
    int32_t L, T, ori_eos_cnt;
    uint64_t seed;
    int32_t *host_seq;
    int32_t *acc_len_out;
    float *p_at_out, *q_at_out;
    int32_t len, calls, admit_iter, finish_iter;
} sd_queue_prompt;
int sd_spec_queue_generate(sd_batch_stream *slots, int n_slots, int slot_cap, sd_queue_prompt *prompts, int n_prompts,
                           int prefill_chunk, int gamma, const sd_sampling *sampling, uint64_t random_seed,
                           const float *r_const, const sd_spec_scratch *scratch, sd_lockstep_log *log, int *passes_out,
                           void *stream, sd_session *donor_draft, sd_session *donor_target, int shared_rows,
                           const struct sd_loop_opts *opts);
/* The passes of one step of that loop (host only; the function the loop calls, once per draft step and once per verify).
 * Inputs: the rows one pass may hold; the logit rows a pass may hold once not every row is one (sd_batch_forward: 64); the
 * active streams' row counts, in order (n_act <= 16), and whether those rows are all logit rows (a verify) or one per
 * stream (a draft step); the joiners' remaining rows in queue order (n_join <= 16); prefill_chunk, the most joiner rows a
 * pass may carry (0: whatever room it has); force_progress.  The active streams are cut into passes of whole streams, in
 * order, as many per pass as the rows allow (at least one, at most 16) - with no joiner that is sd_spec_batch_generate's
 * split.  Each pass then takes joiner rows, first joiner first, one chunk per joiner: up to row_budget minus the pass's
 * rows, up to prefill_chunk, up to 16 items in all, and none when its logit rows exceed mixed_logit_limit.  With
 * force_progress, when a joiner has rows left and no pass took one, a last pass without active streams carries joiner rows
 * only.  passes[p] = active streams [act0, act0 + n_act) and chunks[chunk0 .. chunk0 + n_chunks); a chunk = (joiner, its
 * first row counted from the joiner's next row, rows); a joiner's chunks are consecutive over the passes. */
typedef struct {
    int32_t act0, n_act, chunk0, n_chunks;
} sd_queue_pass;
typedef struct {
    int32_t joiner, row0, rows;
} sd_queue_chunk;
int sd_spec_queue_plan(int row_budget, int mixed_logit_limit, const int32_t *act_rows, int n_act, int logit_rows,
                       const int32_t *join_rows, int n_join, int prefill_chunk, int force_progress, sd_queue_pass *passes,
                       int max_passes, sd_queue_chunk *chunks, int max_chunks, int *n_passes_out, int *n_chunks_out);
/* Session-to-session KV copy.  KV positions [lo, hi) of every layer, K and V, and KV head go from src's arena to each dst's
 * arena, as bytes; one launch on `stream` serves all items, 1..16 of them.  The arenas may hold different numbers of
 * positions.  Refused with SD_ERR_INVALID before any launch: a null argument, n_items outside 1..16, a dst of another model
 * than src's, dst == src, one arena fp8 and the other not, lo < 0, hi < lo, hi past either arena.  An item with hi == lo is
 * skipped, and a call whose items are all empty launches nothing.  fp8 arenas: the stored bytes mean the same in both sessions
 * only under equal scale tables - the caller answers for that.  No cache length is read or written: lengths live with the
 * callers. */
typedef struct {
    sd_session *dst;
    int32_t lo, hi;
} sd_kv_copy_item;
int sd_session_copy_kv(const sd_session *src, const sd_kv_copy_item *items, int n_items, void *stream);
/* The whole loop of multi_speculative_sampling(strategy="iid") (speculative_sampling.py:1379-1716) for the device-RNG mode,
 * no interpreter between iterations.  `width` replicas, each with its own sessions, token buffer and probability arenas;
 * per iteration: gamma draft steps (one pass over the draft weights for all replicas each, sampled straight into
 * seq_w[L+i]), the target over every replica's uncached rows in passes of max_rows_per_forward / n_new replicas,
 * sd_multi_accept_resample, sd_multi_adopt, ONE async copy of `dev_block` to `host_block` and ONE stream wait.
 * dev_block (device) / host_block (pinned host), sd_spec_multi_block_bytes(width, gamma) bytes each: the sd_multi_result
 * followed by the iteration's error words, int32 [width][3*gamma+1] (per replica: gamma draft norm words, gamma draft
 * sample words, gamma+1 target norm words); the caller zeroes dev_block once.
 * `seq` is the sequence's sd_seq_state, sampling / scratch the blocks above.  Its Philox position is advanced per iteration
 * exactly as the Python loop advances it: width draws per draft step (replica w of step i: draw + i*width + w), width draws
 * skipped for the target's discarded sample, then - after a restart at (random_seed, 0) when random_seed != 0, in which case
 * the scan reads r_const (width*gamma device floats) instead - width*gamma uniforms, then one resample draw.
 * The loop ends as sd_seq_state says (on a new EOS the caller cuts), or on an error: seq->err 1 = 'prob error' (a draft
 * sample word, or the resample: then the accepted drafts ARE appended, as the reference has already cut its output there),
 * 2 = 'norm logits error'.  acc_len_out[i] is -1 for an iteration that ended on an error word (it counts as a call, its scan
 * was not read); p_at_out / q_at_out[i*width*gamma ..] are [w][j], gamma columns; the two times are HIP events.
 * Limits: width <= 16, gamma <= 16, 2*width <= max_rows_per_forward (a draft step may carry two rows per replica); a
 * violation returns SD_ERR_INVALID before anything is launched. */
typedef struct {
    sd_session *draft, *target;
    int32_t *seq;                 /* device int32, seq_cap entries */
    float *q_hist, *p_hist;       /* probability arenas by absolute position, row stride ld */
} sd_multi_replica;
size_t sd_spec_multi_block_bytes(int width, int gamma);
int sd_spec_multi_generate(const sd_multi_replica *reps, int width, int gamma, int seq_cap, const sd_sampling *sampling,
                           uint64_t random_seed, const float *r_const, const sd_spec_scratch *scratch, void *dev_block,
                           void *host_block, sd_seq_state *seq, void *stream);
/* Autoregressive sampling (reference autoregressive_sampling.py:9-61) of up to 16 independent streams in lock-step, no
 * interpreter between steps.  Per step: the uncached rows seq[cache_len .. len) of every stream that is not done go through
 * ONE sd_batch_forward; one sd_norm_batch with sample = 1 (on the head's tile maxima where the lock-step draft steps use
 * them) writes stream b's probability row probs_b[len_b - 1] and samples its token with Philox (seed_b, draw_b) straight
 * into seq_b[len_b]; one 64-lane launch gathers {int32 token, int32 flags} per stream into dev_block (flags: bit 0 sample
 * error, bit 1 norm error, bit 2 token == eos_token_id) and clears the error words; ONE async copy of 8 * n_streams bytes to
 * host_block and ONE stream wait end the step.
 * Per stream: its session, device token buffer (int32, indexed by absolute position, capacity > T), probability arena
 * (row stride ld), two device error words (norm error, sample error; zero on entry), host token buffer (capacity >= T,
 * holding the `len` tokens so far) and the in/out state: len, the length T to reach, cache_len, the Philox position.
 * A stream is done when it holds T tokens or its new token is eos_token_id (the EOS is kept); done streams drop out of the
 * later passes.  `draw` advances by one per generated token, cache_len ends at len - 1, `steps` counts the stream's tokens.
 * One stream may arrive with any cache_len < len (the first step then feeds the whole prompt in chunks, as
 * sd_session_forward callers do); with more streams every one arrives with cache_len == len - 1 (sd_batch_prefill).
 * dev_block (device) / host_block (pinned host): sd_ar_block_bytes(n_streams) bytes each = 8 * n_streams rounded up to a
 * multiple of 16 (0 outside 1..16 streams).  norm_workspace: sd_norm_workspace_bytes(n_streams) bytes, or NULL.
 * sampling, head (the model's logit rows and norm mode) and log: the blocks above.
 * An error word ends the loop after that step, whose tokens are not committed: log->err 2 = 'norm logits error' (a norm
 * word, looked at first: the reference normalises before it samples, and the fused sampler sets both words on a row it
 * cannot normalise), 1 = 'prob error' (a sample word alone); log->n_steps counts that step.
 * Limits: n_streams in 1..16 and <= sd_model_max_pass_rows, one model behind all sessions; a violation returns
 * SD_ERR_INVALID before anything is launched.  Behind them opts: every stream samples with sampling's own triple, so a non-NULL
 * opts->row_params is refused. */
typedef struct {
    sd_session *session;
    int32_t *seq;
    float *probs;
    int *err_words;
    int32_t *host_seq;
    int32_t len, T, cache_len;
    uint64_t seed, draw;
    int32_t done, steps;
} sd_ar_stream;
size_t sd_ar_block_bytes(int n_streams);
int sd_ar_batch_generate(sd_ar_stream *streams, int n_streams, const sd_sampling *sampling, const sd_head_scratch *head,
                         void *norm_workspace, void *dev_block, void *host_block, sd_ar_log *log, void *stream,
                         const struct sd_loop_opts *opts);

/* ---- Per-token target log-probabilities.  For a token t that a loop emits at position i, the score is
 * x[t] - log sum_v exp(x[v]) in fp32, x = the target model's raw logit row for position i - 1: rounded to the weights'
 * 16-bit type where the rows still have to be (SD_NORM_ROUND_*), taken BEFORE temperature, top_k and top_p - what the model
 * says, not what the sampler drew from.  Its mean over a call's new tokens is the reference harness' get_score
 * (evaluation.py:109-124) without a second target pass.
 * sd_token_logprobs scores up to 16 items x 17 rows in one launch on `stream` (one workgroup per scored row).  An item is one
 * stream's `rows` consecutive fp32 logit rows (row stride ld >= V; no alignment asked of ld or of the rows), the device
 * tokens to score them at (row r at tokens[r]), `rows` device output floats and `res`, a device result block or NULL: with
 * it only rows r <= res->n_accepted are scored and the other output floats stay untouched, so the launch goes behind the
 * accept / resample launch that fills the block.  `items` is a host array; mode: SD_NORM_ROUND_BF16 / _F16 or 0 (bits 0-1,
 * the other bits are not read).  A token outside [0, V) scores NaN and reads nothing; a NaN in a row gives NaN for that row;
 * -inf entries weigh nothing and a row of nothing else gives NaN.  Refused with SD_ERR_INVALID before any launch: a NULL
 * argument (res excepted), n_items outside 1..16, V < 1, both rounding bits, rows outside 1..17, ld < V. */
typedef struct {
    const float *logits;
    long ld;
    int32_t rows;
    const int32_t *tokens;
    const sd_accept_result *res;
    float *out;
} sd_logprob_item;
int sd_token_logprobs(const sd_logprob_item *items, int n_items, int V, int mode, void *stream);
/* sd_logprob_block: what a loop needs to return those scores with its tokens; caller-owned like the blocks above.  dev
 * (device) and host (pinned host): 16 x 17 floats each, stream (slot) i's slice at i * 17.  logprob_out[k]: a host float array
 * per stream - per prompt in the queue - with the capacity of that stream's host token buffer; entry j is the score of the
 * j-th token the call emitted for it (position L + j, L = its length on entry).  It is member `logprobs` of
 * sd_loop_opts in all four loops; a NULL member is the loop without scores, launch for launch.  With a block, per
 * iteration or step: ONE sd_token_logprobs launch over all active streams behind the accept / resample launch (behind the
 * sampler in the autoregressive loop, one row per stream at seq[len]), ONE more async copy of the float slices beside the
 * copy of the result blocks, ahead of the one wait; after it the stream's n_accepted + 1 floats are appended where its tokens
 * are.  A failed iteration appends none.  Every verify pass of the lock-step loops writes the same logit slab, so in an
 * iteration whose verify takes several passes the loop - with a block only - accepts (sd_accept_batch) and scores a pass's
 * streams before it enqueues the next pass; still one copy and one wait.  The rows are read where the forward left them:
 * scratch->target.logits in the lock-step loops, the head's own slab in the other two.  Refused with SD_ERR_INVALID behind
 * the entry's own refusals, before anything is launched: a NULL dev, host or logprob_out, or a NULL array in it. */
typedef struct { float *dev, *host; float **logprob_out; } sd_logprob_block;

/* ---- Token scoring: the log-probability and the rank of one token per logit row, and the row's top_n ids.  x is an fp32 logit
 * row as sd_token_logprobs reads it (the pending SD_NORM_ROUND_* rounding applied to every entry), t the token it is scored at.
 *   order         ids by value descending, compared as IEEE floats (-0.0 == +0.0), ties to the lower id first - torch.sort(x,
 *                 descending=True, stable=True); -inf entries take part like any value and come last
 *   logprob       x[t] - log sum_v exp(x[v]): sd_token_logprobs' float bit for bit (same accumulator, traversal and reduction)
 *   rank          1 + #{v : x[v] > x[t]} + #{v < t : x[v] == x[t]}, t's 1-based place in the order
 *   top_ids[j], top_logprobs[j]  (j < top_n) the j-th id of the order and its log-probability, from the same (max, sum) pair
 *                 as logprob - bit-equal to it where top_ids[j] == t; entries j >= V are -1 and NaN
 * A row whose log-sum is not finite - it holds a NaN or a +inf, or nothing but -inf - is void: logprob NaN, rank 0, every
 * top_ids entry -1, every top_logprobs entry NaN.  A token outside [0, V) gives logprob NaN and rank 0 and reads nothing; the
 * row's top list is still written.  (quality.score_rows_torch is this text in torch.)
 * sd_score_rows scores up to 16 items x SD_SCORE_MAX_ROWS rows in one launch on `stream` (one workgroup per row; the row is read
 * once from memory and once more from L2, and 65 more times only where over 12288 entries crowd the stripes of top_n lanes -
 * no row of V <= 156672).  An item is `rows` consecutive fp32 logit rows (row stride ld >= V; no alignment asked of ld
 * or of the rows), the device tokens to score them at, and where the results go: `rows` floats and ranks (rank may be NULL)
 * and rows x top_n ids and floats, row-major (both unread when top_n == 0).  `items` is a host array; mode as for
 * sd_token_logprobs.  Refused with SD_ERR_INVALID before any launch, naming the item: a NULL argument (rank excepted; the two
 * top arrays only when top_n > 0), n_items outside 1..16, V < 1, both rounding bits, rows outside 1..SD_SCORE_MAX_ROWS, ld < V,
 * top_n outside 0..SD_SCORE_MAX_TOP. */
#define SD_SCORE_MAX_TOP 20
#define SD_SCORE_MAX_ROWS 80
typedef struct {
    const float *logits;
    long ld;
    int32_t rows;
    const int32_t *tokens;
    float *logprob;
    int32_t *rank;
    int32_t *top_ids;
    float *top_logprobs;
} sd_score_item;
int sd_score_rows(const sd_score_item *items, int n_items, int V, int top_n, int mode, void *stream);
/* sd_score_sequence scores tokens first .. n - 1 of the n device ids `tokens` (each in [0, V), the caller's guarantee as for
 * sd_session_forward; 1 <= first <= n - 1): output entry j is tokens[first + j] scored on the row of position first + j - 1.
 * Positions [0, first - 1) are fed without logit rows, up to the session's max_rows per pass; positions [first - 1, n - 1) in
 * passes whose rows are all logit rows, up to min(slab_rows, the session's rows per such pass) each, and every such pass is
 * followed by ONE sd_score_rows launch on the rows where the forward left them - the head's own slab, its pending rounding as
 * the mode, or `slab` (slab_rows x ld_slab floats, the only logit buffer) - writing straight into `out` at the pass's offset:
 * n - first floats and ranks (rank may be NULL), (n - first) x top_n ids and floats.  Everything is enqueued on `stream` and
 * nothing is waited for.  The session's cache is rewritten from position 0 and holds [0, n - 1) afterwards.  Refused with
 * SD_ERR_INVALID before anything is launched: a NULL argument (out->rank excepted; the top arrays only when top_n > 0), n < 2,
 * first outside 1..n - 1, top_n outside 0..SD_SCORE_MAX_TOP, slab_rows < 1, ld_slab < V, n - 1 > the session's max_seq, a
 * session bound to a tensor-parallel group. */
typedef struct {
    float *logprob;
    int32_t *rank;
    int32_t *top_ids;
    float *top_logprobs;
} sd_score_out;
int sd_score_sequence(sd_session *s, const int32_t *tokens, int n, int first, int top_n, float *slab, long ld_slab, int slab_rows,
                      const sd_score_out *out, void *stream);

/* ---- Per-request repetition, frequency and presence penalties.  A logit row at position pos predicts token pos + 1; its
 * history is seq[0 .. pos], and the stream's prompt is the P tokens it held when the call started.  For a token id t, c_all(t)
 * counts t in seq[0 .. pos] and c_out(t) in seq[P .. pos].  x is the logit as the sampler reads it, the pending SD_NORM_ROUND_*
 * rounding applied.  With repetition r (finite, > 0, neutral 1), frequency f and presence p (finite, neutral 0):
 *   1. c_all(t) > 0 and r != 1:  y = x > 0 ? x / r : x * r       (prompt + output, the usual repetition penalty)
 *   2. c_out(t) > 0:             y = y - fl(f * float(c_out)), then y = y - p      (output tokens only)
 * Each result is one IEEE fp32 operation (a correctly rounded division, no contraction of the product into the subtraction);
 * in an SD_NORM_DT_* mode each of them, the product included, is also rounded to that 16-bit type, as torch's 16-bit CPU
 * kernels do; the three parameters are not rounded.  A token that is not in the history keeps its (rounded) logit bit for bit;
 * NaN and +-inf go through the same operations; a history entry outside [0, V) is ignored.
 * (sampling.utils.apply_penalties is this text in torch.)
 * sd_penalize_rows edits up to 16 items x 17 rows in one launch on `stream` (one workgroup per row and window of 4096 ids): an item is one stream's
 * `rows` consecutive fp32 logit rows `in` (row stride ld_in >= V), where their edited copies go (`out`, row stride ld_out >= V;
 * never `in`: the raw rows are not written, the log-probabilities above keep reading them), the stream's device tokens `seq`,
 * of which row r sees the first hist0 + r, and its prompt length.  No alignment is asked of the rows or the strides.  `mode`
 * is the word the norm launch would get: bits 0-1 the pending rounding, SD_NORM_DT_* the rows' dtype; the norm launch that
 * reads `out` takes the same word with bits 0-1 cleared.  A neutral item (1, 0, 0) is rounded and copied.  The result is a
 * pure function of the inputs (integer counts, every output element written once).  Refused with SD_ERR_INVALID before any
 * launch, naming the item: a NULL argument, n_items outside 1..16, V outside 1..65536, both rounding bits, rows outside 1..17,
 * a stride < V, hist0 < 1, prompt_len < 0, repetition <= 0 or a parameter that is not finite. */
typedef struct { float repetition, frequency, presence; } sd_penalty;
typedef struct {
    const float *in;
    float *out;
    long ld_in, ld_out;
    int32_t rows;
    const int32_t *seq;
    int32_t hist0, prompt_len;
    sd_penalty pen;
} sd_penalty_item;
int sd_penalize_rows(const sd_penalty_item *items, int n_items, int V, int mode, void *stream);
/* sd_penalty_block: what a loop needs to sample from penalised rows; caller-owned.  rows: a device slab of max_rows x ld
 * floats (ld >= V) that holds the logit rows of the loop's largest pass: gamma + 1 in the single-stream loop, the streams in
 * the autoregressive loop, min(rows per target pass, streams x (gamma + 1)) in the lock-step loops.  A 16-byte aligned slab
 * with 4 | ld keeps the norm launch on its two-kernel path.  params[k] belongs to stream k - to prompt k in the queue, where a
 * slot changes penalties when it changes hands.  It is member `penalties` of sd_loop_opts in all four
 * loops; a NULL member, or a block whose params are all neutral, is the loop without penalties, launch for
 * launch.  Otherwise every pass - of a draft step, of the verify, of an autoregressive step - that holds at least one
 * penalised active stream gets ONE sd_penalize_rows launch between the forward and the norm launch, over all its logit rows,
 * one item per stream, hist0 = the position of the stream's first logit row + 1, prompt_len = its length on entry
 * (sd_queue_prompt.L); the norm launch then reads `rows` with the pending rounding bits cleared.  Such a pass does not ask the
 * head for tile maxima (the rule a top_k == 0 stream already imposes); its rows go through the norm workspace.  Passes
 * without a penalised stream, joiner rows, the accept / resample launches, the candidate lists and the Philox draw order are
 * untouched, and sd_token_logprobs keeps reading the raw rows: penalties act on what the sampler draws from, the scores stay
 * what the model says.  The draft rows are penalised like the target rows, so that the acceptance rate holds.  Refused with
 * SD_ERR_INVALID behind the entry's own refusals, before anything is launched, naming the index: a NULL rows or params,
 * ld < V, max_rows too small, repetition <= 0 or a parameter that is not finite. */
typedef struct { float *rows; long ld; int32_t max_rows; const sd_penalty *params; } sd_penalty_block;

/* ---- Per-request logit bias, allowed-token mask and min_tokens: the request fields that restrict what may be sampled.  A
 * logit row at position pos predicts token pos + 1; with P the stream's prompt length on entry, that token is output number
 * j = pos + 1 - P.  y is the logit as the sampler reads it after the penalties above (for a neutral triple: the logit with the
 * pending SD_NORM_ROUND_* rounding applied).  For a request with bias list B, allowed set A (NULL = every id) and min_tokens m:
 *   1. t in B:       y = y + b_t      (one IEEE fp32 addition, no contraction; in an SD_NORM_DT_* mode the result is rounded
 *                                      to that 16-bit type, as the penalty operations are; b_t is not rounded)
 *   2. t not in A:   y = -inf         (also where y is NaN or +inf)
 *   3. t == eos_token_id, eos_token_id >= 0, m > 0 and j < m:   y = -inf
 * in that order, behind the penalties: penalties -> bias -> masks, so that sd_penalize_rows' definition stays what it is and
 * the masks win over everything.  An id that is in no list keeps its bits.  (sampling.utils.apply_logit_edits is this text in
 * torch; it composes after apply_penalties.)
 * sd_logit_edit: bias_ids / bias_vals are two parallel device arrays of n_bias entries, 0 <= n_bias <= SD_EDIT_MAX_BIAS, ids
 * strictly ascending (an id outside [0, V) is ignored; of duplicate ids one value wins, nothing is read or written out of
 * bounds); allowed is a device array of (V + 31) / 32 words, bit t & 31 of word t >> 5 set = token t allowed - a banned id is
 * a cleared bit of the same mask.  Neutral is {NULL, NULL, 0, NULL, 0}.
 * sd_edit_rows is sd_penalize_rows with the edits: the same items, grid (one workgroup per row and window of 4096 ids),
 * alignment freedom and `mode`, out of place, up to 16 items x 17 rows in ONE launch that applies penalties, bias and masks in
 * one pass over each window; row r of an item has j = hist0 + r - prompt_len.  Any part of an item may be neutral; an item that
 * is neutral throughout is rounded and copied.  The result is a pure function of the inputs.  Refused with SD_ERR_INVALID before
 * any launch, naming the item: what sd_penalize_rows refuses, n_bias outside 0..SD_EDIT_MAX_BIAS, n_bias > 0 with a NULL
 * array, min_tokens < 0.  (sd_penalize_rows keeps its own kernel.) */
#define SD_EDIT_MAX_BIAS 1024
typedef struct {
    const int32_t *bias_ids;
    const float *bias_vals;
    int32_t n_bias;
    const uint32_t *allowed;
    int32_t min_tokens;
} sd_logit_edit;
typedef struct {
    const float *in;
    float *out;
    long ld_in, ld_out;
    int32_t rows;
    const int32_t *seq;
    int32_t hist0, prompt_len;
    sd_penalty pen;
    sd_logit_edit edit;
    int32_t eos_token_id;
} sd_logit_edit_item;
int sd_edit_rows(const sd_logit_edit_item *items, int n_items, int V, int mode, void *stream);
/* sd_logit_edit_block: what a loop needs to sample from edited rows; caller-owned.  rows / ld / max_rows: a slab sized as
 * sd_penalty_block's; params[k] belongs to stream k - to prompt k in the queue, where a slot changes its edits when it changes
 * hands.  It is member `edits` of sd_loop_opts in all four loops (logprobs and penalties may be NULL or set beside it);
 * the EOS id is sampling->eos_token_id.  A NULL member, or a block whose params are all neutral, is the call with the other
 * members alone, launch for launch.
 * Otherwise every pass - of a draft step, of the verify, of an autoregressive step - that holds at
 * least one active stream that is penalised or edited gets ONE sd_edit_rows launch between the forward and the norm launch (at
 * most one, whether the pass holds penalised streams, edited streams or both), over all its logit rows, one item per stream;
 * it writes the edit block's slab, the penalty block's slab is not touched, and the pass follows the rules of a penalised pass:
 * no tile maxima, rows through the norm workspace, a norm request that reads the slab with the pending rounding bits cleared.
 * Joiner rows, accept / resample, the candidate lists, the Philox order and the log-probability launch are untouched:
 * sd_token_logprobs keeps reading the raw rows.  Draft rows are edited like target rows, so the acceptance rate holds and the
 * draft never proposes a token the target gives zero mass.  A request whose mask and EOS floor leave no id allowed gives a
 * row of -inf, which the norm launch reports as it reports any such row.  Refused with SD_ERR_INVALID behind the entry's own
 * refusals, before anything is launched, naming the index: a NULL rows or params, ld < V, max_rows too small, n_bias outside
 * 0..SD_EDIT_MAX_BIAS, n_bias > 0 with a NULL array, min_tokens < 0. */
typedef struct { float *rows; long ld; int32_t max_rows; const sd_logit_edit *params; } sd_logit_edit_block;
/* The loops' optional block (the argument blocks above say how it is read).  row_params: per-request sampling parameters in
 * the two lock-step loops, NULL in the other two.  row_params[i] is what stream i of sd_spec_batch_generate samples with, and
 * what prompt i of sd_spec_queue_generate samples with in whichever slot it decodes, so a slot changes parameters when it
 * changes hands.  With an array, sampling->temperature / top_k / top_p are not read (V, ld and eos_token_id are); every draft
 * and verify row is normalised with its stream's triple through sd_norm_batch_rows' launch, and the draft head leaves tile
 * maxima in the passes whose sampled rows all have 1 <= top_k <= 64 and temperature > 0.  Each stream still runs exactly
 * sd_spec_generate's algorithm with its own triple.  Refused, naming the index: a temperature of 0, a negative top_k. */
typedef struct sd_loop_opts {
    const sd_row_sampling *row_params;  /* lock-step loops only: per stream / per prompt */
    const sd_logprob_block *logprobs;
    const sd_penalty_block *penalties;
    const sd_logit_edit_block *edits;
} sd_loop_opts;

/* ---- Grammar-constrained decoding: a per-request token automaton masks every logit row.  The allowed set of a row depends on
 * the tokens the request has emitted so far, so the automaton advances on the device, along the drafted tokens, inside the one
 * launch that already edits a pass's logit rows.
 * sd_grammar: a deterministic automaton over token classes.  All pointers are device pointers and the arrays are caller-owned;
 * the struct itself is copied where it is attached.
 *   masks  n_states x W words, W = (V + 31) / 32: bit t & 31 of word s * W + (t >> 5) set = token t allowed in state s
 *   next   n_states x n_classes: the state after a token of class c in state s, or -1
 *   cls    V entries in [0, n_classes): a token's class; NULL = identity (n_classes == V)
 * States.  A stream has prompt length P on entry of the call; the logit row at position pos predicts output token number
 * j = pos + 1 - P and is masked by state s_j:
 *   s_j = start for j <= 0;   s_{j+1} = step(s_j, seq[P + j]);
 *   step(s, t) = next[s * n_classes + (cls ? cls[t] : t)] when 0 <= s < n_states, 0 <= t < V and that entry lies in
 *   [0, n_states); step(s, t) = -1 (dead) in every other case.  Nothing is read out of bounds for any t or s.
 * Edit order: penalties -> bias -> allowed mask -> grammar -> EOS floor.  With s_j >= 0 a token whose bit in masks[s_j] is
 * clear becomes -inf, whatever the logit holds.  A dead row (s_j < 0) skips the grammar part, and so does a row with j < 0; their
 * other edits still apply.  In valid use a dead row can only follow a drafted token that the target gives zero mass: that token
 * is rejected at that row, so no later row is used - the rule exists so that nothing faults and no spurious row of -inf raises
 * 'norm logits error' on a row nobody samples from.  An id that no part touches keeps its bits.
 * (sampling.utils.apply_grammar is this text in torch; it composes after apply_logit_edits.)
 * State cache.  A stream owns `states`, a device int32 array with states[j] = s_j.  A launch whose first row has j0 >= 1 reads
 * states[j0 - 1] - the caller guarantees it is valid - and writes states[j0 .. j0 + rows); for j0 <= 0 it starts from `start`
 * and writes only indices >= 0.  It never reads an index it writes, so the result is a pure function of its inputs, and no
 * launch walks more than rows + 1 transitions.
 * Why the loops keep states[j0 - 1] valid: an iteration's verify pass covers rows j0 .. j0 + gamma and writes
 * states[j0 .. j0 + gamma] along the drafted tokens.  After n accepted tokens plus the resampled or bonus token the next first
 * row is j0' = j0 + n + 1 <= j0 + gamma + 1.  states[j0' - 1] was written along accepted tokens only, and those did not
 * change.  states[j0'] is re-derived from the new token seq[P + j0' - 1], which overwrites the stale value the rejected draft
 * left.  Each draft step (one row) derives its state from the previous step's state the same way, and the verify rewrites the
 * same values.  An autoregressive step is the one-row case.  A queue slot that changes hands starts again at j0 = 0. */
typedef struct {
    const uint32_t *masks;
    const int32_t *next;
    const int32_t *cls;
    int32_t n_states, n_classes, start;
} sd_grammar;
/* Attaches a grammar to a stream's TARGET session (sd_ar_stream.session in the autoregressive loop), as sd_session_set_kv_fp8
 * and sd_session_set_tp attach their state; g == NULL detaches.  The struct is copied; `states` (device, states_cap ints) is the
 * stream's state cache.  Refused with SD_ERR_INVALID, naming what is wrong: a null session; n_states < 1; n_classes < 1; start
 * outside [0, n_states); a NULL masks, next or states; states_cap < 1; cls == NULL with n_classes different from the model's
 * vocabulary.
 * The four loops that take sd_loop_opts look at their streams' target sessions: a pass of a draft step, of the verify or of an
 * autoregressive step that holds at least one active stream with a grammar is an edited pass, also when penalties and edits are
 * neutral.  Its one launch is sd_grammar_rows (below) into the edit block's slab; the norm request reads the slab and asks for
 * no tile maxima; everything else - joiner rows, accept / resample, candidate lists, the Philox order, sd_token_logprobs on
 * the raw rows - is untouched.  Draft and target rows get the same mask, so every loop's output is distributed as the target's
 * own sampling under the grammar.  A pass without a grammar stream is the pass it was, launch for launch.  Refused behind the
 * entry's own refusals and the members of opts, before anything is written or launched: a stream with a grammar while
 * opts->edits is NULL (the masked rows need the edit block's slab; a block of neutral records is enough); states_cap smaller
 * than the output positions the call can reach, T - P + gamma + 2 (gamma 0 in the autoregressive loop; in the queue the largest
 * T and the smallest L); a stream that arrives with more cached target rows than len - 1.  In the queue the grammar of a slot's
 * session serves every prompt that decodes in the slot, so the queue supports one grammar per call, attached to all slots, each
 * slot with its own `states`; per-prompt grammars in the queue are out of scope.  sd_lookup_generate, sd_lookup_batch_generate
 * and sd_spec_multi_generate have no edit pass and refuse a target session that carries a grammar. */
int sd_session_set_grammar(sd_session *s, const sd_grammar *g, int32_t *states, int32_t states_cap);
/* sd_edit_rows plus the grammar: the same grid, alignment freedom and `mode`, out of place, up to 16 items x 17 rows in ONE
 * launch.  Row r of an item has j = row.hist0 + r - row.prompt_len; the workgroups of a row walk its at most r + 1 transitions
 * from states[j0 - 1] (or from start) themselves, and the row's first workgroup writes states[j0 + r].  An item with a NULL
 * grammar is edited exactly as sd_edit_rows edits it (its states is not read).  Refused with SD_ERR_INVALID before any launch,
 * naming the item: what sd_edit_rows refuses, then per item the grammar refusals of sd_session_set_grammar (with V for the
 * model's vocabulary; no states_cap here: the caller sizes states for j0 + rows). */
typedef struct {
    sd_logit_edit_item row;
    const sd_grammar *grammar;
    int32_t *states;
} sd_grammar_item;
int sd_grammar_rows(const sd_grammar_item *items, int n_items, int V, int mode, void *stream);

/* ------------------------------------------------------------------------------------------
 * Prompt-lookup drafting: speculative decoding without a draft model.  The proposer finds the most recent earlier occurrence
 * of the sequence's last few tokens and proposes the tokens that followed it.  A lookup draft is a deterministic proposal, so
 * its q row is one-hot; with one-hot rows in q_hist the accept / residual kernels above need no change: accept iff
 * r <= p[j] / 1, the residual is max_fn(p - onehot_j).
 *
 * Definition, for one stream with tokens seq[0 .. L), gamma g, ngram_max N and ngram_min m (1 <= m <= N <= SD_LOOKUP_MAX_NGRAM = 8):
 *  - For a continuation index c, 1 <= c <= L - 1, the match length is k(c) = the largest k <= min(N, c) with
 *    seq[c-k .. c) == seq[L-k .. L).  The match may overlap the key itself.
 *  - c counts when k(c) >= m.  Among those, choose the largest k(c), and among equal lengths the largest c (the most recent
 *    occurrence).
 *  - If none counts, use c = L - 1 with match length 0.  This always happens at L = 1.
 *  - The drafted tokens are seq[L + i] = seq[c + (i mod (L - c))], i < g.  This is the sequential copy seq[L+i] = seq[c+i],
 *    which runs into its own output when L - c < g.
 *  - So the proposer always yields g tokens and the loops keep fixed shapes.  A hopeless proposal costs nothing in correctness.
 *  - Per stream it writes the g tokens.  It also writes g one-hot rows: q_hist[(L-1+i)*ld + v] for every v < V becomes 0.0f, or
 *    1.0f at v = seq[L+i].  Columns [V, ld) are untouched, and whatever the rows held before, NaN included, is gone.  It also
 *    writes two device ints, info[0] = match length and info[1] = c.
 *  - The result is a pure function of the inputs.  The kernel reads seq[0..L) and writes seq[L..L+g).
 * A token outside [0, V) is copied like any other and its row is all zero (it is never used as an index).
 *
 * sd_lookup_propose: one launch serves 1..16 items; `items` is a host array; no alignment is asked of ld or the rows; the token
 * buffer holds L + gamma ints and q_hist L + gamma - 1 rows.  Refused with SD_ERR_INVALID before any launch, naming the item:
 * a NULL argument; n_items outside 1..16; gamma outside 1..16; ngram_max outside 1..8; ngram_min outside 1..ngram_max;
 * V < 1 or ld < V; then per item a NULL pointer or L < 1. */
#define SD_LOOKUP_MAX_NGRAM 8
typedef struct { int32_t *seq; int32_t L; float *q_hist; int32_t *info; } sd_lookup_item;
int sd_lookup_propose(const sd_lookup_item *items, int n_items, int V, long ld, int gamma, int ngram_max, int ngram_min,
                      void *stream);
/* sd_spec_generate with the gamma draft forwards replaced by ONE sd_lookup_propose launch; the rest of the iteration is
 * sd_spec_generate's, launch for launch: one target forward over the uncached rows (the whole prompt on the first iteration),
 * the norm launch of the last gamma + 1 rows (candidate lists when the workspace holds them, tile maxima where the head
 * leaves them), sd_accept_resample - or the dense pair for a list-less row - one async copy and one wait.  The blocks are
 * sd_spec_generate's: dev->draft must be NULL; scratch->draft is not read; seq->draft_len is neither read nor written;
 * seq->draft_ms_out[i] receives the proposer's time when set; q_at is 1 for every drafted token.  dev->res_dev and
 * dev->res_host hold sizeof(sd_accept_result) + 8 bytes: the proposer's two info ints follow the result block, and the one
 * copy moves both.  match_len_out (host, one entry per iteration, may be NULL) receives info[0].  The residual runs in the
 * target's norm mode (a one-hot row is exact in every dtype).  Philox position per iteration, d = seq->draw on entry of the
 * iteration: d .. d+gamma reserved and unread (no draft samples, no discarded target sample), d+gamma+1 .. d+2*gamma the accept
 * uniforms, d+2*gamma+1 the residual / bonus sample; the stream advances by 2*gamma + 2.  There is no random_seed / r_const.
 * Refused with SD_ERR_INVALID before anything is written or launched, in this order: a NULL block, a NULL pointer in dev
 * (target, seq, q_hist, p_hist, err_words, res_dev, res_host), seq->host_seq or scratch->target.logits; a non-NULL dev->draft;
 * gamma outside 1..16; ngram_max outside 1..8; ngram_min outside 1..ngram_max; temperature 0; a norm_workspace with
 * max_rows_per_forward < gamma + 1; then sampling->V differing from the target's vocabulary or ld < V. */
int sd_lookup_generate(const sd_spec_stream *dev, int gamma, int ngram_max, int ngram_min, const sd_sampling *sampling,
                       const sd_spec_scratch *scratch, sd_seq_state *seq, int32_t *match_len_out, void *stream);
/* Up to 16 streams in lock-step, each running exactly the algorithm of sd_lookup_generate on its own Philox stream (seed,
 * draw).  Per iteration: ONE sd_lookup_propose launch over the active streams; the verify passes of max_rows_per_forward /
 * (gamma + 1) streams each (sd_batch_forward); the norm launch (sd_norm_batch) with lists when the workspace holds them and
 * one pass holds every stream; sd_accept_resample_batch, or sd_accept_batch without lists; one copy and one wait.  Streams
 * arrive prefilled to target_len == len - 1 with draft == NULL; draft_len is not used.  The streams' result blocks are
 * consecutive as in sd_spec_batch_generate, and 2 * n_streams info ints follow the last block, on the device and on the host:
 * stream i's pair at ints 2i, 2i + 1 behind res[n_streams], moved by the same one copy.  match_len_out (host, may be NULL):
 * n_streams pointers, entry i one int per iteration of stream i (indexed like acc_len_out), or NULL.  A done stream drops out
 * of later passes; the end-of-stream rule (T tokens or a new EOS) and log are sd_spec_batch_generate's.  Refused before
 * anything is written or launched: NULL blocks, n_streams or gamma outside 1..16, n-gram bounds as above, temperature 0; then
 * per stream a NULL pointer, a non-NULL draft, sessions of another model than stream 0's, target_len != len - 1; then result
 * blocks that are not consecutive. */
int sd_lookup_batch_generate(sd_batch_stream *streams, int n_streams, int gamma, int ngram_max, int ngram_min,
                             const sd_sampling *sampling, const sd_spec_scratch *scratch, sd_lockstep_log *log,
                             int32_t **match_len_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Tensor parallelism of one decoder over the GPUs of a node (BASELINE config 5: Llama-2-70b, TP = 8 over xGMI).
 * The reference is single-process: this is new capability behind the same call signatures.
 * A shard is an ordinary sd_model whose config holds the LOCAL head / KV-head / MLP counts (n_heads * head_dim <= hidden)
 * and whose matrices are the Megatron slices: wqkv / w_gate_up by output rows, wo / w_down by input columns.  A session
 * bound to a group all-reduces the fp32 partial outputs of wo and w_down (two per layer) before the residual add.
 * Every rank runs the same decode loop on the same tokens; draft model and sampling are replicated.
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_tp sd_tp;
/* RCCL group: rank 0 obtains a 128-byte id and the host broadcasts it (torch.distributed / any side channel); every
 * rank then joins.  RCCL is resolved with dlopen on first use (the copy the process already holds, if any). */
int sd_tp_unique_id(void *id128);
int sd_tp_create_rccl(int rank, int world, const void *id128, sd_tp **out);
/* Loopback group: `world` ranks inside ONE process on one GPU (each driven by its own host thread and stream; the
 * all-reduce is an event-ordered rendezvous + a sum kernel).  For testing the sharded forward on a one-GPU box. */
int sd_tp_create_loopback(int world, sd_tp **out /* world handles */);
int sd_tp_destroy(sd_tp *t);
int sd_session_set_tp(sd_session *s, sd_tp *t);

/* ------------------------------------------------------------------------------------------
 * Throughput-mode gather: prompt streams are sharded over the ranks (stream s on rank s mod
 * world) and never talk inside the decode loop; at the end every rank contributes its packed token rows
 * [rows][width] int32 (-1 padded) and receives all ranks' rows, [world][rows][width], through ONE ncclAllGather over
 * RCCL / xGMI (KB-scale: latency-bound).  The reference has no counterpart (single process, evaluation.py:524-532 reads
 * the output of its one stream); `sd_comm_unique_id` is ncclGetUniqueId, whose 128 bytes the host hands to every rank
 * (torch.distributed's store / broadcast, or any side channel).  send / recv are device buffers of this rank's GPU.
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_comm sd_comm;
int sd_comm_probe(void);    /* SD_OK when RCCL resolves in this process (dlopen + the five entry points); creates nothing */
int sd_comm_unique_id(void *id128);
int sd_comm_init(int rank, int world, const void *id128, sd_comm **out);
int sd_comm_all_gather_tokens(sd_comm *c, const int32_t *send, int32_t *recv, int rows, int width, void *stream);
int sd_comm_rank(const sd_comm *c, int *rank_out, int *world_out);
int sd_comm_destroy(sd_comm *c);

/* Per-op-class timing for the roofline report: when enabled, every launch inside
 * sd_session_forward is bracketed with HIP events on the launch stream; sd_profile_read
 * synchronises the stream, returns accumulated milliseconds and launch counts per class, and
 * resets them.  Classes: 0 gemm, 1 attention, 2 norm/residual epilogues, 3 qkv-rope-append,
 * 4 activation, 5 embed, 6 logits epilogue. */
#define SD_N_PROFILE_CLASSES 8
int sd_profile_enable(sd_session *s, int on);
int sd_profile_read(sd_session *s, float *ms_out, int *count_out);

#ifdef __cplusplus
}
#endif
#endif /* SPECDEC_H */
