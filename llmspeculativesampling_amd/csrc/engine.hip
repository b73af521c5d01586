// Host side of the decoder engine: model / session handles and the per-forward launch chain.
// Replaces (for one sequence) reference sampling/kvcache_model.py:141-252 -> model forward
// (modeling_llama.py:624-768 / modeling_opt.py:561-759) with a fixed chain of HIP launches over
// a preallocated KV arena; rollback (kvcache_model.py:359-436) is the caller passing a smaller pos0.
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>

#include <chrono>
#include <vector>

#include "model_kernels.h"
#include "small_kernels.h"
#include "rows_kernels.h"
#include "mm_kernels.h"
#include "prefill_attn.h"
#include "fused_kernels.h"
#include "normload_kernels.h"
#include "multi_kernels.h"
#include "kv_copy_kernels.h"
#include "logprob_kernels.h"
#include "score_kernels.h"
#include "penalty_kernels.h"
#include "logit_edit_kernels.h"
#include "grammar_kernels.h"
#include "lookup_kernels.h"
#include "sampler_host.h"

static thread_local char g_err[512] = "";
void sd_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *sd_last_error(void) { return g_err; }
extern "C" int sd_version(void) { return SD_ABI_VERSION; }

struct sd_model {
    sd_model_config cfg;
    sd_model_weights w;
    std::vector<const void *> wqkv, bqkv, wo, bo, wgu, bfc1, wdown, bfc2, n1w, n1b, n2w, n2b;
    std::vector<W12Arg> w12[3];   // [SD_W12_*][layer]: 12-bit records of that matrix (sd_model_set_w12; codes == NULL: none)
};

enum { PC_GEMM = 0, PC_ATTN, PC_NORM, PC_QKV, PC_ACT, PC_EMBED, PC_LOGITS, PC_OTHER };

struct sd_session {
    sd_model *m;
    int max_seq, max_rows;
    int max_pass_rows;  // rows of a call whose rows are all logit rows (sd_model_max_pass_rows, <= max_rows)
    char *kv;        // [L][2][Hkv][max_seq][D]
    char *scratch;
    // carved scratch
    void *x, *h, *qbuf, *attn, *act, *ebuf;
    void *x2;           // second residual-stream buffer of the small-model path (the prologue-fused chain ping-pongs)
    float *spart;       // split-K slabs of the small-model path's O / down GEMMs (its head writes s->part meanwhile)
    void *h2;           // second normalised-operand buffer (small-model path)
    unsigned *ao_ctr;      // arrival counter of the fused attention + O projection launches (monotonic, fused_kernels.h)
    unsigned ao_epoch;     // arrivals expected so far (wraps; compared as a signed difference)
    unsigned *wait_status; // sticky device word: bit 0 a fused attention + O wait timed out, bit 1 a k-split finisher's wait did
    long long *ao_stamps;  // [AO_STAMP_WGS][8] per-workgroup records of the last stamped fused launch (SD_AO_STAMPS=1)
    int resync;            // the next forward re-zeroes the arrival counters and epochs first (set after a failed forward)
    int test_skew, skew_now;   // test hook (sd_session_test_skew_wait): arrivals the NEXT forward's fused waits over-expect
    unsigned *fin_ctr;     // [hidden / 16] arrival counters of the k-split GEMM with residual epilogue (monotonic, normload_kernels.h)
    unsigned fin_epoch;    // arrivals per tile expected so far (wraps; compared as a signed difference)
    float *ssq;            // [16][hidden / 16] per-tile sums of squares left by a residual epilogue (normload_kernels.h)
    size_t spart_floats;
    float *tile_max;    // [SD_MAX_ROWS][vocab / 16] maxima of the head's 16-column tiles (EPI_HEAD)
    int kv_fp8;         // the arena holds fp8 e4m3 (sd_session_set_kv_fp8)
    int prefill_attn_launches;   // attn_prefill_kernel + attn_prefill_blocked_kernel launches so far (sd_session_prefill_attn_launches: the route, for tests)
    int prefill_attn_blocked_launches;   // ... of which attn_prefill_blocked_kernel
    int w12_launches;            // GEMM launches that streamed 12-bit weight records so far (sd_session_w12_launches)
    const float *kv_scale;   // device [L][2][Hkv]
    struct sd_tp *tp;   // tensor-parallel group of this shard (NULL: the model is whole)
    sd_grammar gram;        // the grammar of the stream this session is the target of (sd_session_set_grammar; masks NULL: none)
    int32_t *gram_states;   // ... and the stream's state cache, gram_cap device ints
    int gram_cap;
    float *tp_in, *tp_out;   // [max_rows][hidden] fp32: this rank's partial O / down output, and the all-reduced sum
    float *attn_part;   // [groups*splits <= 64][Hq][TQ][D+2] partial attention sums of the split-key path
    float *part;
    size_t part_floats;
    // profiling
    int prof_on;
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_class;
    size_t ev_used;
    float prof_ms[SD_N_PROFILE_CLASSES];
    int prof_cnt[SD_N_PROFILE_CLASSES];
    hipStream_t prof_stream;
};

static inline size_t esize(int dtype) { return dtype == SD_F32 ? 4 : 2; }
static inline bool is16(int dtype) { return dtype != SD_F32; }
// rounding code of a 16-bit head's fp32 accumulators (SD_NORM_ROUND_*)
static inline int round_code(int dtype) { return dtype == SD_BF16 ? SD_NORM_ROUND_BF16 : (dtype == SD_F16 ? SD_NORM_ROUND_F16 : 0); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static void copy_ptrs(std::vector<const void *> &dst, const void *const *src, int n) {
    dst.assign(n, nullptr);
    if (src)
        for (int i = 0; i < n; ++i) dst[i] = src[i];
}

extern "C" int sd_model_create(const sd_model_config *cfg, const sd_model_weights *w, sd_model **out) {
    SD_REQUIRE(cfg && w && out, "sd_model_create: null argument");
    SD_REQUIRE(cfg->arch == SD_ARCH_LLAMA || cfg->arch == SD_ARCH_OPT, "sd_model_create: unknown arch %d", cfg->arch);
    SD_REQUIRE(cfg->dtype == SD_F32 || cfg->dtype == SD_BF16 || cfg->dtype == SD_F16, "sd_model_create: unknown dtype %d", cfg->dtype);
    SD_REQUIRE(cfg->head_dim == 16 || cfg->head_dim == 32 || cfg->head_dim == 64 || cfg->head_dim == 128,
               "sd_model_create: head_dim %d not in {16,32,64,128}", cfg->head_dim);
    // a tensor-parallel shard holds n_heads / world query heads: its attention width is a fraction of hidden
    SD_REQUIRE(cfg->n_heads * cfg->head_dim <= cfg->hidden && (cfg->n_heads * cfg->head_dim) % 32 == 0,
               "sd_model_create: n_heads*head_dim must be <= hidden and a multiple of 32");
    SD_REQUIRE(cfg->hidden % 4 == 0 && cfg->hidden <= 8192, "sd_model_create: hidden must be a multiple of 4 and <= 8192");
    SD_REQUIRE(cfg->n_kv_heads > 0 && cfg->n_heads % cfg->n_kv_heads == 0, "sd_model_create: bad n_kv_heads");
    if (is16(cfg->dtype)) {
        SD_REQUIRE(cfg->hidden % 32 == 0 && cfg->inter % 32 == 0 && cfg->vocab % 16 == 0 && cfg->opt_proj_dim % 32 == 0,
                   "sd_model_create: the 16-bit paths need hidden/inter/proj %% 32 == 0 and vocab %% 16 == 0");
    }
    SD_REQUIRE(w->embed && w->lm_head && w->wqkv && w->wo && w->w_gate_up && w->w_down && w->norm1_w && w->norm2_w,
               "sd_model_create: missing weight pointers");
    sd_model *m = new sd_model();
    m->cfg = *cfg;
    m->w = *w;
    const int L = cfg->n_layers;
    copy_ptrs(m->wqkv, w->wqkv, L); copy_ptrs(m->bqkv, w->bqkv, L);
    copy_ptrs(m->wo, w->wo, L); copy_ptrs(m->bo, w->bo, L);
    copy_ptrs(m->wgu, w->w_gate_up, L); copy_ptrs(m->bfc1, w->b_fc1, L);
    copy_ptrs(m->wdown, w->w_down, L); copy_ptrs(m->bfc2, w->b_fc2, L);
    copy_ptrs(m->n1w, w->norm1_w, L); copy_ptrs(m->n1b, w->norm1_b, L);
    copy_ptrs(m->n2w, w->norm2_w, L); copy_ptrs(m->n2b, w->norm2_b, L);
    for (auto &v : m->w12) v.assign(L, W12Arg{nullptr, nullptr});
    *out = m;
    return SD_OK;
}

extern "C" int sd_model_destroy(sd_model *m) {
    delete m;
    return SD_OK;
}

extern "C" int sd_pack_weight_bf16(const void *src, void *dst, int N, int K, void *stream) {
    SD_REQUIRE(src && dst && N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0,
               "sd_pack_weight_bf16: need N %% 16 == 0 and K %% 32 == 0 (got %d x %d)", N, K);
    const size_t total = (size_t)N * K / 8;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(pack_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)src,
                       (uint16_t *)dst, N, K);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

// ---- 12-bit weight records (w12.h)
extern "C" int sd_w12_bytes(int N, int K, size_t *codes_bytes, size_t *meta_bytes) {
    SD_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0, "sd_w12_bytes: need N %% 16 == 0 and K %% 32 == 0 (got %d x %d)", N, K);
    const size_t tiles = (size_t)(N / 16) * (K / 32);
    if (codes_bytes) *codes_bytes = tiles * W12_TILE_DWORDS * sizeof(unsigned);
    if (meta_bytes) *meta_bytes = tiles * sizeof(u32x4);
    return SD_OK;
}
// (sd_pack_weight_w12 / sd_unpack_weight_w12: at the end of the file, with the other kernels that read the records)
extern "C" int sd_model_set_w12(sd_model *m, int which, int layer, const void *codes, const void *meta) {
    SD_REQUIRE(m && which >= 0 && which < 3 && layer >= 0 && layer < m->cfg.n_layers, "sd_model_set_w12: bad matrix %d of layer %d", which, layer);
    SD_REQUIRE(m->cfg.dtype == SD_BF16, "sd_model_set_w12: the 12-bit records hold bf16 weights");
    SD_REQUIRE((codes != nullptr) == (meta != nullptr), "sd_model_set_w12: codes and meta come together");
    SD_REQUIRE(((uintptr_t)codes & 127) == 0 && ((uintptr_t)meta & 15) == 0, "sd_model_set_w12: codes must be 128-byte, meta 16-byte aligned");
    m->w12[which][layer] = W12Arg{(const unsigned *)codes, (const u32x4 *)meta};
    return SD_OK;
}

// ---- split-K policy.  A workgroup (4 waves) owns one n-tile x one k-slab and folds its waves in LDS, so
// SB slabs reach HBM.  SB is chosen so that about `target` workgroups exist (>= 4 per CU), with at least
// 8 k-steps (8 KiB of weights) per workgroup.
// Environment tunables, sampled when a session (or a spec handle) is created and by the public one-off GEMM entries - not
// per launch: a draft step is ~40 getenv() scans otherwise, on the host thread that has to keep the GPU fed.
#define SD_STREAM_MAX_ROWS 64                        // rows the streaming kernel's m-tile variants cover
#define SD_ROWS_MAX 144                              // rows the balanced one-workgroup-per-CU kernel covers (9 m-tiles: a 128-token prompt + gamma rows)
struct EnvTun {
    int gemm_ntw = 4, gemm_units = -1, small_path = 1, fuse_embed_qkv = 1;
    int attn_split_keys = 384, attn_keys_per_split = 256;
    int mm_mtw = 0, mm_s = 0, prefill_attn = 1, prefill_attn_block = 0, mm_slabs_min = 24;
    int gemm_rows = 1, cus = 0, fuse_attn_o = 1, ao_stamps = 0, norm_on_load = 2, rows_max = SD_ROWS_MAX;
};
static EnvTun g_env;
static void refresh_env() {
    auto geti = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
    g_env.gemm_ntw = geti("SD_GEMM_NTW", 4);
    g_env.gemm_units = geti("SD_GEMM_UNITS", -1);
    // 1 (default since round 4): a small model's <= 4-row step runs the layers' two norm launches as prologues of QKV / gate-up
    // (llama-68m 94.9 -> 92.3 us, opt-125m 426-440 -> 417 us per draft step); 2: every seam a prologue incl. the head (slower);
    // 0: the per-op chain.  Rounds 2-4 measured the prologue route 75 % slower: that was a 254-VGPR compile of gemm_small
    g_env.small_path = geti("SD_SMALL_PATH", 1);
    g_env.fuse_embed_qkv = geti("SD_FUSE_EMBED_QKV", 1);
    g_env.attn_split_keys = geti("SD_ATTN_SPLIT_KEYS", 384);          // keys per workgroup above which a group's keys are split
    g_env.attn_keys_per_split = std::max(16, geti("SD_ATTN_KEYS_PER_SPLIT", 256));
    g_env.ao_stamps = geti("SD_AO_STAMPS", 0);
    g_env.fuse_attn_o = geti("SD_FUSE_ATTN_O", 1);    // 0: attention and the O projection as two launches (A/B runs, bit-compare tests)
    g_env.norm_on_load = geti("SD_NORM_ON_LOAD", 2);  // 0: residual+norm launches stay; 1: attention -> MLP seam only; 2: both seams (A/B runs, compare tests)
    g_env.prefill_attn = geti("SD_PREFILL_ATTN", 1);  // 0: prefill passes keep attn_kernel's 8-row groups (A/B runs, compare tests)
    g_env.prefill_attn_block = std::max(0, geti("SD_PREFILL_ATTN_BLOCK", 0));   // K > 0: every matrix-core prefill pass takes attn_prefill_blocked_kernel with blocks of K keys (rounded up to 64; tests, sweeps); 0: only past the single tile's LDS limit
    g_env.mm_slabs_min = geti("SD_MM_SLABS_MIN", 24); // rows from which the k-slab GEMMs (O / down) of a pass take gemm_bf16_mm instead of the balanced kernel
    g_env.mm_mtw = geti("SD_MM_MTW", 0);              // (sweeps) m-tiles per wave of gemm_bf16_mm: 2 = 128-row blocks, 4 = 256-row blocks; 0 = by row count
    g_env.mm_s = geti("SD_MM_S", 0);                  // (sweeps) k-slabs of gemm_bf16_mm; 0 = planned

    g_env.gemm_rows = geti("SD_GEMM_ROWS", 1);        // 0: 17..64-row GEMMs stay on the streaming kernel (A/B runs, bit-compare tests)
    g_env.rows_max = std::min(SD_ROWS_MAX, std::max(SD_STREAM_MAX_ROWS, geti("SD_GEMM_ROWS_MAX", SD_ROWS_MAX)));   // 65..this many rows take the balanced kernel, more gemm_bf16_mm
    if (!g_env.cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
            g_env.cus = n;
        else
            (void)hipGetLastError();                  // no device (CPU container): plans are made for the MI355X's 256 CUs
    }
}

static int gemm_ntw(int N, int M) {
    if (M <= 16) return 1;
    const int ntl = N / 16;
    // n-tiles per wave: more of them amortise the activation fragment loads, fewer give more workgroups.  Stream-batched
    // decode, 4 / 6 / 8 / 10 streams x 5 rows (bench.py --batch-streams): 529 / 727 / 861 / 990 tok/s with 4 tiles,
    // 504 / 753 / 808 / 908 with 2; 8 tiles: register pressure, slower everywhere.
    const int want = g_env.gemm_ntw;
    if (want >= 8 && ntl % 8 == 0) return 8;
    if (want >= 4 && ntl % 4 == 0) return 4;
    if (want >= 2 && ntl % 2 == 0) return 2;
    return 1;
}

// The gemm_bf16_stream instance a GEMM of M rows runs on - what dispatch_gemm_bf16 / launch_gemm_bf16 launch and what
// sd_gemm_route reports: MT m-tiles, NTW n-tiles per wave, UNROLL k-steps requested together.  MT == 0: no instance.
struct StreamInst { int MT, NTW, UNROLL; };
constexpr int stream_unroll(int MT, int NTW) { return NTW >= 8 ? 1 : (MT > 2 ? 2 : 4); }   // 4 measured best for decode rows (tools/gemm_bench.py)
// a wave's whole k-range in ONE burst when it is 5..8 k-steps (the draft model's K = 768 GEMMs: 6 per wave), instead of a
// group of four and a second round trip for the rest: the <1, 8> instance, one m-tile and one n-tile per wave only
static bool stream_burst8(int MT, int NTW, int K, int ks_per) {
    const int per_wave = (std::min(ks_per, K / 32) + 3) / 4;
    return MT == 1 && NTW == 1 && per_wave > 4 && per_wave <= 8;
}
static StreamInst stream_instance(int N, int K, int M, int Mpad, int ks_per) {
    const int MT = Mpad / 16;
    if (MT < 1 || MT > 4) return StreamInst{0, 0, 0};
    // rows beyond one m-tile (prefill, stream-batched verify): every activation fragment a wave loads is reused for
    // NTW weight tiles, because activations and weights share the CU's load path (X:W bytes = 16*MT : 16*NTW)
    int ntw = MT == 1 ? 1 : gemm_ntw(N, M);
    if (MT == 2 && ntw > 4) ntw = 4;                              // (no 8-tile instance at 2 m-tiles)
    return StreamInst{MT, ntw, stream_burst8(MT, ntw, K, ks_per) ? 8 : stream_unroll(MT, ntw)};
}

#define TINY_SPLIT_BYTES 24576                       // weights a workgroup streams in a <= 16-row GEMM on a matrix of <= 8 MB
static void gemm_split(int N, int K, int M, int *S_out, int *ks_per_out) {
    const int NTL = N / 16 / gemm_ntw(N, M), KS = K / 32;
    int max_s = KS / 8;
    if (max_s < 1) max_s = 1;
    int S = 1;
    if (g_env.gemm_units >= 0) {
        S = (g_env.gemm_units + NTL / 2) / NTL;
    } else if (M > 16) {
        // many rows: every extra slab costs a write + a read of Mpad*N floats, which at 64 rows rivals the weight bytes
        // (256*S/K of them), so take the S that minimises (weights + slab traffic) / CU-fill efficiency
        const double wbytes = (double)N * K * 2.0, slab = 2.0 * (double)align_up(M, 16) * N * 4.0;
        double best = 1e300;
        for (int c = 1; c <= max_s && c <= 16; ++c) {
            const int blocks = NTL * c;
            if (blocks < 256 && c < max_s && c < 16) continue;
            const double eff = (double)blocks / (double)(((blocks + 255) / 256) * 256);
            const double cost = (wbytes + slab * c) / eff * (blocks < 768 ? 1.25 : 1.0);   // too few workgroups under-fill the load path
            if (cost < best) { best = cost; S = c; }
        }
    } else if ((size_t)N * K * 2 <= ((size_t)8 << 20)) {
        // a matrix of a small model (the draft's O / down projection: 1.2 / 4.7 MB): its launch is latency, not bytes, and
        // every slab is another 16-byte load per column group in the consumer's fold - so few slabs, each workgroup streaming
        // about TINY_SPLIT_BYTES (24 KiB: down 12 -> 4 slabs, O 3 -> 1; on one box llama-68m / opt-125m steps of 91.5 / 415.4 us
        // with the big-matrix policy, 87.3 / 387.6 at 24 KiB, 89.4 / 397.0 at 32, 90.2 / 402.5 at 48, 93.7 / 420.7 at 96 -
        // profiles/r04_draft_step_ab.txt)
        S = (int)((K * 32 + TINY_SPLIT_BYTES / 2) / TINY_SPLIT_BYTES);
    } else if (NTL < 1024) {
        // fewest slabs that give >= 1024 workgroups, preferring a workgroup count that fills all 256 CUs evenly
        // (measured on MI355X: 7.5 workgroups per CU runs 10 % slower than 15 per CU, tools/gemm_bench.py)
        double best = -1.0;
        for (int c = 1; c <= max_s && c <= 16; ++c) {
            const int blocks = NTL * c;
            if (blocks < 1024 && c < max_s && c < 16) continue;
            const double eff = (double)blocks / (double)(((blocks + 255) / 256) * 256);
            if (eff > best + 1e-9) { best = eff; S = c; }
            if (blocks >= 4096) break;
        }
    }
    if (S < 1) S = 1;
    if (S > max_s) S = max_s;
    int ks_per = (KS + S - 1) / S;
    S = (KS + ks_per - 1) / ks_per;
    *S_out = S;
    *ks_per_out = ks_per;
}

// Which kernel a bf16 GEMM over M rows takes and how its k-range is cut - route_gemm is the one place that chooses.  In
// order of preference:
//   * gemm_bf16_stream_w16 (sixteen waves per n-tile): a QKV projection of <= 16 rows with few n-tiles and a long k-range
//     (a tensor-parallel shard's QKV: 80 tiles x K = 8192);
//   * gemm_bf16_mm (mm_kernels.h, 128- or 256-row blocks): the k-slab GEMMs (O / down) of a 24..144-row pass, and every
//     GEMM past 64 rows that the balanced kernel does not take (prefill passes past SD_ROWS_MAX rows).  A k-slab GEMM of a
//     24..144-row pass is faster on it with 128-row blocks and 6 slabs than on the balanced kernel - 12.7 / 28.1 us against
//     15.3 / 29.6 at 40 rows (8 streams x 5), 13.6 / 28.3 against 16.7 / 31.6 at 60, 14.7 / 30.2 against 18.0 / 36.3 at 80,
//     18.1 / 36.2 against 19.7 / 42.5 at 132; equal at 24 - tools/mm_bench.py.  QKV and gate/up with their fused epilogues
//     stay on the balanced kernel: 36.9 / 56.1 us against 52.0 / 60.5 at 80 rows, 44.9 / 70.1 against 50.1 / 74.7 at 132;
//   * gemm_bf16_rows (rows_kernels.h, one workgroup per CU): 17..SD_ROWS_MAX rows when both of its plans for the shape
//     are good;
//   * gemm_bf16_stream: <= 64 rows, always (and the only kernel that gathers or reads row-major activations).
// A route of kind GK_NONE has no kernel: the row limits (sd_model_max_rows, sd_model_max_pass_rows) keep such calls out.
#define SD_MAX_FWD_ROWS 256
struct RowsPlan { bool ok; int S, ksp, NG, grid, nwn, nwk, nld; };
static RowsPlan rows_plan(int N, int K, int M, bool fused);
enum GemmKind { GK_NONE = 0, GK_STREAM, GK_STREAM_W16, GK_ROWS, GK_MM };
enum GemmNeed {
    GN_GATHER = 1,     // X rows are gathered through the row table's xmap (the lm_head of some rows of a pass)
    GN_ROWMAJOR = 2,   // X is plain row-major (the public sd_gemm_bf16)
    GN_FUSED = 4,      // the QKV / activation epilogue runs in the launch: every workgroup keeps its whole k-range (X tiled)
    GN_QKV = 8,        // ... and it is the QKV epilogue
    GN_ONE_SLAB = 16,  // one k-slab where the shape allows it (a tensor-parallel shard's O / down projection: its [M][N]
                       // partial then goes to the all-reduce as it is, without a fold launch in between)
};
struct GemmRoute { int kind, S, ksp, mtw; RowsPlan rp; };
static GemmRoute route_gemm(int N, int K, int M, int need) {
    GemmRoute r = {};
    const bool fused = need & GN_FUSED, x_tiled = !(need & (GN_GATHER | GN_ROWMAJOR));
    const int KS = K / 32, Mpad = (int)align_up(M, 16);
    if ((need & GN_QKV) && M <= 16 && x_tiled && N / 16 <= 128 && KS >= 128) {
        r.kind = GK_STREAM_W16;
        r.S = 1;
        r.ksp = KS;
        return r;
    }
    const bool mm_slabs = !fused && M >= g_env.mm_slabs_min && (size_t)N * K >= ((size_t)16 << 20) && N / 16 / 8 < 64;
    const RowsPlan rp = x_tiled ? rows_plan(N, K, M, fused) : RowsPlan{};
    const bool rows_take = M > SD_STREAM_MAX_ROWS && M <= g_env.rows_max && !mm_slabs && rp.ok;
    if (x_tiled && (M > SD_STREAM_MAX_ROWS || mm_slabs) && !rows_take && (N / 16) % 8 == 0 && KS % 2 == 0 && KS >= 16) {
        // 256-row blocks (mtw 4) or 128-row blocks (mtw 2) x 128 columns.  Fused: the block shape that fills the CUs better
        // (13b at 256 rows: gate/up 216 blocks of 256 rows, QKV 240 blocks of 128).  Otherwise 256-row blocks past 128
        // rows and k-slabs for about one block per CU (tools/mm_bench.py: O / down 6 slabs, QKV 2).
        const int G = g_env.cus > 0 ? g_env.cus : 256, NB = N / 16 / 8;
        auto blocks_of = [&](int mtw) { const int BMT = 4 * mtw; return ((Mpad / 16 + BMT - 1) / BMT) * NB; };
        auto fill = [&](int blocks) { return (double)blocks / (double)(((blocks + G - 1) / G) * G); };
        r.kind = GK_MM;
        r.mtw = Mpad <= 128 ? 2 : 4;
        if (fused && Mpad > 128 && fill(blocks_of(2)) > fill(blocks_of(4)) + 0.05) r.mtw = 2;
        if (g_env.mm_mtw) r.mtw = g_env.mm_mtw;
        const int blocks = blocks_of(r.mtw);
        int S = fused ? 1 : (g_env.mm_s ? g_env.mm_s : std::max(1, (G - G / 16 + blocks / 2) / blocks));
        S = std::min(std::min(S, 8), std::max(1, KS / 8));     // (every slab is a write + a read of Mpad x N floats)
        r.ksp = (int)align_up((KS + S - 1) / S, 2);
        r.S = (KS + r.ksp - 1) / r.ksp;
        return r;
    }
    if (rp.ok) {
        r.kind = GK_ROWS;
        r.rp = rp;
        r.S = rp.S;
        r.ksp = rp.ksp;
        return r;
    }
    if (M > SD_STREAM_MAX_ROWS) return r;
    r.kind = GK_STREAM;
    gemm_split(N, K, M, &r.S, &r.ksp);
    // (<= 16 rows of a shard: one workgroup per n-tile over the whole k-range still gives >= 256 workgroups at hidden >= 4096)
    if (fused || ((need & GN_ONE_SLAB) && M <= 16 && N / 16 >= 256)) {
        r.S = 1;
        r.ksp = KS;
    }
    return r;
}

// The gemm_bf16_mm instance of a route's mtw (launch_gemm_mm launches it, sd_gemm_route reports it): 128-row blocks
// (mtw 2), or 256-row blocks (any other mtw: 4), which hold every row of a pass (<= 256 rows) - their weight tiles are read
// once chip-wide -> non-temporal.  lds: NBUF = 3 stages x KT = 2 k-tiles x (8 W + BMT X) KiB.
struct MmInst { int mtw, nt; size_t lds; };
static MmInst mm_instance(int mtw) {
    const int m = mtw == 2 ? 2 : 4;
    return MmInst{m, m == 4, (size_t)3 * (8 + 4 * m) * 2 * 1024};
}

// gemm_bf16_mm (mm_kernels.h): EPI != EPI_PART needs r.S == 1 (the block holds the whole k-range)
template <int EPI, typename H = bf16_t>
static void launch_gemm_mm(const void *W, const void *X, float *part, int M, int Mpad, int N, int K, const GemmRoute &r,
                           const GemmEpiT<H> &e, hipStream_t st) {
    const MmInst in = mm_instance(r.mtw);
    const int BMT = 4 * in.mtw, MB = (Mpad / 16 + BMT - 1) / BMT, NB = N / 16 / 8;
    const dim3 grid(MB * NB * r.S);
    const size_t lds = in.lds;
    auto go = [&](auto kern) {
        static bool attr = false;                                 // (one flag per instantiation of this lambda = per kernel)
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
            attr = true;
        }
        hipLaunchKernelGGL(kern, grid, dim3(MM_THREADS), lds, st, (const u32x4 *)W, (const u32x4 *)X, part, M, Mpad, N, K, r.S,
                           r.ksp, e);
    };
    if (in.mtw == 2) go(gemm_bf16_mm<2, EPI, H, false>);
    else go(gemm_bf16_mm<4, EPI, H, true>);
}

// ---- 17..SD_ROWS_MAX rows: the balanced one-workgroup-per-CU kernel (rows_kernels.h).  S k-slabs x NG n-groups = one workgroup per
// CU; a fused epilogue needs S == 1.  The plan minimises (weight bytes + slab traffic) / how evenly the n-tiles divide.
static RowsPlan rows_plan(int N, int K, int M, bool fused) {
    RowsPlan p = {};
    if (!g_env.gemm_rows || M <= 16 || M > SD_ROWS_MAX || N % 16 || K % 32) return p;
    const int G = g_env.cus > 0 ? g_env.cus : 256, NT = N / 16, KS = K / 32, Mpad = (int)align_up(M, 16);
    const double wbytes = (double)N * K * 2.0, slab = 2.0 * Mpad * (double)N * 4.0;
    double best = 1e300;
    for (int S = 1; S <= (fused ? 1 : 16); S *= 2) {
        if (G % S || KS / S < 8) break;
        const int NG = G / S, tpg = (NT + NG - 1) / NG;
        if (NT < NG || tpg > GR_MAX_TILES) continue;
        const double eff = (double)NT / NG / tpg;
        const double cost = (wbytes + (fused ? 0.0 : slab * S)) / eff;
        if (cost < best) {
            best = cost;
            p.S = S; p.NG = NG;
            p.ksp = (KS + S - 1) / S;
            p.ok = eff >= 0.8;
        }
    }
    if (p.ok) {
        p.S = (KS + p.ksp - 1) / p.ksp;
        p.grid = p.NG * p.S;
        // wave grid of a workgroup: nwn compute waves per k-group (one n-tile each) x nwk k-groups + loader waves, <= 16
        p.nwn = (NT + p.NG - 1) / p.NG;
        p.nwk = std::min(4, (16 - 1) / p.nwn);
        if (Mpad > 64) p.nwk = std::min(p.nwk, 3);                 // (5 m-tiles: 2 x 4 k-groups x 4 k-steps x 5 KiB exceed the CU's LDS)
        if (Mpad > 80) p.nwk = std::min(p.nwk, 2);                 // (8 / 9 m-tiles: 2 x 2 x 4 x 8 KiB = 128 KiB, x 9 = 144 KiB, is what fits)
        p.nld = std::min(p.nwk, 16 - p.nwn * p.nwk);
    }
    return p;
}

// The gemm_bf16_rows instance of a plan at Mpad rows (launch_gemm_rows launches it, sd_gemm_route reports it): MT m-tiles,
// chunks of CH k-steps, weight bursts of WBM chunks, and the launch's dynamic LDS.  ok: one of the compiled instances.
#define GR_LDS_CAP ((size_t)158 * 1024)
struct RowsInst { int MT, CH, WBM; size_t lds; bool ok; };
static RowsInst rows_instance(int Mpad, const RowsPlan &pl) {
    // m-tiles of the kernel instance: 2..5 as they are, 6..8 all take the 8-tile instance (the loader re-reads the last
    // real tile for the missing ones, the epilogue drops rows >= M)
    const int MT = Mpad / 16 <= 5 ? Mpad / 16 : (Mpad / 16 <= 8 ? 8 : 9);
    // activation panel (2 buffers x nwk k-groups x CH k-steps x MT tiles), reused as the fold buffer (nwn tiles x nwk x
    // MT); chunks of 8 k-steps where the panel fits the CU's LDS (one workgroup per CU owns all of it), else 6 or 4 -
    // with chunks of 4 a compute wave's weight burst spans two chunks (8 KiB requested together: WBM = 2)
    int ch = 4;
    for (int c2 : {8, 6})
        if ((size_t)1024 * MT * 2 * pl.nwk * c2 <= GR_LDS_CAP) { ch = c2; break; }
    if (MT == 2) ch = 8;                                          // (2 x 4 x 8 x 2 KiB always fits)
    if (MT == 3 && ch == 4) ch = 6;                               // (2 x 4 x 6 x 3 KiB = 144 KiB: the widest 3-tile panel)
    RowsInst in = {MT, ch, ch == 4 ? 2 : 1, (size_t)1024 * MT * std::max(2 * pl.nwk * ch, pl.nwk * pl.nwn), false};
    in.ok = MT >= 2 && (MT == 2 ? ch == 8 : MT == 3 ? ch >= 6 : MT == 4 ? true : MT == 5 ? ch <= 6 : ch == 4);
    return in;
}

template <int EPI, typename H>
static int launch_gemm_rows(const void *W, const void *X, float *part, int M, int Mpad, int N, int K, const RowsPlan &pl,
                            const GemmEpiT<H> &e, hipStream_t st) {
    constexpr size_t lds_cap = GR_LDS_CAP;
    const RowsInst in = rows_instance(Mpad, pl);
    const int MT = in.MT, ch = in.CH;
    const size_t lds = in.lds;
    SD_REQUIRE(lds <= lds_cap && Mpad / 16 <= MT, "gemm_rows: %d rows, %zu bytes of LDS", M, lds);
    auto go = [&](auto mt_c, auto ch_c, auto wbm_c) {
        constexpr int MTc = decltype(mt_c)::value, CHc = decltype(ch_c)::value, WBMc = decltype(wbm_c)::value;
        static bool attr = false;                                 // (one flag per instantiation)
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_bf16_rows<MTc, EPI, H, CHc, WBMc>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_cap);
            attr = true;
        }
        hipLaunchKernelGGL((gemm_bf16_rows<MTc, EPI, H, CHc, WBMc>), dim3(pl.grid), dim3(GR_THREADS), lds, st, (const u32x4 *)W,
                           (const u32x4 *)X, part, M, Mpad, N, K, pl.NG, pl.ksp, pl.nwn, pl.nwk, pl.nld, e);
    };
    using std::integral_constant;
    using I1 = integral_constant<int, 1>;
    using I2 = integral_constant<int, 2>;
    if (!in.ok) { sd_set_error("gemm_rows: %d rows (chunk %d)", M, ch); return SD_ERR_INVALID; }
    if (MT == 2) go(integral_constant<int, 2>{}, integral_constant<int, 8>{}, I1{});
    else if (MT == 3) { if (ch == 8) go(integral_constant<int, 3>{}, integral_constant<int, 8>{}, I1{});
                        else go(integral_constant<int, 3>{}, integral_constant<int, 6>{}, I1{}); }
    else if (MT == 4) { if (ch == 8) go(integral_constant<int, 4>{}, integral_constant<int, 8>{}, I1{});
                        else if (ch == 6) go(integral_constant<int, 4>{}, integral_constant<int, 6>{}, I1{});
                        else go(integral_constant<int, 4>{}, integral_constant<int, 4>{}, I2{}); }
    else if (MT == 5) { if (ch == 6) go(integral_constant<int, 5>{}, integral_constant<int, 6>{}, I1{});       // (8 never fits at 5 m-tiles)
                        else go(integral_constant<int, 5>{}, integral_constant<int, 4>{}, I2{}); }
    else if (MT == 8) go(integral_constant<int, 8>{}, integral_constant<int, 4>{}, I2{});
    else go(integral_constant<int, 9>{}, integral_constant<int, 4>{}, I2{});
    return SD_OK;
}

// floats of the k-slabs a GEMM of an N x K weight leaves at up to `rows` rows: the largest of its routes that can run (X in
// the tile layout, or gathered for the lm_head / OPT's project_out; fused epilogues leave no slabs)
static size_t gemm_part_floats(const sd_model_config &c, int N, int K, int rows, bool gathered = false) {
    if (!is16(c.dtype)) return (size_t)rows * N;
    size_t best = 0;
    for (int m = 1; m <= rows; ++m)
        for (int need : {0, gathered ? GN_GATHER : 0}) {
            const GemmRoute r = route_gemm(N, K, m, need);
            if (r.kind != GK_NONE) best = std::max(best, (size_t)r.S * align_up(m, 16) * N);
        }
    return best;
}

static int qkv_cols(const sd_model_config &c) { return (c.n_heads + 2 * c.n_kv_heads) * c.head_dim; }
static int q_dim(const sd_model_config &c) { return c.n_heads * c.head_dim; }     // attention width (== hidden unless sharded)
static int gu_cols(const sd_model_config &c) { return c.arch == SD_ARCH_LLAMA ? 2 * c.inter : c.inter; }
static int embed_dim(const sd_model_config &c) { return c.arch == SD_ARCH_OPT ? c.opt_proj_dim : c.hidden; }

extern "C" size_t sd_session_kv_bytes(const sd_model *m, int max_seq) {
    const sd_model_config &c = m->cfg;
    return (size_t)c.n_layers * 2 * c.n_kv_heads * max_seq * c.head_dim * esize(c.dtype);
}

struct ScratchPlan {
    size_t x, x2, h, h2, aoctr, ssq, finctr, q, attn, act, e, apart, part, spart, tmax, tp_in, tp_out, total, part_floats, spart_floats;
};
static ScratchPlan plan_scratch(const sd_model_config &c, int rows) {
    ScratchPlan p;
    const size_t es = esize(c.dtype);
    const int ed = embed_dim(c);
    const int wide = std::max(c.hidden, ed);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t trows = align_up(rows, 16);                     // GEMM operands live in 16-row tiles (xoff)
    p.x = take((size_t)rows * c.hidden * es);
    p.x2 = take((size_t)SMALL_MAX_ROWS * c.hidden * es);
    p.h = take(trows * wide * es);
    p.h2 = take(trows * wide * es);
    p.aoctr = take(256 + (size_t)AO_STAMP_WGS * 8 * sizeof(long long));   // counter line, status line, stamp records
    p.finctr = take((size_t)(c.hidden / 16 + 1) * sizeof(unsigned));      // per-tile arrival counters of gemm_bf16_stream_fin
    p.ssq = take((size_t)16 * (c.hidden / 16 + 1) * sizeof(float));      // per-tile sums of squares of <= 16 rows (norm on load)
    p.q = take((size_t)rows * c.hidden * es);
    p.attn = take(trows * c.hidden * es);
    p.act = take(trows * c.inter * es);
    p.e = take(trows * ed * es);
    p.apart = take((size_t)64 * c.n_heads * 8 * (c.head_dim + 2) * sizeof(float));
    size_t pf = 0;
    pf = std::max(pf, gemm_part_floats(c, qkv_cols(c), c.hidden, rows));
    pf = std::max(pf, gemm_part_floats(c, c.hidden, q_dim(c), rows));
    pf = std::max(pf, gemm_part_floats(c, gu_cols(c), c.hidden, rows));
    pf = std::max(pf, gemm_part_floats(c, c.hidden, c.inter, rows));
    pf = std::max(pf, gemm_part_floats(c, c.vocab, ed, rows, true));
    if (ed != c.hidden) {
        pf = std::max(pf, gemm_part_floats(c, c.hidden, ed, rows));
        pf = std::max(pf, gemm_part_floats(c, ed, c.hidden, rows, true));
    }
    p.part_floats = pf;
    p.part = take(pf * sizeof(float));
    // small-model path: slabs [S][16][hidden] of its O / down GEMMs, S <= 16
    p.spart_floats = (size_t)16 * 16 * c.hidden;
    p.spart = take(p.spart_floats * sizeof(float));
    p.tmax = take((size_t)SD_MAX_ROWS * (c.vocab / 16 + 1) * sizeof(float));
    p.tp_in = take((size_t)rows * c.hidden * sizeof(float));
    p.tp_out = take((size_t)rows * c.hidden * sizeof(float));
    p.total = off;
    return p;
}

// The rows up to `cap` at which every GEMM of a pass has a route (X in the tile layout), at every smaller count too: the
// per-layer shapes (+ OPT's project_in / project_out), and with `head` the lm_head of a pass whose rows are all logit rows
static int routed_rows(const sd_model_config &c, bool head, int cap) {
    const int ed = embed_dim(c);
    std::vector<std::pair<int, int>> shapes = {{qkv_cols(c), c.hidden}, {c.hidden, q_dim(c)}, {gu_cols(c), c.hidden}, {c.hidden, c.inter}};
    if (ed != c.hidden) shapes.insert(shapes.end(), {{c.hidden, ed}, {ed, c.hidden}});
    if (head) shapes.push_back({c.vocab, ed});
    for (int m = 1; m <= cap; ++m)
        for (const auto &sh : shapes)
            if (route_gemm(sh.first, sh.second, m, 0).kind == GK_NONE) return m - 1;
    return cap;
}

// Rows one sd_session_forward call may carry: 256 when every per-layer GEMM of the model has a route at every row count
// (or the model is fp32, whose simple GEMM has no row limit), else the streaming kernel's 64.
extern "C" int sd_model_max_rows(const sd_model *m) {
    if (!m) return 0;
    refresh_env();
    if (!is16(m->cfg.dtype)) return SD_MAX_FWD_ROWS;
    return routed_rows(m->cfg, false, SD_MAX_FWD_ROWS) == SD_MAX_FWD_ROWS ? SD_MAX_FWD_ROWS : SD_STREAM_MAX_ROWS;
}

// Rows of one pass whose rows are all logit rows (a stream-batched verify): at most SD_MAX_ROWS, and only as many as the
// lm_head has a kernel for (a vocab that is not a multiple of 128 columns - OPT's 50272 - stops at the streaming kernel's 64).
extern "C" int sd_model_max_pass_rows(const sd_model *m) {
    if (!m) return 0;
    const int cap = std::min(SD_MAX_ROWS, sd_model_max_rows(m));
    return is16(m->cfg.dtype) ? routed_rows(m->cfg, true, cap) : cap;
}

extern "C" size_t sd_session_scratch_bytes(const sd_model *m, int max_rows) {
    refresh_env();
    return plan_scratch(m->cfg, std::min(max_rows, sd_model_max_rows(m))).total;
}

extern "C" int sd_session_create(sd_model *m, int max_seq, int max_rows, void *kv_arena, void *scratch,
                                 sd_session **out) {
    SD_REQUIRE(m && kv_arena && scratch && out, "sd_session_create: null argument");
    SD_REQUIRE(max_seq > 0 && max_rows > 0, "sd_session_create: bad sizes");
    if (m->cfg.arch == SD_ARCH_OPT)
        SD_REQUIRE(max_seq <= m->cfg.max_pos, "sd_session_create: OPT is limited to %d positions", m->cfg.max_pos);
    else
        SD_REQUIRE(max_seq <= m->cfg.max_pos, "sd_session_create: rope table has %d rows, max_seq %d", m->cfg.max_pos, max_seq);
    refresh_env();
    sd_session *s = new sd_session();
    s->m = m;
    s->max_seq = max_seq;
    max_rows = std::min(max_rows, sd_model_max_rows(m));
    s->max_rows = max_rows;
    s->max_pass_rows = std::min(max_rows, sd_model_max_pass_rows(m));
    s->kv = (char *)kv_arena;
    s->scratch = (char *)scratch;
    const ScratchPlan p = plan_scratch(m->cfg, max_rows);
    s->x = s->scratch + p.x;
    s->x2 = s->scratch + p.x2;
    s->spart = (float *)(s->scratch + p.spart);
    s->spart_floats = p.spart_floats;
    s->tile_max = (float *)(s->scratch + p.tmax);
    s->tp = nullptr;
    s->kv_fp8 = 0;
    s->kv_scale = nullptr;
    s->gram = sd_grammar{};
    s->gram_states = nullptr;
    s->gram_cap = 0;
    s->prefill_attn_launches = 0;
    s->w12_launches = 0;
    s->prefill_attn_blocked_launches = 0;
    s->tp_in = (float *)(s->scratch + p.tp_in);
    s->tp_out = (float *)(s->scratch + p.tp_out);
    s->h = s->scratch + p.h;
    s->h2 = s->scratch + p.h2;
    s->ao_ctr = (unsigned *)(s->scratch + p.aoctr);
    s->ao_epoch = 0;
    s->wait_status = s->ao_ctr + 32;                              // (a 128-byte line of its own)
    s->ao_stamps = (long long *)(s->ao_ctr + 64);
    s->resync = 0;
    s->test_skew = s->skew_now = 0;
    s->ssq = (float *)(s->scratch + p.ssq);
    s->fin_ctr = (unsigned *)(s->scratch + p.finctr);
    s->fin_epoch = 0;
    SD_HIP_CHECK(hipMemset(s->fin_ctr, 0, (size_t)(m->cfg.hidden / 16 + 1) * sizeof(unsigned)));
    SD_HIP_CHECK(hipMemset(s->ao_ctr, 0, 256 + (size_t)AO_STAMP_WGS * 8 * sizeof(long long)));
    s->qbuf = s->scratch + p.q;
    s->attn = s->scratch + p.attn;
    s->act = s->scratch + p.act;
    s->ebuf = s->scratch + p.e;
    s->attn_part = (float *)(s->scratch + p.apart);
    s->part = (float *)(s->scratch + p.part);
    s->part_floats = p.part_floats;
    s->prof_on = 0;
    s->ev_used = 0;
    s->prof_stream = nullptr;
    memset(s->prof_ms, 0, sizeof(s->prof_ms));
    memset(s->prof_cnt, 0, sizeof(s->prof_cnt));
    *out = s;
    return SD_OK;
}

// Switch the session's KV arena to OCP fp8 e4m3 (BASELINE config 5).  The arena then holds 1 byte per element
// (half of sd_session_kv_bytes for a 16-bit model); `scales` is a device array [n_layers][2][n_kv_heads] (x is stored as
// fp8(x * (1 / scale)), both in fp32 - model_kernels.h, to_fp8); call before the first forward.  The fused QKV epilogue is
// the one store site, so the model must be in the fused layout (every 16-bit model the Python engine builds is).
extern "C" int sd_session_set_kv_fp8(sd_session *s, const float *scales) {
    SD_REQUIRE(s && scales, "sd_session_set_kv_fp8: null argument");
    SD_REQUIRE(is16(s->m->cfg.dtype) && s->m->cfg.head_dim >= 32, "sd_session_set_kv_fp8: needs a 16-bit model with head_dim >= 32");
    SD_REQUIRE(s->m->cfg.fused_layout != 0, "sd_session_set_kv_fp8: needs the fused weight layout (cfg.fused_layout)");
    s->kv_fp8 = 1;
    s->kv_scale = scales;
    return SD_OK;
}

// What every entry refuses in a grammar (`what` names where it sits: "grammar", "item 3: grammar"); V: the vocabulary.
static int check_grammar(const char *who, const char *what, const sd_grammar &g, const int32_t *states, int V) {
    SD_REQUIRE(g.n_states >= 1, "%s: %s: n_states %d < 1", who, what, g.n_states);
    SD_REQUIRE(g.n_classes >= 1, "%s: %s: n_classes %d < 1", who, what, g.n_classes);
    SD_REQUIRE(g.start >= 0 && g.start < g.n_states, "%s: %s: start %d outside [0, %d)", who, what, g.start, g.n_states);
    SD_REQUIRE(g.masks && g.next && states, "%s: %s: null masks, next or states", who, what);
    SD_REQUIRE(V < 0 || g.cls || g.n_classes == V, "%s: %s: no cls table and n_classes %d differs from the vocabulary %d", who, what,
               g.n_classes, V);
    return SD_OK;
}

// Attach a grammar to the session of a stream's target model (include/specdec.h has the definition and the loops' contract);
// g == NULL detaches.  Host state only: nothing is launched, the device arrays stay the caller's.
extern "C" int sd_session_set_grammar(sd_session *s, const sd_grammar *g, int32_t *states, int32_t states_cap) {
    SD_REQUIRE(s, "sd_session_set_grammar: null session");
    if (!g) {
        s->gram = sd_grammar{};
        s->gram_states = nullptr;
        s->gram_cap = 0;
        return SD_OK;
    }
    if (int rc = check_grammar("sd_session_set_grammar", "grammar", *g, states, -1); rc != SD_OK) return rc;   // (reads no session)
    SD_REQUIRE(states_cap >= 1, "sd_session_set_grammar: grammar: states_cap %d < 1", states_cap);
    if (int rc = check_grammar("sd_session_set_grammar", "grammar", *g, states, s->m->cfg.vocab); rc != SD_OK) return rc;
    s->gram = *g;
    s->gram_states = states;
    s->gram_cap = states_cap;
    return SD_OK;
}

// attn_prefill_kernel + attn_prefill_blocked_kernel launches of this session so far (a host counter: the session profile counts one attention-class launch
// whichever kernel ran).  A batched pass counts on its first session.
extern "C" int sd_session_prefill_attn_launches(const sd_session *s) { return s ? s->prefill_attn_launches : 0; }
extern "C" int sd_session_w12_launches(const sd_session *s) { return s ? s->w12_launches : 0; }
// ... of which attn_prefill_blocked_kernel's (a context past the single score tile, or SD_PREFILL_ATTN_BLOCK set)
extern "C" int sd_session_prefill_attn_blocked_launches(const sd_session *s) { return s ? s->prefill_attn_blocked_launches : 0; }

extern "C" int sd_session_destroy(sd_session *s) {
    if (!s) return SD_OK;
    for (hipEvent_t e : s->ev_pool) (void)hipEventDestroy(e);
    delete s;
    return SD_OK;
}

// ---- profiling brackets ------------------------------------------------------------------
struct ProfScope {
    sd_session *s;
    hipStream_t st;
    bool on;
    ProfScope(sd_session *s_, int cls, hipStream_t st_) : s(s_), st(st_), on(s_->prof_on != 0) {
        if (!on) return;
        while (s->ev_pool.size() < s->ev_used + 2) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) { on = false; return; }
            s->ev_pool.push_back(e);
        }
        s->ev_class.push_back(cls);
        (void)hipEventRecord(s->ev_pool[s->ev_used], st);
        s->prof_stream = st;
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(s->ev_pool[s->ev_used + 1], st);
        s->ev_used += 2;
    }
};

extern "C" int sd_profile_enable(sd_session *s, int on) {
    SD_REQUIRE(s, "sd_profile_enable: null session");
    s->prof_on = on;
    return SD_OK;
}

extern "C" int sd_profile_read(sd_session *s, float *ms_out, int *count_out) {
    SD_REQUIRE(s && ms_out && count_out, "sd_profile_read: null argument");
    if (s->ev_used) {
        SD_HIP_CHECK(hipEventSynchronize(s->ev_pool[s->ev_used - 1]));
        for (size_t i = 0; i < s->ev_used; i += 2) {
            float ms = 0.f;
            SD_HIP_CHECK(hipEventElapsedTime(&ms, s->ev_pool[i], s->ev_pool[i + 1]));
            const int c = s->ev_class[i / 2];
            s->prof_ms[c] += ms;
            s->prof_cnt[c] += 1;
        }
    }
    for (int i = 0; i < SD_N_PROFILE_CLASSES; ++i) {
        ms_out[i] = s->prof_ms[i];
        count_out[i] = s->prof_cnt[i];
        s->prof_ms[i] = 0.f;
        s->prof_cnt[i] = 0;
    }
    s->ev_used = 0;
    s->ev_class.clear();
    return SD_OK;
}


// ---- tensor parallelism (BASELINE config 5: Llama-2-70b over 8 GPUs) ---------------------------------
// Megatron-style sharding of one decoder: QKV and gate/up split by output columns (each rank owns n_heads / world query
// heads, n_kv_heads / world KV heads and inter / world MLP columns), O and down split by input rows, so a layer needs two
// all-reduces of the [rows][hidden] partial outputs (fp32: the sum is rounded to the model dtype once, like an unsharded
// dot product).  At gamma + 1 = 5 rows x 8192 that is 160 KB: latency-bound on xGMI, RCCL picks its low-latency
// protocol on its own for such sizes.  The reference has no counterpart (it is single-process); the math
// follows modeling_llama.py:292-393 with pretraining_tp = 1.
//   * RCCL group: one process per GPU, the communicator is created from a unique id the host broadcasts;
//     the library is resolved with dlopen at first use (a process that already holds RCCL - torch does - shares it).
//   * loopback group: all ranks live in ONE process on one GPU, each in its own host thread and stream; the all-reduce
//     is two event-ordered rendezvous and a sum kernel.  It exists so that the sharded forward can be tested on a
//     one-GPU box (tests/test_gpu_native_parity.py) with the very kernels the RCCL path runs.
#include <dlfcn.h>
#include <condition_variable>
#include <mutex>

struct GemmOut {
    int S;
    size_t stride_s;   // floats between k-slices
};

// What the caller of ONE forward asks of its lm_head, and what the head answers (the native loops, spec_loops.h).  No
// request (NULL): logits_kernel writes logits_out.
struct HeadReq {
    bool raw;              // a head that ran unsplit leaves the logits in the GEMM's own output slab (no copy launch)
    float *zero_rows;      // ... and with zero_rows set it also leaves its tile maxima and clears the probability rows
    long zero_ld;          //     zero_rows + i * zero_ld of its logit rows (see EPI_HEAD)
    float *zero_ptr[16];   // (stream-batched pass: the logit rows' probability rows lie in the streams' own arenas - one
    int zero_n;            //  pointer per logit row, zero_n of them, instead of zero_rows + i * zero_ld)
};
struct HeadOut {
    const float *logits;   // where the logit rows are (NULL after a forward without logit rows), their row stride ...
    long ld;
    int round;             // ... and whether they still have to be rounded to the weights' 16-bit type (SD_NORM_ROUND_*)
    const float *tile_max; // the head's tile maxima, NULL when it could not leave them
};

struct TpLoop {
    int world;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long gen = 0;
    const float *bufs[16];
    hipEvent_t ev_in[16], ev_out[16];
    int refs = 0;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const long g = gen;
        if (++arrived == world) { arrived = 0; ++gen; cv.notify_all(); }
        else cv.wait(lk, [&] { return gen != g; });
    }
};

struct sd_tp {
    int rank, world;
    void *comm;          // ncclComm_t
    TpLoop *loop;
};

typedef int (*nccl_allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
typedef int (*nccl_getid_fn)(void *);
struct sd_nccl_id { char b[128]; };                  // ncclUniqueId is passed by value
typedef int (*nccl_initrank_fn)(void **, int, sd_nccl_id, int);
typedef int (*nccl_destroy_fn)(void *);
typedef int (*nccl_allgather_fn)(const void *, void *, size_t, int, void *, hipStream_t);
static struct { void *lib; nccl_allreduce_fn allreduce; nccl_getid_fn getid; nccl_initrank_fn initrank; nccl_destroy_fn destroy;
                nccl_allgather_fn allgather; } g_rccl;

static int rccl_load() {
    if (g_rccl.lib) return SD_OK;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);          // the copy this process already holds, if any
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { sd_set_error("tensor parallelism needs RCCL: %s", dlerror()); return SD_ERR_HIP; }
    g_rccl.allreduce = (nccl_allreduce_fn)dlsym(h, "ncclAllReduce");
    g_rccl.getid = (nccl_getid_fn)dlsym(h, "ncclGetUniqueId");
    g_rccl.initrank = (nccl_initrank_fn)dlsym(h, "ncclCommInitRank");
    g_rccl.destroy = (nccl_destroy_fn)dlsym(h, "ncclCommDestroy");
    g_rccl.allgather = (nccl_allgather_fn)dlsym(h, "ncclAllGather");
    if (!g_rccl.allreduce || !g_rccl.getid || !g_rccl.initrank || !g_rccl.destroy || !g_rccl.allgather) {
        sd_set_error("RCCL is missing ncclAllReduce / ncclAllGather / ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy");
        return SD_ERR_HIP;
    }
    g_rccl.lib = h;
    return SD_OK;
}

extern "C" int sd_tp_unique_id(void *id128) {
    SD_REQUIRE(id128, "sd_tp_unique_id: null buffer");
    int rc = rccl_load();
    if (rc != SD_OK) return rc;
    if (g_rccl.getid(id128) != 0) { sd_set_error("ncclGetUniqueId failed"); return SD_ERR_HIP; }
    return SD_OK;
}

extern "C" int sd_tp_create_rccl(int rank, int world, const void *id128, sd_tp **out) {
    SD_REQUIRE(out && id128 && world >= 1 && rank >= 0 && rank < world, "sd_tp_create_rccl: bad arguments");
    int rc = rccl_load();
    if (rc != SD_OK) return rc;
    sd_nccl_id id;
    memcpy(id.b, id128, 128);
    void *comm = nullptr;
    if (g_rccl.initrank(&comm, world, id, rank) != 0) { sd_set_error("ncclCommInitRank(rank %d of %d) failed", rank, world); return SD_ERR_HIP; }
    sd_tp *t = new sd_tp{rank, world, comm, nullptr};
    *out = t;
    return SD_OK;
}

// ---- throughput-mode gather of the sharded streams' token rows: one ncclAllGather over RCCL / xGMI ----
struct sd_comm { int rank, world; void *comm; };

extern "C" int sd_comm_probe(void) { return rccl_load(); }
extern "C" int sd_comm_unique_id(void *id128) { return sd_tp_unique_id(id128); }

extern "C" int sd_comm_init(int rank, int world, const void *id128, sd_comm **out) {
    SD_REQUIRE(out && id128 && world >= 1 && rank >= 0 && rank < world, "sd_comm_init: bad arguments");
    int rc = rccl_load();
    if (rc != SD_OK) return rc;
    sd_nccl_id id;
    memcpy(id.b, id128, 128);
    void *comm = nullptr;
    if (g_rccl.initrank(&comm, world, id, rank) != 0) { sd_set_error("ncclCommInitRank(rank %d of %d) failed", rank, world); return SD_ERR_HIP; }
    *out = new sd_comm{rank, world, comm};
    return SD_OK;
}

extern "C" int sd_comm_all_gather_tokens(sd_comm *c, const int32_t *send, int32_t *recv, int rows, int width, void *stream) {
    SD_REQUIRE(c && send && recv && rows >= 0 && width >= 1, "sd_comm_all_gather_tokens: bad arguments");
    if (rows == 0) return SD_OK;
    if (g_rccl.allgather(send, recv, (size_t)rows * (size_t)width, /* ncclInt32 */ 2, c->comm, (hipStream_t)stream) != 0) {
        sd_set_error("ncclAllGather of %d x %d token rows failed on rank %d of %d", rows, width, c->rank, c->world);
        return SD_ERR_HIP;
    }
    return SD_OK;
}

extern "C" int sd_comm_rank(const sd_comm *c, int *rank_out, int *world_out) {
    SD_REQUIRE(c && rank_out && world_out, "sd_comm_rank: null argument");
    *rank_out = c->rank; *world_out = c->world;
    return SD_OK;
}

extern "C" int sd_comm_destroy(sd_comm *c) {
    if (!c) return SD_OK;
    if (c->comm && g_rccl.destroy) g_rccl.destroy(c->comm);
    delete c;
    return SD_OK;
}

extern "C" int sd_tp_create_loopback(int world, sd_tp **out /* world handles */) {
    SD_REQUIRE(out && world >= 1 && world <= 16, "sd_tp_create_loopback: 1..16 ranks");
    TpLoop *L = new TpLoop();
    L->world = world;
    L->refs = world;
    for (int r = 0; r < world; ++r) {
        SD_HIP_CHECK(hipEventCreateWithFlags(&L->ev_in[r], hipEventDisableTiming));
        SD_HIP_CHECK(hipEventCreateWithFlags(&L->ev_out[r], hipEventDisableTiming));
        out[r] = new sd_tp{r, world, nullptr, L};
    }
    return SD_OK;
}

extern "C" int sd_tp_destroy(sd_tp *t) {
    if (!t) return SD_OK;
    if (t->comm && g_rccl.destroy) g_rccl.destroy(t->comm);
    if (t->loop) {
        bool last;
        { std::lock_guard<std::mutex> lk(t->loop->mu); last = --t->loop->refs == 0; }
        if (last) {
            for (int r = 0; r < t->loop->world; ++r) { (void)hipEventDestroy(t->loop->ev_in[r]); (void)hipEventDestroy(t->loop->ev_out[r]); }
            delete t->loop;
        }
    }
    delete t;
    return SD_OK;
}

extern "C" int sd_session_set_tp(sd_session *s, sd_tp *t) {
    SD_REQUIRE(s, "sd_session_set_tp: null session");
    // a group of one has nothing to reduce; SD_TP_FORCE=1 keeps it anyway (tests: the RCCL plumbing on a one-GPU box)
    const char *force = getenv("SD_TP_FORCE");
    s->tp = (t && (t->world > 1 || (force && atoi(force)))) ? t : nullptr;
    return SD_OK;
}

// tp_in[i] = sum_s part[s][i]  (rows are M x N contiguous at the start of every slab)
__global__ void tp_fold_kernel(const float *__restrict__ part, int S, size_t stride_s, int total, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float a = 0.f;
    for (int s2 = 0; s2 < S; ++s2) a += part[(size_t)s2 * stride_s + i];
    out[i] = a;
}
struct TpBufs { const float *p[16]; };
__global__ void tp_sum_kernel(TpBufs b, int world, int total, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float a = 0.f;
    for (int r = 0; r < world; ++r) a += b.p[r][i];          // fixed rank order: every rank gets the same bits
    out[i] = a;
}

// After a row-parallel GEMM: fold this rank's k-slabs, all-reduce the [M][N] fp32 partial over the group and point the
// residual epilogue at the sum (one slab).  No-op without a group.
static int tp_reduce(sd_session *s, GemmOut *go, const float **src, int M, int N, hipStream_t st) {
    sd_tp *t = s->tp;
    if (!t) return SD_OK;
    const int total = M * N;
    // one slab (the row-parallel GEMM kept its whole k-range per workgroup): its [M][N] rows ARE this rank's partial - no fold
    const float *mine = *src;
    if (go->S != 1) {
        ProfScope ps(s, PC_OTHER, st);                                  // (a scope of its own: the profile counts fold launches)
        hipLaunchKernelGGL(tp_fold_kernel, dim3((total + 255) / 256), dim3(256), 0, st, *src, go->S, go->stride_s, total, s->tp_in);
        SD_LAUNCH_CHECK();
        mine = s->tp_in;
    }
    {
        ProfScope ps(s, PC_OTHER, st);
        if (t->comm) {
            if (g_rccl.allreduce(mine, s->tp_out, (size_t)total, /* ncclFloat32 */ 7, /* ncclSum */ 0, t->comm, st) != 0) {
                sd_set_error("ncclAllReduce failed");
                return SD_ERR_HIP;
            }
        } else {
            TpLoop *L = t->loop;
            L->bufs[t->rank] = mine;
            SD_HIP_CHECK(hipEventRecord(L->ev_in[t->rank], st));
            L->barrier();                                           // every rank's partial is enqueued
            TpBufs b = {};
            for (int r = 0; r < t->world; ++r) {
                b.p[r] = L->bufs[r];
                if (r != t->rank) SD_HIP_CHECK(hipStreamWaitEvent(st, L->ev_in[r], 0));
            }
            hipLaunchKernelGGL(tp_sum_kernel, dim3((total + 255) / 256), dim3(256), 0, st, b, t->world, total, s->tp_out);
            SD_LAUNCH_CHECK();
            SD_HIP_CHECK(hipEventRecord(L->ev_out[t->rank], st));
            L->barrier();                                           // nobody overwrites its partial before all have read it
            for (int r = 0; r < t->world; ++r)
                if (r != t->rank) SD_HIP_CHECK(hipStreamWaitEvent(st, L->ev_out[r], 0));
        }
    }
    *src = s->tp_out;
    go->S = 1;
    go->stride_s = 0;
    return SD_OK;
}

// ---- launch helpers ----------------------------------------------------------------------

template <int MT, int EPI, int NTW, typename H = bf16_t>
static void launch_gemm_bf16(const void *W, const void *X, float *part, int M, int Mpad, int N, int K, int S,
                             int ks_per, const GemmEpiT<H> &e, hipStream_t st) {
    const int blocks = (N / 16 / NTW) * S;
    constexpr int UNROLL = stream_unroll(MT, NTW);
    if constexpr (MT == 1 && NTW == 1) {
        if (stream_burst8(MT, NTW, K, ks_per)) {
            hipLaunchKernelGGL((gemm_bf16_stream<1, 8, EPI, 1, true, H>), dim3(blocks), dim3(256), 0, st,
                               (const u32x4 *)W, (const H *)X, part, M, Mpad, N, K, S, ks_per, e);
            return;
        }
    }
    hipLaunchKernelGGL((gemm_bf16_stream<MT, UNROLL, EPI, NTW, true, H>), dim3(blocks), dim3(256), 0, st,
                       (const u32x4 *)W, (const H *)X, part, M, Mpad, N, K, S, ks_per, e);
}

template <int EPI, typename H = bf16_t>
static int dispatch_gemm_bf16(const void *W, const void *X, float *part, int M, int Mpad, int N, int K, int S,
                              int ksp, const GemmEpiT<H> &e, hipStream_t st) {
    const StreamInst in = stream_instance(N, K, M, Mpad, ksp);    // (launch_gemm_bf16 takes the UNROLL by the same functions)
    const int MT = in.MT, ntw = in.NTW;
    if (MT == 1) launch_gemm_bf16<1, EPI, 1, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
    else if (MT == 2) { if (ntw == 4) launch_gemm_bf16<2, EPI, 4, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else if (ntw == 2) launch_gemm_bf16<2, EPI, 2, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else launch_gemm_bf16<2, EPI, 1, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st); }
    else if (MT == 3) { if (ntw == 8) launch_gemm_bf16<3, EPI, 8, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else if (ntw == 4) launch_gemm_bf16<3, EPI, 4, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else if (ntw == 2) launch_gemm_bf16<3, EPI, 2, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else launch_gemm_bf16<3, EPI, 1, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st); }
    else if (MT == 4) { if (ntw == 8) launch_gemm_bf16<4, EPI, 8, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else if (ntw == 4) launch_gemm_bf16<4, EPI, 4, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else if (ntw == 2) launch_gemm_bf16<4, EPI, 2, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st);
                        else launch_gemm_bf16<4, EPI, 1, H>(W, X, part, M, Mpad, N, K, S, ksp, e, st); }
    else { sd_set_error("internal: the streaming GEMM got M=%d rows (route_gemm routes <= 64)", M); return SD_ERR_INVALID; }
    return SD_OK;
}

// Launch a bf16 GEMM the way route_gemm routed it.  EPI_PART leaves r.S k-slabs of [Mpad][N] floats in `part`; any other
// epilogue finishes in the launch (a route of one slab).
template <int EPI, typename H = bf16_t>
static int launch_gemm(const GemmRoute &r, const void *W, const void *X, float *part, int M, int N, int K, const GemmEpiT<H> &e,
                       hipStream_t st) {
    const int Mpad = (int)align_up(M, 16);
    auto bad = [&] {
        sd_set_error("internal: GEMM route %d cannot run epilogue %d (M=%d N=%d K=%d)", r.kind, EPI, M, N, K);
        return SD_ERR_INVALID;
    };
    int rc = SD_OK;
    if constexpr (EPI == EPI_HEAD) {                              // (the head's tile maxima: one m-tile of the streaming kernel)
        if (r.kind != GK_STREAM || Mpad != 16) return bad();
        launch_gemm_bf16<1, EPI_HEAD, 1, H>(W, X, part, M, Mpad, N, K, r.S, r.ksp, e, st);
    } else if (r.kind == GK_STREAM)
        rc = dispatch_gemm_bf16<EPI, H>(W, X, part, M, Mpad, N, K, r.S, r.ksp, e, st);
    else if (r.kind == GK_ROWS)
        rc = launch_gemm_rows<EPI, H>(W, X, part, M, Mpad, N, K, r.rp, e, st);
    else if (r.kind == GK_MM)
        launch_gemm_mm<EPI, H>(W, X, part, M, Mpad, N, K, r, e, st);
    else if constexpr (EPI == EPI_QKV_ROPE || EPI == EPI_QKV_PLAIN) {
        if (r.kind != GK_STREAM_W16) return bad();
        hipLaunchKernelGGL((gemm_bf16_stream_w16<EPI, H, 16>), dim3(N / 16), dim3(1024), 0, st, (const u32x4 *)W, (const H *)X, M, N, K, e);
    } else
        return bad();
    if (rc != SD_OK) return rc;
    SD_LAUNCH_CHECK();
    return SD_OK;
}

// X: [M][K] activations, W: [N][K] weights -> split-K slabs in s->part, cut the way `r` says (16-bit models; an fp32 model
// has one kernel and no route).  xtab: the lm_head's row gather (NULL: every row in place - a route made without GN_GATHER)
template <typename H = bf16_t>
static int run_gemm(sd_session *s, const GemmRoute &r, const void *W, const void *X, int M, int N, int K, GemmOut *go,
                    hipStream_t st, const RowTab *xtab = nullptr) {
    const sd_model_config &c = s->m->cfg;
    ProfScope ps(s, PC_GEMM, st);
    if (!is16(c.dtype)) {
        RowTab none = {};
        hipLaunchKernelGGL(gemm_f32_simple, dim3((N + 3) / 4), dim3(256), 0, st, (const float *)W, (const float *)X,
                           s->part, M, N, K, xtab ? *xtab : none, xtab ? 1 : 0);
        SD_LAUNCH_CHECK();
        go->S = 1;
        go->stride_s = (size_t)M * N;
        return SD_OK;
    }
    const int Mpad = (int)align_up(M, 16);
    SD_REQUIRE(r.kind != GK_NONE, "internal: no GEMM kernel for %d rows of %d x %d (past the session's row limits)", M, N, K);
    SD_REQUIRE((size_t)r.S * Mpad * N <= s->part_floats, "run_gemm: partial buffer too small");
    GemmEpiT<H> e = {};
    if (xtab) { e.use_xmap = 1; e.tab = *xtab; }
    const int rc = launch_gemm<EPI_PART, H>(r, W, X, s->part, M, N, K, e, st);
    if (rc != SD_OK) return rc;
    go->S = r.S;
    go->stride_s = (size_t)Mpad * N;
    return SD_OK;
}

// bf16 GEMM whose workgroups keep the whole k-range (SB = 1) and finish with a fused epilogue: r is a GN_FUSED route
// (eight waves per tile for a shard's gate/up - 448 n-tiles - measured slower: 5.94 against 5.86 ms per verify)
template <int EPI, typename H = bf16_t>
static int run_gemm_fused(sd_session *s, const GemmRoute &r, const void *W, const void *X, int M, int N, int K,
                          const GemmEpiT<H> &e, hipStream_t st) {
    ProfScope ps(s, PC_GEMM, st);
    SD_REQUIRE(r.kind != GK_NONE, "internal: no fused GEMM kernel for %d rows of %d x %d (past the session's row limits)", M, N, K);
    return launch_gemm<EPI, H>(r, W, X, nullptr, M, N, K, e, st);
}

#define ATT_MAX_PARTS 64          // groups * splits the partial buffer is sized for
// 160 KiB per workgroup less the kernel's static LDS (the split path's per-row max / denominator)
#define ATT_LDS_MAX ((size_t)160 * 1024 - 512)
// attn_kernel's key splits for a pass of n_groups row groups whose last row sees s_max keys: the dynamic LDS of a workgroup
// (> ATT_LDS_MAX: the pass does not fit - launch_attn's capacity error)
static size_t attn_split_plan(int D, int s_max, int n_groups, int *nsplit_out, int *s_cap_out) {
    auto lds_for = [&](int nsplit, int *s_cap) {
        const int keys = nsplit > 1 ? (((s_max + nsplit - 1) / nsplit + 15) & ~15) : s_max;
        *s_cap = (int)align_up(keys, 64);
        return sizeof(float) * ((size_t)ATT_TQ * D + (size_t)(256 / (D / 8)) * ATT_TQ * D + (size_t)ATT_TQ * *s_cap);
    };
    const int split_keys = g_env.attn_split_keys, keys_per = g_env.attn_keys_per_split;
    int nsplit = 1, s_cap;
    if (s_max > split_keys) {
        nsplit = std::min(8, (s_max + keys_per - 1) / keys_per);
        while (nsplit > 1 && nsplit * n_groups > ATT_MAX_PARTS) --nsplit;
    }
    // very long contexts: more, smaller chunks until one chunk's score rows fit the LDS
    while (lds_for(nsplit, &s_cap) > ATT_LDS_MAX && (nsplit + 1) * n_groups <= ATT_MAX_PARTS) ++nsplit;
    const size_t lds = lds_for(nsplit, &s_cap);
    *nsplit_out = nsplit;
    *s_cap_out = s_cap;
    return lds;
}

// Prefill passes (rows = consecutive positions of a stream) of a 16-bit model with head_dim 64 or 128, the arena in the model
// type or in fp8: 16-row groups, both products on the matrix cores (prefill_attn.h).  Returns false when the pass does not
// qualify (the caller takes attn_kernel).  While the whole score tile of a row group fits PA_LDS_MAX (2048 keys at head_dim
// 128, 2176 at 64) attn_prefill_kernel runs; past that attn_prefill_blocked_kernel with blocks of PA_BLOCK_KEYS keys
// (plan_prefill_attn) - by default where route_prefill_attn finds that it pays or that attn_kernel cannot hold the pass.
#define PA_LDS_MAX (150 * 1024)
#define PA_BLOCK_KEYS 256         // 16 x 260 floats + the V chunk = 34.3 KiB (26.3 at head_dim 64): four workgroups per CU; the sweep's best
struct PaPlan { int kernel, block; size_t lds; };                 // kernel: 0 none, 1 single tile, 2 blocked; block: keys per score tile
static size_t prefill_attn_lds(int keys, int D) {
    return (size_t)PA_ROWS * ((size_t)align_up(keys, 64) + PA_SPAD) * sizeof(float) + (size_t)PA_VCH * PA_VST(D);
}
// block_keys > 0 (SD_PREFILL_ATTN_BLOCK) forces the blocked kernel with blocks of that many keys, rounded up to a multiple
// of 64 and held to what the LDS takes
static PaPlan plan_prefill_attn(int D, int s_max, int block_keys) {
    if ((D != 64 && D != 128) || s_max < 1) return {0, 0, 0};
    if (block_keys > 0) {
        int kb = (int)align_up(block_keys, 64);
        while (prefill_attn_lds(kb, D) > PA_LDS_MAX) kb -= 64;
        return {2, kb, prefill_attn_lds(kb, D)};
    }
    if (prefill_attn_lds(s_max, D) <= PA_LDS_MAX) return {1, (int)align_up(s_max, 64), prefill_attn_lds(s_max, D)};
    return {2, PA_BLOCK_KEYS, prefill_attn_lds(PA_BLOCK_KEYS, D)};
}
extern "C" int sd_prefill_attn_plan(int head_dim, int s_max, int block_keys, int *kernel, int *block, long *lds_bytes) {
    SD_REQUIRE(s_max >= 1 && block_keys >= 0, "sd_prefill_attn_plan: s_max %d, block_keys %d", s_max, block_keys);
    const PaPlan p = plan_prefill_attn(head_dim, s_max, block_keys);
    if (kernel) *kernel = p.kernel;
    if (block) *block = p.block;
    if (lds_bytes) *lds_bytes = (long)p.lds;
    return SD_OK;
}
// Which attention kernel a pass that meets the gate takes: 0 attn_kernel, 1 the single tile, 2 the blocked kernel.  Past the
// tile limit the blocked kernel is the default only where it pays or where nothing else runs.  Measured (DESIGN.md section 6,
// 256-row passes at 2560 and 4096 keys, seven shapes): its three score sweeps are latency-bound while a CU holds one 4-wave
// workgroup, so against attn_kernel's split keys it is 0.47-0.53x at 128 workgroups (heads x 16-row groups), 0.62-0.69x at
// 192, 0.84-0.93x at 256, 1.3-1.45x at 512 and 1.9-2.2x at 1024 - whatever the head dim.  So: at least PA_BLOCKED_WG_PER_CU
// workgroups per CU -> blocked; fewer -> attn_kernel, as before this kernel existed, while its key splits hold the pass
// (attn_split_plan), and the blocked kernel past that, where launch_attn would return SD_ERR_CAPACITY.  A forced block
// (SD_PREFILL_ATTN_BLOCK) takes the blocked kernel always.
#define PA_BLOCKED_WG_PER_CU 2
static int route_prefill_attn(int D, int n_heads, int n_rows, int n_groups, int s_max, int block_keys, int cus) {
    const PaPlan pl = plan_prefill_attn(D, s_max, block_keys);
    if (pl.kernel != 2 || block_keys > 0) return pl.kernel;
    if (n_heads * ((n_rows + PA_ROWS - 1) / PA_ROWS) >= PA_BLOCKED_WG_PER_CU * cus) return 2;
    int nsplit, s_cap;
    return attn_split_plan(D, s_max, n_groups, &nsplit, &s_cap) > ATT_LDS_MAX ? 2 : 0;
}
extern "C" int sd_prefill_attn_route(int head_dim, int n_heads, int n_rows, int s_max, int block_keys, int cus, int *kernel) {
    SD_REQUIRE(kernel && n_heads >= 1 && n_rows >= 1 && s_max >= 1 && block_keys >= 0 && cus >= 0,
               "sd_prefill_attn_route: heads %d, rows %d, s_max %d, block_keys %d, cus %d", n_heads, n_rows, s_max, block_keys, cus);
    if (!cus) {                                                   // (no tunable is resampled here: sessions keep theirs)
        int dev = 0, n = 0;
        if (g_env.cus > 0) cus = g_env.cus;
        else if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) cus = n;
        else { (void)hipGetLastError(); cus = 256; }
    }
    *kernel = route_prefill_attn(head_dim, n_heads, n_rows, (n_rows + ATT_TQ - 1) / ATT_TQ, s_max, block_keys, cus);
    return SD_OK;
}
// The route of one forward pass: which launches it makes and how each of them is cut.  All of it follows from (session, row
// table, s_max, tunables), so plan_forward fills it once, before the layer loop, and the launch helpers read it - they
// decide nothing themselves.  What does differ between layers (a layer's biases, l + 1 < L) stays in the loop.
enum AttnKind { AK_KERNEL = 0, AK_OPROJ, AK_PREFILL };           // attn_kernel (+ combine) | fused attention + O | matrix cores
struct FwdPlan {
    bool small;                       // the small-model decode path (forward_small)
    bool embed_qkv;                   // the embedding and the first pre-norm ride the layer-0 QKV launch
    int attn;                         // AttnKind
    PaPlan pa;                        // AK_PREFILL: kernel, keys per score tile, LDS ...
    PaGroups pg;                      // ... and its 16-row groups
    int s_max, nsplit, s_cap;         // AK_KERNEL: key splits and the keys one holds; AK_OPROJ: one split
    size_t attn_lds;                  // ... and a workgroup's dynamic LDS (AK_KERNEL past ATT_LDS_MAX: launch_attn's capacity error)
    bool seam_o, seam_d;              // norm on load may open at the attention -> MLP seam / the down -> next QKV seam
    GemmRoute qkv, o, gu, down;       // the per-layer GEMMs of a 16-bit model (not of the small path, which cuts its own)
    GemmRoute head;                   // the lm_head with its row gather (16-bit model, logit rows)
    int rn_threads;                   // blockDim of residual_norm_kernel
};

template <typename T>
static bool prefill_attn_ok(const sd_session *s, const RowTab &tab, int s_max) {
    if constexpr (sizeof(T) != 2) return false;
    const sd_model_config &c = s->m->cfg;
    if (!(g_env.prefill_attn && tab.contig && !tab.tree && (c.head_dim == 64 || c.head_dim == 128) && tab.n_rows >= 32 &&
          c.n_heads % c.n_kv_heads == 0))
        return false;
    return route_prefill_attn(c.head_dim, c.n_heads, tab.n_rows, tab.n_groups, s_max, g_env.prefill_attn_block,
                              g_env.cus > 0 ? g_env.cus : 256) != 0;
}
template <typename T, int D, bool KV8>
static void launch_attn_prefill_inst(const sd_model_config &c, const T *q, const PaGroups &pg, int layer, T *out, const PaPlan &pl,
                                     hipStream_t st) {
    static bool attr = false;                                     // (one flag per instance)
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(attn_prefill_kernel<T, D, KV8>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, PA_LDS_MAX);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(attn_prefill_blocked_kernel<T, D, KV8>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, PA_LDS_MAX);
        attr = true;
    }
    if (pl.kernel == 2)
        hipLaunchKernelGGL((attn_prefill_blocked_kernel<T, D, KV8>), dim3(c.n_heads, pg.n), dim3(256), pl.lds, st, q, pg, layer, out,
                           c.n_heads, c.n_kv_heads, c.arch, 1.0f / sqrtf((float)D), pl.block);
    else
        hipLaunchKernelGGL((attn_prefill_kernel<T, D, KV8>), dim3(c.n_heads, pg.n), dim3(256), pl.lds, st, q, pg, layer, out,
                           c.n_heads, c.n_kv_heads, c.arch, 1.0f / sqrtf((float)D), pl.block);
}
// the table's groups are <= ATT_TQ consecutive rows of a stream: two neighbours of one stream make a 16-row group
static void prefill_groups(const RowTab &tab, PaGroups &pg) {
    pg = PaGroups{};
    for (int g = 0; g < tab.n_groups; ++g) {
        const int i = pg.n;
        const bool join = i > 0 && pg.nrows[i - 1] == ATT_TQ && tab.grp_stream[g] == tab.grp_stream[g - 1] &&
                          tab.grp_row0[g] == pg.row0[i - 1] + ATT_TQ && tab.grp_pos[g] == pg.pos[i - 1] + ATT_TQ;
        if (join) { pg.nrows[i - 1] += tab.grp_n[g]; continue; }
        pg.row0[i] = tab.grp_row0[g]; pg.nrows[i] = tab.grp_n[g]; pg.pos[i] = tab.grp_pos[g];
        pg.max_seq[i] = tab.max_seq[tab.grp_stream[g]]; pg.kv[i] = tab.kv_base[tab.grp_stream[g]];
        pg.kv_scale[i] = tab.kv_fp8 ? tab.kv_scale[tab.grp_stream[g]] : nullptr;
        ++pg.n;
    }
}
template <typename T>
static int launch_attn_prefill(sd_session *s, const T *q, const RowTab &tab, const FwdPlan &fp, int layer, T *out, hipStream_t st) {
    const sd_model_config &c = s->m->cfg;
    const PaPlan &pl = fp.pa;
    SD_REQUIRE(pl.kernel != 0, "internal: no prefill attention kernel for head_dim %d", c.head_dim);
    const bool d64 = c.head_dim == 64;
    if (tab.kv_fp8) {
        if (d64) launch_attn_prefill_inst<T, 64, true>(c, q, fp.pg, layer, out, pl, st);
        else launch_attn_prefill_inst<T, 128, true>(c, q, fp.pg, layer, out, pl, st);
    } else {
        if (d64) launch_attn_prefill_inst<T, 64, false>(c, q, fp.pg, layer, out, pl, st);
        else launch_attn_prefill_inst<T, 128, false>(c, q, fp.pg, layer, out, pl, st);
    }
    if (pl.kernel == 2) ++s->prefill_attn_blocked_launches;
    ++s->prefill_attn_launches;
    return SD_OK;
}

template <typename T, int D>
static int launch_attn(sd_session *s, const T *q, const RowTab &tab, const FwdPlan &fp, int layer, T *out, hipStream_t st) {
    const sd_model_config &c = s->m->cfg;
    const size_t lds_max = ATT_LDS_MAX, lds = fp.attn_lds;
    const int nsplit = fp.nsplit, s_cap = fp.s_cap;
    if (lds > lds_max) {
        sd_set_error("attention: %d keys x %d row groups exceed the LDS score tile", fp.s_max, tab.n_groups);
        return SD_ERR_CAPACITY;
    }
    auto launch = [&](auto kv8, auto tree) -> int {
        constexpr bool KV8 = decltype(kv8)::value, TREE = decltype(tree)::value;
        static bool attr = false;                                 // (one flag per instantiation of this lambda)
        if (!attr) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(attn_kernel<T, D, KV8, TREE>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
            attr = true;
        }
        hipLaunchKernelGGL((attn_kernel<T, D, KV8, TREE>), dim3(c.n_heads, tab.n_groups, nsplit), dim3(256), lds, st, q, tab, layer,
                           out, c.n_heads, c.n_kv_heads, c.arch, 1.0f / sqrtf((float)c.head_dim), s_cap, nsplit, s->attn_part);
        return SD_OK;
    };
    using std::true_type;
    using std::false_type;
    if (tab.kv_fp8) {
        if constexpr (sizeof(T) == 2 && D >= 32) {
            if (tab.tree) launch(true_type{}, true_type{}); else launch(true_type{}, false_type{});
        } else { sd_set_error("fp8 KV needs a 16-bit model with head_dim >= 32"); return SD_ERR_INVALID; }
    } else {
        if (tab.tree) launch(false_type{}, true_type{}); else launch(false_type{}, false_type{});
    }
    if (nsplit > 1)
        hipLaunchKernelGGL((attn_combine_kernel<T, D>), dim3(c.n_heads, tab.n_groups), dim3(128), 0, st,
                           (const float *)s->attn_part, tab, out, c.n_heads, nsplit);
    return SD_OK;
}
template <typename T>
static int launch_attn_d(sd_session *s, const T *q, const RowTab &tab, const FwdPlan &fp, int layer, T *out, hipStream_t st) {
    switch (s->m->cfg.head_dim) {
        case 16: return launch_attn<T, 16>(s, q, tab, fp, layer, out, st);
        case 32: return launch_attn<T, 32>(s, q, tab, fp, layer, out, st);
        case 64: return launch_attn<T, 64>(s, q, tab, fp, layer, out, st);
        default: return launch_attn<T, 128>(s, q, tab, fp, layer, out, st);
    }
}

// Attention + O projection in one launch (fused_kernels.h) for <= 8 rows of one stream on a 16-bit model with
// head_dim 128 and K = n_heads * 128 <= 5120: returns false when the shape does not qualify (the caller then takes the two
// launches).  On success the O projection's single slab is in s->part.
#define AO_LDS_MAX (80 * 1024)
#define AO_DELAY_TICKS 300        // 10 ns ticks the O workgroups hold their weight requests back (fused_kernels.h) ...
#define AO_GAP_TICKS 100          // ... and pause after every 8 requests
static size_t attn_oproj_lds(int s_max) {
    constexpr int D = 128;
    const int s_cap = (int)align_up(s_max, 64);
    return sizeof(float) * ((size_t)ATT_TQ * D + (size_t)(256 / (D / 8)) * ATT_TQ * D + (size_t)ATT_TQ * s_cap);
}
template <typename T>
static bool attn_oproj_ok(const sd_session *s, const RowTab &tab, int s_max) {
    const sd_model_config &c = s->m->cfg;
    if constexpr (sizeof(T) != 2) return false;
    if (!g_env.fuse_attn_o || s->tp || tab.tree || tab.kv_fp8 || tab.contig) return false;
    if (c.head_dim != 128 || tab.n_groups > 2 || tab.n_streams != 1 || tab.n_rows > 16) return false;
    const int K = q_dim(c), N = c.hidden;
    if (K % 128 || K / 128 > AO_NKW || N % 16 || s_max > g_env.attn_split_keys) return false;
    const int cus = g_env.cus > 0 ? g_env.cus : 256;
    if (c.n_heads * tab.n_groups + (N / 16 + 1) / 2 > cus) return false;      // every workgroup resident at once, one per CU
    if ((size_t)16 * N > s->part_floats) return false;
    // (a context whose score tile does not fit the launch's LDS budget takes the two launches - never an error: the key
    //  limit SD_ATTN_SPLIT_KEYS is a tuning knob)
    if (attn_oproj_lds(s_max) > AO_LDS_MAX) return false;
    return true;
}
template <typename T>
static int launch_attn_oproj(sd_session *s, const T *q, const RowTab &tab, const FwdPlan &fp, int layer, T *out, const void *wo,
                             bool resid, hipStream_t st) {
    const sd_model_config &c = s->m->cfg;
    const int s_cap = fp.s_cap;
    const size_t lds = fp.attn_lds;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(attn_oproj_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  AO_LDS_MAX);
        attr = true;
    }
    SD_REQUIRE(lds <= AO_LDS_MAX, "attn_oproj: %d keys exceed the launch's LDS budget", fp.s_max);      // (attn_oproj_ok checked)
    // arrivals counted so far, this launch's included; the epoch advances only once the launch is known to be enqueued (a
    // failed launch must not leave every later wait of the session one arrival short)
    const unsigned n_arrive = (unsigned)(c.n_heads * tab.n_groups);
    const unsigned want = s->ao_epoch + n_arrive + (unsigned)s->skew_now;
    hipLaunchKernelGGL((attn_oproj_kernel<T>), dim3(c.n_heads * tab.n_groups + (c.hidden / 16 + 1) / 2), dim3(512), lds, st, q, tab, layer, out, c.n_heads,
                       c.n_kv_heads, c.arch, 1.0f / sqrtf((float)c.head_dim), s_cap, (const u32x4 *)wo, s->part, tab.n_rows, c.hidden,
                       q_dim(c), s->ao_ctr, want, AO_DELAY_TICKS, AO_GAP_TICKS,
                       g_env.ao_stamps ? s->ao_stamps : (long long *)nullptr,
                       (T *)s->x, (T *)s->h, resid ? s->ssq : (float *)nullptr, s->wait_status);
    SD_LAUNCH_CHECK();
    s->ao_epoch += n_arrive;
    return SD_OK;
}

// Norm on load (normload_kernels.h): <= 8 rows of a 16-bit Llama model whose residual rows were left un-normalised (+
// per-tile sums of squares in s->ssq) by a residual epilogue; the consumer GEMM keeps its whole k-range per workgroup.
template <typename T>
static bool norm_on_load_ok(const sd_session *s, const RowTab &tab) {
    const sd_model_config &c = s->m->cfg;
    if constexpr (sizeof(T) != 2) return false;
    if (!g_env.norm_on_load || c.arch != SD_ARCH_LLAMA || !c.fused_layout || s->tp) return false;
    // (9..16 rows: the conversions cost more than the launch they replace - +5.7 us on gate/up at 12 rows, tools/gemm_bench.py)
    return tab.n_rows <= 8 && c.hidden % 1024 == 0 && c.hidden <= 8192;
}
template <int EPI, typename H>
static int launch_gemm_xn(sd_session *s, const void *W, const void *X, int M, int N, int K, const void *norm_w, float eps,
                          GemmEpiT<H> e, hipStream_t st) {
    ProfScope ps(s, PC_GEMM, st);
    SD_REQUIRE(M <= 8 && N % 16 == 0 && K % 1024 == 0 && K <= 8192, "norm-on-load GEMM: M=%d N=%d K=%d", M, N, K);
    e.nrm_ssq = s->ssq; e.nrm_w = (const H *)norm_w; e.nrm_nt = K / 16; e.nrm_eps = eps;
    // k-steps whose M valid rows fit one conversion register (C * 4 * M <= 64 lanes)
    auto go = [&](auto c) {
        hipLaunchKernelGGL((gemm_bf16_stream_xn<EPI, decltype(c)::value, H>), dim3(N / 16), dim3(256), (size_t)K * sizeof(H), st,
                           (const u32x4 *)W, (const H *)X, (float *)nullptr, M, N, K, 1, K / 32, e);
    };
    using std::integral_constant;
    if (M <= 4) go(integral_constant<int, 4>{});
    else if (M == 5) go(integral_constant<int, 3>{});
    else go(integral_constant<int, 2>{});
    SD_LAUNCH_CHECK();
    return SD_OK;
}

// The k-split GEMM (streaming kernel's split) finishing with the residual epilogue: rows -> s->x, s->h (un-normalised), s->ssq
template <typename H>
static int launch_gemm_fin(sd_session *s, const GemmRoute &pl, const void *W, const void *X, int M, int N, int K, const void *bias,
                           hipStream_t st) {
    ProfScope ps(s, PC_GEMM, st);
    SD_REQUIRE(pl.kind == GK_STREAM && M <= 16 && (size_t)pl.S * 16 * N <= s->part_floats, "k-split GEMM with residual epilogue: M=%d N=%d K=%d", M, N, K);
    GemmEpiT<H> e = {};
    e.bias = (const H *)bias; e.res_x = (H *)s->x; e.res_h = (H *)s->h; e.res_ssq = s->ssq;
    const unsigned want = s->fin_epoch + (unsigned)(pl.S - 1) + (unsigned)s->skew_now;
    hipLaunchKernelGGL((gemm_bf16_stream_fin<H>), dim3((N / 16) * pl.S), dim3(256), 0, st, (const u32x4 *)W, (const H *)X, s->part,
                       M, N, K, pl.S, pl.ksp, e, s->fin_ctr, want, s->wait_status);
    SD_LAUNCH_CHECK();
    s->fin_epoch += (unsigned)(pl.S - 1);                         // (advanced only for a launch that was enqueued)
    return SD_OK;
}

// The same two launches reading 12-bit weight records (w12.h) - defined at the end of this file, so that their kernels
// follow every other kernel of the code object (see launch_attn_bf16 below for what a kernel in the middle costs)
static int launch_gemm_xn_w12(sd_session *s, bool qkv, W12Arg W, const void *X, int M, int N, int K, const void *norm_w, float eps,
                              GemmEpiT<bf16_t> e, hipStream_t st);
static int launch_gemm_fin_w12(sd_session *s, const GemmRoute &pl, W12Arg W, const void *X, int M, int N, int K, hipStream_t st);
// the 12-bit records of layer l's matrix `which`, if this pass may read them (bf16 model, a copy registered)
template <typename T>
static W12Arg w12_of(const sd_model *m, int which, int l) {
    if constexpr (std::is_same<T, bf16_t>::value) return m->w12[which][l];
    return W12Arg{nullptr, nullptr};
}

// The tail of every head whose accumulators lie in s->part as S slabs: a caller that takes the raw slab gets it as it is
// when the head ran unsplit, everybody else gets the slabs folded and rounded into logits_out (logits_kernel).
template <typename T>
static int head_finish(sd_session *s, const HeadReq *rq, HeadOut *ho, int S, size_t stride_s, int n_logits, float *logits_out,
                       long ld_logits, hipStream_t st) {
    const sd_model_config &c = s->m->cfg;
    const int V = c.vocab, round_t = (c.logits_bf16_round || c.arch != SD_ARCH_LLAMA) ? round_code(c.dtype) : 0;
    if (rq && rq->raw && ho && S == 1) {                         // (no result struct: nowhere to hand the slab, so fold it)
        ho->logits = s->part; ho->ld = V; ho->round = round_t;
        return SD_OK;
    }
    ProfScope ps(s, PC_LOGITS, st);
    hipLaunchKernelGGL((logits_kernel<T>), dim3((V + 255) / 256, n_logits), dim3(256), 0, st, s->part, S, stride_s, V, round_t,
                       logits_out, ld_logits);
    SD_LAUNCH_CHECK();
    if (ho) { ho->logits = logits_out; ho->ld = ld_logits; ho->round = 0; }
    return SD_OK;
}

// the route of a GEMM a pass runs once (an fp32 model has one kernel and no routes)
static GemmRoute route_of(const sd_model_config &c, int N, int K, int M, int need) {
    return is16(c.dtype) ? route_gemm(N, K, M, need) : GemmRoute{};
}

// A gather table whose first M rows are all in place (a verify pass: every row a logit row) is no gather for the 16-bit GEMMs
static const RowTab *gather_tab(const sd_model_config &c, const RowTab *xt, int M) {
    for (int i = 0; xt && i < M; ++i)
        if (xt->xmap[i] != i || !is16(c.dtype)) return xt;
    return nullptr;
}

// The lm_head over the (normalised, operand-layout) rows `hl`; xt (or NULL) maps logit row i to its row of hl; hr is its
// route as a gathering GEMM (16-bit models).  Native
// iteration: the head also leaves the maximum of every 16-column tile and clears the probability rows, so the
// normalisation that follows needs no candidate pass over V (EPI_HEAD; whole k-range per workgroup).
template <typename T>
static int head_logits(sd_session *s, const GemmRoute &hr, const T *hl, const RowTab *xt, int n_logits, float *logits_out,
                       long ld_logits, const HeadReq *rq, HeadOut *ho, hipStream_t st) {
    using H16 = typename std::conditional<std::is_same<T, float>::value, bf16_t, T>::type;
    sd_model *m = s->m;
    const sd_model_config &c = m->cfg;
    const int ED = embed_dim(c);
    GemmOut go = {1, 0};                                         // (what the EPI_HEAD launch leaves: one slab)
    int rc;
    const bool zero_tab = rq && !rq->zero_rows && rq->zero_n > 0 && rq->zero_n == n_logits;
    if (is16(c.dtype) && rq && rq->raw && (rq->zero_rows || zero_tab) && n_logits <= 16 && c.vocab % 16 == 0 &&
        hr.kind == GK_STREAM && hr.S == 1) {
        GemmEpiT<H16> e = {};
        if (xt) { e.use_xmap = 1; e.tab = *xt; }
        e.tile_max = s->tile_max; e.zero_rows = rq->zero_rows; e.zero_ld = rq->zero_ld;
        if (zero_tab)
            for (int i = 0; i < n_logits; ++i) e.zero_ptr[i] = rq->zero_ptr[i];
        {
            ProfScope ps(s, PC_GEMM, st);
            if ((rc = launch_gemm<EPI_HEAD, H16>(hr, m->w.lm_head, hl, s->part, n_logits, c.vocab, ED, e, st)) != SD_OK) return rc;
        }
        if (ho) ho->tile_max = s->tile_max;
    } else {
        xt = gather_tab(c, xt, n_logits);
        const GemmRoute r = xt ? hr : route_of(c, c.vocab, ED, n_logits, 0);
        if ((rc = run_gemm<H16>(s, r, m->w.lm_head, hl, n_logits, c.vocab, ED, &go, st, xt)) != SD_OK) return rc;
    }
    return head_finish<T>(s, rq, ho, go.S, go.stride_s, n_logits, logits_out, ld_logits, st);
}

// whether a pass takes the small-model decode path (forward_small)
static bool small_path_ok(const sd_session *s, const RowTab &tab) {
    const sd_model_config &c = s->m->cfg;
    if (!g_env.small_path || c.dtype != SD_BF16 || !c.fused_layout || tab.contig || s->tp) return false;
    if (tab.n_rows > SMALL_MAX_ROWS || tab.n_logit_rows > SMALL_MAX_ROWS) return false;
    if (c.hidden > 2048 || c.hidden % 32 != 0 || embed_dim(c) != c.hidden) return false;
    if (c.arch == SD_ARCH_OPT && !c.opt_pre_ln) return false;          // post-LN keeps the stand-alone norm launches
    if (!s->m->w.final_norm_w) return false;
    return true;
}

// k-slabs of the small path's O / down GEMMs: the streaming GEMM's own policy (bit-identical slabs, what the parity tests
// compare against), at most the 16 slabs s->spart holds
static void small_split(int N, int K, int *S_out, int *ksp_out) {
    const int KS = K / 32;
    gemm_split(N, K, 1, S_out, ksp_out);
    if (*S_out > 16) { *ksp_out = (KS + 15) / 16; *S_out = (KS + *ksp_out - 1) / *ksp_out; }
}

template <int PRO, int EPI>
static int launch_small(sd_session *s, const void *W, const void *X, float *part, int M, int N, int K, int S, int ksp,
                        const GemmEpi &e, const SmallPro &p, hipStream_t st) {
    ProfScope ps(s, PC_GEMM, st);
    const size_t lds = PRO == PRO_TILED ? 0 : (size_t)M * (K + SMALL_XPAD) * sizeof(bf16_t);
    hipLaunchKernelGGL((gemm_small<PRO, EPI>), dim3((N / 16) * S), dim3(256), lds, st, (const u32x4 *)W, (const bf16_t *)X,
                       part, M, N, K, S, ksp, e, p);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

// the QKV epilogue of layer l: rope / scale -> q buffer, K / V appended in place
template <typename H>
static GemmEpiT<H> qkv_epi(const sd_session *s, const RowTab &tab, int l) {
    const sd_model *m = s->m;
    const sd_model_config &c = m->cfg;
    GemmEpiT<H> e = {};
    e.out = (H *)s->qbuf; e.bias = (const H *)m->bqkv[l];
    e.cos_t = (const H *)m->w.rope_cos; e.sin_t = (const H *)m->w.rope_sin;
    e.Hq = c.n_heads; e.Hkv = c.n_kv_heads; e.D = c.head_dim; e.layer = l; e.tab = tab;
    e.q_scale = 1.0f / sqrtf((float)c.head_dim);
    return e;
}
// the gate/up (fc1) epilogue of layer l: SiLU * up / ReLU -> activation buffer
template <typename H>
static GemmEpiT<H> act_epi(const sd_session *s, int l) {
    GemmEpiT<H> e = {};
    e.out = (H *)s->act; e.bias = (const H *)s->m->bfc1[l]; e.n_out = s->m->cfg.inter;
    return e;
}
// the embedding prologue of a layer-0 QKV launch: rows -> s->x, operand = their first pre-norm.  For the 1..4 new rows of a
// small model (the draft's decode step) every workgroup normalises the rows itself while its weight tiles are in flight:
// one launch instead of two, 6.7 us against 5.0 + 5.0 on llama-68m (tools/draft_step_bench.py)
static SmallPro embed_pro(const sd_session *s, const FwdPlan &fp) {
    const sd_model *m = s->m;
    const sd_model_config &c = m->cfg;
    const bool llama = c.arch == SD_ARCH_LLAMA;
    SmallPro p = {};
    p.embed = (const bf16_t *)m->w.embed; p.pos_embed = llama ? nullptr : (const bf16_t *)m->w.pos_embed;
    p.pos_off = 2; p.vocab = c.vocab; p.r_out = (bf16_t *)s->x;       // OPT offset (modeling_opt.py:104)
    p.nw = (const bf16_t *)m->n1w[0]; p.nb = (const bf16_t *)m->n1b[0]; p.eps = c.norm_eps; p.kind = llama ? NORM_RMS : NORM_LN;
    p.H = c.hidden; p.rn_threads = fp.rn_threads;
    return p;
}
// the QKV launch of the small-model kernel for layer e.layer, behind prologue p (rope on Llama)
template <int PRO>
static int launch_small_qkv(sd_session *s, const GemmEpi &e, const SmallPro &p, hipStream_t st) {
    const sd_model_config &c = s->m->cfg;
    const void *W = s->m->wqkv[e.layer];
    const int M = e.tab.n_rows, N = qkv_cols(c), H = c.hidden;
    return c.arch == SD_ARCH_LLAMA ? launch_small<PRO, EPI_QKV_ROPE>(s, W, nullptr, nullptr, M, N, H, 1, H / 32, e, p, st)
                                   : launch_small<PRO, EPI_QKV_PLAIN>(s, W, nullptr, nullptr, M, N, H, 1, H / 32, e, p, st);
}

// residual rows x += fold(S slabs of src) + bias, and their norm (mode RES_*) -> operand rows s->h
template <typename T>
static int resid_norm(sd_session *s, const FwdPlan &fp, int M, T *x, const float *src, int S, size_t stride_s, const void *bias,
                      const void *nw, const void *nb, int mode, hipStream_t st) {
    const sd_model_config &c = s->m->cfg;
    ProfScope ps(s, PC_NORM, st);
    hipLaunchKernelGGL((residual_norm_kernel<T>), dim3(M), dim3(fp.rn_threads), 0, st, x, src, S, stride_s, c.hidden, (const T *)bias,
                       (const T *)nw, (const T *)nb, c.norm_eps, c.arch == SD_ARCH_LLAMA ? NORM_RMS : NORM_LN, mode, (T *)s->h);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

// Decide the route of a pass (FwdPlan)
template <typename T>
static void plan_forward(const sd_session *s, const RowTab &tab, int s_max, FwdPlan &fp) {
    const sd_model_config &c = s->m->cfg;
    const int H = c.hidden, M = tab.n_rows, ED = embed_dim(c);
    const bool llama = c.arch == SD_ARCH_LLAMA, pre = llama || c.opt_pre_ln, fused = is16(c.dtype) && c.fused_layout != 0;
    // residual+norm keeps the row in registers: 2 groups of 4 columns per thread (H <= 8192)
    fp.rn_threads = (int)std::min<size_t>(1024, std::max<size_t>(64, align_up((H / 4 + RN_RG - 1) / RN_RG, 64)));
    fp.s_max = s_max; fp.nsplit = fp.s_cap = 0; fp.attn_lds = 0; fp.pa = PaPlan{};         // (everything but pg, which only
    fp.qkv = fp.o = fp.gu = fp.down = fp.head = GemmRoute{};                                // AK_PREFILL fills and reads)
    fp.small = small_path_ok(s, tab);
    fp.embed_qkv = fp.small || (c.dtype == SD_BF16 && g_env.fuse_embed_qkv && fused && pre && (llama || ED == H) && !tab.contig &&
                                M <= SMALL_MAX_ROWS && H <= 2048 && H % 32 == 0);
    if (!fp.small && attn_oproj_ok<T>(s, tab, s_max)) {
        fp.attn = AK_OPROJ;
        fp.nsplit = 1; fp.s_cap = (int)align_up(s_max, 64); fp.attn_lds = attn_oproj_lds(s_max);
    } else if (!fp.small && prefill_attn_ok<T>(s, tab, s_max)) {
        fp.attn = AK_PREFILL;
        fp.pa = plan_prefill_attn(c.head_dim, s_max, g_env.prefill_attn_block);
        prefill_groups(tab, fp.pg);
    } else {
        fp.attn = AK_KERNEL;
        fp.attn_lds = attn_split_plan(c.head_dim, s_max, tab.n_groups, &fp.nsplit, &fp.s_cap);
    }
    // the residual add in the producer's epilogue, the norm in the consumer's operand load (no launch between)
    const bool seams = pre && fused && norm_on_load_ok<T>(s, tab);
    fp.seam_o = seams && fp.attn == AK_OPROJ;
    fp.seam_d = seams && g_env.norm_on_load > 1;
    if (!is16(c.dtype)) return;
    if (!fp.small) {
        // (a shard's O / down projection: one slab, which the all-reduce takes as it is)
        const int row_par = s->tp ? GN_ONE_SLAB : 0;
        fp.qkv = route_gemm(qkv_cols(c), H, M, fused ? GN_FUSED | GN_QKV : 0);
        fp.o = route_gemm(H, q_dim(c), M, row_par);
        fp.gu = route_gemm(gu_cols(c), H, M, fused ? GN_FUSED : 0);
        fp.down = route_gemm(H, c.inter, M, row_par);
    }
    if (tab.n_logit_rows > 0) fp.head = route_gemm(c.vocab, ED, tab.n_logit_rows, GN_GATHER);
}

// launch_attn_d<bf16_t>, defined behind forward_impl: the kernels of the code object lie in the order in which this file
// first instantiates them, and moving attn_kernel's bf16 instances in front of the small path's GEMMs made launches of
// unchanged kernels 0.2-0.4 us slower (profiles/forward_refactor_ab.json)
static int launch_attn_bf16(sd_session *s, const bf16_t *q, const RowTab &tab, const FwdPlan &fp, int layer, bf16_t *out, hipStream_t st);

// ---- small-model decode path (small_kernels.h): 5 launches per layer + the head --------------------------------
static int forward_small(sd_session *s, const RowTab &tab, const FwdPlan &fp, float *logits_out, long ld_logits, const HeadReq *rq,
                         HeadOut *ho, hipStream_t st) {
    sd_model *m = s->m;
    const sd_model_config &c = m->cfg;
    const int H = c.hidden, I = c.inter, L = c.n_layers, M = tab.n_rows, n_logits = tab.n_logit_rows;
    const bool llama = c.arch == SD_ARCH_LLAMA;
    const int norm_kind = llama ? NORM_RMS : NORM_LN;
    bf16_t *R[2] = {(bf16_t *)s->x, (bf16_t *)s->x2};
    bf16_t *qb = (bf16_t *)s->qbuf, *at = (bf16_t *)s->attn, *ac = (bf16_t *)s->act;
    int cur = 0;                                                   // R[cur] holds the residual stream
    int rc;
    // SD_SMALL_PATH=1: the two norm launches of a layer become prologues of QKV / gate-up; O, down and the head keep the
    // per-op chain's kernels.  =2: every seam a prologue and gemm_small for O / down (the round-2 route, kept for A/B)
    const bool all_pro = g_env.small_path >= 2;
    // the epilogue descriptors are built once per pass (3 KB each, and this is the draft step's host thread): a layer changes
    // its bias and its number
    GemmEpi qe = qkv_epi<bf16_t>(s, tab, 0), ae = act_epi<bf16_t>(s, 0);
    const GemmEpi no_epi = {};
    int S_o, ksp_o, S_d, ksp_d;
    small_split(H, q_dim(c), &S_o, &ksp_o);
    small_split(H, I, &S_d, &ksp_d);
    SD_REQUIRE((size_t)std::max(S_o, S_d) * 16 * H <= s->spart_floats, "forward_small: slab buffer too small");

    auto resid_pro = [&](int S, const bf16_t *bias, const void *nw, const void *nb, bool write_r) {
        SmallPro p = {};
        p.slab = s->spart; p.S = S; p.stride_s = (size_t)16 * H; p.bias = bias;
        p.r_in = R[cur]; p.r_out = write_r ? R[cur ^ 1] : nullptr;
        p.nw = (const bf16_t *)nw; p.nb = (const bf16_t *)nb; p.eps = c.norm_eps; p.kind = norm_kind; p.H = H;
        p.rn_threads = fp.rn_threads;
        return p;
    };
    for (int l = 0; l < L; ++l) {
        // ---- QKV: prologue = embedding (layer 0) or previous layer's down slabs + residual, then input norm
        qe.bias = (const bf16_t *)m->bqkv[l]; qe.layer = l;
        if (l == 0) {
            rc = launch_small_qkv<PRO_EMBED>(s, qe, embed_pro(s, fp), st);
        } else {
            rc = launch_small_qkv<PRO_RESID>(s, qe, resid_pro(S_d, (const bf16_t *)m->bfc2[l - 1], m->n1w[l], m->n1b[l], true), st);
            cur ^= 1;
        }
        if (rc != SD_OK) return rc;
        // ---- attention over the arena
        {
            ProfScope ps(s, PC_ATTN, st);
            if ((rc = launch_attn_bf16(s, qb, tab, fp, l, at, st)) != SD_OK) return rc;
            SD_LAUNCH_CHECK();
        }
        // the slabs of O / down: gemm_small (SD_SMALL_PATH=2) or the streaming kernel, which leaves the same slabs - [S][16][H],
        // the same k-split, the same sums - and runs 0.1-0.9 us faster than gemm_small<PRO_TILED> on these shapes
        auto slab_gemm = [&](const void *W, const bf16_t *X, int K, int S, int ksp) -> int {
            if (all_pro) return launch_small<PRO_TILED, EPI_PART>(s, W, X, s->spart, M, H, K, S, ksp, no_epi, SmallPro{}, st);
            ProfScope ps(s, PC_GEMM, st);
            const int rc2 = dispatch_gemm_bf16<EPI_PART, bf16_t>(W, X, s->spart, M, 16, H, K, S, ksp, no_epi, st);
            SD_LAUNCH_CHECK();
            return rc2;
        };
        // ---- O projection -> slabs
        if ((rc = slab_gemm(m->wo[l], at, q_dim(c), S_o, ksp_o)) != SD_OK) return rc;
        // ---- gate/up (fc1): prologue = O slabs + residual + post-attention norm; epilogue = SiLU * up / ReLU
        ae.bias = (const bf16_t *)m->bfc1[l];
        const SmallPro p = resid_pro(S_o, (const bf16_t *)m->bo[l], m->n2w[l], m->n2b[l], true);
        rc = llama ? launch_small<PRO_RESID, EPI_ACT_SILU>(s, m->wgu[l], nullptr, nullptr, M, gu_cols(c), H, 1, H / 32, ae, p, st)
                   : launch_small<PRO_RESID, EPI_ACT_RELU>(s, m->wgu[l], nullptr, nullptr, M, gu_cols(c), H, 1, H / 32, ae, p, st);
        if (rc != SD_OK) return rc;
        cur ^= 1;
        // ---- down projection (fc2) -> slabs
        if ((rc = slab_gemm(m->wdown[l], ac, I, S_d, ksp_d)) != SD_OK) return rc;
    }
    if (n_logits > 0 && !all_pro) {
        // ---- head: the final residual + norm keeps its launch.  As a prologue of the lm_head every one of its 2000-3142
        // workgroups folds the slabs and normalises the rows for itself: 18.5 us against 4.4 + 9.6 on llama-68m, 31.4 against
        // 4.3 + 14.2 on opt-125m (rocprofv3, profiles/r04_small_path_*.txt)
        if ((rc = resid_norm<bf16_t>(s, fp, M, R[cur], s->spart, S_d, (size_t)16 * H, m->bfc2[L - 1], m->w.final_norm_w, m->w.final_norm_b,
                                     RES_PRE, st)) != SD_OK)
            return rc;
        return head_logits<bf16_t>(s, fp.head, (const bf16_t *)s->h, &tab, n_logits, logits_out, ld_logits, rq, ho, st);
    }
    if (n_logits > 0) {
        // ---- head (SD_SMALL_PATH=2): prologue = last down slabs + residual + final norm on the rows that need logits
        GemmEpi e = {};
        e.use_xmap = 1; e.tab = tab;
        SmallPro p = resid_pro(S_d, (const bf16_t *)m->bfc2[L - 1], m->w.final_norm_w, m->w.final_norm_b, false);
        SD_REQUIRE((size_t)16 * c.vocab <= s->part_floats, "forward_small: logits slab too small");
        // (tile maxima only for the loop that names ONE block of probability rows: the per-stream table is head_logits' own)
        if (rq && rq->raw && rq->zero_rows && c.vocab % 16 == 0) {
            e.tile_max = s->tile_max; e.zero_rows = rq->zero_rows; e.zero_ld = rq->zero_ld;
            if ((rc = launch_small<PRO_RESID, EPI_HEAD>(s, m->w.lm_head, nullptr, s->part, n_logits, c.vocab, H, 1, H / 32, e, p, st)) != SD_OK) return rc;
            if (ho) ho->tile_max = s->tile_max;
        } else {
            if ((rc = launch_small<PRO_RESID, EPI_PART>(s, m->w.lm_head, nullptr, s->part, n_logits, c.vocab, H, 1, H / 32, e, p, st)) != SD_OK) return rc;
        }
        return head_finish<bf16_t>(s, rq, ho, 1, (size_t)16 * c.vocab, n_logits, logits_out, ld_logits, st);
    }
    return SD_OK;
}

template <typename T>
static int forward_impl(sd_session *s, const RowTab &tab, int s_max, float *logits_out, long ld_logits, const HeadReq *rq,
                        HeadOut *ho, hipStream_t st) {
    // 16-bit storage type of the MFMA GEMMs (the fp32 instantiation never launches them; it only has to compile)
    using H16 = typename std::conditional<std::is_same<T, float>::value, bf16_t, T>::type;
    const int n_new = tab.n_rows, n_logits = tab.n_logit_rows;
    sd_model *m = s->m;
    const sd_model_config &c = m->cfg;
    FwdPlan fp;
    plan_forward<T>(s, tab, s_max, fp);
    if (fp.small) return forward_small(s, tab, fp, logits_out, ld_logits, rq, ho, st);
    const int H = c.hidden, D = c.head_dim, I = c.inter, L = c.n_layers, ED = embed_dim(c);
    const bool llama = c.arch == SD_ARCH_LLAMA, pre = llama || c.opt_pre_ln, fused = is16(c.dtype) && c.fused_layout != 0;
    const bool plain_embed = llama || ED == H;                             // no input projection
    const int norm_kind = llama ? NORM_RMS : NORM_LN, pos_off = 2;           // OPT offset (modeling_opt.py:104)
    const T *pos_embed = llama ? (const T *)nullptr : (const T *)m->w.pos_embed;
    T *x = (T *)s->x, *h = (T *)s->h, *qb = (T *)s->qbuf, *at = (T *)s->attn, *ac = (T *)s->act, *eb = (T *)s->ebuf;
    const size_t norm_lds = (size_t)(H + 32) * sizeof(float);
    GemmOut go;
    int rc;

    // ---- embeddings -> residual rows x, first pre-norm -> operand rows h (one launch when there is no input projection),
    // unless both are the prologue of the layer-0 QKV launch below
    if (!fp.embed_qkv && plain_embed && pre) {
        ProfScope ps(s, PC_EMBED, st);
        hipLaunchKernelGGL((embed_norm_kernel<T>), dim3(n_new), dim3(256), norm_lds, st, tab, (const T *)m->w.embed, H, pos_embed,
                           pos_off, x, (const T *)m->n1w[0], (const T *)m->n1b[0], c.norm_eps, norm_kind, h, c.vocab);
        SD_LAUNCH_CHECK();
    } else if (!fp.embed_qkv) {
        if (plain_embed) {
            ProfScope ps(s, PC_EMBED, st);
            hipLaunchKernelGGL((embed_kernel<T>), dim3(n_new), dim3(256), 0, st, tab, (const T *)m->w.embed, H, pos_embed, pos_off,
                               x, 0, c.vocab);
            SD_LAUNCH_CHECK();
        } else {                                                  // OPT project_in
            {
                ProfScope ps(s, PC_EMBED, st);
                hipLaunchKernelGGL((embed_kernel<T>), dim3(n_new), dim3(256), 0, st, tab, (const T *)m->w.embed, ED,
                                   (const T *)nullptr, 0, eb, 1, c.vocab);
                SD_LAUNCH_CHECK();
            }
            if ((rc = run_gemm<H16>(s, route_of(c, H, ED, n_new, 0), m->w.project_in, eb, n_new, H, ED, &go, st)) != SD_OK) return rc;
            ProfScope ps(s, PC_EMBED, st);
            hipLaunchKernelGGL((reduce_addpos_kernel<T>), dim3(n_new), dim3(256), 0, st, s->part, go.S, go.stride_s, H,
                               (const T *)m->w.pos_embed, tab, pos_off, x);
            SD_LAUNCH_CHECK();
        }
        ProfScope ps(s, PC_NORM, st);                             // ---- first pre-norm
        if (pre)
            hipLaunchKernelGGL((norm_kernel<T>), dim3(n_new), dim3(256), norm_lds, st, x, H, (const T *)m->n1w[0],
                               (const T *)m->n1b[0], c.norm_eps, norm_kind, h);
        else
            hipLaunchKernelGGL((to_operand_kernel<T>), dim3(n_new), dim3(256), 0, st, (const T *)x, H, h);
        SD_LAUNCH_CHECK();
    }
    for (int l = 0; l < L; ++l) {
        // a seam opens where the producer has no bias; the last layer keeps its residual+norm launch (the final norm feeds the head)
        const bool xn_q = fp.seam_d && l > 0 && !m->bfc2[l - 1];        // layer l - 1's down projection left un-normalised rows
        const bool xn_o = fp.seam_o && !m->bo[l];
        const bool xn_d = fp.seam_d && l + 1 < L && !m->bfc2[l];
        // ---- QKV projection -> rope / scale -> q buffer + in-place KV append (fused into the GEMM's epilogue with the fused
        // weight layout, else slabs for the stand-alone epilogue)
        if (l == 0 && fp.embed_qkv) {
            if ((rc = launch_small_qkv<PRO_EMBED>(s, qkv_epi<bf16_t>(s, tab, 0), embed_pro(s, fp), st)) != SD_OK) return rc;
        } else if (xn_q && w12_of<T>(m, SD_W12_QKV, l).codes) {
            rc = launch_gemm_xn_w12(s, true, w12_of<T>(m, SD_W12_QKV, l), h, n_new, qkv_cols(c), H, m->n1w[l], c.norm_eps, qkv_epi<bf16_t>(s, tab, l), st);
            if (rc != SD_OK) return rc;
        } else if (xn_q) {
            rc = launch_gemm_xn<EPI_QKV_ROPE, H16>(s, m->wqkv[l], h, n_new, qkv_cols(c), H, m->n1w[l], c.norm_eps, qkv_epi<H16>(s, tab, l), st);
            if (rc != SD_OK) return rc;
        } else if (fused) {
            const GemmEpiT<H16> e = qkv_epi<H16>(s, tab, l);
            rc = llama ? run_gemm_fused<EPI_QKV_ROPE, H16>(s, fp.qkv, m->wqkv[l], h, n_new, qkv_cols(c), H, e, st)
                       : run_gemm_fused<EPI_QKV_PLAIN, H16>(s, fp.qkv, m->wqkv[l], h, n_new, qkv_cols(c), H, e, st);
            if (rc != SD_OK) return rc;
        } else {
            if ((rc = run_gemm<H16>(s, fp.qkv, m->wqkv[l], h, n_new, qkv_cols(c), H, &go, st)) != SD_OK) return rc;
            ProfScope ps(s, PC_QKV, st);
            hipLaunchKernelGGL((qkv_epilogue_kernel<T>), dim3(n_new, c.n_heads + 2 * c.n_kv_heads),
                               dim3(std::max(D / 2, 64)), 0, st, s->part, go.S, go.stride_s, qkv_cols(c),
                               (const T *)m->bqkv[l], (const T *)m->w.rope_cos, (const T *)m->w.rope_sin, c.arch,
                               1.0f / sqrtf((float)D), c.n_heads, c.n_kv_heads, D, tab, l, qb, 0);
            SD_LAUNCH_CHECK();
        }
        // ---- attention over the arena (AK_OPROJ: and the O projection, its single slab left in s->part)
        {
            ProfScope ps(s, PC_ATTN, st);
            if constexpr (!std::is_same<T, float>::value) {            // (the fp32 instantiation has neither kernel)
                if (fp.attn == AK_OPROJ) rc = launch_attn_oproj<T>(s, qb, tab, fp, l, at, m->wo[l], xn_o, st);
                else if (fp.attn == AK_PREFILL) rc = launch_attn_prefill<T>(s, qb, tab, fp, l, at, st);
            }
            if (fp.attn == AK_KERNEL) rc = launch_attn_d<T>(s, qb, tab, fp, l, at, st);
            if (rc != SD_OK) return rc;
            SD_LAUNCH_CHECK();
        }
        // ---- output projection + residual (+ norm feeding the MLP)
        if (fp.attn == AK_OPROJ) go = GemmOut{1, (size_t)16 * H};
        else if ((rc = run_gemm<H16>(s, fp.o, m->wo[l], at, n_new, H, q_dim(c), &go, st)) != SD_OK) return rc;
        const float *osrc = s->part;
        if ((rc = tp_reduce(s, &go, &osrc, n_new, H, st)) != SD_OK) return rc;
        if (!xn_o && (rc = resid_norm<T>(s, fp, n_new, x, osrc, go.S, go.stride_s, m->bo[l], pre ? m->n2w[l] : m->n1w[l],
                                         pre ? m->n2b[l] : m->n1b[l], pre ? RES_PRE : RES_POST, st)) != SD_OK)
            return rc;
        // ---- gate/up (fc1) -> SiLU * up / ReLU -> activation buffer
        if (xn_o && w12_of<T>(m, SD_W12_GATE_UP, l).codes) {
            rc = launch_gemm_xn_w12(s, false, w12_of<T>(m, SD_W12_GATE_UP, l), h, n_new, gu_cols(c), H, m->n2w[l], c.norm_eps, act_epi<bf16_t>(s, l), st);
            if (rc != SD_OK) return rc;
        } else if (xn_o) {
            rc = launch_gemm_xn<EPI_ACT_SILU, H16>(s, m->wgu[l], h, n_new, gu_cols(c), H, m->n2w[l], c.norm_eps, act_epi<H16>(s, l), st);
            if (rc != SD_OK) return rc;
        } else if (fused) {
            const GemmEpiT<H16> e = act_epi<H16>(s, l);
            rc = llama ? run_gemm_fused<EPI_ACT_SILU, H16>(s, fp.gu, m->wgu[l], h, n_new, gu_cols(c), H, e, st)
                       : run_gemm_fused<EPI_ACT_RELU, H16>(s, fp.gu, m->wgu[l], h, n_new, gu_cols(c), H, e, st);
            if (rc != SD_OK) return rc;
        } else {
            if ((rc = run_gemm<H16>(s, fp.gu, m->wgu[l], h, n_new, gu_cols(c), H, &go, st)) != SD_OK) return rc;
            ProfScope ps(s, PC_ACT, st);
            hipLaunchKernelGGL((act_kernel<T>), dim3((I + 255) / 256, n_new), dim3(256), 0, st, s->part, go.S,
                               go.stride_s, I, gu_cols(c), c.arch, (const T *)m->bfc1[l], ac, 0);
            SD_LAUNCH_CHECK();
        }
        // ---- down projection (fc2) + residual (+ the next norm).  With the norm-on-load seam its last k-slab's workgroups add
        // the residual and the next layer's QKV normalises on load (no residual+norm launch)
        if (xn_d && w12_of<T>(m, SD_W12_DOWN, l).codes) {
            if ((rc = launch_gemm_fin_w12(s, fp.down, w12_of<T>(m, SD_W12_DOWN, l), ac, n_new, H, I, st)) != SD_OK) return rc;
        } else if (xn_d) {
            if ((rc = launch_gemm_fin<H16>(s, fp.down, m->wdown[l], ac, n_new, H, I, nullptr, st)) != SD_OK) return rc;
        } else {
            if ((rc = run_gemm<H16>(s, fp.down, m->wdown[l], ac, n_new, H, I, &go, st)) != SD_OK) return rc;
            const float *dsrc = s->part;
            if ((rc = tp_reduce(s, &go, &dsrc, n_new, H, st)) != SD_OK) return rc;
            int mode = RES_NONE;
            const void *nw = nullptr, *nb = nullptr;
            if (!pre) { mode = RES_POST; nw = m->n2w[l]; nb = m->n2b[l]; }
            else if (l + 1 < L) { mode = RES_PRE; nw = m->n1w[l + 1]; nb = m->n1b[l + 1]; }
            else if (m->w.final_norm_w) { mode = RES_PRE; nw = m->w.final_norm_w; nb = m->w.final_norm_b; }
            if ((rc = resid_norm<T>(s, fp, n_new, x, dsrc, go.S, go.stride_s, m->bfc2[l], nw, nb, mode, st)) != SD_OK) return rc;
        }
    }

    if (n_logits == 0) return SD_OK;
    // only the rows tab.xmap lists feed the head (the last rows of each stream)
    const T *hl = h;
    const RowTab *xt = &tab;
    if (ED != H) {                                              // OPT project_out (modeling_opt.py:744-745)
        xt = gather_tab(c, xt, n_logits);
        const GemmRoute r = route_of(c, ED, H, n_logits, xt ? GN_GATHER : 0);
        if ((rc = run_gemm<H16>(s, r, m->w.project_out, hl, n_logits, ED, H, &go, st, xt)) != SD_OK) return rc;
        ProfScope ps(s, PC_LOGITS, st);
        hipLaunchKernelGGL((reduce_rows_kernel<T>), dim3((ED + 255) / 256, n_logits), dim3(256), 0, st, s->part, go.S, go.stride_s,
                           ED, eb);
        SD_LAUNCH_CHECK();
        hl = eb;
        xt = nullptr;
    }
    return head_logits<T>(s, fp.head, hl, xt, n_logits, logits_out, ld_logits, rq, ho, st);
}

// fill the attention groups and the lm_head row map of a table whose rows are already laid out stream by stream
static void finish_table(RowTab &tab) {
    tab.n_groups = 0;
    if (tab.contig == 2) {                          // runs of several streams: groups of ATT_TQ consecutive rows inside a run
        for (int i = 0; i < tab.n_streams; ++i)
            for (int r = tab.seg_row0[i]; r < tab.seg_row0[i + 1]; r += ATT_TQ) {
                const int g = tab.n_groups++;
                tab.grp_row0[g] = r;
                tab.grp_n[g] = std::min(ATT_TQ, tab.seg_row0[i + 1] - r);
                tab.grp_pos[g] = tab.seg_pos0[i] + (r - tab.seg_row0[i]);
                tab.grp_stream[g] = i;
            }
        return;
    }
    if (tab.contig) {                               // up to 256 rows = 32 groups of ATT_TQ consecutive positions
        for (int r = 0; r < tab.n_rows; r += ATT_TQ) {
            const int g = tab.n_groups++;
            tab.grp_row0[g] = r;
            tab.grp_n[g] = std::min(ATT_TQ, tab.n_rows - r);
            tab.grp_pos[g] = tab.pos0 + r;
            tab.grp_stream[g] = 0;
        }
        return;
    }
    int r = 0;
    while (r < tab.n_rows) {
        int n = 1;
        while (r + n < tab.n_rows && n < ATT_TQ && tab.row_stream[r + n] == tab.row_stream[r] &&
               (tab.tree || tab.row_pos[r + n] == tab.row_pos[r] + n))     // tree rows group by storage order
            ++n;
        tab.grp_row0[tab.n_groups] = r;
        tab.grp_n[tab.n_groups] = n;
        tab.grp_pos[tab.n_groups] = tab.row_pos[r];
        tab.grp_stream[tab.n_groups] = tab.row_stream[r];
        ++tab.n_groups;
        r += n;
    }
}

static int launch_attn_bf16(sd_session *s, const bf16_t *q, const RowTab &tab, const FwdPlan &fp, int layer, bf16_t *out, hipStream_t st) {
    return launch_attn_d<bf16_t>(s, q, tab, fp, layer, out, st);
}

// stream i of a table: the session's arena and the stream's token buffer
static void bind_stream(RowTab &tab, int i, const sd_session *s, const int32_t *tokens) {
    tab.tok_base[i] = tokens;
    tab.kv_base[i] = s->kv;
    tab.max_seq[i] = s->max_seq;
    tab.kv_fp8 = s->kv_fp8;
    tab.kv_scale[i] = s->kv_scale;
}

static int run_forward(sd_session *s, const RowTab &tab, int s_max, float *logits_out, long ld_logits, const HeadReq *rq,
                       HeadOut *ho, void *stream) {
    int rc;
    if (ho) *ho = HeadOut{};                                     // (a forward without logit rows leaves it empty)
    if (s->resync) {
        // the previous forward of this session failed part-way (or ran with a test skew): its fused launches' arrival counters
        // and the host's epochs may disagree, and every later wait would then run into its 20 ms limit.  Stream-ordered
        // re-zeroing behind whatever of that forward did run puts both back in step.
        SD_HIP_CHECK(hipMemsetAsync(s->fin_ctr, 0, (size_t)(s->m->cfg.hidden / 16 + 1) * sizeof(unsigned), (hipStream_t)stream));
        SD_HIP_CHECK(hipMemsetAsync(s->ao_ctr, 0, 128, (hipStream_t)stream));
        s->ao_epoch = s->fin_epoch = 0;
        s->resync = 0;
    }
    s->skew_now = s->test_skew;
    s->test_skew = 0;
    if (s->m->cfg.dtype == SD_BF16)
        rc = forward_impl<bf16_t>(s, tab, s_max, logits_out, ld_logits, rq, ho, (hipStream_t)stream);
    else if (s->m->cfg.dtype == SD_F16)
        rc = forward_impl<f16_t>(s, tab, s_max, logits_out, ld_logits, rq, ho, (hipStream_t)stream);
    else
        rc = forward_impl<float>(s, tab, s_max, logits_out, ld_logits, rq, ho, (hipStream_t)stream);
    if (rc != SD_OK || s->skew_now) s->resync = 1;
    s->skew_now = 0;
    return rc;
}

static int session_forward(sd_session *s, const int32_t *tokens, int n_new, int pos0, int n_logits, float *logits_out,
                           long ld_logits, const HeadReq *rq, HeadOut *ho, void *stream) {
    SD_REQUIRE(s && tokens, "sd_session_forward: null argument");
    SD_REQUIRE(n_new >= 1 && pos0 >= 0, "sd_session_forward: n_new=%d pos0=%d", n_new, pos0);
    SD_REQUIRE(n_logits >= 0 && n_logits <= n_new, "sd_session_forward: n_logits=%d of n_new=%d", n_logits, n_new);
    SD_REQUIRE(n_logits == 0 || logits_out, "sd_session_forward: logits_out is null");
    // (logit rows are gathered by the streaming kernel, <= 64 rows per call, unless every row of the call is one)
    const int max_logits = n_logits == n_new ? s->max_pass_rows : SD_STREAM_MAX_ROWS;
    if (n_new > s->max_rows || n_new > SD_MAX_FWD_ROWS || n_logits > max_logits || pos0 + n_new > s->max_seq) {
        sd_set_error("sd_session_forward: n_new=%d (max_rows %d, <=%d), n_logits=%d (<=%d), pos0+n_new=%d (max_seq %d)",
                     n_new, s->max_rows, SD_MAX_FWD_ROWS, n_logits, max_logits, pos0 + n_new, s->max_seq);
        return SD_ERR_CAPACITY;
    }
    RowTab tab = {};
    tab.n_rows = n_new;
    tab.n_streams = 1;
    tab.n_logit_rows = n_logits;
    bind_stream(tab, 0, s, tokens - pos0);      // indexed by absolute position, only ever read at pos0 .. pos0+n_new-1
    if (n_new > SD_MAX_ROWS) {                      // prefill chunk: positions are implicit
        tab.contig = 1;
        tab.pos0 = pos0;
    } else {
        for (int i = 0; i < n_new; ++i) { tab.row_pos[i] = pos0 + i; tab.row_stream[i] = 0; }
    }
    for (int i = 0; i < n_logits; ++i) tab.xmap[i] = (unsigned char)(n_new - n_logits + i);   // n_new <= 256
    finish_table(tab);
    return run_forward(s, tab, pos0 + n_new, logits_out, ld_logits, rq, ho, stream);
}

extern "C" int sd_session_forward(sd_session *s, const int32_t *tokens, int n_new, int pos0, int n_logits,
                                  float *logits_out, long ld_logits, void *stream) {
    return session_forward(s, tokens, n_new, pos0, n_logits, logits_out, ld_logits, nullptr, nullptr, stream);
}

// Tree verify (reference kvcache_model.py:38-136 forward_tree_attention + modeling_llama.py:684-689): the n rows are
// the nodes of a draft token tree.  Node i has token tokens[i], position positions[i] (its depth: RoPE / learned
// position), sees all `base_len` cached positions and the nodes whose bit is set in masks[i] (ancestors + itself, bit j
// = node j, j <= i), and its K / V rows are appended at arena slot base_len + i.  Logits come out for all n nodes.
extern "C" int sd_session_forward_tree(sd_session *s, const int32_t *tokens, const int32_t *positions, const uint64_t *masks,
                                       int n, int base_len, float *logits_out, long ld_logits, void *stream) {
    SD_REQUIRE(s && tokens && positions && masks && logits_out, "sd_session_forward_tree: null argument");
    SD_REQUIRE(n >= 1 && n <= SD_MAX_TREE && base_len >= 0, "sd_session_forward_tree: 1..%d nodes", SD_MAX_TREE);
    if (n > s->max_rows || base_len + n > s->max_seq) {
        sd_set_error("sd_session_forward_tree: %d nodes after %d positions exceed max_rows %d / max_seq %d", n, base_len,
                     s->max_rows, s->max_seq);
        return SD_ERR_CAPACITY;
    }
    RowTab tab = {};
    tab.n_rows = n;
    tab.n_streams = 1;
    tab.n_logit_rows = n;
    tab.tree = 1;
    tab.tree_base = base_len;
    bind_stream(tab, 0, s, tokens);              // tree rows: the token of node i is tokens[i] (tab_tok)
    for (int i = 0; i < n; ++i) {
        SD_REQUIRE(positions[i] >= 0 && positions[i] < s->m->cfg.max_pos, "sd_session_forward_tree: position %d out of range", positions[i]);
        SD_REQUIRE((masks[i] >> i) & 1ull, "sd_session_forward_tree: node %d must see itself", i);
        SD_REQUIRE(i == 63 || (masks[i] >> (i + 1)) == 0, "sd_session_forward_tree: node %d sees a later node", i);
        tab.row_pos[i] = positions[i];
        tab.row_stream[i] = 0;
        tab.tree_mask[i] = masks[i];
        tab.xmap[i] = (unsigned char)i;
    }
    finish_table(tab);
    return run_forward(s, tab, base_len + n, logits_out, ld_logits, nullptr, nullptr, stream);
}

// Gather-compaction of the KV arena after a tree verify (reference kvcache_model.py:326-353 rollback_tree_attention,
// one kept path): the rows at slots base + idx[j] (idx ascending, j < k) move to base + j in every layer / head.
__global__ void kv_compact_kernel(char *kv, int max_seq, int row_bytes, int base, const int *__restrict__ idx, int k) {
    extern __shared__ __attribute__((aligned(16))) char sm[];
    char *arena = kv + (size_t)blockIdx.x * max_seq * row_bytes;       // one (layer, k|v, head) plane per workgroup
    const int n16 = row_bytes / 16;
    for (int i = threadIdx.x; i < k * n16; i += blockDim.x) {
        const int j = i / n16, c = i - j * n16;
        reinterpret_cast<uint4 *>(sm)[i] = reinterpret_cast<const uint4 *>(arena + (size_t)(base + idx[j]) * row_bytes)[c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k * n16; i += blockDim.x) {
        const int j = i / n16, c = i - j * n16;
        reinterpret_cast<uint4 *>(arena + (size_t)(base + j) * row_bytes)[c] = reinterpret_cast<const uint4 *>(sm)[i];
    }
}

// debugging aid (tools/ao_stamps.py): the per-workgroup records the last fused attention + O launch left (SD_AO_STAMPS=1):
// out[w][8] for workgroup w < n_wgs <= AO_STAMP_WGS - see AO_ST_* in fused_kernels.h
extern "C" int sd_session_ao_stamps(sd_session *s, long long *out, int n_wgs) {
    SD_REQUIRE(s && out && n_wgs >= 1 && n_wgs <= AO_STAMP_WGS, "sd_session_ao_stamps: 1..%d workgroup records", AO_STAMP_WGS);
    SD_HIP_CHECK(hipMemcpy(out, s->ao_stamps, (size_t)n_wgs * 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return SD_OK;
}

// Sticky status of the in-launch waits of this session's fused launches (attention + O projection: bit 0; k-split GEMM with
// the residual epilogue: bit 1).  A wait that ran into its 20 ms limit poisons its output with NaN - the sampler then
// reports 'norm logits error' - and sets its bit here, so the host can tell a timed-out hand-off from a model that
// produced NaN.  Reads and clears the word; call with the session's stream idle.
extern "C" int sd_session_fused_status(sd_session *s, unsigned *status_out) {
    SD_REQUIRE(s && status_out, "sd_session_fused_status: null argument");
    SD_HIP_CHECK(hipMemcpy(status_out, s->wait_status, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (*status_out) {
        SD_HIP_CHECK(hipMemset(s->wait_status, 0, sizeof(unsigned)));
        s->resync = 1;                                            // the counters may be short of the epochs now
    }
    return SD_OK;
}

// TEST HOOK: the fused launches of the NEXT forward of this session expect `extra` more arrivals than will come, so their
// waits run into the time limit (tests/: the timeout branch must surface as NaN logits / 'norm logits error' and a status
// bit, never as finite numbers).  The forward after that re-synchronises counters and epochs.
extern "C" int sd_session_test_skew_wait(sd_session *s, int extra) {
    SD_REQUIRE(s && extra >= 0 && extra <= 1024, "sd_session_test_skew_wait: extra in 0..1024");
    s->test_skew = extra;
    return SD_OK;
}

extern "C" int sd_session_compact_kv(sd_session *s, int base_len, const int32_t *idx_dev, int k, void *stream) {
    SD_REQUIRE(s && idx_dev && k >= 0 && k <= SD_MAX_TREE && base_len >= 0 && base_len + k <= s->max_seq,
               "sd_session_compact_kv: bad arguments");
    if (k == 0) return SD_OK;
    const sd_model_config &c = s->m->cfg;
    const int row_bytes = c.head_dim * (s->kv_fp8 ? 1 : (int)esize(c.dtype));
    SD_REQUIRE(row_bytes % 16 == 0, "sd_session_compact_kv: KV rows must be multiples of 16 bytes");
    const int planes = c.n_layers * 2 * c.n_kv_heads;
    hipLaunchKernelGGL(kv_compact_kernel, dim3(planes), dim3(256), (size_t)k * row_bytes, (hipStream_t)stream, s->kv, s->max_seq,
                       row_bytes, base_len, idx_dev, k);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

// Stream-batched forward: the new rows of up to 16 independent sequences go through ONE pass
// over the weights.  Every item names its own session (KV arena), token buffer (device int32, indexed by absolute
// position), cache length pos0, number of new rows and how many of its last rows need logits.  Activations use
// items[0].session's scratch; all sessions must belong to the same model.  Logit rows come out packed in item order.
static int batch_forward(const sd_batch_item *items, int n_items, float *logits_out, long ld_logits, const HeadReq *rq,
                         HeadOut *ho, void *stream) {
    SD_REQUIRE(items && n_items >= 1 && n_items <= SD_MAX_STREAMS, "sd_batch_forward: 1..%d items", SD_MAX_STREAMS);
    sd_session *s0 = items[0].session;
    SD_REQUIRE(s0, "sd_batch_forward: null session");
    RowTab tab = {};
    int rows = 0, nlog = 0, s_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_batch_item &it = items[i];
        SD_REQUIRE(it.session && it.seq && it.session->m == s0->m, "sd_batch_forward: item %d: null or foreign session", i);
        SD_REQUIRE(it.n_new >= 1 && it.pos0 >= 0 && it.n_logits >= 0 && it.n_logits <= it.n_new,
                   "sd_batch_forward: item %d: n_new=%d pos0=%d n_logits=%d", i, it.n_new, it.pos0, it.n_logits);
        if (it.pos0 + it.n_new > it.session->max_seq || rows + it.n_new > std::min(s0->max_rows, SD_MAX_ROWS)) {
            sd_set_error("sd_batch_forward: item %d overflows (rows %d+%d of %d, positions %d of %d)", i, rows, it.n_new,
                         std::min(s0->max_rows, SD_MAX_ROWS), it.pos0 + it.n_new, it.session->max_seq);
            return SD_ERR_CAPACITY;
        }
        SD_REQUIRE(it.session->kv_fp8 == s0->kv_fp8, "sd_batch_forward: item %d: KV arenas of different dtypes", i);
        bind_stream(tab, i, it.session, it.seq);
        for (int r = 0; r < it.n_new; ++r) {
            tab.row_pos[rows + r] = it.pos0 + r;
            tab.row_stream[rows + r] = (unsigned char)i;
        }
        for (int r = 0; r < it.n_logits; ++r) tab.xmap[nlog++] = (unsigned char)(rows + it.n_new - it.n_logits + r);
        rows += it.n_new;
        s_max = std::max(s_max, it.pos0 + it.n_new);
    }
    SD_REQUIRE(nlog == 0 || logits_out, "sd_batch_forward: logits_out is null");
    const int max_logits = nlog == rows ? s0->max_pass_rows : SD_STREAM_MAX_ROWS;   // (as in sd_session_forward)
    if (nlog > max_logits) {
        sd_set_error("sd_batch_forward: %d logit rows of %d exceed one pass (<= %d)", nlog, rows, max_logits);
        return SD_ERR_CAPACITY;
    }
    tab.n_rows = rows;
    tab.n_streams = n_items;
    tab.n_logit_rows = nlog;
    finish_table(tab);
    return run_forward(s0, tab, s_max, logits_out, ld_logits, rq, ho, stream);
}

extern "C" int sd_batch_forward(const sd_batch_item *items, int n_items, float *logits_out, long ld_logits,
                                void *stream) {
    return batch_forward(items, n_items, logits_out, ld_logits, nullptr, nullptr, stream);
}

// Batched prefill (throughput mode): the prompts of several streams through ONE pass over the weights - up to
// SD_MAX_FWD_ROWS rows and SD_MAX_GROUPS attention groups in all, every stream's rows a contiguous run of positions
// (RowTab contig = 2), no logits.  Replaces stream-by-stream prefill passes of the same weights.
extern "C" int sd_batch_prefill(const sd_batch_item *items, int n_items, void *stream) {
    SD_REQUIRE(items && n_items >= 1 && n_items <= SD_MAX_STREAMS, "sd_batch_prefill: 1..%d items", SD_MAX_STREAMS);
    sd_session *s0 = items[0].session;
    SD_REQUIRE(s0, "sd_batch_prefill: null session");
    RowTab tab = {};
    int rows = 0, groups = 0, s_max = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_batch_item &it = items[i];
        SD_REQUIRE(it.session && it.seq && it.session->m == s0->m, "sd_batch_prefill: item %d: null or foreign session", i);
        SD_REQUIRE(it.n_new >= 1 && it.pos0 >= 0 && it.n_logits == 0, "sd_batch_prefill: item %d: n_new=%d pos0=%d n_logits=%d",
                   i, it.n_new, it.pos0, it.n_logits);
        SD_REQUIRE(it.session->kv_fp8 == s0->kv_fp8, "sd_batch_prefill: item %d: KV arenas of different dtypes", i);
        groups += (it.n_new + ATT_TQ - 1) / ATT_TQ;
        if (it.pos0 + it.n_new > it.session->max_seq || rows + it.n_new > std::min(s0->max_rows, SD_MAX_FWD_ROWS) ||
            groups > SD_MAX_GROUPS) {
            sd_set_error("sd_batch_prefill: item %d overflows (rows %d+%d of %d, %d attention groups of %d, positions %d of %d)", i,
                         rows, it.n_new, std::min(s0->max_rows, SD_MAX_FWD_ROWS), groups, SD_MAX_GROUPS, it.pos0 + it.n_new,
                         it.session->max_seq);
            return SD_ERR_CAPACITY;
        }
        bind_stream(tab, i, it.session, it.seq);
        tab.seg_row0[i] = rows;
        tab.seg_pos0[i] = it.pos0;
        rows += it.n_new;
        s_max = std::max(s_max, it.pos0 + it.n_new);
    }
    tab.seg_row0[n_items] = rows;
    tab.contig = 2;
    tab.n_rows = rows;
    tab.n_streams = n_items;
    tab.n_logit_rows = 0;
    finish_table(tab);
    return run_forward(s0, tab, s_max, nullptr, 0, nullptr, nullptr, stream);
}

// ---- standalone weight-streaming GEMM (unit tests + kernel-level roofline runs) --------------
__global__ void reduce_f32_kernel(const float *__restrict__ part, int S, size_t stride_s, int total,
                                  float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    out[i] = reduce_part<float>(part, S, stride_s, (size_t)i, nullptr, 0);
}

extern "C" int sd_pack_activation_bf16(const void *x_rowmajor, void *x_tiled, int M, int K, void *stream) {
    SD_REQUIRE(x_rowmajor && x_tiled && M >= 1 && K >= 32 && K % 32 == 0, "sd_pack_activation_bf16: need M>=1, K%%32==0");
    hipLaunchKernelGGL((to_operand_kernel<bf16_t>), dim3(M), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t *)x_rowmajor, K, (bf16_t *)x_tiled);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

static_assert(SD_GEMM_NONE == GK_NONE && SD_GEMM_STREAM == GK_STREAM && SD_GEMM_STREAM_W16 == GK_STREAM_W16 &&
              SD_GEMM_ROWS == GK_ROWS && SD_GEMM_MM == GK_MM, "specdec.h publishes GemmKind");
static_assert(SD_GN_GATHER == GN_GATHER && SD_GN_ROWMAJOR == GN_ROWMAJOR && SD_GN_FUSED == GN_FUSED && SD_GN_QKV == GN_QKV &&
              SD_GN_ONE_SLAB == GN_ONE_SLAB, "specdec.h publishes GemmNeed");

// The planner's decision for one GEMM, with the kernel instance the launch helpers take for it - by the functions they call
extern "C" int sd_gemm_route(int N, int K, int M, int need, sd_gemm_route_info *out) {
    SD_REQUIRE(out, "sd_gemm_route: null argument");
    SD_REQUIRE(M >= 1 && M <= SD_MAX_FWD_ROWS && N >= 16 && K >= 32 && N % 16 == 0 && K % 32 == 0,
               "sd_gemm_route: need 1<=M<=%d, N%%16==0, K%%32==0", SD_MAX_FWD_ROWS);
    SD_REQUIRE(need >= 0 && need < 32, "sd_gemm_route: need is a set of SD_GN_* bits");
    refresh_env();
    const GemmRoute r = route_gemm(N, K, M, need);
    const int Mpad = (int)align_up(M, 16);
    sd_gemm_route_info o = {};
    o.kind = r.kind; o.S = r.S; o.ksp = r.ksp; o.mtw = r.mtw;
    if (r.kind == GK_STREAM) {
        const StreamInst in = stream_instance(N, K, M, Mpad, r.ksp);
        o.inst_mt = in.MT; o.inst_ntw = in.NTW; o.inst_unroll = in.UNROLL;
    } else if (r.kind == GK_STREAM_W16) {
        o.inst_mt = 1; o.inst_ntw = 1;
    } else if (r.kind == GK_ROWS) {
        const RowsInst in = rows_instance(Mpad, r.rp);
        o.NG = r.rp.NG; o.grid = r.rp.grid; o.nwn = r.rp.nwn; o.nwk = r.rp.nwk; o.nld = r.rp.nld;
        if (in.ok && Mpad / 16 <= in.MT) { o.inst_mt = in.MT; o.inst_ch = in.CH; o.inst_wbm = in.WBM; }
        o.lds_bytes = (int32_t)in.lds;
    } else if (r.kind == GK_MM) {
        const MmInst in = mm_instance(r.mtw);
        o.inst_mt = 4 * in.mtw; o.inst_nt = in.nt; o.lds_bytes = (int32_t)in.lds;
    }
    o.part_floats = r.kind == GK_NONE ? 0 : (uint64_t)r.S * Mpad * N;
    *out = o;
    return SD_OK;
}

extern "C" size_t sd_session_part_floats(const sd_model *m, int max_rows) {
    if (!m) return 0;
    refresh_env();
    return plan_scratch(m->cfg, std::min(max_rows, sd_model_max_rows(m))).part_floats;
}

extern "C" int sd_gemm_bf16_need(const void *w_packed, const void *x, int M, int N, int K, int need, float *part,
                                 size_t part_floats, float *out, int *splits_out, void *stream) {
    SD_REQUIRE(w_packed && x && part, "sd_gemm_bf16: null argument");
    refresh_env();
    SD_REQUIRE(M >= 1 && M <= SD_MAX_FWD_ROWS && N % 16 == 0 && K % 32 == 0,
               "sd_gemm_bf16: need 1<=M<=%d, N%%16==0, K%%32==0", SD_MAX_FWD_ROWS);
    SD_REQUIRE(need >= 0 && need < 32 && !(need & (GN_GATHER | GN_QKV)),
               "sd_gemm_bf16_need: need %d (a row gather needs a row table, the QKV route its epilogue)", need);
    const bool x_tiled = !(need & GN_ROWMAJOR);
    const GemmRoute r = route_gemm(N, K, M, need);
    SD_REQUIRE(r.kind != GK_NONE, "sd_gemm_bf16: more than 64 rows need the tile layout (x_tiled) and N %% 128 == 0");
    const int Mpad = (int)align_up(M, 16);
    SD_REQUIRE((size_t)r.S * Mpad * N <= part_floats, "sd_gemm_bf16: part buffer needs %zu floats", (size_t)r.S * Mpad * N);
    hipStream_t st = (hipStream_t)stream;
    GemmEpi e = {};
    e.x_rowmajor = x_tiled ? 0 : 1;
    if (launch_gemm<EPI_PART>(r, w_packed, x, part, M, N, K, e, st) != SD_OK) return SD_ERR_INVALID;
    if (out) {
        hipLaunchKernelGGL(reduce_f32_kernel, dim3((M * N + 255) / 256), dim3(256), 0, st, part, r.S,
                           (size_t)Mpad * N, M * N, out);
        SD_LAUNCH_CHECK();
    }
    if (splits_out) *splits_out = r.S;
    return SD_OK;
}

extern "C" int sd_gemm_bf16(const void *w_packed, const void *x, int x_tiled, int M, int N, int K, float *part,
                            size_t part_floats, float *out, int *splits_out, void *stream) {
    return sd_gemm_bf16_need(w_packed, x, M, N, K, x_tiled ? 0 : GN_ROWMAJOR, part, part_floats, out, splits_out, stream);
}

// ---- the native decode loops (sd_spec_*, sd_multi_adopt): same translation unit, they use sd_session and the forwards above
#include "spec_loops.h"

// ---- the norm-on-load and the finishing GEMM on 12-bit weight records (forward declarations above launch_gemm_xn's users).
// Last in the file: their kernels are the last of the code object.
static int launch_gemm_xn_w12(sd_session *s, bool qkv, W12Arg W, const void *X, int M, int N, int K, const void *norm_w, float eps,
                              GemmEpiT<bf16_t> e, hipStream_t st) {
    ProfScope ps(s, PC_GEMM, st);
    SD_REQUIRE(M <= 8 && N % 16 == 0 && K % 1024 == 0 && K <= 8192, "norm-on-load GEMM: M=%d N=%d K=%d", M, N, K);
    e.nrm_ssq = s->ssq; e.nrm_w = (const bf16_t *)norm_w; e.nrm_nt = K / 16; e.nrm_eps = eps;
    auto go = [&](auto epi, auto c) {
        hipLaunchKernelGGL((gemm_bf16_stream_xn<decltype(epi)::value, decltype(c)::value, bf16_t, WFetchW12>), dim3(N / 16), dim3(256),
                           (size_t)K * sizeof(bf16_t), st, W, (const bf16_t *)X, (float *)nullptr, M, N, K, 1, K / 32, e);
    };
    auto by_rows = [&](auto epi) {
        using std::integral_constant;
        if (M <= 4) go(epi, integral_constant<int, 4>{});
        else if (M == 5) go(epi, integral_constant<int, 3>{});
        else go(epi, integral_constant<int, 2>{});
    };
    if (qkv) by_rows(std::integral_constant<int, EPI_QKV_ROPE>{});
    else by_rows(std::integral_constant<int, EPI_ACT_SILU>{});
    SD_LAUNCH_CHECK();
    ++s->w12_launches;
    return SD_OK;
}
static int launch_gemm_fin_w12(sd_session *s, const GemmRoute &pl, W12Arg W, const void *X, int M, int N, int K, hipStream_t st) {
    ProfScope ps(s, PC_GEMM, st);
    SD_REQUIRE(pl.kind == GK_STREAM && M <= 16 && (size_t)pl.S * 16 * N <= s->part_floats, "k-split GEMM with residual epilogue: M=%d N=%d K=%d", M, N, K);
    GemmEpiT<bf16_t> e = {};
    e.res_x = (bf16_t *)s->x; e.res_h = (bf16_t *)s->h; e.res_ssq = s->ssq;
    const unsigned want = s->fin_epoch + (unsigned)(pl.S - 1) + (unsigned)s->skew_now;
    hipLaunchKernelGGL((gemm_bf16_stream_fin<bf16_t, WFetchW12>), dim3((N / 16) * pl.S), dim3(256), 0, st, W, (const bf16_t *)X, s->part,
                       M, N, K, pl.S, pl.ksp, e, s->fin_ctr, want, s->wait_status);
    SD_LAUNCH_CHECK();
    s->fin_epoch += (unsigned)(pl.S - 1);
    ++s->w12_launches;
    return SD_OK;
}
extern "C" int sd_pack_weight_w12(const void *w_tiled, void *codes, void *meta, int N, int K, int *status_dev, void *stream) {
    SD_REQUIRE(w_tiled && codes && meta && status_dev && N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0,
               "sd_pack_weight_w12: need N %% 16 == 0 and K %% 32 == 0 (got %d x %d) and no null pointer", N, K);
    SD_REQUIRE(((uintptr_t)codes & 127) == 0 && ((uintptr_t)meta & 15) == 0, "sd_pack_weight_w12: codes must be 128-byte, meta 16-byte aligned");
    SD_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int), (hipStream_t)stream));
    hipLaunchKernelGGL(w12_pack_kernel<0>, dim3((unsigned)((size_t)(N / 16) * (K / 32))), dim3(64), 0, (hipStream_t)stream,
                       (const u32x4 *)w_tiled, (unsigned *)codes, (u32x4 *)meta, status_dev);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
extern "C" int sd_unpack_weight_w12(const void *codes, const void *meta, void *w_tiled, int N, int K, void *stream) {
    SD_REQUIRE(w_tiled && codes && meta && N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0,
               "sd_unpack_weight_w12: need N %% 16 == 0 and K %% 32 == 0 (got %d x %d) and no null pointer", N, K);
    hipLaunchKernelGGL(w12_unpack_kernel<0>, dim3((unsigned)((size_t)(N / 16) * (K / 32))), dim3(64), 0, (hipStream_t)stream,
                       W12Arg{(const unsigned *)codes, (const u32x4 *)meta}, (u32x4 *)w_tiled);
    SD_LAUNCH_CHECK();
    return SD_OK;
}
