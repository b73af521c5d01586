// sampler_host.h - what the host side of sampling.hip shares with the decode loops (engine.hip / spec_loops.h): the request
// of one norm launch, and the entries of sampling.hip that are not in the public header.  Host only.
#pragma once
#include "common.h"

// One norm_logits launch (norm_probs_kernel, behind norm_cand_kernel where a workspace serves it).  Every optional field is
// off when zero-initialised.
struct NormRequest {
    const float *logits;      // input rows: `rows` of them, V columns, row stride ld_in
    int rows, V;
    long ld_in;
    float temperature;        // parameters; mode: SD_NORM_ROUND_* | SD_NORM_DT_*
    int top_k;
    float top_p;
    int mode;
    float *probs_out;         // dense output rows (row stride ld_out) and one error word per row, or NULL
    long ld_out;
    int *err;
    const float *noise;       // the fused sample of a single row, on when tok_out is set: Exp(1) noise, or Philox (seed, draw)
    uint64_t seed, draw;
    int *tok_out, *samp_err;
    int table_sample;         // a batched launch (its row table carries the outputs): every row also draws its token
    void *workspace;          // CandRows of `rows` rows for the two-kernel path
    const float *tile_max;    // the head left tile maxima [rows][V / 16] and cleared the output rows (EPI_HEAD)
    void *lists;              // one CandList per row comes back (sd_cand_list_bytes)
    int filter_only;          // top_k_top_p_filter's result instead of probabilities
    int *route;               // test hook: the rows' route words
    const sd_row_sampling *row_params;   // sd_norm_batch_tiles only: row r is filtered with row_params[r], and temperature /
                                         // top_k / top_p above are not read
};

// norm_logits of rows whose head left tile maxima (or NULL) and cleared probs_out; with tok_out also the sample that follows a
// draft step (rows == 1)
int sd_norm_rows_with_tiles(const NormRequest &rq, void *stream);
// sd_norm_batch on a request: row r of rq.logits goes to rows[r] (rq's own outputs are not read), rq.lists + r receives its list
int sd_norm_batch_tiles(const NormRequest &rq, const sd_norm_row *rows, int sample, void *stream);
// the bytes of the CandRows that lie in front of a workspace's candidate lists
size_t sd_norm_candrow_bytes(int rows);
// sd_resample on Philox with an iteration's error words folded into res->flags bit 3
int sd_resample_with_errors(const float *p_hist, const float *q_hist, long ld, int V, int32_t *seq, int gamma,
                            uint64_t philox_seed, uint64_t draw_index, sd_accept_result *res, const int *err_flags,
                            int n_err, int dtype_mode, void *stream);
