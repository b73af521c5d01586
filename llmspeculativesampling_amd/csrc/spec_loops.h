// spec_loops.h - the native decode loops (single stream, lock-step streams with or without a prompt queue, width-w iid,
// autoregressive streams) and the steps
// they share.  Host code - and the one small kernel of the autoregressive loop's hand-off - included at the end of
// engine.hip, whose sd_session, HeadReq / HeadOut and session_forward / batch_forward it uses; the sampler entries that are
// not public come from sampler_host.h.
#pragma once

// feed seq[from, upto) in chunks of at most max_rows; logits come out for the last n_logits rows, all of them from the
// final call (a chunk never ends inside the logits rows), so that call's output slab can be handed to the norm as is
static int feed_rows(sd_session *ses, const int32_t *seq, int from, int upto, int n_logits, float *logits, long ld,
                     const HeadReq *rq, HeadOut *ho, void *stream) {
    const int first_logit = upto - n_logits;
    int done = from;
    while (done < upto) {
        int m = std::min(ses->max_rows, upto - done);
        if (done < first_logit && done + m > first_logit && done + m < upto) m = first_logit - done;
        const int lo = std::max(first_logit, done);
        const int nl = std::max(0, done + m - lo);
        const int rc = session_forward(ses, seq + done, m, done, nl, nl ? logits + (size_t)(lo - first_logit) * ld : nullptr, ld,
                                       rq, ho, stream);
        if (rc != SD_OK) return rc;
        done += m;
    }
    return SD_OK;
}

// EPI_HEAD's tile maxima serve the top-k candidate search only (1 <= k <= 64, positive temperature, 16 | V >= 4096)
static bool head_tiles_ok(int top_k, float temperature, int V, long ld) {
    return top_k >= 1 && top_k <= 64 && temperature > 0.0f && V % 16 == 0 && V >= 4096 && V <= 65536 && ld % 4 == 0;
}

// The norm launch of a loop's logit rows: the loop's sampling parameters, the rows where the forward left them (their pending
// rounding joins the model's mode) and the head's tile maxima.  The caller adds what differs: the row count, the outputs, the
// draws, the workspace, the lists.
static NormRequest norm_request(const sd_sampling &sm, int mode, const HeadOut &ho) {
    NormRequest rq = {};
    rq.logits = ho.logits; rq.V = sm.V; rq.ld_in = ho.ld;
    rq.temperature = sm.temperature; rq.top_k = sm.top_k; rq.top_p = sm.top_p; rq.mode = ho.round | mode;
    rq.tile_max = ho.tile_max;
    return rq;
}
// ... of a forward that was asked for nothing but its logit rows in the model's scratch
static HeadOut scratch_rows(const sd_head_scratch &h) { return HeadOut{h.logits, h.ld_logits, 0, nullptr}; }

// ---- steps the loops share ------------------------------------------------------------------------------------
// In-loop failure handling of the three native loops: every failure sets `rc` and leaves the loop, so the common epilogue
// (write-back of the in/out cursor state) always runs.
#define SD_LOOP_HIP(expr)                                                                                   \
    if (hipError_t _e = (expr); _e != hipSuccess) {                                                         \
        sd_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);          \
        rc = SD_ERR_HIP;                                                                                    \
        break;                                                                                              \
    }
// Waits for `ev` by polling (a blocking wait parks the thread, and the launches of the next iteration's draft steps - which
// the GPU consumes as fast as they arrive - then start from a cold core); bounded in wall-clock time.
static int poll_event(hipEvent_t ev, const char *who) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return SD_OK;
        if (q != hipErrorNotReady) { sd_set_error("%s: %s", who, hipGetErrorString(q)); return SD_ERR_HIP; }
        if ((spins & 0xfff) == 0xfff &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 60.0) {
            sd_set_error("%s: the iteration's result did not arrive within 60 s", who);
            return SD_ERR_HIP;
        }
    }
}

// The events of one call of a loop: `timing` events for hipEventElapsedTime and the one whose completion ends an
// iteration; destroyed on every way out.
struct LoopEvents {
    hipEvent_t t[4] = {nullptr, nullptr, nullptr, nullptr}, done = nullptr;
    bool ok = true;                                               // false: a creation failed (the error text is set)
    LoopEvents(int timing, const char *who) {
        for (int i = 0; i < timing && ok; ++i) ok = hipEventCreate(&t[i]) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess;
        if (!ok) sd_set_error("%s: hipEventCreate failed", who);
    }
    ~LoopEvents() {
        for (hipEvent_t e : t) if (e) (void)hipEventDestroy(e);
        if (done) (void)hipEventDestroy(done);
    }
    LoopEvents(const LoopEvents &) = delete;                     // (owns its events)
};

// The Philox draws of one iteration of one stream (single-stream and lock-step loops; the width-w loop counts W per step)
struct Draws {
    uint64_t seed_draft, draft0;         // draft step i samples with (seed_draft, draft0 + i)
    uint64_t seed, scan0, resample;      // accept scan and residual / bonus sample
    uint64_t draw;                       // the stream's next draw after this iteration (its seed is `seed`)
};
static Draws next_draws(uint64_t seed, uint64_t draw, int g, uint64_t random_seed) {
    Draws d = {seed, draw};                                       // gamma draft samples, then the discarded target sample
    draw += (uint64_t)g + 1;
    if (random_seed) { seed = random_seed; draw = 0; }            // :1976-1977: the stream restarts before every uniform
    else { d.scan0 = draw; draw += (uint64_t)g; }                 // (under random_seed the scan takes r_const)
    d.seed = seed; d.resample = draw++; d.draw = draw;
    return d;
}

// Draft step i of one stream / replica whose sequence has L tokens and whose draft cache holds draft_len: the uncached
// rows, logits for the last, sampled with (seed, draw) into seq[L + i].  `err` are the stream's 3 * gamma + 1 error words.
static void draft_step_rows(sd_batch_item &it, sd_norm_row &row, sd_session *draft, int32_t *seq, float *q_hist, long ld, int *err,
                            int g, int L, int i, int draft_len, uint64_t seed, uint64_t draw) {
    it.session = draft; it.seq = seq; it.pos0 = draft_len;
    it.n_new = L + i - draft_len; it.n_logits = 1;
    row.probs_out = q_hist + (size_t)(L + i - 1) * ld; row.tok_out = seq + (L + i);
    row.err = err + i; row.sample_err = err + g + i;
    row.exp_noise = nullptr; row.philox_seed = seed; row.draw_index = draw;
}

// The verify rows of one stream / replica: every uncached row of its L + gamma tokens is a logit row; their norm rows are
// appended to `rows` (rows past the gamma-th share the last target error word).
static void verify_pass_rows(sd_batch_item &it, std::vector<sd_norm_row> &rows, sd_session *target, const int32_t *seq, float *p_hist,
                             long ld, int *err, int g, int L, int target_len) {
    const int nn = L + g - target_len;
    it.session = target; it.seq = seq; it.pos0 = target_len;
    it.n_new = nn; it.n_logits = nn;
    for (int r = 0; r < nn; ++r) {
        sd_norm_row row = {};
        row.probs_out = p_hist + (size_t)(L + g - nn + r) * ld;
        row.err = err + 2 * g + std::min(r, g);
        rows.push_back(row);
    }
}

// Log entry `slot` of the acceptance statistics: the gamma target / draft probabilities of the drafted tokens
static void log_ratios(float *p_at_out, float *q_at_out, size_t slot, int g, const float *p_at, const float *q_at) {
    for (int i = 0; i < g; ++i) {
        if (p_at_out) p_at_out[slot * g + i] = p_at[i];
        if (q_at_out) q_at_out[slot * g + i] = q_at[i];
    }
}

// Commits a result block to a sequence of L tokens: the accepted drafts and the next token are appended, both caches
// roll back to n + 1 (speculative_sampling.py:2000, :2015 / 2023; the draft never holds the last drafted token).  A block
// whose resample raised (flags & 2; only the width-w loop commits one) keeps the accepted drafts and nothing else: false.
static bool commit_result(const sd_accept_result &r, int L, int g, int32_t *host_seq, int *len, int *draft_len, int *target_len) {
    for (int i = 0; i < r.n_accepted; ++i) host_seq[(*len)++] = r.drafted[i];
    if (r.flags & 2) return false;
    host_seq[(*len)++] = r.next_token;
    *draft_len = std::min(L + g - 1, r.n + 1);
    *target_len = r.n + 1;
    return true;
}

// ---- per-token target log-probabilities (include/specdec.h has the definition and the loops' contract) -----------
extern "C" int sd_token_logprobs(const sd_logprob_item *items, int n_items, int V, int mode, void *stream) {
    SD_REQUIRE(items, "sd_token_logprobs: null argument");
    SD_REQUIRE(n_items >= 1 && n_items <= LOGPROB_MAX_ITEMS, "sd_token_logprobs: n_items %d outside 1..%d", n_items, LOGPROB_MAX_ITEMS);
    SD_REQUIRE(V >= 1 && (mode & 3) != 3, "sd_token_logprobs: V %d, mode %#x", V, mode);
    LogprobTab t = {};
    int max_rows = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_logprob_item &it = items[i];
        SD_REQUIRE(it.logits && it.tokens && it.out, "sd_token_logprobs: item %d: null argument", i);
        SD_REQUIRE(it.rows >= 1 && it.rows <= LOGPROB_MAX_ROWS, "sd_token_logprobs: item %d: rows %d outside 1..%d", i, it.rows,
                   LOGPROB_MAX_ROWS);
        SD_REQUIRE(it.ld >= V, "sd_token_logprobs: item %d: ld %ld < V %d", i, it.ld, V);
        t.logits[i] = it.logits; t.tokens[i] = it.tokens; t.res[i] = it.res; t.out[i] = it.out; t.ld[i] = it.ld; t.rows[i] = it.rows;
        max_rows = std::max(max_rows, (int)it.rows);
    }
    return launch_token_logprobs(t, n_items, max_rows, V, mode & 3, (hipStream_t)stream);
}

#include "score_entries.h"                                       // sd_score_rows, sd_score_sequence

enum { LP_SLICE = LOGPROB_MAX_ROWS };                             // floats per stream in sd_logprob_block.dev / host
// what the loops refuse in a logprob block (behind the entry's own refusals): n arrays, one per stream / prompt
static int check_logprob_block(const char *who, const sd_logprob_block *lp, int n) {
    SD_REQUIRE(lp->dev && lp->host && lp->logprob_out, "%s: logprobs: null pointer", who);
    for (int i = 0; i < n; ++i) SD_REQUIRE(lp->logprob_out[i], "%s: logprobs: logprob_out[%d] is null", who, i);
    return SD_OK;
}
// The gamma + 1 target rows of a stream whose sequence had L tokens: row r scores seq[L + r], the gamma drafted tokens and,
// at seq[L + n_accepted], the token the resample appended.  `slot`: the stream's slice of the block.
static sd_logprob_item verify_logprob_item(const sd_logprob_block &lp, int slot, const float *logits, long ld, int g,
                                           const int32_t *seq, int L, const sd_accept_result *res_dev) {
    return sd_logprob_item{logits, ld, g + 1, seq + L, res_dev, lp.dev + (size_t)slot * LP_SLICE};
}
// After the wait: the n_accepted + 1 scores of a committed result go where commit_result put its tokens (emitted-token numbers
// first .. first + n_accepted)
static void commit_logprobs(const sd_logprob_block &lp, int slot, float *out, int first, const sd_accept_result &r) {
    for (int i = 0; i <= r.n_accepted; ++i) out[first + i] = lp.host[(size_t)slot * LP_SLICE + i];
}

// ---- per-request penalties (include/specdec.h has the definition and the loops' contract) ------------------------
static bool penalty_neutral(const sd_penalty &p) { return p.repetition == 1.0f && p.frequency == 0.0f && p.presence == 0.0f; }
// what every entry refuses in a parameter triple (`what` names it: "item", "stream", "prompt")
static int check_penalty(const char *who, const char *what, int i, const sd_penalty &p) {
    SD_REQUIRE(std::isfinite(p.repetition) && std::isfinite(p.frequency) && std::isfinite(p.presence),
               "%s: %s %d: penalties (%g, %g, %g) must be finite", who, what, i, p.repetition, p.frequency, p.presence);
    SD_REQUIRE(p.repetition > 0.0f, "%s: %s %d: repetition penalty %g must be > 0", who, what, i, p.repetition);
    return SD_OK;
}

// What sd_penalize_rows and sd_edit_rows share: the call's own refusals ...
static int check_row_edit_call(const char *who, const void *items, int n_items, int V, int mode) {
    SD_REQUIRE(items, "%s: null argument", who);
    SD_REQUIRE(n_items >= 1 && n_items <= PEN_MAX_ITEMS, "%s: n_items %d outside 1..%d", who, n_items, PEN_MAX_ITEMS);
    SD_REQUIRE(V >= 1 && V <= 65536 && (mode & 3) != 3, "%s: V %d outside 1..65536, or both rounding bits (mode %#x)", who, V, mode);
    return SD_OK;
}
// ... and item i, refused or put into its column of the table (sd_logit_edit_item starts with sd_penalty_item's fields)
template <class Item>
static int penalty_tab_item(const char *who, PenaltyTab &t, int i, const Item &it, int V, int *max_rows) {
    SD_REQUIRE(it.in && it.out && it.seq, "%s: item %d: null argument", who, i);
    SD_REQUIRE(it.rows >= 1 && it.rows <= PEN_MAX_ROWS, "%s: item %d: rows %d outside 1..%d", who, i, it.rows, PEN_MAX_ROWS);
    SD_REQUIRE(it.ld_in >= V && it.ld_out >= V, "%s: item %d: ld %ld / %ld < V %d", who, i, it.ld_in, it.ld_out, V);
    SD_REQUIRE(it.hist0 >= 1 && it.prompt_len >= 0, "%s: item %d: hist0 %d < 1 or prompt_len %d < 0", who, i, it.hist0, it.prompt_len);
    if (int rc = check_penalty(who, "item", i, it.pen); rc != SD_OK) return rc;
    t.in[i] = it.in; t.out[i] = it.out; t.seq[i] = it.seq; t.ld_in[i] = it.ld_in; t.ld_out[i] = it.ld_out;
    t.rows[i] = it.rows; t.hist0[i] = it.hist0; t.prompt_len[i] = it.prompt_len;
    t.repetition[i] = it.pen.repetition; t.frequency[i] = it.pen.frequency; t.presence[i] = it.pen.presence;
    *max_rows = std::max(*max_rows, (int)it.rows);
    return SD_OK;
}

extern "C" int sd_penalize_rows(const sd_penalty_item *items, int n_items, int V, int mode, void *stream) {
    if (int rc = check_row_edit_call("sd_penalize_rows", items, n_items, V, mode); rc != SD_OK) return rc;
    PenaltyTab t = {};
    int max_rows = 0;
    for (int i = 0; i < n_items; ++i)
        if (int rc = penalty_tab_item("sd_penalize_rows", t, i, items[i], V, &max_rows); rc != SD_OK) return rc;
    return launch_penalize_rows(t, n_items, max_rows, V, mode, (hipStream_t)stream);
}

// what the loops refuse in a penalty block (behind the entry's own refusals): n triples, one per `what`, and a slab of at
// least need_rows rows.  *pb becomes NULL when every triple is neutral: the call is then the call without a block.
static int check_penalty_block(const char *who, const char *what, const sd_penalty_block **pb, int n, int V, int need_rows) {
    const sd_penalty_block *b = *pb;
    SD_REQUIRE(b->rows && b->params, "%s: penalties: null pointer", who);
    SD_REQUIRE(b->ld >= V, "%s: penalties: ld %ld < V %d", who, b->ld, V);
    SD_REQUIRE(b->max_rows >= need_rows, "%s: penalties: a slab of %d rows, the largest pass has %d", who, b->max_rows, need_rows);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (int rc = check_penalty(who, what, i, b->params[i]); rc != SD_OK) return rc;
        any = any || !penalty_neutral(b->params[i]);
    }
    if (!any) *pb = nullptr;
    return SD_OK;
}

// ---- per-request logit bias, allowed mask and min_tokens (include/specdec.h has the definition and the loops' contract) ----
static bool edit_neutral(const sd_logit_edit &e) { return e.n_bias == 0 && !e.allowed && e.min_tokens == 0; }
static int check_edit(const char *who, const char *what, int i, const sd_logit_edit &e) {
    SD_REQUIRE(e.n_bias >= 0 && e.n_bias <= SD_EDIT_MAX_BIAS, "%s: %s %d: n_bias %d outside 0..%d", who, what, i, e.n_bias, SD_EDIT_MAX_BIAS);
    SD_REQUIRE(e.n_bias == 0 || (e.bias_ids && e.bias_vals), "%s: %s %d: %d bias entries and a null array", who, what, i, e.n_bias);
    SD_REQUIRE(e.min_tokens >= 0, "%s: %s %d: min_tokens %d < 0", who, what, i, e.min_tokens);
    return SD_OK;
}

// item i's edits in their columns of the table
static void edit_tab_item(EditTab &e, int i, const sd_logit_edit_item &it) {
    e.bias_ids[i] = it.edit.bias_ids; e.bias_vals[i] = it.edit.bias_vals; e.n_bias[i] = it.edit.n_bias;
    e.allowed[i] = it.edit.allowed; e.min_tokens[i] = it.edit.min_tokens; e.eos[i] = it.eos_token_id;
}

extern "C" int sd_edit_rows(const sd_logit_edit_item *items, int n_items, int V, int mode, void *stream) {
    if (int rc = check_row_edit_call("sd_edit_rows", items, n_items, V, mode); rc != SD_OK) return rc;
    EditTab e = {};
    int max_rows = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_logit_edit_item &it = items[i];
        if (int rc = penalty_tab_item("sd_edit_rows", e.pen, i, it, V, &max_rows); rc != SD_OK) return rc;
        if (int rc = check_edit("sd_edit_rows", "item", i, it.edit); rc != SD_OK) return rc;
        edit_tab_item(e, i, it);
    }
    return launch_edit_rows(e, n_items, max_rows, V, mode, (hipStream_t)stream);
}

// ---- grammar-constrained decoding (include/specdec.h has the definition and the loops' contract) ------------------------
extern "C" int sd_grammar_rows(const sd_grammar_item *items, int n_items, int V, int mode, void *stream) {
    const char *const who = "sd_grammar_rows";
    if (int rc = check_row_edit_call(who, items, n_items, V, mode); rc != SD_OK) return rc;
    GrammarTab g = {};
    int max_rows = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_logit_edit_item &it = items[i].row;
        if (int rc = penalty_tab_item(who, g.edit.pen, i, it, V, &max_rows); rc != SD_OK) return rc;
        if (int rc = check_edit(who, "item", i, it.edit); rc != SD_OK) return rc;
        edit_tab_item(g.edit, i, it);
    }
    for (int i = 0; i < n_items; ++i) {
        const sd_grammar *gr = items[i].grammar;
        if (!gr) continue;                                        // edited exactly as sd_edit_rows edits it
        char what[32];
        snprintf(what, sizeof what, "item %d: grammar", i);
        if (int rc = check_grammar(who, what, *gr, items[i].states, V); rc != SD_OK) return rc;
        g.masks[i] = gr->masks; g.next[i] = gr->next; g.cls[i] = gr->cls; g.states[i] = items[i].states;
        g.n_states[i] = gr->n_states; g.n_classes[i] = gr->n_classes; g.start[i] = gr->start;
    }
    return launch_grammar_rows(g, n_items, max_rows, V, mode, (hipStream_t)stream);
}
static bool has_grammar(const sd_session *t) { return t && t->gram.masks; }
// what the loops refuse in the grammars of their n streams' target sessions (behind opts): a state cache that is smaller than
// the output positions the call can reach, need[i] for `what` i
static int check_grammar_states(const char *who, const char *what, const sd_session *const *ses, int n, const int *need) {
    for (int i = 0; i < n; ++i)
        SD_REQUIRE(!has_grammar(ses[i]) || ses[i]->gram_cap >= need[i],
                   "%s: grammar: %s %d: states_cap %d is smaller than the %d output positions the call can reach (T - P + gamma + 2)",
                   who, what, i, ses[i]->gram_cap, need[i]);
    return SD_OK;
}

// what the loops refuse in an edit block, as check_penalty_block does; *eb becomes NULL when every record is neutral
static int check_edit_block(const char *who, const char *what, const sd_logit_edit_block **eb, int n, int V, int need_rows) {
    const sd_logit_edit_block *b = *eb;
    SD_REQUIRE(b->rows && b->params, "%s: edits: null pointer", who);
    SD_REQUIRE(b->ld >= V, "%s: edits: ld %ld < V %d", who, b->ld, V);
    SD_REQUIRE(b->max_rows >= need_rows, "%s: edits: a slab of %d rows, the largest pass has %d", who, b->max_rows, need_rows);
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (int rc = check_edit(who, what, i, b->params[i]); rc != SD_OK) return rc;
        any = any || !edit_neutral(b->params[i]);
    }
    if (!any) *eb = nullptr;
    return SD_OK;
}

// What a loop edits its logit rows by: the penalty block, the edit block or both, as ONE slab and two parameter tables, of
// which either may be absent (NULL: neutral for everyone).  With an edit table the pass's launch is sd_edit_rows into the
// edit block's slab, without one sd_penalize_rows into the penalty block's.
struct RowEdits {
    float *rows; long ld; int max_rows;
    const sd_penalty *pen;
    const sd_logit_edit *edit;
    int eos;
    bool grammar;                                                 // a stream of the call has a grammar: its passes are edited passes
    // request k, decoding on target session t
    bool edited(int k, const sd_session *t) const {
        return (pen && !penalty_neutral(pen[k])) || (edit && !edit_neutral(edit[k])) || (grammar && has_grammar(t));
    }
};

// what the lock-step loops refuse in a parameter array (`what` names its entries: "stream", "prompt")
static int check_row_params(const char *who, const char *what, const sd_row_sampling *params, int n) {
    for (int i = 0; i < n; ++i) {
        SD_REQUIRE(params[i].temperature != 0.0f, "%s: %s %d: temperature must be non-zero", who, what, i);
        SD_REQUIRE(params[i].top_k >= 0, "%s: %s %d: top_k %d is negative", who, what, i, params[i].top_k);
    }
    return SD_OK;
}

// An entry's sd_loop_opts as its loop reads them: every member NULL when the call carries nothing of the kind.
struct LoopOpts {
    const sd_row_sampling *params = nullptr;                      // per stream - with a queue, per prompt (NULL: sm's triple for everyone)
    const sd_logprob_block *lp = nullptr;
    RowEdits re_block;
    const RowEdits *re = nullptr;                                 // &re_block, or NULL when nothing is left to edit
};
// Checks `opts` (NULL: four NULL members) behind the entry's own refusals - row_params, logprobs, penalties, edits, in that
// order - and resolves it into *o.  n: the streams / prompts (`what`) the members are indexed by; need_rows: the logit rows of
// the loop's largest pass; the two loops that sample with sm's own triple pass row_params_allowed = false.
// ses: the n_ses target sessions of the call's streams (entries may be NULL); one of them with a grammar keeps the edit block
// in use whatever its records hold, and is refused without one.
static int resolve_loop_opts(const char *who, const char *what, const sd_loop_opts *opts, int n, int V, int need_rows, int eos,
                             bool row_params_allowed, LoopOpts *o, const sd_session *const *ses, int n_ses) {
    int gram = -1;
    for (int i = n_ses - 1; i >= 0; --i)
        if (has_grammar(ses[i])) gram = i;
    if (!opts) {
        SD_REQUIRE(gram < 0, "%s: grammar: the target session of stream %d has a grammar but opts->edits is NULL: the masked rows need "
                   "the edit block's slab (a block of neutral records is enough)", who, gram);
        return SD_OK;
    }
    if (opts->row_params) {
        SD_REQUIRE(row_params_allowed, "%s: row_params: this loop samples with sampling's own triple", who);
        if (int rc = check_row_params(who, what, opts->row_params, n); rc != SD_OK) return rc;
    }
    if (opts->logprobs)
        if (int rc = check_logprob_block(who, opts->logprobs, n); rc != SD_OK) return rc;
    const sd_penalty_block *pb = opts->penalties;
    const sd_logit_edit_block *eb = opts->edits;
    if (pb)
        if (int rc = check_penalty_block(who, what, &pb, n, V, need_rows); rc != SD_OK) return rc;
    if (eb)
        if (int rc = check_edit_block(who, what, &eb, n, V, need_rows); rc != SD_OK) return rc;
    SD_REQUIRE(gram < 0 || opts->edits, "%s: grammar: the target session of stream %d has a grammar but opts->edits is NULL: the masked "
               "rows need the edit block's slab (a block of neutral records is enough)", who, gram);
    if (gram >= 0) eb = opts->edits;                              // (neutral records or not)
    o->params = opts->row_params; o->lp = opts->logprobs;
    if (eb) o->re_block = RowEdits{eb->rows, eb->ld, eb->max_rows, pb ? pb->params : nullptr, eb->params, eos, gram >= 0};
    else if (pb) o->re_block = RowEdits{pb->rows, pb->ld, pb->max_rows, pb->params, nullptr, eos, false};
    if (pb || eb) o->re = &o->re_block;
    return SD_OK;
}
// The item of stream / prompt `k`'s `rows` logit rows, the first at position `pos`: packed from row `r0` of the pass's raw
// rows `src` and of the slab
static sd_logit_edit_item edit_item(const RowEdits &re, int k, const HeadOut &src, int r0, int rows, const int32_t *seq, int pos,
                                    int prompt_len) {
    return sd_logit_edit_item{src.logits + (size_t)r0 * src.ld, re.rows + (size_t)r0 * re.ld, src.ld, re.ld, rows, seq, pos + 1, prompt_len,
                              re.pen ? re.pen[k] : sd_penalty{1.0f, 0.0f, 0.0f},
                              re.edit ? re.edit[k] : sd_logit_edit{nullptr, nullptr, 0, nullptr, 0}, re.eos};
}
// The one launch of an edited pass over its n items; ses[j]: the target session of item j's stream.  A pass that holds a
// stream with a grammar takes sd_grammar_rows, every other pass the launch it took before grammars existed.
static int edit_rows(const RowEdits &re, const sd_logit_edit_item *items, int n, int V, int mode, void *stream,
                     const sd_session *const *ses) {
    bool gram = false;
    for (int j = 0; re.grammar && j < n; ++j) gram = gram || has_grammar(ses[j]);
    if (gram) {
        sd_grammar_item gi[PEN_MAX_ITEMS];
        for (int j = 0; j < n && j < PEN_MAX_ITEMS; ++j)
            gi[j] = sd_grammar_item{items[j], has_grammar(ses[j]) ? &ses[j]->gram : nullptr, ses[j] ? ses[j]->gram_states : nullptr};
        return sd_grammar_rows(gi, n, V, mode, stream);
    }
    if (re.edit) return sd_edit_rows(items, n, V, mode, stream);
    sd_penalty_item pi[PEN_MAX_ITEMS];
    for (int j = 0; j < n && j < PEN_MAX_ITEMS; ++j) {
        const sd_logit_edit_item &it = items[j];
        pi[j] = sd_penalty_item{it.in, it.out, it.ld_in, it.ld_out, it.rows, it.seq, it.hist0, it.prompt_len, it.pen};
    }
    return sd_penalize_rows(pi, n, V, mode, stream);
}
// The norm request of an edited pass reads the slab: already rounded, no tile maxima
static void norm_from_edited(NormRequest &nr, const RowEdits &re) {
    nr.logits = re.rows; nr.ld_in = re.ld; nr.mode &= ~3; nr.tile_max = nullptr;
}

// What drafts an iteration's gamma tokens when no draft model does (NULL in a loop: the draft model's gamma steps): one
// sd_lookup_propose launch over the active streams.  The proposer's two info ints of stream i are at info + 2 * i, behind
// the streams' result blocks, and ride along in the iteration's one copy.
struct LookupDraft {
    int ngram_max, ngram_min;
    int32_t *info_dev;
    const int32_t *info_host;
    int32_t *const *match_len_out;                                // one array per stream; NULL, or a NULL array: not logged
    // after the wait: the match length of stream `slot`'s iteration number `call`
    void log_match(int slot, int call) const {
        if (match_len_out && match_len_out[slot]) match_len_out[slot][call] = info_host[2 * slot];
    }
};
// p - q, max_fn and the draw of the accept / resample are in the rows' dtype when both models keep 16-bit rows; a lookup
// draft's one-hot rows go with the target's
static int accept_mode(const sd_spec_scratch &sc, const LookupDraft *lookup) {
    return lookup || sc.target.norm_mode == sc.draft.norm_mode ? sc.target.norm_mode : 0;
}

// ---- one whole speculative iteration, enqueued natively ---------------------------------------
// reference sampling/speculative_sampling.py:1934-2031 for the device-RNG mode: gamma x (draft forward +
// norm_sample) - draft_steps, or one proposer launch -, then verify_half: one target forward over the uncached rows +
// norm_probs, accept scan, residual / bonus sample, and the 208-byte result block is copied to pinned host memory.  Nothing
// here synchronises; single_stream_loop waits on the stream once per iteration.
//
// The draft model's half: gamma steps; the sampled token goes straight into seq[] where the next step's embed reads it
static int draft_steps(const sd_spec_stream &dv, int g, const sd_sampling &sm, const sd_spec_scratch &sc, const Draws &d, int L,
                       int draft_len, void *stream, const RowEdits *re, int prompt_len) {
    int rc;
    const bool tiles_ok = !re && head_tiles_ok(sm.top_k, sm.temperature, sm.V, sm.ld);   // (an edited pass takes no tile maxima)
    int *const err = dv.err_words;     // [0..gamma) norm err of draft rows, [gamma..2gamma) sample err, [2gamma..3gamma+1) target rows
    HeadReq rq = {};
    HeadOut ho = {};
    rq.raw = true; rq.zero_ld = sm.ld;                           // (zero_rows: per forward, below)
    for (int i = 0; i < g; ++i) {
        const int upto = L + i;
        float *q_row = dv.q_hist + (size_t)(upto - 1) * sm.ld;
        rq.zero_rows = tiles_ok ? q_row : nullptr;                   // the head clears the row and leaves tile maxima
        if ((rc = feed_rows(dv.draft, dv.seq, draft_len, upto, 1, sc.draft.logits, sc.draft.ld_logits, &rq, &ho, stream)) != SD_OK)
            return rc;
        draft_len = upto;
        NormRequest nr = norm_request(sm, sc.draft.norm_mode, ho);
        if (re) {                                                 // the row at position upto - 1, edited out of place
            const sd_logit_edit_item it = edit_item(*re, 0, ho, 0, 1, dv.seq, upto - 1, prompt_len);
            const sd_session *const ts = dv.target;
            if ((rc = edit_rows(*re, &it, 1, sm.V, nr.mode, stream, &ts)) != SD_OK) return rc;
            norm_from_edited(nr, *re);
        }
        nr.rows = 1; nr.probs_out = q_row; nr.ld_out = sm.ld; nr.err = err + i;
        nr.seed = d.seed_draft; nr.draw = d.draft0 + (uint64_t)i; nr.tok_out = dv.seq + upto; nr.samp_err = err + g + i;
        nr.workspace = sc.norm_workspace;
        if ((rc = sd_norm_rows_with_tiles(nr, stream)) != SD_OK) return rc;
    }
    return SD_OK;
}

// The verify half of an iteration: seq[L .. L + gamma) and the q rows
// L-1 .. L+gamma-2 are where the draft half (gamma draft steps, or one proposer launch) left them.  One target forward over
// the uncached rows, the edits, the norm launch, accept scan + residual / bonus sample in `res_mode`, the log-prob launch,
// and the copy of `res_bytes` from the result block (what follows the block rides along).  Timed: ev.t[2] .. t[3] around the
// forward and the norm.
static int verify_half(const sd_spec_stream &dv, int g, const sd_sampling &sm, const sd_spec_scratch &sc, const Draws &d,
                       int L, int target_len, const float *r_const, int res_mode, size_t res_bytes, const LoopEvents &ev, bool timed,
                       void *stream, const LoopOpts &o, int prompt_len) {
    const sd_logprob_block *const lp = o.lp;
    const RowEdits *const re = o.re;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    const bool tiles_ok = !re && head_tiles_ok(sm.top_k, sm.temperature, sm.V, sm.ld);   // (an edited pass takes no tile maxima)
    int *const err = dv.err_words;
    HeadReq rq = {};
    HeadOut ho = {};
    rq.raw = true; rq.zero_ld = sm.ld;
    if (timed) SD_HIP_CHECK(hipEventRecord(ev.t[2], st));
    // the target rows' candidate lists (behind the CandRows of the workspace) let the residual / bonus sample skip its
    // passes over V; they exist when all gamma + 1 rows of this iteration are normalised here
    void *lists = nullptr;
    // ---- target: every uncached row in one pass (the whole prompt on the first call), logits for the last gamma+1
    {
        const int upto = L + g;
        const int rows = std::min(upto - target_len, g + 1);
        if (sc.norm_workspace && rows == g + 1) lists = (char *)sc.norm_workspace + sd_norm_candrow_bytes(g + 1);
        float *p_rows = dv.p_hist + (size_t)(upto - rows) * sm.ld;
        rq.zero_rows = tiles_ok ? p_rows : nullptr;
        if ((rc = feed_rows(dv.target, dv.seq, target_len, upto, rows, sc.target.logits, sc.target.ld_logits, &rq, &ho, stream)) != SD_OK)
            return rc;
        NormRequest nr = norm_request(sm, sc.target.norm_mode, ho);
        if (re) {
            const sd_logit_edit_item it = edit_item(*re, 0, ho, 0, rows, dv.seq, upto - rows, prompt_len);
            const sd_session *const ts = dv.target;
            if ((rc = edit_rows(*re, &it, 1, sm.V, nr.mode, stream, &ts)) != SD_OK) return rc;
            norm_from_edited(nr, *re);
        }
        nr.rows = rows; nr.probs_out = p_rows; nr.ld_out = sm.ld; nr.err = err + 2 * g;
        nr.workspace = sc.norm_workspace; nr.lists = lists;
        if ((rc = sd_norm_rows_with_tiles(nr, stream)) != SD_OK) return rc;
    }
    if (timed) SD_HIP_CHECK(hipEventRecord(ev.t[3], st));
    // ---- accept scan + residual / bonus sample
    if (lists) {
        if ((rc = sd_accept_resample(dv.p_hist, dv.q_hist, sm.ld, sm.V, dv.seq, L, g, r_const, d.seed, d.scan0, d.resample, dv.res_dev,
                                     err, 3 * g + 1, res_mode, lists, st)) != SD_OK)
            return rc;
    } else {
        if ((rc = sd_accept_scan(dv.p_hist, dv.q_hist, sm.ld, dv.seq, L, g, r_const, d.seed, d.scan0, dv.res_dev, stream)) != SD_OK)
            return rc;
        if ((rc = sd_resample_with_errors(dv.p_hist, dv.q_hist, sm.ld, sm.V, dv.seq, g, d.seed, d.resample, dv.res_dev, err, 3 * g + 1,
                                          res_mode, stream)) != SD_OK)
            return rc;
    }
    if (lp) {                                                     // `ho` is the target's: its gamma + 1 rows where the head left them
        const sd_logprob_item it = verify_logprob_item(*lp, 0, ho.logits, ho.ld, g, dv.seq, L, dv.res_dev);
        if ((rc = sd_token_logprobs(&it, 1, sm.V, ho.round | sc.target.norm_mode, stream)) != SD_OK) return rc;
        SD_HIP_CHECK(hipMemcpyAsync(lp->host, lp->dev, sizeof(float) * (size_t)(g + 1), hipMemcpyDeviceToHost, st));
    }
    SD_HIP_CHECK(hipMemcpyAsync(dv.res_host, dv.res_dev, res_bytes, hipMemcpyDeviceToHost, st));
    return SD_OK;
}

// The loop of one stream: per iteration the draft half (the draft model's gamma steps, or `lookup`'s one launch), the verify
// half, one wait, the commit.  `who`: the entry that was called.  Timed: the draft phase is ev.t[0] .. t[1], the verify
// phase ev.t[2] .. t[3].  With `lookup` there is no draft session: s->draft_len is neither read nor written.
static int single_stream_loop(const char *who, const sd_spec_stream &dv, int g, const sd_sampling &sm, const sd_spec_scratch &sc,
                              sd_seq_state *s, uint64_t random_seed, const float *r_const, void *stream, const LoopOpts &o,
                              const LookupDraft *lookup) {
    hipStream_t st = (hipStream_t)stream;
    const int L0 = s->len;
    const bool timed = s->draft_ms_out || s->target_ms_out;
    LoopEvents ev(timed ? 4 : 0, who);
    if (!ev.ok) return SD_ERR_HIP;
    const int res_mode = accept_mode(sc, lookup);
    const size_t res_bytes = sizeof(sd_accept_result) + (lookup ? 2 * sizeof(int32_t) : 0);
    int eos_total = s->ori_eos_cnt, no_draft_len = 0;
    int *const draft_len = lookup ? &no_draft_len : &s->draft_len;
    s->n_iters = s->err = 0;
    int rc = SD_OK;
    while (s->len < s->T && s->n_iters < s->max_iters) {
        const int L = s->len, iters = s->n_iters;
        if (lookup) SD_REQUIRE(L >= 1 && s->target_len >= 0 && s->target_len < L + g, "%s: L=%d target_len=%d", who, L, s->target_len);
        // (a lookup iteration leaves draws d .. d + gamma unread - no draft samples, no discarded target sample: one layout)
        const Draws d = next_draws(s->seed, s->draw, g, random_seed);
        s->seed = d.seed; s->draw = d.draw;
        if (!lookup) {                                            // (refused with the draws taken)
            SD_REQUIRE(L >= 1 && *draft_len >= 0 && *draft_len < L && s->target_len >= 0 && s->target_len < L + g,
                       "%s: L=%d draft_len=%d target_len=%d", who, L, *draft_len, s->target_len);
            SD_REQUIRE(!o.lp || s->target_len <= L - 1, "%s: logprobs: target_len %d of %d tokens leaves fewer than gamma + 1 target rows",
                       who, s->target_len, L);
        }
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[0], st));
        if (lookup) {
            const sd_lookup_item item = {dv.seq, L, dv.q_hist, lookup->info_dev};
            rc = sd_lookup_propose(&item, 1, sm.V, sm.ld, g, lookup->ngram_max, lookup->ngram_min, stream);
        } else {
            rc = draft_steps(dv, g, sm, sc, d, L, *draft_len, stream, o.re, L0);
        }
        if (rc != SD_OK) break;
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[1], st));
        if ((rc = verify_half(dv, g, sm, sc, d, L, s->target_len, r_const, res_mode, res_bytes, ev, timed, stream, o, L0)) != SD_OK) break;
        SD_LOOP_HIP(hipEventRecord(ev.done, st));
        if ((rc = poll_event(ev.done, who)) != SD_OK) break;
        const sd_accept_result r = *dv.res_host;
        if (r.flags & 2) { s->err = 1; break; }
        if (r.flags & 8) {                                        // which word: a draft sample error (a draft model's only), or a norm error
            bool samp = false;
            if (!lookup) {
                std::vector<int> ew(3 * g + 1);
                SD_LOOP_HIP(hipMemcpy(ew.data(), dv.err_words, sizeof(int) * ew.size(), hipMemcpyDeviceToHost));
                for (int i = g; i < 2 * g; ++i) samp = samp || ew[i] != 0;
            }
            s->err = samp ? 1 : 2;
            // a NaN row may be the poison of a timed-out in-launch wait (fused_kernels.h / normload_kernels.h): say so
            unsigned wd = 0, wt = 0;
            if ((lookup || hipMemcpy(&wd, dv.draft->wait_status, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess) &&
                hipMemcpy(&wt, dv.target->wait_status, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess && (wd | wt)) {
                if (lookup)
                    sd_set_error("%s: a fused launch's in-launch wait timed out (status target %#x; sd_session_fused_status): its rows "
                                 "were poisoned with NaN", who, wt);
                else
                    sd_set_error("%s: a fused launch's in-launch wait timed out (status draft %#x, target %#x; "
                                 "sd_session_fused_status): its rows were poisoned with NaN", who, wd, wt);
            }
            break;
        }
        if (timed) {
            float dms = 0.f, tms = 0.f;
            SD_LOOP_HIP(hipEventElapsedTime(&dms, ev.t[0], ev.t[1]));
            SD_LOOP_HIP(hipEventElapsedTime(&tms, ev.t[2], ev.t[3]));
            if (s->draft_ms_out) s->draft_ms_out[iters] = dms;
            if (s->target_ms_out) s->target_ms_out[iters] = tms;
        }
        const int l = r.n_accepted, n = r.n;
        if (s->acc_len_out) s->acc_len_out[iters] = l;
        if (lookup) lookup->log_match(0, iters);
        log_ratios(s->p_at_out, s->q_at_out, (size_t)iters, g, r.p_at, r.q_at);
        ++s->n_iters;
        if (!(n >= L - 1 && l >= 0 && l <= g)) {
            sd_set_error("%s: inconsistent result block (n %d, L %d, accepted %d)", who, n, L, l);
            rc = SD_ERR_INVALID;
            break;
        }
        commit_result(r, L, g, s->host_seq, &s->len, draft_len, &s->target_len);          // (flags & 2 left the loop above)
        if (o.lp) commit_logprobs(*o.lp, 0, o.lp->logprob_out[0], L - L0, r);
        for (int i = L; i < s->len; ++i) eos_total += s->host_seq[i] == sm.eos_token_id;
        if (eos_total > s->ori_eos_cnt) break;                    // the caller cuts after the first new EOS (:2033-2041)
    }
    return rc;
}

// The device-RNG loop without the interpreter between iterations (reference speculative_sampling.py:1934-2046).
extern "C" int sd_spec_generate(const sd_spec_stream *dev, int gamma, const sd_sampling *sampling, const sd_spec_scratch *scratch,
                                sd_seq_state *s, uint64_t random_seed, const float *r_const, void *stream, const sd_loop_opts *opts) {
    SD_REQUIRE(dev && sampling && scratch && s && dev->draft && dev->target && dev->seq && dev->q_hist && dev->p_hist &&
               dev->err_words && dev->res_dev && dev->res_host && s->host_seq && scratch->draft.logits && scratch->target.logits,
               "sd_spec_generate: null argument");
    SD_REQUIRE(gamma >= 1 && gamma <= 16, "sd_spec_generate: gamma %d outside 1..16", gamma);
    SD_REQUIRE(!random_seed || r_const, "sd_spec_generate: random_seed needs its uniform (r_const)");
    const sd_sampling &sm = *sampling;
    SD_REQUIRE(sm.temperature != 0.0f, "sd_spec_generate: temperature must be non-zero");
    SD_REQUIRE(!scratch->norm_workspace || scratch->max_rows_per_forward >= gamma + 1,
               "sd_spec_generate: a norm workspace of %d rows, the target's gamma %d + 1 rows keep their lists there",
               scratch->max_rows_per_forward, gamma);
    SD_REQUIRE(sm.V == dev->draft->m->cfg.vocab && sm.V == dev->target->m->cfg.vocab && sm.ld >= sm.V,
               "sd_spec_generate: V %d (ld %ld), the models' vocabularies are %d / %d", sm.V, sm.ld, dev->draft->m->cfg.vocab,
               dev->target->m->cfg.vocab);
    LoopOpts o;
    const sd_session *const ts = dev->target;
    if (int rc = resolve_loop_opts("sd_spec_generate", "stream", opts, 1, sm.V, gamma + 1, sm.eos_token_id, false, &o, &ts, 1); rc != SD_OK)
        return rc;
    const int states_need = s->T - s->len + gamma + 2;
    if (int rc = check_grammar_states("sd_spec_generate", "stream", &ts, 1, &states_need); rc != SD_OK) return rc;
    SD_REQUIRE(!has_grammar(ts) || s->target_len <= s->len - 1, "sd_spec_generate: grammar: target_len %d of %d tokens: the first "
               "verify pass must start at the prompt's last row", s->target_len, s->len);
    refresh_env();
    return single_stream_loop("sd_spec_generate", *dev, gamma, sm, *scratch, s, random_seed, r_const, stream, o, nullptr);
}

// ---- the prompt queue of the lock-step loop ---------------------------------------------------------------------
// The passes of one draft step or one verify (include/specdec.h has the contract): whole active streams per pass, then the
// joiners' rows where a pass has room.  Host only; lockstep_loop calls it for every step it enqueues.
extern "C" int sd_spec_queue_plan(int row_budget, int mixed_logit_limit, const int32_t *act_rows, int n_act, int logit_rows,
                                  const int32_t *join_rows, int n_join, int prefill_chunk, int force_progress,
                                  sd_queue_pass *passes, int max_passes, sd_queue_chunk *chunks, int max_chunks,
                                  int *n_passes_out, int *n_chunks_out) {
    SD_REQUIRE(passes && chunks && n_passes_out && n_chunks_out, "sd_spec_queue_plan: null argument");
    SD_REQUIRE(row_budget >= 1 && mixed_logit_limit >= 0 && prefill_chunk >= 0, "sd_spec_queue_plan: row_budget %d, logit limit %d, "
               "prefill_chunk %d", row_budget, mixed_logit_limit, prefill_chunk);
    SD_REQUIRE(n_act >= 0 && n_act <= SD_MAX_STREAMS && n_join >= 0 && n_join <= SD_MAX_STREAMS && (n_act == 0 || act_rows) &&
               (n_join == 0 || join_rows), "sd_spec_queue_plan: 0..%d active streams and joiners", SD_MAX_STREAMS);
    for (int j = 0; j < n_act; ++j) SD_REQUIRE(act_rows[j] >= 1, "sd_spec_queue_plan: active stream %d has %d rows", j, act_rows[j]);
    int left[SD_MAX_STREAMS], off[SD_MAX_STREAMS];
    bool waiting = false;
    for (int j = 0; j < n_join; ++j) {
        SD_REQUIRE(join_rows[j] >= 0, "sd_spec_queue_plan: joiner %d has %d rows left", j, join_rows[j]);
        left[j] = join_rows[j]; off[j] = 0;
        waiting = waiting || left[j] > 0;
    }
    int np = 0, nc = 0;
    // the joiner rows pass `p` carries next to `rows` rows of `items` active streams, `logits` of them logit rows
    auto ride = [&](sd_queue_pass &p, int rows, int items, int logits) -> bool {
        int room = logits > mixed_logit_limit ? 0 : row_budget - rows;
        if (prefill_chunk > 0) room = std::min(room, prefill_chunk);
        p.chunk0 = nc; p.n_chunks = 0;
        for (int j = 0; j < n_join && room > 0 && items < SD_MAX_STREAMS; ++j) {
            const int c = std::min(left[j], room);
            if (c <= 0) continue;
            if (nc >= max_chunks) return false;
            chunks[nc++] = sd_queue_chunk{j, off[j], c};
            ++p.n_chunks; ++items;
            left[j] -= c; off[j] += c; room -= c;
        }
        return true;
    };
    bool fits = true;
    for (int a = 0; a < n_act && fits;) {
        int rows = 0, m = 0;
        while (a + m < n_act && m < SD_MAX_STREAMS && (m == 0 || rows + act_rows[a + m] <= row_budget)) rows += act_rows[a + m++];
        if (np >= max_passes) { fits = false; break; }
        sd_queue_pass &p = passes[np++];
        p.act0 = a; p.n_act = m;
        fits = ride(p, rows, m, logit_rows ? rows : m);
        a += m;
    }
    if (fits && force_progress && waiting && nc == 0) {           // the progress guarantee: a pass of joiner rows only
        if (np >= max_passes) fits = false;
        else {
            sd_queue_pass &p = passes[np++];
            p.act0 = n_act; p.n_act = 0;
            fits = ride(p, 0, 0, 0);
        }
    }
    if (!fits) {
        sd_set_error("sd_spec_queue_plan: the plan exceeds %d passes / %d chunks", max_passes, max_chunks);
        return SD_ERR_CAPACITY;
    }
    *n_passes_out = np; *n_chunks_out = nc;
    return SD_OK;
}

// What the queue adds to the lock-step loop (NULL there: every stream arrives loaded and prefilled)
struct PromptQueue {
    sd_queue_prompt *prompts;
    int n_prompts, prefill_chunk;
    int next = 0;                                                 // the first prompt that still waits
    int occ[SD_MAX_STREAMS];                                      // the prompt in slot i, -1: free
    bool joining[SD_MAX_STREAMS];                                 // ... whose rows [0, L-1) are not all cached yet
    int target_passes = 0, draft_passes = 0, extra_passes = 0, prefill_passes = 0;
    // a shared prompt prefix: the donors hold positions [0, shared_rows) of the two models
    sd_session *donor_draft = nullptr, *donor_target = nullptr;
    int shared_rows = 0;
    int prompt_rows = 0, copied_rows = 0;                         // target rows forwarded for prompts; KV rows copied per model
};

// An iteration boundary of the queue: done streams hand their results to their prompts and free their slots, waiting
// prompts take free slots as joiners, joiners whose two caches hold L-1 positions become active.
static int queue_boundary(PromptQueue &q, sd_batch_stream *slots, int n_slots, int iters, int g, hipStream_t st) {
    sd_kv_copy_item d_copy[SD_MAX_STREAMS], t_copy[SD_MAX_STREAMS];   // the shared prefix rows of the prompts admitted here
    int n_copy = 0;
    for (int i = 0; i < n_slots; ++i) {
        sd_batch_stream &s = slots[i];
        if (q.occ[i] >= 0 && s.done) {
            sd_queue_prompt &p = q.prompts[q.occ[i]];
            p.len = s.len; p.calls = s.calls; p.finish_iter = iters - 1;
            q.occ[i] = -1;
        }
        while (q.occ[i] < 0 && q.next < q.n_prompts) {
            sd_queue_prompt &p = q.prompts[q.next];
            p.len = p.L; p.calls = 0; p.admit_iter = p.finish_iter = iters;
            if (p.L >= p.T) { ++q.next; continue; }               // nothing to generate: the prompt is the result
            SD_HIP_CHECK(hipMemcpyAsync(s.seq, p.tokens, sizeof(int32_t) * (size_t)p.L, hipMemcpyHostToDevice, st));
            SD_HIP_CHECK(hipMemsetAsync(s.err_words, 0, sizeof(int) * (size_t)(3 * g + 1), st));
            SD_HIP_CHECK(hipMemsetAsync(s.res_dev, 0, sizeof(sd_accept_result), st));
            s.host_seq = p.host_seq; s.len = p.L; s.T = p.T; s.ori_eos_cnt = p.ori_eos_cnt;
            // the shared prefix comes from the donors; the last prompt token is always fed as the first decode row
            const int c = std::min(q.shared_rows, p.L - 1);
            s.draft_len = s.target_len = c;
            if (c > 0) {
                d_copy[n_copy] = sd_kv_copy_item{s.draft, 0, c};
                t_copy[n_copy++] = sd_kv_copy_item{s.target, 0, c};
                q.copied_rows += c;
            }
            s.seed = p.seed; s.draw = 0; s.done = 0; s.calls = 0;
            s.acc_len_out = p.acc_len_out; s.p_at_out = p.p_at_out; s.q_at_out = p.q_at_out;
            q.occ[i] = q.next++;
            q.joining[i] = true;
        }
        if (q.occ[i] >= 0 && q.joining[i] && s.draft_len == s.len - 1 && s.target_len == s.len - 1) {
            q.joining[i] = false;
            q.prompts[q.occ[i]].admit_iter = iters;
        }
    }
    if (n_copy) {                                                 // one launch per model, ahead of every forward of the iteration
        if (int rc = sd_session_copy_kv(q.donor_draft, d_copy, n_copy, st); rc != SD_OK) return rc;
        if (int rc = sd_session_copy_kv(q.donor_target, t_copy, n_copy, st); rc != SD_OK) return rc;
    }
    return SD_OK;
}

// No stream is active: what the joiners still miss of their rows [0, L-1) goes through sd_batch_prefill passes, packed in
// queue order - up to the sessions' row budget, 32 attention groups of 8 rows and 16 items per pass, a long prompt in chunks.
static int queue_idle_prefill(PromptQueue &q, sd_batch_stream *slots, const std::vector<int> &join, void *stream) {
    std::vector<sd_batch_item> items;
    for (int side = 0; side < 2; ++side) {
        int cap = SD_MAX_FWD_ROWS, rows = 0, groups = 0, rc;
        for (int i : join) cap = std::min(cap, (side ? slots[i].target : slots[i].draft)->max_rows);
        items.clear();
        auto flush = [&]() -> int {
            if (items.empty()) return SD_OK;
            const int r = sd_batch_prefill(items.data(), (int)items.size(), stream);
            if (side) { ++q.target_passes; ++q.extra_passes; ++q.prefill_passes; } else ++q.draft_passes;
            items.clear(); rows = groups = 0;
            return r;
        };
        for (int i : join) {
            sd_batch_stream &s = slots[i];
            int &have = side ? s.target_len : s.draft_len;
            while (have < s.len - 1) {
                const int c = std::min({s.len - 1 - have, cap - rows, (SD_MAX_GROUPS - groups) * ATT_TQ});
                if (c <= 0 || (int)items.size() >= SD_MAX_STREAMS) { if ((rc = flush()) != SD_OK) return rc; continue; }
                items.push_back(sd_batch_item{side ? s.target : s.draft, s.seq, have, c, 0});
                have += c; rows += c; groups += (c + ATT_TQ - 1) / ATT_TQ;
                if (side) q.prompt_rows += c;
            }
        }
        if ((rc = flush()) != SD_OK) return rc;
    }
    return SD_OK;
}

// rows per target pass of a lock-step loop: every verify row is a logit row (sd_model_max_pass_rows, 64 for a model whose
// lm_head or per-layer GEMMs stop at the streaming kernel)
static int target_pass_rows(const sd_batch_stream *streams, const sd_spec_scratch &sc) {
    return std::min(sc.max_rows_per_forward, streams[0].target ? streams[0].target->max_pass_rows : SD_MAX_ROWS);
}

// The lock-step loop of sampling/batch.py in native code (reference algorithm per stream: speculative_sampling.py:1934-2046),
// with or without a prompt queue behind the streams' slots.
// `who`: the entry that was called.  o's members are indexed by stream - with a queue, by prompt.  `lookup` (never with a
// queue): one proposer launch drafts for the active streams, which have no draft sessions; their draft_len stays as it is.
static int lockstep_loop(const char *who, sd_batch_stream *streams, int n_streams, PromptQueue *q, const LookupDraft *lookup, int gamma,
                         const sd_sampling &sm, uint64_t random_seed, const float *r_const, const sd_spec_scratch &sc,
                         sd_lockstep_log *log, void *stream, const LoopOpts &o) {
    SD_REQUIRE(!(q && lookup), "%s: a prompt queue behind a lookup drafter", who);
    const sd_row_sampling *const params = o.params;
    const sd_logprob_block *const lp = o.lp;
    const RowEdits *const re = o.re;
    hipStream_t st = (hipStream_t)stream;
    const int g = gamma, n_err = 3 * g + 1;
    // rows per target pass and per draft pass (sd_batch_forward's own limit)
    const int pass_rows = target_pass_rows(streams, sc);
    const int draft_rows = std::min(streams[0].draft ? streams[0].draft->max_rows : SD_MAX_ROWS, SD_MAX_ROWS);
    // the iteration's one copy: the streams' result blocks and, behind them, a lookup drafter's info ints
    const size_t res_bytes = (size_t)n_streams * (sizeof(sd_accept_result) + (lookup ? 2 * sizeof(int32_t) : 0));
    LoopEvents ev(2, who);
    if (!ev.ok) return SD_ERR_HIP;
    log->n_iters = log->err = 0;
    int rc = SD_OK;
    int &iters = log->n_iters;
    std::vector<sd_batch_stream *> act;
    std::vector<int> Ls, join;
    std::vector<Draws> draws;
    std::vector<sd_batch_item> items;
    std::vector<sd_norm_row> rows;
    std::vector<sd_row_sampling> prows;                           // the parameters of rows[] (with `params` only)
    std::vector<sd_accept_item> aitems;
    std::vector<const void *> list_of;
    int32_t act_rows[SD_MAX_STREAMS], join_rows[SD_MAX_STREAMS];
    sd_queue_pass passes[SD_MAX_STREAMS + 1];
    sd_queue_chunk chunks[(SD_MAX_STREAMS + 1) * SD_MAX_STREAMS];
    int n_passes = 0, n_chunks = 0;
    // the passes of a draft step (side 0) or of the verify (side 1) over act_rows[], joiners riding where there is room
    auto plan = [&](int side, bool force) -> int {
        for (size_t k = 0; k < join.size(); ++k) {
            const sd_batch_stream &s = streams[join[k]];
            join_rows[k] = s.len - 1 - (side ? s.target_len : s.draft_len);
        }
        return sd_spec_queue_plan(side ? pass_rows : draft_rows, SD_STREAM_MAX_ROWS, act_rows, (int)act.size(), side, join_rows,
                                  (int)join.size(), q ? q->prefill_chunk : 0, force, passes, SD_MAX_STREAMS + 1, chunks,
                                  (SD_MAX_STREAMS + 1) * SD_MAX_STREAMS, &n_passes, &n_chunks);
    };
    // the joiner items of pass `p`, behind its active streams' items (no logit rows: the logit rows stay packed in stream order)
    auto add_joiners = [&](const sd_queue_pass &p, int side) {
        for (int k = p.chunk0; k < p.chunk0 + p.n_chunks; ++k) {
            sd_batch_stream &s = streams[join[chunks[k].joiner]];
            int &have = side ? s.target_len : s.draft_len;
            items.push_back(sd_batch_item{side ? s.target : s.draft, s.seq, have, chunks[k].rows, 0});
            have += chunks[k].rows;
            if (side) q->prompt_rows += chunks[k].rows;
        }
        if (!q) return;
        ++(side ? q->target_passes : q->draft_passes);
        if (side && p.n_act == 0) ++q->extra_passes;
    };
    // SD_BATCH_FUSED_TAIL=0: the round-1 sampling tail (logits copy, candidate pass + norm per draft step; dense accept scan +
    // resample) - kept for A/B runs and as the reference the fused tail is tested against; read per call, and not at all with a
    // lookup drafter, whose loop has the fused tail only
    const bool fused_tail = lookup || !(getenv("SD_BATCH_FUSED_TAIL") && atoi(getenv("SD_BATCH_FUSED_TAIL")) == 0);
    const bool tiles_ok = head_tiles_ok(sm.top_k, sm.temperature, sm.V, sm.ld);
    int L0[SD_MAX_STREAMS];                                       // (logprobs, penalties without a queue) the streams' lengths on entry
    // the request a stream runs - its index into o's tables: a queue's slot changes parameters, penalties and edits when it
    // changes hands - and that request's prompt length
    auto request_of = [&](const sd_batch_stream &s) { return q ? q->occ[&s - streams] : (int)(&s - streams); };
    auto prompt_len_of = [&](const sd_batch_stream &s) { return q ? q->prompts[request_of(s)].L : L0[&s - streams]; };
    std::vector<sd_logprob_item> litems;
    // penalties and edits: the launch over a pass's logit rows - m streams from act[a0], stream j's n_rows(j) rows packed in
    // stream order in `src`, the first at position pos0(j) - ahead of the norm launch `nr`, which then reads the slab.  A pass
    // without a penalised or edited stream is left alone.
    auto pass_edited = [&](int a0, int m) {
        bool any = false;
        for (int j = 0; re && j < m; ++j) any = any || re->edited(request_of(*act[a0 + j]), act[a0 + j]->target);
        return any;
    };
    sd_logit_edit_item pitems[SD_MAX_STREAMS];
    const sd_session *pses[SD_MAX_STREAMS];
    sd_lookup_item lkitems[SD_MAX_STREAMS];
    auto edit_pass = [&](int a0, int m, const HeadOut &src, auto n_rows, auto pos0, NormRequest &nr) -> int {
        int r0 = 0;
        for (int j = 0; j < m; ++j) {
            const sd_batch_stream &s = *act[a0 + j];
            const int slot = (int)(&s - streams), nr_j = n_rows(j);
            if (nr_j > PEN_MAX_ROWS || r0 + nr_j > re->max_rows) {
                sd_set_error("%s: %s: stream %d has %d logit rows in a pass of more than %d (a launch takes %d per stream, the "
                             "slab holds %d)", who, re->edit ? "edits" : "penalties", slot, nr_j, r0, PEN_MAX_ROWS, re->max_rows);
                return SD_ERR_INVALID;
            }
            pitems[j] = edit_item(*re, request_of(s), src, r0, nr_j, s.seq, pos0(j), prompt_len_of(s));
            pses[j] = s.target;
            r0 += nr_j;
        }
        if (int prc = edit_rows(*re, pitems, m, sm.V, nr.mode, stream, pses); prc != SD_OK) return prc;
        norm_from_edited(nr, *re);
        return SD_OK;
    };
    for (int i = 0; i < n_streams; ++i) {
        L0[i] = streams[i].len;
        streams[i].done = q ? 1 : 0; streams[i].calls = 0;
        if (q) { q->occ[i] = -1; q->joining[i] = false; }
    }
    for (;;) {
        for (int i = 0; i < n_streams; ++i)
            if (!streams[i].done && streams[i].len >= streams[i].T) streams[i].done = 1;
        if (q && (rc = queue_boundary(*q, streams, n_streams, iters, g, st)) != SD_OK) break;
        act.clear(); join.clear();
        for (int i = 0; i < n_streams; ++i) {
            if (streams[i].done) continue;
            if (q && q->joining[i]) join.push_back(i);
            else act.push_back(&streams[i]);
        }
        if (q) std::sort(join.begin(), join.end(), [&](int a, int b) { return q->occ[a] < q->occ[b]; });
        if (act.empty()) {
            if (join.empty()) break;
            if ((rc = queue_idle_prefill(*q, streams, join, stream)) != SD_OK) break;
            continue;                                             // (the boundary makes them active)
        }
        const int n = (int)act.size();
        Ls.resize(n); draws.resize(n);
        double ctx = 0.0;
        for (int j = 0; j < n; ++j) {
            Ls[j] = act[j]->len;
            draws[j] = next_draws(act[j]->seed, act[j]->draw, g, random_seed);
            // the draft model's samples are taken: a failed forward leaves the stream here, seed untouched.  (A lookup iteration
            // leaves draws d .. d + gamma unread, and the stream where it was until both halves are enqueued.)
            if (!lookup) act[j]->draw += (uint64_t)g;
            ctx += Ls[j];
        }
        // ---- draft: one proposer launch, or gamma steps, over all active streams
        if (lookup) {
            for (int j = 0; j < n; ++j) {
                sd_batch_stream &s = *act[j];
                lkitems[j] = sd_lookup_item{s.seq, Ls[j], s.q_hist, lookup->info_dev + 2 * (&s - streams)};
            }
            rc = sd_lookup_propose(lkitems, n, sm.V, sm.ld, g, lookup->ngram_max, lookup->ngram_min, stream);
        }
        bool rode = false;                                        // a joiner's draft rows rode a pass of this iteration
        for (int i = 0; i < (lookup ? 0 : g) && rc == SD_OK; ++i) {
            for (int j = 0; j < n; ++j) act_rows[j] = Ls[j] + i - act[j]->draft_len;
            if ((rc = plan(0, i == g - 1 && !rode)) != SD_OK) break;
            rode = rode || n_chunks > 0;
            for (int p = 0; p < n_passes && rc == SD_OK; ++p) {
                const int a0 = passes[p].act0, m = passes[p].n_act;
                items.assign(m, sd_batch_item{});
                rows.assign(m, sd_norm_row{});
                // per-request parameters: the head is asked for tile maxima when every sampled row of THIS pass can use them
                bool pass_tiles = tiles_ok;
                if (params) {
                    prows.resize(m);
                    pass_tiles = true;
                    for (int j = 0; j < m; ++j) {
                        prows[j] = params[request_of(*act[a0 + j])];
                        pass_tiles = pass_tiles && head_tiles_ok(prows[j].top_k, prows[j].temperature, sm.V, sm.ld);
                    }
                }
                const bool pen_pass = pass_edited(a0, m);         // (its rows take no tile maxima)
                pass_tiles = pass_tiles && !pen_pass;
                for (int j = 0; j < m; ++j) {
                    sd_batch_stream &s = *act[a0 + j];
                    draft_step_rows(items[j], rows[j], s.draft, s.seq, s.q_hist, sm.ld, s.err_words, g, Ls[a0 + j], i, s.draft_len,
                                    draws[a0 + j].seed_draft, draws[a0 + j].draft0 + (uint64_t)i);
                    s.draft_len = Ls[a0 + j] + i;
                }
                add_joiners(passes[p], 0);
                // the single-stream loop's sampler feed (draft_steps): the head leaves the logits in its own slab, the
                // maximum of every 16-column tile, and clears the streams' probability rows - no logits copy, no candidate pass
                HeadReq rq = {};
                HeadOut ho = {};
                rq.raw = fused_tail;
                rq.zero_n = fused_tail && pass_tiles && m <= 16 ? m : 0;
                for (int j = 0; j < rq.zero_n; ++j) rq.zero_ptr[j] = rows[j].probs_out;
                if ((rc = batch_forward(items.data(), (int)items.size(), sc.draft.logits, sc.draft.ld_logits, &rq, &ho, stream)) != SD_OK) break;
                if (m == 0) continue;                             // (joiner rows only)
                const HeadOut src = fused_tail ? ho : scratch_rows(sc.draft);
                NormRequest nr = norm_request(sm, sc.draft.norm_mode, src);
                if (pen_pass && (rc = edit_pass(a0, m, src, [](int) { return 1; }, [&](int j) { return Ls[a0 + j] + i - 1; }, nr)) != SD_OK)
                    break;
                nr.rows = m; nr.workspace = sc.norm_workspace; nr.row_params = params ? prows.data() : nullptr;
                rc = sd_norm_batch_tiles(nr, rows.data(), 1, stream);
            }
        }
        if (rc != SD_OK) break;
        // ---- verify: the uncached rows of every stream, as many whole streams per pass over the target weights as it holds
        for (int j = 0; j < n; ++j) act_rows[j] = Ls[j] + g - act[j]->target_len;
        if ((rc = plan(1, true)) != SD_OK) break;
        // the residual / bonus sample works on the target rows' candidate lists when ONE verify pass holds all streams (the
        // workspace keeps the lists of one pass)
        const bool lists_on = fused_tail && sc.norm_workspace && passes[0].n_act == n;
        char *const list_base = sc.norm_workspace ? (char *)sc.norm_workspace + sd_norm_candrow_bytes(sc.max_rows_per_forward) : nullptr;
        const size_t list_stride = sd_cand_list_bytes(1);
        list_of.assign(n, nullptr);
        const int res_mode = accept_mode(sc, lookup);
        // the accept item of active stream j
        auto accept_item = [&](int j) {
            const sd_batch_stream &s = *act[j];
            sd_accept_item it = {};
            it.p_hist = s.p_hist; it.q_hist = s.q_hist; it.seq = s.seq; it.L = Ls[j];
            it.r = r_const; it.exp_noise = nullptr;
            it.philox_seed = draws[j].seed; it.draw_scan = draws[j].scan0; it.draw_resample = draws[j].resample;
            it.res = s.res_dev; it.err_flags = s.err_words; it.n_err = n_err;
            return it;
        };
        // logprobs: every verify pass writes the same slab, sc.target.logits, so when the verify takes several passes each
        // pass's streams are accepted and scored before the next pass is enqueued (no lists then: lists_on needs one pass)
        const bool by_pass = lp && passes[0].n_act != n;
        litems.clear();
        SD_LOOP_HIP(hipEventRecord(ev.t[0], st));
        for (int p = 0; p < n_passes && rc == SD_OK; ++p) {
            const int a0 = passes[p].act0, m = passes[p].n_act;
            items.assign(m, sd_batch_item{});
            rows.clear(); prows.clear();
            for (int j = 0; j < m; ++j) {
                sd_batch_stream &s = *act[a0 + j];
                verify_pass_rows(items[j], rows, s.target, s.seq, s.p_hist, sm.ld, s.err_words, g, Ls[a0 + j], s.target_len);
                if (params) prows.resize(rows.size(), params[request_of(s)]);   // (every row of the stream takes its triple)
            }
            add_joiners(passes[p], 1);
            if ((rc = batch_forward(items.data(), (int)items.size(), sc.target.logits, sc.target.ld_logits, nullptr, nullptr, stream)) != SD_OK)
                break;
            if (m == 0) continue;                                 // (joiner rows only)
            // one pass holds every stream: the rows' candidate lists (behind the CandRows of the workspace) serve the
            // residual / bonus sample below
            NormRequest nr = norm_request(sm, sc.target.norm_mode, scratch_rows(sc.target));
            if (pass_edited(a0, m) && (rc = edit_pass(a0, m, scratch_rows(sc.target), [&](int j) { return items[j].n_new; },
                                                      [&](int j) { return items[j].pos0; }, nr)) != SD_OK)
                break;
            nr.rows = (int)rows.size(); nr.workspace = sc.norm_workspace; nr.lists = lists_on ? list_base : nullptr;
            nr.row_params = params ? prows.data() : nullptr;
            rc = sd_norm_batch_tiles(nr, rows.data(), 0, stream);
            if (lists_on) {
                int r0 = 0;
                for (int j = 0; j < m; ++j) {                       // stream j's lists are valid when all its gamma + 1 rows are here
                    list_of[a0 + j] = items[j].n_new == g + 1 ? list_base + (size_t)r0 * list_stride : nullptr;
                    r0 += items[j].n_new;
                }
            }
            if (!lp || rc != SD_OK) continue;
            // the streams' last gamma + 1 logit rows, packed in stream order in the slab
            const size_t l0 = litems.size();
            for (int j = 0, r0 = 0; j < m; r0 += items[j++].n_new) {
                const sd_batch_stream &s = *act[a0 + j];
                if (items[j].n_new < g + 1) {
                    sd_set_error("%s: logprobs: stream %d has %d verify rows, fewer than gamma + 1", who, (int)(&s - streams), items[j].n_new);
                    rc = SD_ERR_INVALID;
                    break;
                }
                litems.push_back(verify_logprob_item(*lp, (int)(&s - streams), sc.target.logits + (size_t)(r0 + items[j].n_new - (g + 1)) * sc.target.ld_logits,
                                                     sc.target.ld_logits, g, s.seq, Ls[a0 + j], s.res_dev));
            }
            if (!by_pass || rc != SD_OK) continue;
            aitems.clear();
            for (int j = 0; j < m; ++j) aitems.push_back(accept_item(a0 + j));
            if ((rc = sd_accept_batch(aitems.data(), m, sm.ld, sm.V, g, res_mode, stream)) != SD_OK) break;
            rc = sd_token_logprobs(litems.data() + l0, m, sm.V, sc.target.norm_mode, stream);
        }
        if (rc != SD_OK) break;
        SD_LOOP_HIP(hipEventRecord(ev.t[1], st));
        // ---- accept scan + residual / bonus sample, all streams in two launches.  The scan reads probability rows L-1 ..
        // L+gamma-1 only, and this iteration wrote every one of them: the q rows in its draft steps, the p rows in the verify's
        // sd_norm_batch_tiles above, which writes whole rows.  So a slot's p_hist / q_hist never show a previous occupant.
        for (int j = 0; j < n; ++j) {
            sd_batch_stream &s = *act[j];
            s.seed = draws[j].seed; s.draw = draws[j].draw;       // both forwards are enqueued: the rest of the iteration's draws
        }
        if (!by_pass) {
            aitems.clear();
            for (int j = 0; j < n; ++j) aitems.push_back(accept_item(j));
            if (lists_on) rc = sd_accept_resample_batch(aitems.data(), n, sm.ld, sm.V, g, res_mode, list_of.data(), stream);
            else rc = sd_accept_batch(aitems.data(), n, sm.ld, sm.V, g, res_mode, stream);
            if (rc != SD_OK) break;
            if (lp && (rc = sd_token_logprobs(litems.data(), n, sm.V, sc.target.norm_mode, stream)) != SD_OK) break;
        }
        if (lp)
            SD_LOOP_HIP(hipMemcpyAsync(lp->host, lp->dev, sizeof(float) * (size_t)n_streams * LP_SLICE, hipMemcpyDeviceToHost, st));
        SD_LOOP_HIP(hipMemcpyAsync(streams[0].res_host, streams[0].res_dev, res_bytes, hipMemcpyDeviceToHost, st));
        SD_LOOP_HIP(hipEventRecord(ev.done, st));
        if ((rc = poll_event(ev.done, who)) != SD_OK) break;
        if (iters < log->max_iters_log) {
            float ms = 0.f;
            if (log->verify_ms_out && hipEventElapsedTime(&ms, ev.t[0], ev.t[1]) == hipSuccess) log->verify_ms_out[iters] = ms;
            if (log->verify_streams_out) log->verify_streams_out[iters] = n;
            if (log->verify_ctx_out) log->verify_ctx_out[iters] = (float)(ctx / n + g);
        }
        ++iters;
        bool failed = false;
        for (int j = 0; j < n; ++j) {
            sd_batch_stream &s = *act[j];
            const sd_accept_result r = *s.res_host;
            if (r.flags & (2 | 8)) { failed = true; break; }
            if (s.acc_len_out) s.acc_len_out[s.calls] = r.n_accepted;
            if (lookup) lookup->log_match((int)(&s - streams), s.calls);
            log_ratios(s.p_at_out, s.q_at_out, (size_t)s.calls, g, r.p_at, r.q_at);
            ++s.calls;
            int no_draft_len = 0;
            commit_result(r, Ls[j], g, s.host_seq, &s.len, lookup ? &no_draft_len : &s.draft_len, &s.target_len);
            if (lp)                                              // a queue's slot writes to the array of the prompt it runs
                commit_logprobs(*lp, (int)(&s - streams), lp->logprob_out[request_of(s)], Ls[j] - prompt_len_of(s), r);
            int eos_total = 0;
            for (int i = 0; i < s.len; ++i) eos_total += s.host_seq[i] == sm.eos_token_id;
            if (eos_total > s.ori_eos_cnt) s.done = 1;            // the caller cuts after the first new EOS
        }
        if (failed) { log->err = 1; break; }
    }
    return rc;
}

static int check_result_blocks(const char *who, const sd_batch_stream *streams, int n_streams) {
    for (int i = 1; i < n_streams; ++i)
        SD_REQUIRE(streams[i].res_dev == streams[0].res_dev + i && streams[i].res_host == streams[0].res_host + i,
                   "%s: the streams' result blocks must be consecutive", who);
    return SD_OK;
}

// the logit rows of a lock-step loop's largest pass: whole streams of gamma + 1 verify rows, as many as a target pass holds
static int lockstep_penalty_rows(const sd_batch_stream *streams, int n_streams, int gamma, const sd_spec_scratch &sc) {
    return std::min(std::max(target_pass_rows(streams, sc), gamma + 1), n_streams * (gamma + 1));
}

extern "C" int sd_spec_batch_generate(sd_batch_stream *streams, int n_streams, int gamma, const sd_sampling *sampling,
                                      uint64_t random_seed, const float *r_const, const sd_spec_scratch *scratch,
                                      sd_lockstep_log *log, void *stream, const sd_loop_opts *opts) {
    const char *const who = "sd_spec_batch_generate";
    SD_REQUIRE(streams && n_streams >= 1 && n_streams <= 16 && gamma >= 1 && gamma <= 16 && sampling && scratch && log &&
               scratch->draft.logits && scratch->target.logits, "%s: bad arguments", who);
    SD_REQUIRE(!random_seed || r_const, "%s: random_seed needs its uniform (r_const)", who);
    if (int rc = check_result_blocks(who, streams, n_streams); rc != SD_OK) return rc;
    LoopOpts o;
    const sd_session *ts[SD_MAX_STREAMS];
    int states_need[SD_MAX_STREAMS];
    for (int i = 0; i < n_streams; ++i) {
        ts[i] = streams[i].target;
        states_need[i] = streams[i].T - streams[i].len + gamma + 2;
    }
    if (int rc = resolve_loop_opts(who, "stream", opts, n_streams, sampling->V, lockstep_penalty_rows(streams, n_streams, gamma, *scratch),
                                   sampling->eos_token_id, true, &o, ts, n_streams); rc != SD_OK)
        return rc;
    if (int rc = check_grammar_states(who, "stream", ts, n_streams, states_need); rc != SD_OK) return rc;
    for (int i = 0; i < n_streams; ++i)
        SD_REQUIRE(!has_grammar(ts[i]) || streams[i].target_len <= streams[i].len - 1, "%s: grammar: stream %d: target_len %d of %d "
                   "tokens: the first verify pass must start at the prompt's last row", who, i, streams[i].target_len, streams[i].len);
    return lockstep_loop(who, streams, n_streams, nullptr, nullptr, gamma, *sampling, random_seed, r_const, *scratch, log, stream, o);
}

// ---- prompt-lookup drafting (include/specdec.h has the definition and the loops' contract) ------------------------
// what the three entries refuse in gamma and the n-gram bounds, in that order
static int check_lookup_bounds(const char *who, int gamma, int ngram_max, int ngram_min) {
    SD_REQUIRE(gamma >= 1 && gamma <= LOOKUP_MAX_GAMMA, "%s: gamma %d outside 1..%d", who, gamma, LOOKUP_MAX_GAMMA);
    SD_REQUIRE(ngram_max >= 1 && ngram_max <= SD_LOOKUP_MAX_NGRAM, "%s: ngram_max %d outside 1..%d", who, ngram_max, SD_LOOKUP_MAX_NGRAM);
    SD_REQUIRE(ngram_min >= 1 && ngram_min <= ngram_max, "%s: ngram_min %d outside 1..ngram_max %d", who, ngram_min, ngram_max);
    return SD_OK;
}

extern "C" int sd_lookup_propose(const sd_lookup_item *items, int n_items, int V, long ld, int gamma, int ngram_max, int ngram_min,
                                 void *stream) {
    const char *const who = "sd_lookup_propose";
    SD_REQUIRE(items, "%s: null argument", who);
    SD_REQUIRE(n_items >= 1 && n_items <= LOOKUP_MAX_ITEMS, "%s: n_items %d outside 1..%d", who, n_items, LOOKUP_MAX_ITEMS);
    if (int rc = check_lookup_bounds(who, gamma, ngram_max, ngram_min); rc != SD_OK) return rc;
    SD_REQUIRE(V >= 1 && ld >= V, "%s: V %d < 1 or ld %ld < V", who, V, ld);
    LookupTab t = {};
    for (int i = 0; i < n_items; ++i) {
        const sd_lookup_item &it = items[i];
        SD_REQUIRE(it.seq && it.q_hist && it.info, "%s: item %d: null argument", who, i);
        SD_REQUIRE(it.L >= 1, "%s: item %d: L %d < 1", who, i, it.L);
        t.seq[i] = it.seq; t.q_hist[i] = it.q_hist; t.info[i] = it.info; t.L[i] = it.L;
    }
    return launch_lookup_propose(t, n_items, V, ld, gamma, ngram_max, ngram_min, (hipStream_t)stream);
}

// The prompt-lookup loop of one stream: sd_spec_generate's loop with one proposer launch where the gamma draft steps are.
extern "C" int sd_lookup_generate(const sd_spec_stream *dev, int gamma, int ngram_max, int ngram_min, const sd_sampling *sampling,
                                  const sd_spec_scratch *scratch, sd_seq_state *s, int32_t *match_len_out, void *stream) {
    const char *const who = "sd_lookup_generate";
    SD_REQUIRE(dev && sampling && scratch && s && dev->target && dev->seq && dev->q_hist && dev->p_hist && dev->err_words &&
               dev->res_dev && dev->res_host && s->host_seq && scratch->target.logits, "%s: null argument", who);
    SD_REQUIRE(!dev->draft, "%s: a draft session: prompt lookup drafts without a model (dev->draft must be NULL)", who);
    if (int rc = check_lookup_bounds(who, gamma, ngram_max, ngram_min); rc != SD_OK) return rc;
    const sd_sampling &sm = *sampling;
    SD_REQUIRE(sm.temperature != 0.0f, "%s: temperature must be non-zero", who);
    SD_REQUIRE(!scratch->norm_workspace || scratch->max_rows_per_forward >= gamma + 1,
               "%s: a norm workspace of %d rows, the target's gamma %d + 1 rows keep their lists there", who,
               scratch->max_rows_per_forward, gamma);
    SD_REQUIRE(sm.V == dev->target->m->cfg.vocab && sm.ld >= sm.V, "%s: V %d (ld %ld), the target's vocabulary is %d", who, sm.V, sm.ld,
               dev->target->m->cfg.vocab);
    SD_REQUIRE(!has_grammar(dev->target), "%s: the target session carries a grammar: this loop has no edit pass (detach it: "
               "sd_session_set_grammar(s, NULL, NULL, 0))", who);
    refresh_env();
    // the two info ints are behind the result block; no options block in this entry: nothing to edit or score
    const LookupDraft lookup = {ngram_max, ngram_min, reinterpret_cast<int32_t *>(dev->res_dev + 1),
                                reinterpret_cast<const int32_t *>(dev->res_host + 1), &match_len_out};
    return single_stream_loop(who, *dev, gamma, sm, *scratch, s, 0, nullptr, stream, LoopOpts(), &lookup);
}

// The lock-step prompt-lookup loop: lockstep_loop with one proposer launch over the active streams where the gamma draft
// steps are; the info ints ride behind the streams' result blocks in the iteration's one copy.
extern "C" int sd_lookup_batch_generate(sd_batch_stream *streams, int n_streams, int gamma, int ngram_max, int ngram_min,
                                        const sd_sampling *sampling, const sd_spec_scratch *scratch, sd_lockstep_log *log,
                                        int32_t **match_len_out, void *stream) {
    const char *const who = "sd_lookup_batch_generate";
    SD_REQUIRE(streams && sampling && scratch && log && scratch->target.logits, "%s: null argument", who);
    SD_REQUIRE(n_streams >= 1 && n_streams <= SD_MAX_STREAMS, "%s: n_streams %d outside 1..%d", who, n_streams, SD_MAX_STREAMS);
    if (int rc = check_lookup_bounds(who, gamma, ngram_max, ngram_min); rc != SD_OK) return rc;
    const sd_sampling &sm = *sampling;
    const sd_spec_scratch &sc = *scratch;
    SD_REQUIRE(sm.temperature != 0.0f, "%s: temperature must be non-zero", who);
    for (int i = 0; i < n_streams; ++i) {
        const sd_batch_stream &s = streams[i];
        SD_REQUIRE(s.target && s.seq && s.q_hist && s.p_hist && s.err_words && s.res_dev && s.res_host && s.host_seq,
                   "%s: stream %d: null pointer", who, i);
        SD_REQUIRE(!s.draft, "%s: stream %d: a draft session: prompt lookup drafts without a model (draft must be NULL)", who, i);
        SD_REQUIRE(s.target->m == streams[0].target->m, "%s: stream %d: a session of another model than stream 0's", who, i);
        SD_REQUIRE(!has_grammar(s.target), "%s: stream %d: the target session carries a grammar: this loop has no edit pass (detach it: "
                   "sd_session_set_grammar(s, NULL, NULL, 0))", who, i);
        SD_REQUIRE(s.len >= 1 && s.target_len == s.len - 1, "%s: stream %d: every stream arrives prefilled (target_len %d, len %d - 1)",
                   who, i, s.target_len, s.len);
    }
    SD_REQUIRE(sm.V == streams[0].target->m->cfg.vocab && sm.ld >= sm.V, "%s: V %d (ld %ld), the target's vocabulary is %d", who, sm.V,
               sm.ld, streams[0].target->m->cfg.vocab);
    if (int rc = check_result_blocks(who, streams, n_streams); rc != SD_OK) return rc;
    refresh_env();
    // 2 info ints per stream behind the blocks; no options block in this entry: nothing to edit or score
    const LookupDraft lookup = {ngram_max, ngram_min, reinterpret_cast<int32_t *>(streams[0].res_dev + n_streams),
                                reinterpret_cast<const int32_t *>(streams[0].res_host + n_streams), match_len_out};
    return lockstep_loop(who, streams, n_streams, nullptr, &lookup, gamma, sm, 0, nullptr, sc, log, stream, LoopOpts());
}

// The prompt queue: without donors (shared_rows 0) every prompt starts with empty caches.
extern "C" int sd_spec_queue_generate(sd_batch_stream *slots, int n_slots, int slot_cap, sd_queue_prompt *prompts, int n_prompts,
                                      int prefill_chunk, int gamma, const sd_sampling *sampling, uint64_t random_seed,
                                      const float *r_const, const sd_spec_scratch *scratch, sd_lockstep_log *log, int *passes_out,
                                      void *stream, sd_session *donor_draft, sd_session *donor_target, int shared_rows,
                                      const sd_loop_opts *opts) {
    const char *const who = "sd_spec_queue_generate";
    SD_REQUIRE(n_slots >= 1 && n_slots <= 16, "%s: n_slots %d outside 1..16", who, n_slots);
    SD_REQUIRE(gamma >= 1 && gamma <= 16, "%s: gamma %d outside 1..16", who, gamma);
    SD_REQUIRE(n_prompts >= 1 && prefill_chunk >= 0, "%s: n_prompts %d, prefill_chunk %d", who, n_prompts, prefill_chunk);
    SD_REQUIRE(slots && prompts && sampling && scratch && log && scratch->draft.logits && scratch->target.logits,
               "%s: null argument", who);
    SD_REQUIRE(!random_seed || r_const, "%s: random_seed needs its uniform (r_const)", who);
    SD_REQUIRE(shared_rows >= 0 && (shared_rows > 0) == (donor_draft != nullptr) && (shared_rows > 0) == (donor_target != nullptr),
               "%s: shared_rows %d needs both donor sessions, and 0 rows none", who, shared_rows);
    for (int i = 0; i < n_slots; ++i) {
        const sd_batch_stream &s = slots[i];
        SD_REQUIRE(s.draft && s.target && s.seq && s.q_hist && s.p_hist && s.err_words && s.res_dev && s.res_host,
                   "%s: slot %d: null pointer", who, i);
        SD_REQUIRE(s.draft->m == slots[0].draft->m && s.target->m == slots[0].target->m,
                   "%s: slot %d: sessions of another model than slot 0's", who, i);
    }
    if (shared_rows > 0) {
        SD_REQUIRE(donor_draft->m == slots[0].draft->m && donor_target->m == slots[0].target->m,
                   "%s: the donors are sessions of other models than the slots'", who);
        SD_REQUIRE(shared_rows <= donor_draft->max_seq && shared_rows <= donor_target->max_seq,
                   "%s: shared_rows %d, the donors hold %d / %d positions", who, shared_rows, donor_draft->max_seq,
                   donor_target->max_seq);
        SD_REQUIRE(donor_draft->kv_fp8 == slots[0].draft->kv_fp8 && donor_target->kv_fp8 == slots[0].target->kv_fp8,
                   "%s: the donors' KV arenas have another dtype than the slots'", who);
    }
    if (int rc = check_result_blocks(who, slots, n_slots); rc != SD_OK) return rc;
    for (int k = 0; k < n_prompts; ++k) {
        const sd_queue_prompt &p = prompts[k];
        SD_REQUIRE(p.tokens && p.host_seq && p.L >= 1, "%s: prompt %d: null pointer or L %d < 1", who, k, p.L);
        const int need = std::max(p.L, p.T) + gamma + 2;
        SD_REQUIRE(need <= slot_cap, "%s: prompt %d needs %d positions per slot, slot_cap is %d", who, k, need, slot_cap);
    }
    for (int i = 0; i < n_slots; ++i)
        SD_REQUIRE(slots[i].draft->max_seq >= slot_cap - 2 && slots[i].target->max_seq >= slot_cap - 2,
                   "%s: slot %d: KV arenas of %d / %d positions, slot_cap %d needs %d", who, i, slots[i].draft->max_seq,
                   slots[i].target->max_seq, slot_cap, slot_cap - 2);
    LoopOpts o;
    const sd_session *ts[SD_MAX_STREAMS];
    int states_need[SD_MAX_STREAMS], t_max = prompts[0].T, l_min = prompts[0].L;
    for (int k = 1; k < n_prompts; ++k) { t_max = std::max(t_max, (int)prompts[k].T); l_min = std::min(l_min, (int)prompts[k].L); }
    for (int i = 0; i < n_slots; ++i) { ts[i] = slots[i].target; states_need[i] = t_max - l_min + gamma + 2; }
    if (int rc = resolve_loop_opts(who, "prompt", opts, n_prompts, sampling->V, lockstep_penalty_rows(slots, n_slots, gamma, *scratch),
                                   sampling->eos_token_id, true, &o, ts, n_slots); rc != SD_OK)
        return rc;
    if (int rc = check_grammar_states(who, "slot", ts, n_slots, states_need); rc != SD_OK) return rc;
    PromptQueue q;
    q.prompts = prompts; q.n_prompts = n_prompts; q.prefill_chunk = prefill_chunk;
    q.donor_draft = donor_draft; q.donor_target = donor_target; q.shared_rows = shared_rows;
    const int rc = lockstep_loop(who, slots, n_slots, &q, nullptr, gamma, *sampling, random_seed, r_const, *scratch, log, stream, o);
    if (passes_out) {
        const int v[6] = {q.target_passes, q.draft_passes, q.extra_passes, q.prefill_passes, q.prompt_rows, q.copied_rows};
        std::copy(v, v + 6, passes_out);
    }
    return rc;
}

// ---- the width-w loop of sampling/multi.py in native code (reference speculative_sampling.py:1379-1716, strategy "iid")
extern "C" int sd_multi_adopt(const sd_multi_adopt_item *items, int width, const sd_multi_result *res, int L, int gamma,
                              int draft_lo, int target_lo, int draft_planes, int draft_max_seq, int draft_row_bytes,
                              int target_planes, int target_max_seq, int target_row_bytes, int seq_cap, void *stream) {
    SD_REQUIRE(items && res && width >= 1 && width <= 16, "sd_multi_adopt: 1..16 replicas");
    SD_REQUIRE(gamma >= 1 && gamma <= 16 && L >= 1, "sd_multi_adopt: bad gamma / L");
    SD_REQUIRE(draft_planes >= 0 && target_planes >= 0 && draft_row_bytes > 0 && target_row_bytes > 0 && draft_lo >= 0 &&
               target_lo >= 0, "sd_multi_adopt: bad arena shape");
    // the widest ranges the device may derive: draft [lo, L+gamma-1), target [lo, L+gamma), tokens [L, L+gamma+1)
    SD_REQUIRE((draft_planes == 0 || L + gamma - 1 <= draft_max_seq) && (target_planes == 0 || L + gamma <= target_max_seq) &&
               L + gamma + 1 <= seq_cap, "sd_multi_adopt: L %d + gamma %d overruns an arena (max_seq %d / %d) or a token buffer (%d)",
               L, gamma, draft_max_seq, target_max_seq, seq_cap);
    AdoptTab t = {};
    for (int w = 0; w < width; ++w) {
        SD_REQUIRE(items[w].seq && (draft_planes == 0 || items[w].draft_kv) && (target_planes == 0 || items[w].target_kv),
                   "sd_multi_adopt: replica %d: null pointer", w);
        t.d_kv[w] = (char *)items[w].draft_kv; t.t_kv[w] = (char *)items[w].target_kv; t.seq[w] = items[w].seq;
    }
    if (width == 1) return SD_OK;                                 // nobody to copy to
    const AdoptArena d = {draft_planes, draft_max_seq, draft_row_bytes, draft_lo};
    const AdoptArena tg = {target_planes, target_max_seq, target_row_bytes, target_lo};
    hipLaunchKernelGGL(multi_adopt_kernel, dim3(draft_planes + target_planes + 1, width), dim3(128), 0, (hipStream_t)stream, t, width,
                       res, L, gamma, d, tg, seq_cap);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

static inline int kv_planes(const sd_session *s) { return s->m->cfg.n_layers * 2 * s->m->cfg.n_kv_heads; }
static inline int kv_row_bytes(const sd_session *s) { return s->m->cfg.head_dim * (s->kv_fp8 ? 1 : (int)esize(s->m->cfg.dtype)); }

extern "C" int sd_session_copy_kv(const sd_session *src, const sd_kv_copy_item *items, int n_items, void *stream) {
    SD_REQUIRE(src && items, "sd_session_copy_kv: null argument");
    SD_REQUIRE(n_items >= 1 && n_items <= 16, "sd_session_copy_kv: n_items %d outside 1..16", n_items);
    KvCopyTab t = {};
    int n = 0, longest = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_kv_copy_item &it = items[i];
        SD_REQUIRE(it.dst, "sd_session_copy_kv: item %d: null argument", i);
        SD_REQUIRE(it.dst->m == src->m, "sd_session_copy_kv: item %d: a session of another model than the source's", i);
        SD_REQUIRE(it.dst != src, "sd_session_copy_kv: item %d: source and destination are one session", i);
        SD_REQUIRE(!it.dst->kv_fp8 == !src->kv_fp8, "sd_session_copy_kv: item %d: one arena is fp8 and the other is not", i);
        SD_REQUIRE(it.lo >= 0 && it.hi >= it.lo && it.hi <= src->max_seq && it.hi <= it.dst->max_seq,
                   "sd_session_copy_kv: item %d: positions [%d, %d) of arenas of %d (source) and %d positions", i, it.lo, it.hi,
                   src->max_seq, it.dst->max_seq);
        if (it.hi == it.lo) continue;
        t.dst[n] = it.dst->kv; t.dst_max_seq[n] = it.dst->max_seq; t.lo[n] = it.lo; t.hi[n] = it.hi;
        longest = std::max(longest, it.hi - it.lo);
        ++n;
    }
    if (n == 0) return SD_OK;                                     // nothing to copy
    const int planes = kv_planes(src), row_bytes = kv_row_bytes(src);
    SD_REQUIRE(planes >= 1 && planes <= 65535, "sd_session_copy_kv: %d KV planes exceed a grid dimension", planes);
    // a workgroup moves up to 16 KiB (four 16-byte accesses per lane); a shorter run is one chunk, rounded to whole vectors
    const size_t run = (size_t)longest * row_bytes;
    const int chunk = (int)std::min<size_t>(KV_COPY_CHUNK_MAX, (run + 15) / 16 * 16);
    const size_t chunks = (run + chunk - 1) / chunk;
    SD_REQUIRE(chunks <= 0x7fffffffu, "sd_session_copy_kv: a run of %zu bytes per plane is too long", run);
    hipLaunchKernelGGL(session_copy_kv_kernel, dim3((unsigned)chunks, planes, n), dim3(KV_COPY_THREADS), 0, (hipStream_t)stream,
                       src->kv, src->max_seq, row_bytes, chunk, t);
    SD_LAUNCH_CHECK();
    return SD_OK;
}

extern "C" size_t sd_spec_multi_block_bytes(int width, int gamma) {
    if (width < 1 || gamma < 1) return 0;
    return sizeof(sd_multi_result) + sizeof(int32_t) * (size_t)width * (3 * gamma + 1);
}

extern "C" int sd_spec_multi_generate(const sd_multi_replica *reps, int width, int gamma, int seq_cap, const sd_sampling *sampling,
                                      uint64_t random_seed, const float *r_const, const sd_spec_scratch *scratch, void *dev_block,
                                      void *host_block, sd_seq_state *s, void *stream) {
    SD_REQUIRE(width >= 1 && width <= 16, "sd_spec_multi_generate: width %d outside 1..16", width);
    SD_REQUIRE(gamma >= 1 && gamma <= 16, "sd_spec_multi_generate: gamma %d outside 1..16", gamma);
    SD_REQUIRE(reps && sampling && scratch && s && scratch->draft.logits && scratch->target.logits && dev_block && host_block &&
               s->host_seq, "sd_spec_multi_generate: null argument");
    const sd_sampling &sm = *sampling;
    const sd_spec_scratch &sc = *scratch;
    SD_REQUIRE(!random_seed || r_const, "sd_spec_multi_generate: random_seed needs its uniforms (r_const)");
    SD_REQUIRE(sm.V > 0 && sm.ld >= sm.V, "sd_spec_multi_generate: bad V / ld");
    for (int w = 0; w < width; ++w) {
        const sd_multi_replica &r = reps[w];
        SD_REQUIRE(r.draft && r.target && r.seq && r.q_hist && r.p_hist, "sd_spec_multi_generate: replica %d: null pointer", w);
        SD_REQUIRE(r.draft->m == reps[0].draft->m && r.target->m == reps[0].target->m && r.draft->max_seq == reps[0].draft->max_seq &&
                   r.target->max_seq == reps[0].target->max_seq && r.draft->kv_fp8 == reps[0].draft->kv_fp8 &&
                   r.target->kv_fp8 == reps[0].target->kv_fp8, "sd_spec_multi_generate: replica %d: sessions differ from replica 0's", w);
        SD_REQUIRE(!has_grammar(r.target), "sd_spec_multi_generate: replica %d: the target session carries a grammar: this loop has no "
                   "edit pass (detach it: sd_session_set_grammar(s, NULL, NULL, 0))", w);
    }
    const int g = gamma, W = width, n_err = 3 * g + 1;
    const int pass_rows = std::min(sc.max_rows_per_forward, reps[0].target->max_pass_rows);
    SD_REQUIRE(2 * W <= pass_rows && 2 * W <= std::min(reps[0].draft->max_rows, SD_MAX_ROWS),
               "sd_spec_multi_generate: width %d: a draft step may carry 2 rows per replica, a pass holds %d", W, pass_rows);
    SD_REQUIRE(g + 1 <= pass_rows, "sd_spec_multi_generate: gamma %d + 1 verify rows exceed one pass (%d rows)", g, pass_rows);
    SD_REQUIRE(s->len >= 1 && s->T + g + 1 <= seq_cap, "sd_spec_multi_generate: token buffers of %d hold T %d + gamma + 1", seq_cap, s->T);
    hipStream_t st = (hipStream_t)stream;
    sd_multi_result *res_dev = (sd_multi_result *)dev_block;
    int *err_dev = (int *)((char *)dev_block + sizeof(sd_multi_result));
    const sd_multi_result *res_host = (const sd_multi_result *)host_block;
    const int *err_host = (const int *)((const char *)host_block + sizeof(sd_multi_result));
    const size_t block_bytes = sd_spec_multi_block_bytes(W, g);
    const bool timed = s->draft_ms_out || s->target_ms_out;
    LoopEvents ev(timed ? 3 : 0, "sd_spec_multi_generate");
    if (!ev.ok) return SD_ERR_HIP;
    std::vector<sd_batch_item> items;
    std::vector<sd_norm_row> rows;
    sd_multi_item mitems[16];
    sd_multi_adopt_item aitems[16];
    for (int w = 0; w < W; ++w) {
        mitems[w].p_hist = reps[w].p_hist; mitems[w].q_hist = reps[w].q_hist; mitems[w].seq = reps[w].seq;
        aitems[w].draft_kv = reps[w].draft->kv; aitems[w].target_kv = reps[w].target->kv; aitems[w].seq = reps[w].seq;
    }
    const int res_mode = sc.target.norm_mode == sc.draft.norm_mode ? sc.target.norm_mode : 0;
    int eos_total = s->ori_eos_cnt;
    s->n_iters = s->err = 0;
    int rc = SD_OK;
    while (s->len < s->T && s->n_iters < s->max_iters) {
        const int L = s->len, d_lo = s->draft_len, t_lo = s->target_len, iters = s->n_iters;
        if (!(d_lo >= 0 && d_lo < L && t_lo >= 0 && t_lo < L + g)) {
            sd_set_error("sd_spec_multi_generate: cache lengths %d / %d do not fit a sequence of %d tokens", d_lo, t_lo, L);
            rc = SD_ERR_INVALID;
            break;
        }
        // ---- gamma draft steps, all replicas per pass over the draft weights
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[0], st));
        for (int i = 0; i < g && rc == SD_OK; ++i) {
            const uint64_t draw0 = s->draw;
            s->draw += (uint64_t)W;
            items.assign(W, sd_batch_item{});
            rows.assign(W, sd_norm_row{});
            for (int w = 0; w < W; ++w)                            // one shared stream: replica w takes draw0 + w
                draft_step_rows(items[w], rows[w], reps[w].draft, reps[w].seq, reps[w].q_hist, sm.ld, err_dev + w * n_err, g, L, i,
                                s->draft_len, s->seed, draw0 + (uint64_t)w);
            if ((rc = batch_forward(items.data(), W, sc.draft.logits, sc.draft.ld_logits, nullptr, nullptr, stream)) != SD_OK) break;
            NormRequest nr = norm_request(sm, sc.draft.norm_mode, scratch_rows(sc.draft));
            nr.rows = W; nr.workspace = sc.norm_workspace;
            rc = sd_norm_batch_tiles(nr, rows.data(), 1, stream);
            s->draft_len = L + i;
        }
        if (rc != SD_OK) break;
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[1], st));
        // ---- the target over every replica's uncached rows, whole replicas per pass
        const int n_new = L + g - t_lo;
        const int per_pass = std::max(1, pass_rows / n_new);
        for (int a = 0; a < W && rc == SD_OK; a += per_pass) {
            const int m = std::min(per_pass, W - a);
            items.assign(m, sd_batch_item{});
            rows.clear();
            for (int j = 0; j < m; ++j) {
                const sd_multi_replica &r = reps[a + j];
                verify_pass_rows(items[j], rows, r.target, r.seq, r.p_hist, sm.ld, err_dev + (a + j) * n_err, g, L, t_lo);
            }
            if ((rc = batch_forward(items.data(), m, sc.target.logits, sc.target.ld_logits, nullptr, nullptr, stream)) != SD_OK) break;
            NormRequest nr = norm_request(sm, sc.target.norm_mode, scratch_rows(sc.target));
            nr.rows = (int)rows.size(); nr.workspace = sc.norm_workspace;
            rc = sd_norm_batch_tiles(nr, rows.data(), 0, stream);
        }
        if (rc != SD_OK) break;
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[2], st));
        s->draw += (uint64_t)W;                                   // the target's own sample, drawn and thrown away
        // ---- replica scan + residual / bonus sample (one launch), winner broadcast (one launch), one copy, one wait
        if (random_seed) { s->seed = random_seed; s->draw = 0; }   // the reseed quirk: the stream restarts before the uniforms
        const uint64_t d_scan = s->draw;
        s->draw += (uint64_t)W * g;
        const uint64_t d_res = s->draw++;
        if ((rc = sd_multi_accept_resample(mitems, W, sm.ld, sm.V, L, g, r_const, s->seed, d_scan, d_res, res_dev, res_mode, stream)) != SD_OK)
            break;
        if ((rc = sd_multi_adopt(aitems, W, res_dev, L, g, d_lo, t_lo, kv_planes(reps[0].draft), reps[0].draft->max_seq,
                                 kv_row_bytes(reps[0].draft), kv_planes(reps[0].target), reps[0].target->max_seq,
                                 kv_row_bytes(reps[0].target), seq_cap, stream)) != SD_OK)
            break;
        SD_LOOP_HIP(hipMemcpyAsync(host_block, dev_block, block_bytes, hipMemcpyDeviceToHost, st));
        SD_LOOP_HIP(hipEventRecord(ev.done, st));
        if ((rc = poll_event(ev.done, "sd_spec_multi_generate")) != SD_OK) break;
        // error words first, a draft sample word before a norm word (multi.py: the scan's result is not looked at then,
        // and the resample draw is not taken)
        bool any = false, samp = false;
        for (int w = 0; w < W; ++w)
            for (int i = 0; i < n_err; ++i)
                if (err_host[w * n_err + i]) { any = true; samp = samp || (i >= g && i < 2 * g); }
        if (any) {
            s->err = samp ? 1 : 2;
            --s->draw;
            if (s->acc_len_out) s->acc_len_out[iters] = -1;       // the iteration ran (it counts as a call) but was not scanned
            ++s->n_iters;
            break;
        }
        const sd_accept_result r = res_host->chosen;
        const int l = r.n_accepted, n = r.n;
        if (!(res_host->choice >= 0 && res_host->choice < W && l >= 0 && l <= g && n == L + l - 1)) {
            sd_set_error("sd_spec_multi_generate: inconsistent result block (choice %d, n %d, L %d, accepted %d)", res_host->choice,
                         n, L, l);
            rc = SD_ERR_INVALID;
            break;
        }
        if (timed) {
            float dms = 0.f, tms = 0.f;
            SD_LOOP_HIP(hipEventElapsedTime(&dms, ev.t[0], ev.t[1]));
            SD_LOOP_HIP(hipEventElapsedTime(&tms, ev.t[1], ev.t[2]));
            if (s->draft_ms_out) s->draft_ms_out[iters] = dms;
            if (s->target_ms_out) s->target_ms_out[iters] = tms;
        }
        if (s->acc_len_out) s->acc_len_out[iters] = l;
        for (int w = 0; w < W; ++w)                               // (the block keeps 16 ratios per replica)
            log_ratios(s->p_at_out, s->q_at_out, (size_t)iters * W + w, g, res_host->p_at + w * 16, res_host->q_at + w * 16);
        ++s->n_iters;
        if (!commit_result(r, L, g, s->host_seq, &s->len, &s->draft_len, &s->target_len)) { s->err = 1; break; }   // the resample raised
        if (r.flags & 4) s->target_len = L + g;
        for (int i = L; i < s->len; ++i) eos_total += s->host_seq[i] == sm.eos_token_id;
        if (eos_total > s->ori_eos_cnt) break;                    // the caller cuts after the first new EOS
    }
    return rc;
}

// ---- autoregressive sampling of up to 16 lock-step streams (reference autoregressive_sampling.py:9-61 per stream)
// What one step hands to the host: per stream its fresh token and flag bits (1 sample error, 2 norm error, 4 token == eos)
struct ArSlot { int32_t token, flags; };
// The streams of one step by value, indexed by stream; a stream that sits the step out has seq == NULL
struct ArTab {
    const int32_t *seq[16];
    int *err[16];                 // {norm error, sample error}
    int len[16];                  // the step sampled seq[len]
};

// One 64-lane workgroup, lane b for stream b: the 8-byte slot of every stream in one vector store each, and the two error
// words cleared for the next step.  Ordered behind the sampler by the stream alone.
__global__ __launch_bounds__(64) void ar_collect_kernel(ArTab t, int n_streams, int eos, ArSlot *__restrict__ out) {
    const int b = threadIdx.x;
    if (b >= n_streams || b >= 16) return;
    ArSlot s = {0, 0};
    if (t.seq[b]) {
        int *e = t.err[b];
        s.token = t.seq[b][t.len[b]];
        s.flags = (e[1] != 0 ? 1 : 0) | (e[0] != 0 ? 2 : 0) | (s.token == eos ? 4 : 0);
        e[0] = 0; e[1] = 0;
    }
    *reinterpret_cast<int2 *>(out + b) = make_int2(s.token, s.flags);
}

extern "C" size_t sd_ar_block_bytes(int n_streams) {
    if (n_streams < 1 || n_streams > 16) return 0;
    return ((size_t)n_streams * sizeof(ArSlot) + 15) & ~(size_t)15;
}

extern "C" int sd_ar_batch_generate(sd_ar_stream *streams, int n_streams, const sd_sampling *sampling, const sd_head_scratch *head,
                                    void *norm_workspace, void *dev_block, void *host_block, sd_ar_log *log, void *stream,
                                    const sd_loop_opts *opts) {
    SD_REQUIRE(n_streams >= 1 && n_streams <= 16, "sd_ar_batch_generate: n_streams %d outside 1..16", n_streams);
    SD_REQUIRE(streams && sampling && head && log && head->logits && dev_block && host_block, "sd_ar_batch_generate: null argument");
    const sd_sampling &sm = *sampling;
    SD_REQUIRE(sm.V > 0 && sm.ld >= sm.V && sm.temperature != 0.0f, "sd_ar_batch_generate: bad V / ld / temperature");
    for (int b = 0; b < n_streams; ++b) {
        const sd_ar_stream &s = streams[b];
        SD_REQUIRE(s.session && s.seq && s.probs && s.err_words && s.host_seq, "sd_ar_batch_generate: stream %d: null pointer", b);
        SD_REQUIRE(s.len >= 1 && s.cache_len >= 0 && s.cache_len < s.len, "sd_ar_batch_generate: stream %d: cache_len %d of %d tokens",
                   b, s.cache_len, s.len);
        SD_REQUIRE(n_streams == 1 || s.cache_len == s.len - 1,
                   "sd_ar_batch_generate: stream %d: with more than one stream every stream arrives prefilled (cache_len %d, len %d - 1)",
                   b, s.cache_len, s.len);
    }
    for (int b = 0; b < n_streams; ++b)
        SD_REQUIRE(streams[b].session->m == streams[0].session->m, "sd_ar_batch_generate: stream %d: session of another model", b);
    SD_REQUIRE(n_streams <= streams[0].session->max_pass_rows, "sd_ar_batch_generate: %d streams exceed one pass (%d rows)", n_streams,
               streams[0].session->max_pass_rows);
    LoopOpts o;
    const sd_session *ts[16];
    int states_need[16];
    for (int b = 0; b < n_streams; ++b) { ts[b] = streams[b].session; states_need[b] = streams[b].T - streams[b].len + 2; }
    if (int rc = resolve_loop_opts("sd_ar_batch_generate", "stream", opts, n_streams, sm.V, n_streams, sm.eos_token_id, false, &o, ts,
                                   n_streams);
        rc != SD_OK)
        return rc;
    if (int rc = check_grammar_states("sd_ar_batch_generate", "stream", ts, n_streams, states_need); rc != SD_OK) return rc;
    const sd_logprob_block *const lp = o.lp;
    const RowEdits *const re = o.re;
    hipStream_t st = (hipStream_t)stream;
    const bool timed = log->step_ms_out != nullptr;
    LoopEvents ev(timed ? 2 : 0, "sd_ar_batch_generate");
    if (!ev.ok) return SD_ERR_HIP;
    const bool tiles_ok = head_tiles_ok(sm.top_k, sm.temperature, sm.V, sm.ld);
    const ArSlot *slots = (const ArSlot *)host_block;
    std::vector<sd_batch_item> items;
    std::vector<sd_norm_row> rows;
    int act[16], L0[16];                                          // (L0, logprobs: the streams' lengths on entry)
    for (int b = 0; b < n_streams; ++b) { streams[b].done = 0; streams[b].steps = 0; L0[b] = streams[b].len; }
    log->n_steps = log->err = 0;
    int rc = SD_OK;
    for (;;) {
        int n = 0;
        for (int b = 0; b < n_streams; ++b) {
            sd_ar_stream &s = streams[b];
            if (!s.done && s.len >= s.T) s.done = 1;
            if (!s.done) act[n++] = b;
        }
        if (n == 0) break;
        // ---- an autoregressive step is draft step 0 of a gamma = 1 iteration run on the stream's own model: the uncached
        // rows, logits for the last, sampled with (seed, draw) into seq[len]; error words {norm, sample}
        items.assign(n, sd_batch_item{});
        rows.assign(n, sd_norm_row{});
        ArTab tab = {};
        HeadReq rq = {};
        HeadOut ho = {};
        rq.raw = true;                                            // the lock-step draft step's sampler feed (see there)
        bool pen_step = false;                                    // a step with a penalised or edited stream takes no tile maxima
        for (int j = 0; re && j < n; ++j) pen_step = pen_step || re->edited(act[j], streams[act[j]].session);
        rq.zero_n = tiles_ok && !pen_step ? n : 0;
        for (int j = 0; j < n; ++j) {
            sd_ar_stream &s = streams[act[j]];
            draft_step_rows(items[j], rows[j], s.session, s.seq, s.probs, sm.ld, s.err_words, 1, s.len, 0, s.cache_len, s.seed, s.draw);
            rq.zero_ptr[j] = rows[j].probs_out;
            tab.seq[act[j]] = s.seq; tab.err[act[j]] = s.err_words; tab.len[act[j]] = s.len;
        }
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[0], st));
        if (n_streams == 1 && items[0].n_new > 1)                 // the prompt: chunked like the interpreter loop's first forward
            rc = feed_rows(items[0].session, items[0].seq, items[0].pos0, items[0].pos0 + items[0].n_new, 1, head->logits, head->ld_logits,
                           &rq, &ho, stream);
        else
            rc = batch_forward(items.data(), n, head->logits, head->ld_logits, &rq, &ho, stream);
        if (rc != SD_OK) break;
        NormRequest nr = norm_request(sm, head->norm_mode, ho);
        if (pen_step) {                                           // stream act[j]'s one row, at position len - 1
            sd_logit_edit_item pi[16];
            const sd_session *ps[16];
            for (int j = 0; j < n; ++j) {
                const sd_ar_stream &s = streams[act[j]];
                pi[j] = edit_item(*re, act[j], ho, j, 1, s.seq, s.len - 1, L0[act[j]]);
                ps[j] = s.session;
            }
            if ((rc = edit_rows(*re, pi, n, sm.V, nr.mode, stream, ps)) != SD_OK) break;
            norm_from_edited(nr, *re);
        }
        nr.rows = n; nr.workspace = norm_workspace;
        if ((rc = sd_norm_batch_tiles(nr, rows.data(), 1, stream)) != SD_OK) break;
        if (lp) {                                                 // behind the sampler: stream b's one row, scored at seq[len]
            sd_logprob_item li[16];
            for (int j = 0; j < n; ++j) {
                const sd_ar_stream &s = streams[act[j]];
                li[j] = sd_logprob_item{ho.logits + (size_t)j * ho.ld, ho.ld, 1, s.seq + s.len, nullptr, lp->dev + (size_t)act[j] * LP_SLICE};
            }
            if ((rc = sd_token_logprobs(li, n, sm.V, ho.round | head->norm_mode, stream)) != SD_OK) break;
            SD_LOOP_HIP(hipMemcpyAsync(lp->host, lp->dev, sizeof(float) * ((size_t)(n_streams - 1) * LP_SLICE + 1), hipMemcpyDeviceToHost, st));
        }
        // ---- the hand-off: 8 bytes per stream, one copy, one wait
        hipLaunchKernelGGL(ar_collect_kernel, dim3(1), dim3(64), 0, st, tab, n_streams, sm.eos_token_id, (ArSlot *)dev_block);
        SD_LOOP_HIP(hipGetLastError());
        SD_LOOP_HIP(hipMemcpyAsync(host_block, dev_block, sizeof(ArSlot) * (size_t)n_streams, hipMemcpyDeviceToHost, st));
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[1], st));
        SD_LOOP_HIP(hipEventRecord(ev.done, st));
        if ((rc = poll_event(ev.done, "sd_ar_batch_generate")) != SD_OK) break;
        if (log->n_steps < log->max_steps_log) {
            float ms = 0.f;
            if (timed && hipEventElapsedTime(&ms, ev.t[0], ev.t[1]) == hipSuccess) log->step_ms_out[log->n_steps] = ms;
            if (log->step_streams_out) log->step_streams_out[log->n_steps] = n;
        }
        ++log->n_steps;
        int flags = 0;
        for (int j = 0; j < n; ++j) flags |= slots[act[j]].flags;
        // the norm word first: the reference normalises before it samples (autoregressive_sampling.py:48-50), and the fused
        // sampler sets both words on a row it cannot normalise
        if (flags & 3) { log->err = (flags & 2) ? 2 : 1; break; }
        for (int j = 0; j < n; ++j) {
            sd_ar_stream &s = streams[act[j]];
            const ArSlot r = slots[act[j]];
            s.host_seq[s.len] = r.token;
            if (lp) lp->logprob_out[act[j]][s.len - L0[act[j]]] = lp->host[(size_t)act[j] * LP_SLICE];
            s.cache_len = s.len;                                  // every token but the new one is cached
            ++s.len; ++s.draw; ++s.steps;
            if (r.flags & 4) s.done = 1;                          // the EOS is kept (:55)
        }
    }
    return rc;
}
