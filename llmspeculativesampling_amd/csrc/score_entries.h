// score_entries.h - token scoring (include/specdec.h has the definition): sd_score_rows, the launch of score_kernels.h, and
// sd_score_sequence, the scoring pass over a whole sequence.  Host code, included by spec_loops.h behind feed_rows.
#pragma once

static_assert(SD_SCORE_MAX_ROWS >= SD_MAX_ROWS, "one sd_score_rows launch takes every row of a pass of logit rows");

extern "C" int sd_score_rows(const sd_score_item *items, int n_items, int V, int top_n, int mode, void *stream) {
    SD_REQUIRE(items, "sd_score_rows: null argument");
    SD_REQUIRE(n_items >= 1 && n_items <= SCORE_MAX_ITEMS, "sd_score_rows: n_items %d outside 1..%d", n_items, SCORE_MAX_ITEMS);
    SD_REQUIRE(V >= 1 && (mode & 3) != 3, "sd_score_rows: V %d, mode %#x", V, mode);
    SD_REQUIRE(top_n >= 0 && top_n <= SD_SCORE_MAX_TOP, "sd_score_rows: top_n %d outside 0..%d", top_n, SD_SCORE_MAX_TOP);
    ScoreTab t = {};
    int max_rows = 0;
    for (int i = 0; i < n_items; ++i) {
        const sd_score_item &it = items[i];
        SD_REQUIRE(it.logits && it.tokens && it.logprob, "sd_score_rows: item %d: null argument", i);
        SD_REQUIRE(top_n == 0 || (it.top_ids && it.top_logprobs), "sd_score_rows: item %d: top_n %d and a null top array", i, top_n);
        SD_REQUIRE(it.rows >= 1 && it.rows <= SD_SCORE_MAX_ROWS, "sd_score_rows: item %d: rows %d outside 1..%d", i, it.rows,
                   SD_SCORE_MAX_ROWS);
        SD_REQUIRE(it.ld >= V, "sd_score_rows: item %d: ld %ld < V %d", i, it.ld, V);
        t.logits[i] = it.logits; t.tokens[i] = it.tokens; t.logprob[i] = it.logprob; t.rank[i] = it.rank;
        t.top_ids[i] = it.top_ids; t.top_logprobs[i] = it.top_logprobs; t.ld[i] = it.ld; t.rows[i] = it.rows;
        max_rows = std::max(max_rows, (int)it.rows);
    }
    return launch_score_rows(t, n_items, max_rows, V, top_n, mode & 3, (hipStream_t)stream);
}

extern "C" int sd_score_sequence(sd_session *s, const int32_t *tokens, int n, int first, int top_n, float *slab, long ld_slab,
                                 int slab_rows, const sd_score_out *out, void *stream) {
    SD_REQUIRE(s && tokens && slab && out && out->logprob, "sd_score_sequence: null argument");
    SD_REQUIRE(top_n >= 0 && top_n <= SD_SCORE_MAX_TOP, "sd_score_sequence: top_n %d outside 0..%d", top_n, SD_SCORE_MAX_TOP);
    SD_REQUIRE(top_n == 0 || (out->top_ids && out->top_logprobs), "sd_score_sequence: top_n %d and a null top array", top_n);
    SD_REQUIRE(n >= 2, "sd_score_sequence: n %d < 2: a token is scored on the row of the one before it", n);
    SD_REQUIRE(first >= 1 && first <= n - 1, "sd_score_sequence: first %d outside 1..%d", first, n - 1);
    SD_REQUIRE(slab_rows >= 1, "sd_score_sequence: slab_rows %d < 1", slab_rows);
    const int V = s->m->cfg.vocab;
    SD_REQUIRE(ld_slab >= V, "sd_score_sequence: ld_slab %ld < V %d", ld_slab, V);
    SD_REQUIRE(n - 1 <= s->max_seq, "sd_score_sequence: %d positions, max_seq %d", n - 1, s->max_seq);
    SD_REQUIRE(!s->tp, "sd_score_sequence: the session is bound to a tensor-parallel group");
    refresh_env();
    int rc;
    // the prompt: positions [0, first - 1), no logit rows
    if (first > 1 && (rc = feed_rows(s, tokens, 0, first - 1, 0, nullptr, 0, nullptr, nullptr, stream)) != SD_OK) return rc;
    // positions [first - 1, n - 1): every row of a pass is a logit row, scored where the head left it
    HeadReq rq = {};
    rq.raw = true;
    const int per_pass = std::max(1, std::min(slab_rows, s->max_pass_rows));
    for (int pos = first - 1, m; pos < n - 1; pos += m) {
        m = std::min(per_pass, n - 1 - pos);
        HeadOut ho = {};
        if ((rc = session_forward(s, tokens + pos, m, pos, m, slab, ld_slab, &rq, &ho, stream)) != SD_OK) return rc;
        const size_t j = (size_t)(pos - (first - 1));
        const sd_score_item it = {ho.logits, ho.ld, m, tokens + pos + 1, out->logprob + j, out->rank ? out->rank + j : nullptr,
                                  top_n ? out->top_ids + j * top_n : nullptr, top_n ? out->top_logprobs + j * top_n : nullptr};
        if ((rc = sd_score_rows(&it, 1, V, top_n, ho.round, stream)) != SD_OK) return rc;
    }
    return SD_OK;
}
