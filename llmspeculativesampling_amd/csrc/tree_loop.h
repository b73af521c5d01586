// tree_loop.h - the native loop of token-tree speculative sampling (sd_tree_generate; include/specdec.h has the contract,
// DESIGN.md the method).  Host code, included behind spec_loops.h at the end of engine.hip: it uses that file's loop
// helpers (LoopEvents, poll_event, SD_LOOP_HIP) and the engine's forward_tree_rows / session_forward, and reaches the
// sampler through the public entries (sd_norm_probs, sd_tree_draw, sd_tree_accept).  Single stream, device Philox.
#pragma once

// ARENA INVARIANT.  At the top of every iteration both arenas hold exactly the len - 1 positions in front of the root.
// During it the draft arena holds the tree's nodes of levels 0 .. D - 1 at slots base + node id (one forward_tree_from call
// per level, no node forwarded twice), the target arena all n nodes.  After the accept walk both keep the path: slot
// base + path[j] -> base + j.  A leaf the walk ended at is the one node the draft never forwarded: its K / V row is
// appended by a one-row draft forward without logits right behind the compaction (position base + D, a plain causal
// row by then), so the invariant holds again with len grown by depth + 1.
// ABSENT SLOTS (token -1: fewer tokens with mass than slots, as on every top_k = 1 call with b > 1) and their subtrees keep
// their rows in both passes - the tree's shape, and with it the row tables, never vary: the embedding clamps -1 to token 0
// (embed_kernel, model_kernels.h), the rows are computed, sd_tree_draw gives such a parent no children and sd_tree_accept
// skips the slot, so nothing reads their logits and no kept path holds their K / V rows.
static_assert(SD_TREE_MAX_NODES == SD_MAX_TREE, "the sampler's node limit is the tree forward's (64-bit ancestor masks)");
extern "C" int sd_tree_generate(const sd_tree_stream *dev, const int32_t *branching, int depth, const sd_sampling *sampling,
                                const sd_spec_scratch *scratch, sd_seq_state *s, void *stream) {
    SD_REQUIRE(dev && branching && sampling && scratch && s, "sd_tree_generate: null argument");
    SD_REQUIRE(dev->draft && dev->target && dev->tokens && dev->q_rows && dev->p_rows && dev->workspace && dev->err_words &&
               dev->path_idx && dev->res_dev && dev->res_host && s->host_seq && scratch->draft.logits && scratch->target.logits,
               "sd_tree_generate: null argument");
    sd_tree_topology tp;
    if (int rc = sd_tree_topology_fill(branching, depth, &tp); rc != SD_OK) return rc;
    const sd_sampling &sm = *sampling;
    const sd_spec_scratch &sc = *scratch;
    sd_session *draft = dev->draft, *target = dev->target;
    SD_REQUIRE(sm.temperature != 0.0f, "sd_tree_generate: temperature must be non-zero");
    SD_REQUIRE(sm.V > 0 && sm.ld >= sm.V && sm.V == draft->m->cfg.vocab && sm.V == target->m->cfg.vocab,
               "sd_tree_generate: V %d (ld %ld), the models' vocabularies are %d / %d", sm.V, sm.ld, draft->m->cfg.vocab,
               target->m->cfg.vocab);
    SD_REQUIRE(s->len >= 1 && s->draft_len == s->len - 1 && s->target_len == s->len - 1,
               "sd_tree_generate: cache lengths %d / %d: both models must hold the %d tokens in front of the root", s->draft_len,
               s->target_len, s->len - 1);
    const int n = tp.n, D = tp.depth, P = tp.level_start[D];       // P: the nodes with children are ids 0 .. P - 1
    const int widest = tp.level_start[D] - tp.level_start[D - 1];   // the draft's last call: level D - 1
    SD_REQUIRE(n <= target->max_rows && widest <= draft->max_rows && n <= SD_STREAM_MAX_ROWS,
               "sd_tree_generate: a tree of %d nodes (widest draft level %d) exceeds the sessions' max_rows %d / %d", n, widest,
               target->max_rows, draft->max_rows);
    SD_REQUIRE(!draft->tp && !target->tp, "sd_tree_generate: tensor-parallel sessions are not supported");
    SD_REQUIRE(!has_grammar(target) && !has_grammar(draft), "sd_tree_generate: a session carries a grammar: this loop has no edit pass");
    hipStream_t st = (hipStream_t)stream;
    const bool timed = s->draft_ms_out || s->target_ms_out;
    LoopEvents ev(timed ? 3 : 0, "sd_tree_generate");
    if (!ev.ok) return SD_ERR_HIP;
    uint64_t masks[SD_TREE_MAX_NODES];
    int32_t pos[SD_TREE_MAX_NODES];
    masks[0] = 1ull;
    for (int i = 1; i < n; ++i) masks[i] = masks[tp.parent[i]] | (1ull << i);
    auto norm_ws = [&](int rows) { return rows <= sc.max_rows_per_forward ? sc.norm_workspace : nullptr; };
    int eos_total = s->ori_eos_cnt;
    s->n_iters = s->err = 0;
    int rc = SD_OK;
    while (s->len < s->T && s->n_iters < s->max_iters) {
        const int L = s->len, base = L - 1, iters = s->n_iters;
        if (base + n > draft->max_seq || base + n > target->max_seq) {
            sd_set_error("sd_tree_generate: %d positions + %d nodes exceed the arenas (%d / %d)", base, n, draft->max_seq, target->max_seq);
            rc = SD_ERR_CAPACITY;
            break;
        }
        for (int i = 0; i < n; ++i) pos[i] = base + tp.level[i];
        const uint64_t w0 = s->draw;
        s->draw += (uint64_t)(P + n);
        // ---- the draft grows the tree: level d's nodes forward, their rows normalise, their children are drawn
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[0], st));
        for (int d = 0; d < D && rc == SD_OK; ++d) {
            const int first = tp.level_start[d], cnt = tp.level_start[d + 1] - first, b = tp.branching[d];
            if ((rc = forward_tree_rows("sd_tree_generate (draft)", draft, dev->tokens, pos, masks, first, first + cnt, base, cnt,
                                        sc.draft.logits, sc.draft.ld_logits, stream)) != SD_OK) break;
            if ((rc = sd_norm_probs(sc.draft.logits, cnt, sm.V, sc.draft.ld_logits, sm.temperature, sm.top_k, sm.top_p,
                                    sc.draft.norm_mode, dev->q_rows + (size_t)first * sm.ld, sm.ld, dev->err_words + first,
                                    norm_ws(cnt), stream)) != SD_OK) break;
            rc = sd_tree_draw(dev->q_rows + (size_t)first * sm.ld, cnt, sm.V, sm.ld, b, dev->tokens + first, nullptr, 0, s->seed,
                              w0 + (uint64_t)first, dev->tokens + tp.level_start[d + 1], b, stream);
        }
        if (rc != SD_OK) break;
        // ---- one target pass over all n nodes
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[1], st));
        if ((rc = forward_tree_rows("sd_tree_generate (target)", target, dev->tokens, pos, masks, 0, n, base, n, sc.target.logits,
                                    sc.target.ld_logits, stream)) != SD_OK) break;
        if ((rc = sd_norm_probs(sc.target.logits, n, sm.V, sc.target.ld_logits, sm.temperature, sm.top_k, sm.top_p,
                                sc.target.norm_mode, dev->p_rows, sm.ld, dev->err_words + SD_TREE_MAX_NODES, norm_ws(n), stream)) != SD_OK)
            break;
        if (timed) SD_LOOP_HIP(hipEventRecord(ev.t[2], st));
        // ---- the accept walk (one launch), one copy, one wait
        if ((rc = sd_tree_accept(&tp, dev->tokens, dev->p_rows, dev->q_rows, sm.ld, sm.V, dev->workspace, nullptr, nullptr, s->seed,
                                 w0 + (uint64_t)P, w0 + (uint64_t)(P + n - 1), dev->res_dev, dev->path_idx, dev->tokens,
                                 dev->err_words, 2 * SD_TREE_MAX_NODES, stream)) != SD_OK) break;
        SD_LOOP_HIP(hipMemcpyAsync(dev->res_host, dev->res_dev, sizeof(sd_tree_result), hipMemcpyDeviceToHost, st));
        SD_LOOP_HIP(hipEventRecord(ev.done, st));
        if ((rc = poll_event(ev.done, "sd_tree_generate")) != SD_OK) break;
        const sd_tree_result r = *dev->res_host;
        ++s->n_iters;
        if (r.flags & (8 | 2)) {                                   // a norm word first, as the reference raises in that order
            s->err = (r.flags & 8) ? 2 : 1;
            if (s->acc_len_out) s->acc_len_out[iters] = -1;
            break;
        }
        const int a = r.depth;
        bool sane = a >= 0 && a <= D && r.path[0] == 0 && r.next_token >= 0 && r.next_token < sm.V;
        for (int j = 1; sane && j <= a; ++j) sane = r.path[j] > r.path[j - 1] && r.path[j] < n && tp.parent[r.path[j]] == r.path[j - 1];
        if (!sane) {
            sd_set_error("sd_tree_generate: inconsistent result block (depth %d, next token %d)", a, r.next_token);
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
        if (s->acc_len_out) s->acc_len_out[iters] = a;
        // ---- both arenas keep the path (see the invariant above)
        const bool leaf = a == D;
        if (a >= 1) {
            if ((rc = sd_session_compact_kv(target, base, dev->path_idx, a + 1, stream)) != SD_OK) break;
            if ((rc = sd_session_compact_kv(draft, base, dev->path_idx, leaf ? a : a + 1, stream)) != SD_OK) break;
            if (leaf && (rc = session_forward(draft, dev->tokens + r.path[a], 1, base + a, 0, nullptr, 0, nullptr, nullptr, stream)) != SD_OK)
                break;
        }
        for (int j = 1; j <= a; ++j) s->host_seq[s->len++] = r.tokens[j];
        s->host_seq[s->len++] = r.next_token;
        s->draft_len = s->target_len = base + a + 1;
        for (int i = L; i < s->len; ++i) eos_total += s->host_seq[i] == sm.eos_token_id;
        if (eos_total > s->ori_eos_cnt) break;                    // the caller cuts after the first new EOS
    }
    return rc;
}
