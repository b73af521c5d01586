"""Grammar-constrained decoding (`pytest -m gpu`): sd_grammar_rows bit for bit against apply_grammar o apply_logit_edits o
apply_penalties on the CPU, with the state cache held to a host simulation; the launch's purity under the overlap the draft
steps and the verify produce; the refusals that read a session; and the five native entries against the CPU oracle run on
models whose logits carry the grammar mask (tests/grammar_model.py), each prompt under its own Philox variates."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle
from grammar_model import GrammarModel
from philox_replay import PhiloxOracleNoise
from test_gpu_logit_edits import N_ROWS, SPECIAL_IDS
from test_gpu_logprobs import _bf16_pair, _corr_oracles
from test_gpu_native_parity import _st
from test_gpu_penalties import BUDGETS, ITEMS, LENS, MODES, PARAMS, ROWS, SEEDS, SENTINEL, _as_read, _loop_prompts, _same_bits
from test_gpu_spec_queue import _models, _prompts
from test_grammar_cpu import grammar_a
from llmspeculativesampling_amd.sampling import TokenGrammar
from llmspeculativesampling_amd.sampling._loop_common import allowed_mask_words
from llmspeculativesampling_amd.sampling.utils import apply_grammar, apply_logit_edits, apply_penalties

pytestmark = pytest.mark.gpu

NEUTRAL_PEN = (1.0, 0.0, 0.0)
POISON, GUARD = 0x5A5A5A5A, -77                                   # planted in states[j0 ..) / behind states[j0 + rows) and in front of j0 - 1


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


# ----------------------------------------------------------------------------- K: the kernel
def _random_grammar(V, n_states, identity, rng):
    """next with about a third of its entries -1; class 0 (token 0 with identity classes) is allowed everywhere, so no state
    is empty."""
    K = V if identity else 7
    nxt = rng.integers(0, n_states, size=(n_states, K))
    nxt[rng.random((n_states, K)) < 0.33] = -1
    nxt[:, 0] = rng.integers(0, n_states, size=n_states)
    return TokenGrammar(nxt, int(rng.integers(0, n_states)), 2, V, classes=None if identity else np.arange(V) % 7)


def _walk(g, state, n, rng, V, bad_at=None, bad_token=None):
    """n output tokens along allowed transitions from `state`; at index bad_at a token the state does not allow (or
    bad_token), behind which the tokens are random."""
    toks, s = [], state
    for k in range(n):
        if s < 0 or k == bad_at:
            if k == bad_at and bad_token is not None:
                t = bad_token
            elif s >= 0:
                allowed = set(g.allowed_ids(s).tolist())
                t = next(int(t) for t in rng.permutation(V) if int(t) not in allowed)
            else:
                t = int(rng.integers(0, V))
        else:
            t = int(rng.choice(g.allowed_ids(s)))
        toks.append(t)
        s = g.step(s, t)
    return toks


# per item: (grammar index or None, j0, what goes wrong in the history, edits).  Grammars: 0 = 5 states / id mod 7, 1 = 40 states
# / id mod 7, 2 = 5 states / identity, 3 = 40 states / identity.  Edits: a = allowed mask, b = bias, p = penalties, m = min_tokens.
ITEM_TABLE = [
    (0, 0, None, ""),            # 17 rows from the start state
    (1, 7, None, "a"),           # 1 row behind a cached state
    (2, -3, None, "b"),          # 16 rows, the first three inside the prompt
    (3, 0, None, "p"),           # 2 rows
    (0, 0, ("bad", 4), "abp"),   # 9 rows: output token 4 is not allowed, rows 5.. are dead and unmasked
    (None, 3, None, "abp"),      # 17 rows without a grammar: sd_edit_rows' output
    (2, 6, None, ""),            # 3 rows
    (1, 2, ("big", 7), "a"),     # 17 rows: output token 7 is an id >= V
    (0, -5, None, "p"),          # 8 rows, five inside the prompt
    (3, 9, None, "am"),          # 17 rows behind a cached state, EOS floored for some
    (1, 3, ("bad", 4), ""),      # 4 rows: dead from row 2 on
    (2, 0, None, "abpm"),        # 17 rows, every edit
    (0, 1, None, ""),            # 17 rows, output rows misaligned against the input (scalar throughout)
    (None, 0, None, ""),         # 6 rows without a grammar and without edits: rounded and copied
    (1, 4, ("cache", -1), "b"),  # 17 rows behind a cached state that is dead: every row unmasked
    (3, -2, None, "a"),          # 12 rows
]
P_LEN = 11                                                        # every item's prompt


@functools.lru_cache(maxsize=None)
def _kernel_case(V):
    rng = np.random.default_rng(V + 5)
    grammars = [_random_grammar(V, n, ident, rng) for n, ident in ((5, False), (40, False), (5, True), (40, True))]
    x = torch.from_numpy(rng.standard_normal((ITEMS * ROWS, V)).astype(np.float32)) * 8
    x[:, SPECIAL_IDS] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])
    x[:, V - 1] = float("nan")
    x[::2, 0] = -0.0
    items = []
    for i, (gi, j0, wrong, edits) in enumerate(ITEM_TABLE):
        rows = N_ROWS[i]
        g = grammars[gi] if gi is not None else None
        n_out = max(j0, 0) + rows                                  # output tokens in seq: rows read seq[P .. P + j0 + rows - 1)
        bad_at, bad_token, cached = None, None, None
        if wrong and wrong[0] == "bad":
            bad_at = wrong[1]
        if wrong and wrong[0] == "big":
            bad_at, bad_token = wrong[1], V + 3
        out = _walk(g, g.start, n_out, rng, V, bad_at, bad_token) if g else rng.integers(0, V, size=n_out).tolist()
        prompt = rng.integers(0, V, size=P_LEN).tolist()
        seq = prompt + out
        # the states the definition gives: s_j = start for j <= 0, then along the output tokens
        states = {}
        if g:
            if wrong and wrong[0] == "cache":
                cached = wrong[1]
            elif j0 >= 1:
                cached = g.state_after(out[:j0 - 1])
            for r in range(rows):
                j = j0 + r
                if j <= 0:
                    states[j] = g.start
                else:
                    base = max(j0 - 1, 0)
                    s0 = cached if j0 >= 1 else g.start
                    states[j] = g.state_after(out[base:j], s0 if 0 <= s0 < g.n_states else -1)
        spec = dict(g=g, gi=gi, j0=j0, rows=rows, seq=seq, hist0=P_LEN + j0, states=states, cached=cached,
                    pen=(1.8, 1.5, -0.7) if "p" in edits else NEUTRAL_PEN, bias={}, mask=None, m=0, eos=int(rng.integers(0, V)))
        if "b" in edits:
            ids = sorted({0, 3, 4095, 4096, 4097, 4099, V - 1, *SPECIAL_IDS, *rng.choice(V, size=20, replace=False).tolist()} & set(range(V)))
            spec["bias"] = dict(zip(ids, (rng.standard_normal(len(ids)) * 5).astype(np.float32).tolist()))
        if "a" in edits:
            spec["mask"] = allowed_mask_words(V, rng.choice(V, size=V // 2, replace=False).tolist(), [14])
        if "m" in edits:
            spec["m"] = max(1, j0 + rows // 2)                    # j crosses it inside the item's rows
        items.append(spec)
    return grammars, x, items


@pytest.mark.parametrize("V", [8229, 130])
@pytest.mark.parametrize("mode", ["fp32", "dt_bf16", "dt_f16"])
def test_k1_kernel_bit_for_bit_against_the_definitions(hip, mode, V):
    """One launch of 16 items x 1..17 rows over slabs of odd row stride; item i's input rows start i % 4 elements past a 16-byte
    boundary, the output rows of items 12..15 at another offset (scalar throughout).  V = 8229 is three windows with a last mask
    word 5 bits wide; V = 130 one window.  Every row equals apply_grammar(apply_logit_edits(apply_penalties(row)), s_j) with s_j
    from the host simulation - rows inside the prompt and dead rows unmasked -; states[max(j0, 0) .. j0 + rows) equals the
    simulation where poison stood, the guards around it and the cached states[j0 - 1] keep their values; the NULL-grammar items
    equal sd_edit_rows' own output; rows past an item's count, the padding columns and the input keep their bytes; a second
    run gives the same bytes."""
    m = MODES[mode]
    grammars, x, specs = _kernel_case(V)
    if m & 48 and not m & 3:
        x = _as_read(x, m).float()
    ld = V + 2 if V % 2 else V + 3                                # odd
    assert ld % 2 == 1
    span = (ROWS * ld + 4 + 3) // 4 * 4
    in_off = [i % 4 for i in range(ITEMS)]
    out_off = [o if i < 12 else (o + 1 + i % 3) % 4 for i, o in enumerate(in_off)]
    slab = torch.zeros(ITEMS * span + 4, dtype=torch.float32)
    for i in range(ITEMS):
        slab[i * span + in_off[i]:][:ROWS * ld].view(ROWS, ld)[:, :V] = x[i * ROWS:(i + 1) * ROWS]
    dev_in = slab.cuda()
    keep = dev_in.clone()
    out = torch.full((ITEMS * span + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    out_edit = torch.full((ITEMS * span + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    seqs = [torch.tensor(s["seq"], dtype=torch.int64).to(torch.int32).cuda() for s in specs]
    ids = [torch.tensor(sorted(s["bias"]), dtype=torch.int32).cuda() for s in specs]
    vals = [torch.tensor([s["bias"][t] for t in sorted(s["bias"])], dtype=torch.float32).cuda() for s in specs]
    masks = [torch.from_numpy(s["mask"].view(np.int32)).cuda() if s["mask"] is not None else None for s in specs]
    devg = [g.to_device("cuda") for g in grammars]
    SPAN_S = 48                                                   # a state cache per item: j0 + rows <= 9 + 17
    states_host = torch.full((ITEMS, SPAN_S), GUARD, dtype=torch.int32)
    for i, s in enumerate(specs):
        if s["g"] is None:
            continue
        lo, hi = max(s["j0"], 0), s["j0"] + s["rows"]
        states_host[i, 8 + lo:8 + hi] = POISON                    # (index j lives at 8 + j: guards on both sides)
        if s["j0"] >= 1:
            states_host[i, 8 + s["j0"] - 1] = s["cached"]
    states = states_host.cuda()
    items = (hip.L.SdGrammarItem * ITEMS)()
    plain = (hip.L.SdLogitEditItem * ITEMS)()
    null_items = [i for i, s in enumerate(specs) if s["g"] is None]
    for i, (it, s) in enumerate(zip(items, specs)):
        row = it.row
        setattr(row, "in", dev_in.data_ptr() + 4 * (i * span + in_off[i]))
        row.out, row.ld_in, row.ld_out, row.rows = out.data_ptr() + 4 * (i * span + out_off[i]), ld, ld, s["rows"]
        row.seq, row.hist0, row.prompt_len, row.pen = seqs[i].data_ptr(), s["hist0"], P_LEN, hip.L.SdPenalty(*s["pen"])
        nb = len(s["bias"])
        row.edit = hip.L.SdLogitEdit(ids[i].data_ptr() if nb else None, vals[i].data_ptr() if nb else None, nb,
                                     masks[i].data_ptr() if masks[i] is not None else None, s["m"])
        row.eos_token_id = s["eos"]
        it.grammar = devg[s["gi"]].pointer() if s["g"] is not None else None
        it.states = states.data_ptr() + 4 * (i * SPAN_S + 8) if s["g"] is not None else None
    for k, i in enumerate(null_items):                            # the same items through sd_edit_rows, into a slab of their own
        C.memmove(C.byref(plain[k]), C.byref(items[i].row), C.sizeof(hip.L.SdLogitEditItem))
        plain[k].out = out_edit.data_ptr() + 4 * (i * span + out_off[i])
    assert {s["gi"] for s in specs} == {None, 0, 1, 2, 3} and min(s["j0"] for s in specs) < 0
    runs = []
    for _ in range(2):
        assert hip.lib.sd_grammar_rows(items, ITEMS, V, m, _st()) == 0, hip.lib.sd_last_error()
        torch.cuda.synchronize()
        runs.append((out.cpu(), states.cpu()))
    assert hip.lib.sd_edit_rows(plain, len(null_items), V, m, _st()) == 0, hip.lib.sd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(dev_in.view(torch.int32), keep.view(torch.int32))
    got_states = runs[0][1]
    edit_rows = out_edit.cpu()
    masked_rows = dead_rows = prompt_rows = 0
    for i, s in enumerate(specs):
        blk = runs[0][0][i * span:(i + 1) * span]
        got = blk[out_off[i]:][:ROWS * ld].view(ROWS, ld)
        assert blk[:out_off[i]].eq(SENTINEL).all() and got[:-1, V:].eq(SENTINEL).all() and got[s["rows"]:, :V].eq(SENTINEL).all(), i
        g = s["g"]
        if g is None:
            assert torch.equal(blk, edit_rows[i * span:(i + 1) * span]), i      # sd_edit_rows' bytes, sentinels included
            assert got_states[i].eq(GUARD).all()
        else:
            want_states = states_host[i].clone()
            for j, v in s["states"].items():
                if j >= 0:
                    want_states[8 + j] = v
            assert torch.equal(got_states[i], want_states), (i, got_states[i].tolist(), want_states.tolist())
        for r in range(s["rows"]):
            row = _as_read(x[i * ROWS + r], m)
            j = s["j0"] + r
            y = apply_penalties(row, s["seq"][:s["hist0"] + r], P_LEN, *s["pen"])
            y = apply_logit_edits(y, j, s["eos"], s["bias"], s["mask"], s["m"])
            if g is not None and j >= 0:
                before = y
                y = apply_grammar(y, g, s["states"][j])
                live = s["states"][j] >= 0
                masked_rows += live
                dead_rows += not live
                assert live or _same_bits(y.float(), before.float())
            elif g is not None:
                prompt_rows += 1
            assert _same_bits(got[r, :V].view(torch.float32), y.float()), (mode, V, "item", i, "row", r, "state", s["states"].get(j))
    assert masked_rows > 100 and dead_rows >= 17 + 3 + 2 and prompt_rows == 3 + 5 + 2


def test_k2_overlapping_launches_equal_one_launch(hip):
    """Rows j0 .. j0 + 4 and then rows j0 + 2 .. j0 + 6 - the second launch reads the states[j0 + 1] the first wrote, as a
    draft step reads its predecessor's state and the verify rewrites them all - give the rows and states of ONE launch over
    rows j0 .. j0 + 6."""
    V, ld, P, j0 = 8229, 8232, 10, 2
    rng = np.random.default_rng(9)
    g = _random_grammar(V, 5, False, rng)
    outs = _walk(g, g.start, j0 + 7, rng, V)
    seq = torch.tensor(rng.integers(0, V, size=P).tolist() + outs, dtype=torch.int32, device="cuda")
    x = torch.from_numpy(rng.standard_normal((7, ld)).astype(np.float32)).cuda()
    dg = g.to_device("cuda")
    mask = torch.from_numpy(allowed_mask_words(V, None, [5, 4096]).view(np.int32)).cuda()

    def launch(out, states, r0, rows):
        it = (hip.L.SdGrammarItem * 1)()
        setattr(it[0].row, "in", x[r0].data_ptr())
        it[0].row.out, it[0].row.ld_in, it[0].row.ld_out, it[0].row.rows = out[r0].data_ptr(), ld, ld, rows
        it[0].row.seq, it[0].row.hist0, it[0].row.prompt_len = seq.data_ptr(), P + j0 + r0, P
        it[0].row.pen, it[0].row.eos_token_id = hip.L.SdPenalty(1.2, 0.0, 0.5), -1
        it[0].row.edit = hip.L.SdLogitEdit(None, None, 0, mask.data_ptr(), 0)
        it[0].grammar, it[0].states = dg.pointer(), states.data_ptr()
        assert hip.lib.sd_grammar_rows(it, 1, V, 0, _st()) == 0, hip.lib.sd_last_error()

    def fresh():
        st = torch.full((16,), POISON, dtype=torch.int32, device="cuda")
        st[j0 - 1] = g.state_after(outs[:j0 - 1])
        return torch.full((7, ld), SENTINEL, dtype=torch.int32, device="cuda"), st
    one, st_one = fresh()
    launch(one, st_one, 0, 7)
    two, st_two = fresh()
    launch(two, st_two, 0, 5)
    launch(two, st_two, 2, 5)
    torch.cuda.synchronize()
    assert torch.equal(one, two) and torch.equal(st_one, st_two)
    assert st_one[j0:j0 + 7].tolist() == [g.state_after(outs[:j]) for j in range(j0, j0 + 7)] and min(st_one[j0:j0 + 7].tolist()) >= 0
    assert st_one[j0 + 7:].eq(POISON).all() and st_one[:j0 - 1].eq(POISON).all()


# ----------------------------------------------------------------------------- R: the refusals that read a session
P_ = 0x1000                                                       # a placeholder pointer: every refusal comes before any use


def test_r1_refusals_that_read_a_session(hip):
    """Every loop call here has T == len: even if a refusal were missing, the loop would find nothing to do and launch nothing
    on its placeholder buffers."""
    L_, lib = hip.L, hip.lib
    dm, tm = _models("corr")[4:]
    V = tm.cfg.vocab_size
    ds, ts = dm.new_session(64), tm.new_session(64)
    said = lambda: lib.sd_last_error().decode()
    g = grammar_a(V, 2).to_device("cuda")
    states = torch.zeros(4, dtype=torch.int32, device="cuda")
    ident = L_.SdGrammar(P_, P_, None, 5, V - 1, 0)
    assert lib.sd_session_set_grammar(ts.handle, C.pointer(ident), P_, 8) == L_.SD_ERR_INVALID
    assert said() == f"sd_session_set_grammar: grammar: no cls table and n_classes {V - 1} differs from the vocabulary {V}"
    assert lib.sd_session_set_grammar(ts.handle, g.pointer(), states.data_ptr(), 4) == 0, said()
    host = np.zeros(64, dtype=np.int32)
    sampling = L_.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=V, ld=V, eos_token_id=2)
    head = L_.SdHeadScratch(logits=P_, ld_logits=V, norm_mode=0)
    scratch = L_.SdSpecScratch(draft=head, target=head, norm_workspace=None, max_rows_per_forward=64)
    edits = (L_.SdLogitEdit * 2)()
    eb = L_.SdLogitEditBlock(P_, V, 64, edits)
    with_slab, no_slab = L_.SdLoopOpts(edits=C.pointer(eb)), L_.SdLoopOpts(logprobs=None)
    NO_SLAB = "has a grammar but opts->edits is NULL: the masked rows need the edit block's slab (a block of neutral records is enough)"
    CAP = "states_cap 4 is smaller than the 6 output positions the call can reach (T - P + gamma + 2)"

    def single(opts):
        dev = L_.SdSpecStream(ds.handle, ts.handle, P_, P_, P_, P_, P_, P_)
        st = L_.SdSeqState(host_seq=host.ctypes.data, len=5, T=5, max_iters=4, n_iters=-7, err=-7)
        rc = lib.sd_spec_generate(dev, 4, sampling, scratch, st, 0, None, None, opts)
        assert rc == 0 or (st.n_iters, st.err) == (-7, -7)         # refused: nothing was written
        return rc

    def batch(opts):
        arr = (L_.SdBatchStream * 1)()
        for f in ("seq", "q_hist", "p_hist", "err_words", "res_dev", "res_host", "host_seq"):
            setattr(arr[0], f, P_)
        arr[0].draft, arr[0].target, arr[0].len, arr[0].T, arr[0].draft_len, arr[0].target_len = ds.handle, ts.handle, 5, 5, 4, 4
        log = L_.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7)
        rc = lib.sd_spec_batch_generate(arr, 1, 4, sampling, 0, None, scratch, log, None, opts)
        assert rc == 0 or (log.n_iters, log.err) == (-7, -7)
        return rc

    def queue(opts):
        arr, prompts = (L_.SdBatchStream * 1)(), (L_.SdQueuePrompt * 2)()
        for f in ("seq", "q_hist", "p_hist", "err_words", "res_dev", "res_host"):
            setattr(arr[0], f, P_)
        arr[0].draft, arr[0].target = ds.handle, ts.handle
        for p, (L, T) in zip(prompts, ((5, 5), (3, 3))):
            p.tokens, p.host_seq, p.L, p.T = P_, P_, L, T
        log = L_.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7)
        rc = lib.sd_spec_queue_generate(arr, 1, 32, prompts, 2, 0, 4, sampling, 0, None, scratch, log, None, None, None, None, 0, opts)
        assert rc == 0 or (log.n_iters, log.err) == (-7, -7)
        return rc

    def ar(opts):
        arr = (L_.SdArStream * 1)()
        for f in ("seq", "probs", "err_words", "host_seq"):
            setattr(arr[0], f, P_)
        arr[0].session, arr[0].len, arr[0].T, arr[0].cache_len = ts.handle, 5, 5, 4
        log = L_.SdArLog(None, None, 0, -7, -7)
        rc = lib.sd_ar_batch_generate(arr, 1, sampling, head, None, P_, P_, log, None, opts)
        assert rc == 0 or (log.n_steps, log.err) == (-7, -7)
        return rc
    try:
        for name, call, what in (("sd_spec_generate", single, "stream"), ("sd_spec_batch_generate", batch, "stream"),
                                 ("sd_spec_queue_generate", queue, "slot"), ("sd_ar_batch_generate", ar, "stream")):
            for opts in (None, no_slab):
                assert call(opts) == L_.SD_ERR_INVALID, name
                assert said() == f"{name}: grammar: the target session of stream 0 {NO_SLAB}", said()
            if name == "sd_ar_batch_generate":                    # no gamma there: T - P + 2 = 2 fits a cache of 4
                assert call(with_slab) == 0, said()
                continue
            assert call(with_slab) == L_.SD_ERR_INVALID, name
            # (the queue: the largest T and the smallest L, 5 - 3 + 4 + 2)
            cap = CAP.replace("the 6 output", "the 8 output") if name == "sd_spec_queue_generate" else CAP
            assert said() == f"{name}: grammar: {what} 0: {cap}", said()
        assert lib.sd_session_set_grammar(ts.handle, g.pointer(), states.data_ptr(), 1) == 0
        assert ar(with_slab) == L_.SD_ERR_INVALID
        assert said() == "sd_ar_batch_generate: grammar: stream 0: " + CAP.replace("states_cap 4", "states_cap 1").replace("the 6 output", "the 2 output")
        # a stream that arrives with its last prompt row already cached has no row to start the automaton at
        big = torch.zeros(64, dtype=torch.int32, device="cuda")
        assert lib.sd_session_set_grammar(ts.handle, g.pointer(), big.data_ptr(), 64) == 0
        dev = L_.SdSpecStream(ds.handle, ts.handle, P_, P_, P_, P_, P_, P_)
        st = L_.SdSeqState(host_seq=host.ctypes.data, len=5, T=5, target_len=5, max_iters=4, n_iters=-7, err=-7)
        assert lib.sd_spec_generate(dev, 4, sampling, scratch, st, 0, None, None, with_slab) == L_.SD_ERR_INVALID
        assert "grammar: target_len 5 of 5 tokens" in said()
        # the loops without an options block have no edit pass
        look = L_.SdSpecStream(None, ts.handle, P_, P_, P_, P_, P_, P_)
        st = L_.SdSeqState(host_seq=host.ctypes.data, len=5, T=5, max_iters=4, n_iters=-7, err=-7)
        assert lib.sd_lookup_generate(look, 4, 3, 1, sampling, scratch, st, None, None) == L_.SD_ERR_INVALID
        assert said().startswith("sd_lookup_generate: the target session carries a grammar: this loop has no edit pass")
        arr = (L_.SdBatchStream * 1)()
        for f in ("seq", "q_hist", "p_hist", "err_words", "res_dev", "res_host", "host_seq"):
            setattr(arr[0], f, P_)
        arr[0].target, arr[0].len, arr[0].T, arr[0].target_len = ts.handle, 5, 5, 4
        log = L_.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7)
        assert lib.sd_lookup_batch_generate(arr, 1, 4, 3, 1, sampling, scratch, log, None, None) == L_.SD_ERR_INVALID
        assert said().startswith("sd_lookup_batch_generate: stream 0: the target session carries a grammar")
        reps = (L_.SdMultiReplica * 1)(L_.SdMultiReplica(ds.handle, ts.handle, P_, P_, P_))
        st = L_.SdSeqState(host_seq=host.ctypes.data, len=5, T=5, max_iters=4, n_iters=-7, err=-7)
        assert lib.sd_spec_multi_generate(reps, 1, 4, 64, sampling, 0, None, scratch, P_, P_, st, None) == L_.SD_ERR_INVALID
        assert said().startswith("sd_spec_multi_generate: replica 0: the target session carries a grammar")
        # detached, the same calls pass the grammar checks (and, with T == len, find nothing to do)
        assert lib.sd_session_set_grammar(ts.handle, None, None, 0) == 0
        assert single(None) == 0 and ar(None) == 0, said()
    finally:
        lib.sd_session_set_grammar(ts.handle, None, None, 0)


# ----------------------------------------------------------------------------- L: the loops
EOS, GAMMA, MAX_LEN = 2, 4, 24
CHOICES = [[7, 300, 41], [7, 300], [7, 8, 8, 9]]                  # three choices of 2 - 4 tokens that share their first


@functools.lru_cache(maxsize=None)
def _grammars():
    V = _models("corr")[0].vocab_size
    return grammar_a(V, EOS), TokenGrammar.from_choices(CHOICES, V, EOS)


# prompt i's request: grammar A with a penalty triple, a bias list and min_tokens; B; A alone; B; A with a penalty
REQS = [dict(g=0, pen=(1.8, 0.0, 0.5), bias={EOS: 4.0, 17: -2.0, 300: 1.5}, m=5), dict(g=1), dict(g=0), dict(g=1), dict(g=0, pen=(1.0, 1.5, 0.5))]


def _req(i, g=None):
    r = REQS[i]
    gi = r["g"] if g is None else g
    return dict(grammar=None if gi < 0 else _grammars()[gi], pen=r.get("pen", NEUTRAL_PEN), bias=r.get("bias"), m=r.get("m", 0))


def _kw(r):
    return dict(repetition_penalty=r["pen"][0], frequency_penalty=r["pen"][1], presence_penalty=r["pen"][2], logit_bias=r["bias"],
                min_tokens=r["m"], grammar=r["grammar"])


def _cols(reqs, grammar=True):
    kw = dict(repetition_penalty=[r["pen"][0] for r in reqs], frequency_penalty=[r["pen"][1] for r in reqs],
              presence_penalty=[r["pen"][2] for r in reqs], logit_bias=[r["bias"] for r in reqs], min_tokens=[r["m"] for r in reqs])
    if grammar:
        kw["grammar"] = [r["grammar"] for r in reqs]
    return kw


def _wrap(om, L, r):
    return GrammarModel(om, L, EOS, r["grammar"], r["pen"], r["bias"], None, (), r["m"])


def _lib():
    from llmspeculativesampling_amd import _lib
    return _lib


def _spec_oracle(i, g):
    """Prompt i's oracle run on the wrapped fp32 pair under its own Philox variates and (T, k, p), its request's edits and
    grammar g (0 = A, 1 = B, -1 = none; None = its request's own).  Computed once per (i, g) and shared by the tests."""
    return _spec_oracle_run(i, REQS[i]["g"] if g is None else g)


@functools.lru_cache(maxsize=None)
def _spec_oracle_run(i, g):
    od, ot = _corr_oracles()
    pf, (T, k, p), r = _loop_prompts()[i], PARAMS[i], _req(i, g)
    L = pf.shape[1]
    return oracle.speculative_sampling(pf, _wrap(od, L, r), _wrap(ot, L, r), EOS, None, MAX_LEN, details=True, gamma=GAMMA, temperature=T,
                                       top_k=k, top_p=p, noise=PhiloxOracleNoise(_lib().lib, SEEDS[i], GAMMA, _st))


def _assert_run(want, got, gd, what):
    (w, wd) = want
    np.testing.assert_array_equal(got.cpu().numpy(), w.cpu().numpy(), err_msg=what)
    assert gd["acc_len"] == wd["acc_len"], what
    assert gd["target_call_times"] == wd["target_call_times"] and gd["approx_call_times"] == wd["approx_call_times"], what


def _is_choice(new):
    return new in [c + [EOS] for c in CHOICES]


def test_l1a_single_stream_equals_the_oracle_token_for_token(hip):
    """speculative_sampling, every prompt with its own request (grammar A with or without edits, grammar B), against the oracle
    on GrammarModel-wrapped models: tokens, accepted lengths and call counts.  Every grammar-B output is one of the choices
    followed by EOS; the grammar-A iterations include ones with no, some and all drafts accepted, so every hand-over of the
    state cache is exercised."""
    dm, tm = _models("corr")[4:]
    A, B = _grammars()
    prompts = [p.cuda() for p in _loop_prompts()]
    n = len(prompts)
    # on the CPU: the grammars bite, and the cases the hand-over has
    plain = _spec_oracle(0, -1)
    assert not A.accepts_prefix(plain[0][0, LENS[0]:].tolist())
    acc = [a for i in range(n) for a in _spec_oracle(i, 0)[1]["acc_len"]]
    assert 0 in acc and GAMMA in acc and any(0 < a < GAMMA for a in acc), acc
    for i in range(n):
        new = _spec_oracle(i, None)[0][0, LENS[i]:].tolist()
        assert _is_choice(new) if REQS[i]["g"] == 1 else A.accepts_prefix(new), (i, new)
    assert EOS not in _spec_oracle(0, None)[0][0, LENS[0]:LENS[0] + 5].tolist()
    # single stream
    for i, pf in enumerate(prompts):
        T, k, p = PARAMS[i]
        out, det = hip.S.speculative_sampling(pf, dm, tm, EOS, None, MAX_LEN, gamma=GAMMA, details=True, temperature=T, top_k=k, top_p=p,
                                              rng=hip.noise.DeviceNoise(SEEDS[i]), **_kw(_req(i)))
        _assert_run(_spec_oracle(i, None), out, det, f"single stream, prompt {i}")


def test_l1b_batch_of_two_grammars_and_none_equals_the_oracle(hip):
    """speculative_sampling_batch, three streams: A with edits, B, none."""
    dm, tm = _models("corr")[4:]
    A, B = _grammars()
    prompts = [p.cuda() for p in _loop_prompts()]
    reqs = [_req(0), _req(1), _req(2, -1)]
    t = {}
    outs, ds = hip.S.speculative_sampling_batch(prompts[:3], dm, tm, EOS, None, MAX_LEN, gamma=GAMMA, details=True, seeds=SEEDS[:3],
                                                temperature=[q[0] for q in PARAMS[:3]], top_k=[q[1] for q in PARAMS[:3]],
                                                top_p=[q[2] for q in PARAMS[:3]], _timing=t, **_cols(reqs))
    for i, want in enumerate((_spec_oracle(0, None), _spec_oracle(1, None), _spec_oracle(2, -1))):
        _assert_run(want, outs[i], ds[i], f"batch, stream {i}")
    assert t["grammar_states"][2] is None and _is_choice(outs[1][0, LENS[1]:].tolist())
    for i, g in ((0, A), (1, B)):                                 # the state cache: states[j] = the state output token j was drawn in
        new = outs[i][0, LENS[i]:].tolist()
        assert t["grammar_states"][i][:len(new)].tolist() == [g.state_after(new[:j]) for j in range(len(new))], i


def test_l1c_queue_equals_the_oracle_where_a_slot_changes_hands(hip):
    """speculative_sampling_queue_grammar: five prompts through two slots under ONE grammar, each with its own edits, so a
    slot changes hands and its states restart - under A against the oracle, then under B, where every prompt ends on a choice
    and EOS."""
    dm, tm = _models("corr")[4:]
    A, B = _grammars()
    prompts = [p.cuda() for p in _loop_prompts()]
    n = len(prompts)
    reqs = [_req(i, 0) for i in range(n)]
    t = {}
    outs, ds = hip.S.speculative_sampling_queue_grammar(prompts, dm, tm, EOS, None, MAX_LEN, gamma=GAMMA, details=True, seeds=SEEDS, slots=2,
                                                        prefill_chunk=8, temperature=[q[0] for q in PARAMS], top_k=[q[1] for q in PARAMS],
                                                        top_p=[q[2] for q in PARAMS], _timing=t, grammar=A, **_cols(reqs, grammar=False))
    assert any(a > 0 for a in t["admit_iter"]) and len(t["grammar_states"]) == 2
    for i in range(n):
        _assert_run(_spec_oracle(i, 0), outs[i], ds[i], f"queue, prompt {i}")
        assert A.accepts_prefix(outs[i][0, LENS[i]:].tolist())
    # ... and grammar B through the queue: every prompt ends on a choice and EOS
    outs, ds = hip.S.speculative_sampling_queue_grammar(prompts, dm, tm, EOS, None, MAX_LEN, gamma=GAMMA, details=True, seeds=SEEDS, slots=2,
                                                        temperature=[q[0] for q in PARAMS], top_k=[q[1] for q in PARAMS],
                                                        top_p=[q[2] for q in PARAMS], grammar=B)
    for i in range(n):
        assert _is_choice(outs[i][0, LENS[i]:].tolist()), (i, outs[i][0, LENS[i]:].tolist())
        if REQS[i]["g"] == 1:                                     # (prompts 1 and 3 run B without edits in their own request too)
            _assert_run(_spec_oracle(i, None), outs[i], ds[i], f"queue under B, prompt {i}")


def test_l1_autoregressive_entries_equal_the_oracle_token_for_token(hip):
    tm = _models("corr")[5]
    ot = _corr_oracles()[1]
    A, B = _grammars()
    prompts = _loop_prompts()[:3]
    reqs = [_req(0), _req(1), _req(2, -1)]
    wants = [oracle.autoregressive_sampling(pf, _wrap(ot, pf.shape[1], r), MAX_LEN, EOS, 1.0, 20, 0.9,
                                            noise=PhiloxOracleNoise(hip.lib, s, 1, _st)) for pf, s, r in zip(prompts, SEEDS, reqs)]
    assert A.accepts_prefix(wants[0][0, LENS[0]:].tolist()) and _is_choice(wants[1][0, LENS[1]:].tolist())
    assert not A.accepts_prefix(wants[2][0, LENS[2]:].tolist())
    t = {}
    outs = hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts], tm, MAX_LEN, EOS, top_k=20, top_p=0.9, seeds=SEEDS[:3], _timing=t,
                                               **_cols(reqs))
    for i, (o, w) in enumerate(zip(outs, wants)):
        np.testing.assert_array_equal(o.cpu().numpy(), w.numpy(), err_msg=f"stream {i}")
    new = outs[0][0, LENS[0]:].tolist()
    assert t["grammar_states"][0][:len(new)].tolist() == [A.state_after(new[:j]) for j in range(len(new))] and t["grammar_states"][2] is None
    for i, (pf, s, r) in enumerate(zip(prompts, SEEDS, reqs)):
        o = hip.S.autoregressive_sampling(pf.cuda(), tm, MAX_LEN, EOS, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(s), **_kw(r))
        np.testing.assert_array_equal(o.cpu().numpy(), wants[i].numpy(), err_msg=f"single stream {i}")


def test_l2_bf16_pair_follows_the_grammar_and_leaves_the_states_of_its_output(hip):
    """The bf16 pair (V = 8192: two windows, the draft head would leave tile maxima), four streams under grammar A and one
    without: every emitted token is accepted, and the device state cache after the call equals state_after of every prefix of
    the output."""
    cfg, dm, tm, _ = _bf16_pair()
    lens = [12, 5, 20, 9]
    prompts = [p.cuda() for p in _prompts(cfg.vocab_size, lens, 1500)]
    A = grammar_a(cfg.vocab_size, None)
    kw = dict(gamma=GAMMA, top_k=20, top_p=0.9, seeds=[61, 62, 63, 64])
    plain = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 16, **kw)
    t = {}
    outs, ds = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 16, details=True, _timing=t, grammar=[A, A, None, A], **kw)
    assert torch.equal(outs[2], plain[2])                         # the neighbour without a grammar is left alone
    for i in (0, 1, 3):
        new = outs[i][0, lens[i]:].tolist()
        assert len(new) >= 16 and A.accepts_prefix(new), (i, new)     # (an iteration may carry a stream past its length)
        assert not A.accepts_prefix(plain[i][0, lens[i]:].tolist())
        assert t["grammar_states"][i][:len(new)].tolist() == [A.state_after(new[:j]) for j in range(len(new))], i
    assert any(0 < a < GAMMA for d in ds for a in d["acc_len"])
    o = hip.S.speculative_sampling(prompts[0], dm, tm, -1, None, 16, gamma=GAMMA, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(61), grammar=A)
    assert o.shape[1] >= lens[0] + 16 and A.accepts_prefix(o[0, lens[0]:].tolist())     # (the single-stream loop's passes round otherwise)


def test_l3_a_grammar_that_allows_everything_changes_nothing(hip):
    """One state, every id allowed: tokens, acc_len and log-probs are those of the call without a grammar - the plain call (a
    neutral edit block is the call without one) and, in the queue, the call whose edited passes a banned id forces on - in
    all five entries."""
    dm, tm = _models("corr")[4:]
    V = tm.cfg.vocab_size
    free = TokenGrammar(np.zeros((1, 1), dtype=np.int64), 0, EOS, V, classes=np.zeros(V, dtype=np.int64))
    prompts = [p.cuda() for p in _loop_prompts()]
    on = dict(banned_token_ids=[V - 1])                           # an edited pass in the call without a grammar too
    kw = dict(gamma=GAMMA, top_k=20, top_p=0.9)
    a = hip.S.speculative_sampling_queue_grammar(prompts, dm, tm, EOS, None, BUDGETS, details=True, seeds=SEEDS, slots=2, logprobs=True, **kw, **on)
    b = hip.S.speculative_sampling_queue_grammar(prompts, dm, tm, EOS, None, BUDGETS, details=True, seeds=SEEDS, slots=2, logprobs=True,
                                                 grammar=free, **kw, **on)
    c = hip.S.speculative_sampling_queue_grammar(prompts, dm, tm, EOS, None, BUDGETS, details=True, seeds=SEEDS, slots=2, logprobs=True,
                                                 grammar=free, **kw)
    plain = hip.S.speculative_sampling_queue_logprobs(prompts, dm, tm, EOS, None, BUDGETS, details=True, seeds=SEEDS, slots=2, **kw)
    for x, y in ((a, b), (plain, c)):
        for (oa, ob), (da, db), (la, lb) in zip(zip(x[0], y[0]), zip(x[1], y[1]), zip(x[2], y[2])):
            assert torch.equal(oa, ob) and da["acc_len"] == db["acc_len"] and torch.equal(la, lb)
    a = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, EOS, None, 12, seeds=SEEDS[:4], details=True, logprobs=True, **kw)
    b = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, EOS, None, 12, seeds=SEEDS[:4], details=True, logprobs=True, grammar=free, **kw)
    for oa, ob, da, db, la, lb in zip(a[0], b[0], a[1], b[1], a[2], b[2]):
        assert torch.equal(oa, ob) and da["acc_len"] == db["acc_len"] and torch.equal(la, lb)
    na, nb = hip.noise.DeviceNoise(9), hip.noise.DeviceNoise(9)
    a = hip.S.speculative_sampling(prompts[2], dm, tm, EOS, None, 12, rng=na, logprobs=True, **kw)
    b = hip.S.speculative_sampling(prompts[2], dm, tm, EOS, None, 12, rng=nb, logprobs=True, grammar=free, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (na.seed, na.draw) == (nb.seed, nb.draw)
    a = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 10, EOS, top_k=20, top_p=0.9, seeds=SEEDS[:3], logprobs=True)
    b = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 10, EOS, top_k=20, top_p=0.9, seeds=SEEDS[:3], logprobs=True, grammar=[free, None, free])
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    a = hip.S.autoregressive_sampling(prompts[1], tm, 10, EOS, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(4))
    b = hip.S.autoregressive_sampling(prompts[1], tm, 10, EOS, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(4), grammar=free)
    assert torch.equal(a, b)
