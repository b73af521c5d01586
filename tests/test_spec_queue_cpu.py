"""Host-side checks of the prompt queue of the lock-step speculative loop (speculative_sampling_queue,
sd_spec_queue_generate, sd_spec_queue_plan): argument refusal before a model is built, the ABI of the new symbols and
structs, and the invariants of the pass plan - the function the native loop itself calls.  No GPU needed."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

NEW = ["sd_spec_queue_generate", "sd_spec_queue_plan"]
MIXED = 64                                                        # logit rows of a pass once not every row is one


# ----------------------------------------------------------------------------- the Python entry point
def test_queue_is_exported_with_the_issue_signature():
    import llmspeculativesampling_amd.sampling as S
    assert callable(S.speculative_sampling_queue) and "speculative_sampling_queue" in S.__all__
    sig = inspect.signature(S.speculative_sampling_queue)
    assert list(sig.parameters) == ["prefixes", "approx_model", "target_model", "eos_token_id", "pad_token_id", "max_len", "gamma",
                                    "temperature", "top_k", "top_p", "random_seed", "details", "seeds", "slots", "prefill_chunk",
                                    "_timing"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(gamma=4, temperature=1, top_k=0, top_p=0, random_seed=None, details=False, seeds=None, slots=8,
                     prefill_chunk=0, _timing=None)


def test_bad_arguments_raise_before_a_model_is_built():
    """The models are None: anything that reached as_specdec_model would raise TypeError, not ValueError."""
    import llmspeculativesampling_amd.sampling as S
    p = [torch.ones((1, 3), dtype=torch.int64), torch.ones((1, 1), dtype=torch.int64)]
    q = lambda prefixes, max_len=4, **kw: S.speculative_sampling_queue(prefixes, None, None, 2, None, max_len, **kw)   # noqa: E731
    for slots in (0, 17, -1, 2.0, None):
        with pytest.raises(ValueError, match="slots"):
            q(p, slots=slots)
    with pytest.raises(ValueError, match="prefixes"):
        q([])
    with pytest.raises(ValueError, match="seeds"):
        q(p, seeds=[1])
    with pytest.raises(ValueError, match="seeds"):
        q(p, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="max_len"):
        q(p, max_len=[4])
    with pytest.raises(ValueError, match="max_len"):
        q(p, max_len=[4, 4, 4])
    for bad in (torch.ones((2, 3), dtype=torch.int64), torch.ones((1, 0), dtype=torch.int64), torch.ones(3, dtype=torch.int64),
                torch.ones((1, 1, 3), dtype=torch.int64), [1, 2, 3]):
        with pytest.raises(ValueError, match=r"prefixes\[1\]"):
            q([p[0], bad])
    with pytest.raises(ValueError, match="prefill_chunk"):
        q(p, prefill_chunk=-1)
    with pytest.raises(TypeError):                                # well-formed arguments do reach the models
        q(p, max_len=[4, 2], seeds=[1, 2], slots=16)


def test_existing_batch_function_still_refuses_a_17th_stream():
    import llmspeculativesampling_amd.sampling as S
    src = inspect.getsource(S.speculative_sampling_batch)
    assert "1 <= B <= 16" in src
    assert "slots" not in inspect.signature(S.speculative_sampling_batch).parameters


# ----------------------------------------------------------------------------- ABI
def test_queue_symbols_are_exported_and_declared():
    """(Argument counts and classes of every symbol against the header: test_abi_cpu.py.)"""
    from llmspeculativesampling_amd import _lib
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and bound[name][0] is C.c_int, name
    # the batch loop's arguments - the same three blocks among them - plus slot_cap, prompts, n_prompts, prefill_chunk, passes_out
    # and, behind the stream, the two donors and their row count; both end in the sd_loop_opts
    streams, n, *rest, stream, opts = bound["sd_spec_batch_generate"][1]
    blocks = [C.POINTER(_lib.SdSampling), C.POINTER(_lib.SdSpecScratch), C.POINTER(_lib.SdLockstepLog)]
    assert [a for a in rest if a in blocks] == blocks and opts == C.POINTER(_lib.SdLoopOpts)
    assert list(bound["sd_spec_queue_generate"][1]) == [streams, n, C.c_int, C.POINTER(_lib.SdQueuePrompt), C.c_int, C.c_int, *rest,
                                                        C.c_void_p, stream, C.c_void_p, C.c_void_p, C.c_int, opts]


@pytest.mark.parametrize("cname,pyname,size", [("sd_queue_prompt", "SdQueuePrompt", 80), ("sd_queue_pass", "SdQueuePass", 16),
                                               ("sd_queue_chunk", "SdQueueChunk", 12)])
def test_queue_struct_layouts_match_the_header(cname, pyname, size):
    from llmspeculativesampling_amd import _lib
    assert _lib.C_STRUCTS[cname] is getattr(_lib, pyname) and C.sizeof(getattr(_lib, pyname)) == size


def queue_blocks(p):
    """The three argument blocks of a queue call on the placeholder buffer ``p``; the log's outputs are preset to -7."""
    from llmspeculativesampling_amd import _lib
    head = _lib.SdHeadScratch(logits=p, ld_logits=128, norm_mode=0)
    return (_lib.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=128, ld=128, eos_token_id=2),
            _lib.SdSpecScratch(draft=head, target=head, norm_workspace=None, max_rows_per_forward=64),
            _lib.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7))


def test_queue_generate_refuses_bad_arguments_before_any_launch():
    from llmspeculativesampling_amd import _lib
    lib = _lib.lib
    buf = (C.c_char * 256)()
    sampling, scratch, log = queue_blocks(C.addressof(buf))
    slots = (_lib.SdBatchStream * 16)()
    prompts = (_lib.SdQueuePrompt * 2)()

    def call(n_slots=2, slot_cap=64, n_prompts=2, chunk=0, gamma=4, sl=slots, pr=prompts, sm=sampling, sc=scratch, lg=log):
        return lib.sd_spec_queue_generate(sl, n_slots, slot_cap, pr, n_prompts, chunk, gamma, sm, 0, None, sc, lg, None, None,
                                          None, None, 0, None)

    for n in (0, 17, -1):
        assert call(n_slots=n) == _lib.SD_ERR_INVALID and re.search(r"n_slots -?\d+ outside 1\.\.16", lib.sd_last_error().decode())
    for g in (0, 17):
        assert call(gamma=g) == _lib.SD_ERR_INVALID and b"gamma" in lib.sd_last_error()
    assert call(n_prompts=0) == _lib.SD_ERR_INVALID and b"n_prompts 0" in lib.sd_last_error()
    assert call(chunk=-1) == _lib.SD_ERR_INVALID and b"prefill_chunk -1" in lib.sd_last_error()
    assert call(sl=None) == _lib.SD_ERR_INVALID and b"null argument" in lib.sd_last_error()
    assert call(pr=None) == _lib.SD_ERR_INVALID and b"null argument" in lib.sd_last_error()
    for block in ("sm", "sc", "lg"):
        assert call(**{block: None}) == _lib.SD_ERR_INVALID and b"sd_spec_queue_generate: null argument" in lib.sd_last_error()
    assert call() == _lib.SD_ERR_INVALID and b"slot 0: null pointer" in lib.sd_last_error()
    assert (log.n_iters, log.err) == (-7, -7)                     # nothing was written, nothing ran
    with pytest.raises(ValueError, match="sd_spec_queue_generate"):
        _lib.check(_lib.SD_ERR_INVALID, "sd_spec_queue_generate")


# ----------------------------------------------------------------------------- the pass plan
def _plan(budget, act, logit_rows, join, chunk=0, force=1, limit=MIXED):
    """-> [(active stream indices, [(joiner, first row, rows)])] per pass"""
    from llmspeculativesampling_amd import _lib
    a = (C.c_int32 * max(1, len(act)))(*act)
    j = (C.c_int32 * max(1, len(join)))(*join)
    passes, chunks = (_lib.SdQueuePass * 17)(), (_lib.SdQueueChunk * 272)()
    n_p, n_c = C.c_int(-1), C.c_int(-1)
    rc = _lib.lib.sd_spec_queue_plan(budget, limit, a, len(act), int(logit_rows), j, len(join), chunk, int(force), passes, 17, chunks,
                                     272, C.byref(n_p), C.byref(n_c))
    assert rc == _lib.SD_OK, _lib.lib.sd_last_error()
    out, seen = [], 0
    for p in passes[:n_p.value]:
        assert p.chunk0 == seen                                   # the chunk lists follow each other
        seen += p.n_chunks
        out.append((list(range(p.act0, p.act0 + p.n_act)), [(c.joiner, c.row0, c.rows) for c in chunks[p.chunk0:p.chunk0 + p.n_chunks]]))
    assert seen == n_c.value
    return out


def _check(budget, act, logit_rows, join, chunk, force=1):
    plan = _plan(budget, act, logit_rows, join, chunk, force)
    # every active stream exactly once, whole, in order
    assert [a for acts, _ in plan for a in acts] == list(range(len(act)))
    nxt = [0] * len(join)
    for acts, chunks in plan:
        rows = sum(act[a] for a in acts)
        jrows = sum(c[2] for c in chunks)
        assert len(acts) + len(chunks) <= 16
        assert rows + jrows <= budget or (len(acts) == 1 and not chunks)       # (one stream too large for any pass is the engine's to refuse)
        if chunks:
            assert (rows if logit_rows else len(acts)) <= MIXED                # a mixed pass
            assert chunk == 0 or jrows <= chunk
        assert len({c[0] for c in chunks}) == len(chunks)                      # one chunk per joiner and pass
        assert [c[0] for c in chunks] == sorted(c[0] for c in chunks)          # queue order
        for jn, row0, n in chunks:
            assert n >= 1 and row0 == nxt[jn]                                  # consecutive, in position order
            nxt[jn] += n
    for jn, left in enumerate(join):
        assert nxt[jn] <= left
        if nxt[jn] and jn:                                        # first come, first served: whoever is ahead got no less
            assert all(nxt[k] == join[k] or nxt[k] >= 1 for k in range(jn))
    waiting = [jn for jn, left in enumerate(join) if left > 0]
    if waiting and force:
        assert nxt[waiting[0]] >= 1                               # the progress guarantee
    assert all(acts for acts, _ in plan[:-1])                     # only the last pass may be joiners alone ...
    if plan and not plan[-1][0]:
        assert force and plan[-1][1] and not any(ch for _, ch in plan[:-1])    # ... and only when no other pass had room
    return plan


def test_plan_invariants_on_random_inputs():
    rng = np.random.default_rng(20261018)
    for _ in range(400):
        budget = int(rng.choice([1, 5, 9, 17, 32, 64, 72, 80]))
        logit_rows = bool(rng.integers(2))
        n_act = int(rng.integers(0, 17))
        gamma1 = int(rng.integers(2, 18))
        act = [gamma1] * n_act if logit_rows else [int(x) for x in rng.integers(1, 3, size=n_act)]
        join = [int(x) for x in rng.choice([0, 1, 2, 7, 8, 39, 300], size=int(rng.integers(0, 17 - max(n_act, 1) + 1)))]
        chunk = int(rng.choice([0, 1, 8, 100]))
        _check(budget, act, logit_rows, join, chunk, force=int(rng.integers(2)))


@pytest.mark.parametrize("gamma", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("pass_rows", [64, 80])
def test_plan_without_joiners_is_the_batch_loops_split(gamma, pass_rows):
    """pass_rows / (gamma + 1) streams per verify pass, all streams in one draft pass."""
    per = max(1, pass_rows // (gamma + 1))
    for n in range(1, 17):
        want = [list(range(a, min(a + per, n))) for a in range(0, n, per)]
        for join in ([], [0], [0, 0]):
            plan = _check(pass_rows, [gamma + 1] * n, True, join, 0)
            assert [acts for acts, _ in plan] == want and not any(ch for _, ch in plan)
        assert [acts for acts, _ in _check(pass_rows, [1 + (i % 2) for i in range(n)], False, [], 0)] == [list(range(n))]


def test_plan_edge_rows():
    # 16 active streams plus a joiner would be 17 items: the joiner's rows get a pass of their own
    plan = _check(80, [1] * 16, False, [9], 0)
    assert plan == [(list(range(16)), []), ([], [(0, 0, 9)])]
    assert _check(80, [1] * 16, False, [9], 0, force=0) == [(list(range(16)), [])]
    # 13 streams x 5 logit rows = 65 > 64: no joiner row in that pass although 15 rows are free
    plan = _check(80, [5] * 13, True, [13], 0)
    assert plan == [(list(range(13)), []), ([], [(0, 0, 13)])]
    assert _check(80, [5] * 12, True, [40], 0) == [(list(range(12)), [(0, 0, 20)])]            # 60 logit rows: 20 rows ride
    assert _check(80, [5] * 13, False, [13], 0)[0][1] == [(0, 0, 13)]                          # (13 logit rows of 65: mixed is fine)
    # room of 0 rows: 80 of 80 rows taken, and a second pass of whole streams that has room
    assert _check(80, [5] * 16, False, [3], 0) == [(list(range(16)), []), ([], [(0, 0, 3)])]
    assert _check(64, [9] * 8, True, [30, 4], 8) == [(list(range(7)), [(0, 0, 1)]), ([7], [(0, 1, 8)])]
    # a joiner with 0 rows left takes no item and does not count as waiting
    assert _check(80, [5] * 3, True, [0, 12], 8) == [([0, 1, 2], [(1, 0, 8)])]
    assert _check(80, [5] * 13, True, [0, 0], 0) == [(list(range(13)), [])]
    assert _check(80, [], True, [0], 0) == []
    # no active stream at all: the joiners alone, in queue order, up to the chunk
    assert _check(80, [], True, [50, 50], 0) == [([], [(0, 0, 50), (1, 0, 30)])]
    assert _check(80, [], True, [5, 50], 8) == [([], [(0, 0, 5), (1, 0, 3)])]


def test_plan_refuses_bad_arguments():
    from llmspeculativesampling_amd import _lib
    passes, chunks = (_lib.SdQueuePass * 17)(), (_lib.SdQueueChunk * 272)()
    n = C.c_int(-7)
    one = (C.c_int32 * 17)(*([1] * 17))
    f = _lib.lib.sd_spec_queue_plan
    assert f(0, 64, one, 1, 1, one, 1, 0, 1, passes, 17, chunks, 272, C.byref(n), C.byref(n)) == _lib.SD_ERR_INVALID
    assert f(80, 64, one, 17, 1, one, 1, 0, 1, passes, 17, chunks, 272, C.byref(n), C.byref(n)) == _lib.SD_ERR_INVALID
    assert f(80, 64, one, 1, 1, one, 1, -1, 1, passes, 17, chunks, 272, C.byref(n), C.byref(n)) == _lib.SD_ERR_INVALID
    assert f(80, 64, one, 1, 1, one, 1, 0, 1, None, 17, chunks, 272, C.byref(n), C.byref(n)) == _lib.SD_ERR_INVALID
    assert f(5, 64, one, 16, 1, one, 0, 0, 1, passes, 2, chunks, 272, C.byref(n), C.byref(n)) == _lib.SD_ERR_CAPACITY
    assert n.value == -7
