"""RequestOptions (sampling/_loop_common.py): the one place the native-loop wrappers parse, check and attach a request's options.
No GPU: the blocks are built on the CPU (``pin_memory`` is a no-op here) and ``grammar.lib`` is a recording stand-in, as
test_logit_edits_cpu.py does for ArRun.  What the leaf parsers accept and refuse is in their own files (test_row_sampling_cpu,
test_penalties_cpu, test_logit_edits_cpu, test_grammar_cpu); here: which members of sd_loop_opts a set of options gives, the one
slab-rows rule, that every bound grammar comes off again, the refusal texts and the order of the stages."""
import importlib
import itertools
import types

import pytest
import torch

from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd import sampling as S
from llmspeculativesampling_amd.sampling import _loop_common as LC
from llmspeculativesampling_amd.sampling import grammar as G

V, EOS, N = 64, 2, 3
GRAMMAR = G.TokenGrammar.from_choices([[3, 4], [5]], V, EOS)
SET = dict(sampling=([1.0, 0.7, 1.0], 20, 0.9), logprobs=True, penalties=(1.0, 0.0, 0.5), edits=({5: 1.0}, None, [7], 0), grammar=GRAMMAR)


class _GrammarLib:
    """Stands in for grammar.lib: writes down (session handle, set or taken off) per sd_session_set_grammar and refuses to set
    one on the session ``fail``."""

    def __init__(self, fail=None):
        self.calls, self.fail = [], fail

    def sd_session_set_grammar(self, handle, grammar, states, cap):
        self.calls.append((handle, grammar is not None))
        return _lib.SD_ERR_INVALID if grammar is not None and handle == self.fail else _lib.SD_OK


@pytest.fixture
def glib(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    lib = _GrammarLib()
    monkeypatch.setattr(G, "lib", lib)
    return lib


def _attach(opts, sessions=N):
    return opts.attach("cpu", V, 5, [12] * opts.n, [types.SimpleNamespace(handle=i + 1) for i in range(sessions)], [8] * sessions)


def _members(opts) -> set:
    return {f for f, _ in _lib.SdLoopOpts._fields_ if opts is not None and getattr(opts, f)}


def test_every_neutral_spelling_gives_the_null_block(glib):
    for kw in (dict(), dict(sampling=None), dict(sampling=(1, 0, 0)), dict(sampling=(0.7, 20, 0.9)), dict(logprobs=False),
               dict(penalties=(1.0, 0.0, 0.0)), dict(penalties=(1, 0, 0)), dict(edits=(None, None, None, 0)), dict(edits=({}, None, [], 0)),
               dict(edits=([None, {}, None], [None] * 3, [[], None, []], [0, 0, 0])), dict(grammar=None), dict(grammar=[None] * 3)):
        opts = LC.RequestOptions.parse(N, "stream", EOS, **kw)
        assert (opts.sampling, opts.penalties, opts.edits, opts.grammar) == (None,) * 4 and not opts.logprobs, kw
        opts.bind(V)
        with _attach(opts) as blocks:
            assert blocks.loop_opts is None and blocks.members == (None,) * 4 and blocks.grammar_states is None, kw
    assert glib.calls == []


@pytest.mark.parametrize("names", [c for r in range(6) for c in itertools.combinations(SET, r)], ids=lambda c: "+".join(c) or "nothing")
def test_the_members_a_set_of_options_gives(glib, names):
    opts = LC.RequestOptions.parse(N, "stream", EOS, **{k: SET[k] for k in names})
    opts.bind(V)
    want = {dict(sampling="row_params", grammar="edits").get(k, k) for k in names}
    with _attach(opts) as blocks:
        assert _members(blocks.loop_opts) == want and (blocks.loop_opts is None) == (not names)
        if "sampling" in names:
            assert [(r.temperature, r.top_k) for r in blocks.loop_opts.row_params[:N]] == [(1.0, 20), (pytest.approx(0.7), 20), (1.0, 20)]
        if "logprobs" in names:
            assert blocks.logprob_tensor(1, 4, "cpu").shape == (1, 4)
        if "penalties" in names and want & {"edits"}:
            assert blocks.eb.block.rows == blocks.pb.rows.data_ptr()          # one slab for both
        if "grammar" in names:
            assert glib.calls == [(1, True), (2, True), (3, True)]
            assert [tuple(s.shape) for s in blocks.grammar_states] == [(8,)] * N and blocks.eb.rows.shape == (5, V)
            if "edits" not in names:                                          # the edit block is there for its slab alone
                assert blocks.eb._ids is None and blocks.eb._vals is None and blocks.eb._masks is None and opts.edits is None
                assert [(p.n_bias, p.allowed, p.min_tokens) for p in blocks.eb._params] == [(0, None, 0)] * N
        else:
            assert blocks.grammar_states is None
    assert glib.calls == ([(h, True) for h in (1, 2, 3)] + [(h, False) for h in (1, 2, 3)] if "grammar" in names else [])


def test_the_queue_binds_its_one_grammar_to_the_slots_sessions(glib):
    opts = LC.RequestOptions.parse(5, "prompt", EOS, grammar=GRAMMAR)          # 5 prompts in 2 slots
    with _attach(opts, sessions=2) as blocks:
        assert len(blocks.grammar_states) == 2 and len(blocks.eb._params) == 5
    assert glib.calls == [(1, True), (2, True), (1, False), (2, False)]


def test_slab_rows_on_a_hand_table():
    # (gamma, streams, rows a pass may carry) -> min(max(per_pass, gamma + 1), streams * (gamma + 1)), worked out by hand
    for (gamma, B, per_pass), want in (((4, 1, 64), 5), ((4, 1, 2), 5), ((1, 1, 0), 2), ((16, 1, 256), 17),      # one stream: gamma + 1
                                       ((4, 4, 3), 5), ((4, 4, 5), 5), ((4, 4, 12), 12), ((4, 4, 20), 20),     # per_pass < gamma + 1 ...
                                       ((4, 2, 64), 10), ((4, 16, 64), 64), ((4, 16, 256), 80),                  # ... > B * (gamma + 1)
                                       ((16, 16, 256), 256), ((16, 16, 300), 272), ((8, 8, 64), 64), ((2, 3, 64), 9)):
        assert LC.slab_rows(gamma, B, per_pass) == want, (gamma, B, per_pass)
    assert [LC.slab_rows(ar_streams=B) for B in (1, 2, 7, 16)] == [1, 2, 7, 16]


def test_every_bound_session_is_detached_exactly_once(glib, monkeypatch):
    opts = LC.RequestOptions.parse(N, "stream", EOS, grammar=[GRAMMAR, None, GRAMMAR])
    both = [(1, True), (3, True), (1, False), (3, False)]
    with _attach(opts) as blocks:
        assert blocks.grammar_states[1] is None
    assert glib.calls == both                                                 # a normal exit
    del glib.calls[:]
    with pytest.raises(KeyError):
        with _attach(opts):
            raise KeyError("the body")
    assert glib.calls == both                                                 # the body raised
    failing = _GrammarLib(fail=3)
    monkeypatch.setattr(G, "lib", failing)
    with pytest.raises(ValueError, match="sd_session_set_grammar"):
        with _attach(opts):
            raise AssertionError("not reached")
    assert failing.calls == [(1, True), (3, True), (1, False)]                # session 3 was never bound


NATIVE = ('grammar needs the native loop: rng="device" (or a device noise object)',
          'logit_bias / allowed_token_ids / banned_token_ids / min_tokens need the native loop: rng="device" (or a device noise object)',
          'repetition / frequency / presence penalties need the native loop: rng="device" (or a device noise object)',
          'logprobs=True needs the native loop: rng="device" (or a device noise object)')
TENSOR_PARALLEL = ("grammar is not available with a tensor-parallel target model",
                   "logit_bias / allowed_token_ids / banned_token_ids / min_tokens are not available with a tensor-parallel target model",
                   "repetition / frequency / presence penalties are not available with a tensor-parallel target model",
                   "logprobs=True is not available with a tensor-parallel target model")
ORDER = ("grammar", "edits", "penalties", "logprobs")


def _said(fn, *args, **kw) -> str:
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    return str(e.value)


def test_require_native_and_require_target_rows_say_what_they_said_in_the_stated_order():
    tp = types.SimpleNamespace(tp_group=object())
    for suffix in (" and verbose=False", ", not _native=False"):
        for i, name in enumerate(ORDER):
            alone = LC.RequestOptions.parse(1, "stream", EOS, **{name: SET[name]})
            assert _said(alone.require_native, False, suffix) == NATIVE[i] + suffix
            assert _said(alone.require_target_rows, tp) == TENSOR_PARALLEL[i]
            rest = LC.RequestOptions.parse(1, "stream", EOS, **{k: SET[k] for k in ORDER[i:]})    # the first of those set speaks
            assert _said(rest.require_native, False, suffix) == NATIVE[i] + suffix
            assert _said(rest.require_target_rows, tp) == TENSOR_PARALLEL[i]
            for opts in (alone, rest):
                opts.require_native(True, suffix)
                opts.require_target_rows(types.SimpleNamespace(tp_group=None))
                opts.require_target_rows(object())
    nothing = LC.RequestOptions.parse(1, "stream", EOS, sampling=([0.7], 20, 0.9))                  # row parameters ask for neither
    nothing.require_native(False, " and verbose=False")
    nothing.require_target_rows(tp)


def _model(tp):
    return types.SimpleNamespace(tp_group=tp, device="cpu", cfg=types.SimpleNamespace(vocab_size=V, is_encoder_decoder=False))


X = torch.tensor([[3, 4, 5]])
ENTRIES = {
    "speculative_sampling": ("speculative_sampling", lambda m, **kw: S.speculative_sampling(X, m, m, EOS, None, 4, **kw)),
    "autoregressive_sampling": ("autoregressive_sampling", lambda m, **kw: S.autoregressive_sampling(X, m, 4, EOS, **kw)),
    "speculative_sampling_batch": ("batch", lambda m, **kw: S.speculative_sampling_batch([X, X], m, m, EOS, None, 4, **kw)),
    "autoregressive_sampling_batch": ("batch", lambda m, **kw: S.autoregressive_sampling_batch([X, X], m, 4, EOS, **kw)),
    "speculative_sampling_queue_edits": ("batch", lambda m, **kw: S.speculative_sampling_queue_edits([X, X], m, m, EOS, None, 4, **kw)),
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_call_wrong_at_every_stage_is_refused_stage_by_stage(monkeypatch, entry):
    """parse -> native loop -> tensor-parallel -> bind: a call that is wrong at all of them is refused for the first, and mended
    stage by stage for the next.  The models are stand-ins (``as_specdec_model`` hands them through): no stage before ``bind``
    reads more of one than ``tp_group``, and ``bind`` reads the vocabulary size."""
    mod, call = ENTRIES[entry]
    m = importlib.import_module("llmspeculativesampling_amd.sampling." + mod)
    monkeypatch.setattr(m, "as_specdec_model", lambda model: model)
    if hasattr(m, "same_device"):
        monkeypatch.setattr(m, "same_device", lambda *models: None)
    single = "batch" not in entry and "queue" not in entry
    kw = dict(repetition_penalty=0.0, banned_token_ids=[V], **(dict(rng="host") if single else {}))
    assert _said(call, _model(object()), **kw).startswith("repetition_penalty: ")
    kw["repetition_penalty"] = 1.5
    if single:
        assert _said(call, _model(object()), **kw).startswith(NATIVE[1])      # (edits come before penalties)
        kw["rng"] = "device"
    assert _said(call, _model(object()), **kw) == TENSOR_PARALLEL[1]
    assert _said(call, _model(None), **kw).startswith(f"banned_token_ids: {'prompt' if 'queue' in entry else 'stream'} 0: token id {V} outside")
