"""Grammar-constrained decoding, what needs no GPU: the ABI of the two new entries, every refusal that is reached without a
session (sd_grammar_rows' on placeholder pointers, sd_session_set_grammar's checks of the grammar itself), the TokenGrammar
builder, the definition (apply_grammar against a plain-Python restatement) and the loop reference: the CPU oracle on
GrammarModel-wrapped models emits only what the grammar accepts.  (A session is created on a device, so the refusals that read
one - a vocabulary mismatch, the loops' - are in test_gpu_grammar.py.)"""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import abi_header
import oracle
from grammar_model import GrammarModel
from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.config import load_config
from llmspeculativesampling_amd.sampling import TokenGrammar
from llmspeculativesampling_amd.sampling import grammar as G
from llmspeculativesampling_amd.sampling.utils import apply_grammar
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict
import llmspeculativesampling_amd.sampling as S

P = 0x1000                                                        # a placeholder pointer: every refusal comes before any use


# ----------------------------------------------------------------------------- ABI
def test_the_new_symbols_and_structs_match_the_header_and_the_abi_stays_7():
    protos, structs = abi_header.parse()
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sd_session_set_grammar", "sd_grammar_rows"):
        assert name in protos and name in bound and hasattr(_lib.lib, name)
        res, args = bound[name]
        assert abi_header.ctypes_class(res) == protos[name][0]
        assert [abi_header.ctypes_class(a) for a in args] == protos[name][1], name
    for name, cls in (("sd_grammar", _lib.SdGrammar), ("sd_grammar_item", _lib.SdGrammarItem)):
        fields, size = structs[name]
        assert _lib.C_STRUCTS[name] is cls and C.sizeof(cls) == size
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == fields
    assert C.sizeof(_lib.SdGrammar) == 40 and C.sizeof(_lib.SdGrammarItem) == 136
    assert protos["sd_grammar_rows"][2][0] == "sd_grammar_item" and protos["sd_session_set_grammar"][2][:2] == ["sd_session", "sd_grammar"]
    # additive: the ABI, the options block and the edit structs are what they were
    assert _lib.lib.sd_version() == 7 and C.sizeof(_lib.SdLoopOpts) == 32
    assert (C.sizeof(_lib.SdLogitEdit), C.sizeof(_lib.SdLogitEditItem), C.sizeof(_lib.SdLogitEditBlock)) == (40, 120, 32)


def test_the_keyword_is_last_and_keyword_only_and_the_queue_has_a_sibling():
    for name in ("speculative_sampling", "speculative_sampling_batch", "autoregressive_sampling", "autoregressive_sampling_batch",
                 "speculative_sampling_queue_grammar"):
        params = inspect.signature(getattr(S, name)).parameters
        assert list(params)[-1] == "grammar" and params["grammar"].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params["grammar"].default is None
    a = inspect.signature(S.speculative_sampling_queue_edits).parameters
    b = inspect.signature(S.speculative_sampling_queue_grammar).parameters
    assert list(b) == list(a) + ["grammar"] and all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    for f in (S.speculative_sampling_queue, S.speculative_sampling_queue_shared, S.speculative_sampling_queue_logprobs,
              S.speculative_sampling_queue_requests, S.speculative_sampling_queue_edits):
        assert "grammar" not in inspect.signature(f).parameters      # pinned by their own tests: no new keyword
    assert "speculative_sampling_queue_grammar" in S.__all__ and "TokenGrammar" in S.__all__


# ----------------------------------------------------------------------------- refusals
def _said():
    return _lib.lib.sd_last_error().decode()


def _item(grammar=None, states=P, **over):
    it = _lib.SdGrammarItem()
    setattr(it.row, "in", P)
    it.row.out, it.row.ld_in, it.row.ld_out, it.row.rows, it.row.seq = P, 128, 128, 3, P
    it.row.hist0, it.row.prompt_len, it.row.pen, it.row.eos_token_id = 4, 2, _lib.SdPenalty(1.0, 0.0, 0.0), 2
    for k, v in over.items():
        setattr(it.row, k, v)
    it.grammar = C.pointer(grammar) if grammar is not None else None
    it.states = states
    return it


GOOD = dict(masks=P, next=P, cls=P, n_states=5, n_classes=7, start=0)
BAD_GRAMMARS = [(dict(n_states=0), "n_states 0 < 1"), (dict(n_classes=0), "n_classes 0 < 1"), (dict(start=5), "start 5 outside [0, 5)"),
                (dict(start=-1), "start -1 outside [0, 5)"), (dict(masks=None), "null masks, next or states"),
                (dict(next=None), "null masks, next or states")]


def test_sd_grammar_rows_refuses_before_any_launch():
    V = 128
    rows = lambda *items: (_lib.SdGrammarItem * len(items))(*items)
    call = lambda arr, n, v=V, mode=0: _lib.lib.sd_grammar_rows(arr, n, v, mode, None)
    ok = _lib.SdGrammar(**GOOD)
    # the call's own refusals and everything sd_edit_rows refuses, under this entry's name
    for args, text in (((None, 1), "null argument"), ((rows(_item(ok)), 0), "n_items 0 outside 1..16"), ((rows(_item(ok)), 17), "n_items 17"),
                       ((rows(_item(ok)), 1, 0), "V 0 outside"), ((rows(_item(ok)), 1, 65537), "V 65537 outside"),
                       ((rows(_item(ok)), 1, V, 3), "both rounding bits")):
        assert call(*args) == _lib.SD_ERR_INVALID and _said().startswith("sd_grammar_rows: ") and text in _said(), (_said(), text)
    E = _lib.SdLogitEdit
    for over, text in ((dict(rows=0), "rows 0 outside 1..17"), (dict(rows=18), "rows 18 outside"), (dict(ld_in=V - 1), "< V 128"),
                       (dict(ld_out=V - 1), "< V 128"), (dict(hist0=0), "hist0 0 < 1"), (dict(prompt_len=-1), "prompt_len -1 < 0"),
                       (dict(seq=None), "null argument"), (dict(out=None), "null argument"),
                       (dict(pen=_lib.SdPenalty(0.0, 0, 0)), "repetition penalty 0 must be > 0"),
                       (dict(pen=_lib.SdPenalty(1.0, float("nan"), 0)), "must be finite"),
                       (dict(edit=E(P, P, -1, None, 0)), "n_bias -1 outside"), (dict(edit=E(P, P, 1025, None, 0)), "n_bias 1025 outside"),
                       (dict(edit=E(None, P, 2, None, 0)), "2 bias entries and a null array"), (dict(edit=E(None, None, 0, P, -1)), "min_tokens -1 < 0")):
        assert call(rows(_item(ok), _item(ok, **over)), 2) == _lib.SD_ERR_INVALID, over
        assert _said().startswith("sd_grammar_rows: item 1: ") and text in _said(), (_said(), text)
    # then the grammar's, per item; an item with a NULL grammar is not looked at (its states may be NULL)
    for over, text in BAD_GRAMMARS:
        bad = _lib.SdGrammar(**{**GOOD, **over})
        assert call(rows(_item(None, states=None), _item(ok), _item(bad)), 3) == _lib.SD_ERR_INVALID, over
        assert _said() == f"sd_grammar_rows: item 2: grammar: {text}", _said()
    assert call(rows(_item(ok), _item(ok, states=None)), 2) == _lib.SD_ERR_INVALID
    assert _said() == "sd_grammar_rows: item 1: grammar: null masks, next or states"
    ident = _lib.SdGrammar(**{**GOOD, "cls": None})
    assert call(rows(_item(ident)), 1) == _lib.SD_ERR_INVALID
    assert _said() == "sd_grammar_rows: item 0: grammar: no cls table and n_classes 7 differs from the vocabulary 128"
    # a row refusal of a later item comes before a grammar refusal of an earlier one ("everything sd_edit_rows refuses, then ...")
    assert call(rows(_item(_lib.SdGrammar(**{**GOOD, "n_states": 0})), _item(ok, rows=0)), 2) == _lib.SD_ERR_INVALID
    assert "item 1: rows 0" in _said()


def test_sd_session_set_grammar_refuses_a_bad_grammar_before_it_reads_the_session():
    set_g = _lib.lib.sd_session_set_grammar
    ok = _lib.SdGrammar(**GOOD)
    assert set_g(None, C.pointer(ok), P, 8) == _lib.SD_ERR_INVALID and _said() == "sd_session_set_grammar: null session"
    for over, text in BAD_GRAMMARS:
        bad = _lib.SdGrammar(**{**GOOD, **over})
        assert set_g(P, C.pointer(bad), P, 8) == _lib.SD_ERR_INVALID, over
        assert _said() == f"sd_session_set_grammar: grammar: {text}", _said()
    assert set_g(P, C.pointer(ok), None, 8) == _lib.SD_ERR_INVALID and _said() == "sd_session_set_grammar: grammar: null masks, next or states"
    for cap in (0, -3):
        assert set_g(P, C.pointer(ok), P, cap) == _lib.SD_ERR_INVALID
        assert _said() == f"sd_session_set_grammar: grammar: states_cap {cap} < 1"


def test_the_wrappers_refuse_before_a_model_is_touched():
    x = torch.zeros((1, 3), dtype=torch.int64)
    g = TokenGrammar(np.zeros((1, 1), dtype=np.int64), 0, 2, 8, classes=np.zeros(8, dtype=np.int64))
    for kw in (dict(), dict(rng="host"), dict(rng="device", verbose=True)):
        with pytest.raises(ValueError, match="grammar needs the native loop"):
            S.speculative_sampling(x, None, None, 2, None, 4, grammar=g, **kw)
    for kw in (dict(), dict(rng="device", _native=False)):
        with pytest.raises(ValueError, match="grammar needs the native loop"):
            S.autoregressive_sampling(x, None, 4, 2, grammar=g, **kw)
    tp = type("M", (), {"tp_group": object()})()
    with pytest.raises(ValueError, match="grammar is not available with a tensor-parallel target"):
        S.speculative_sampling(x, None, tp, 2, None, 4, grammar=g, rng="device")
    with pytest.raises(ValueError, match="tensor-parallel"):
        S.speculative_sampling_batch([x], None, tp, 2, None, 4, grammar=[g])
    with pytest.raises(ValueError, match="tensor-parallel"):
        S.autoregressive_sampling_batch([x], tp, 4, 2, grammar=g)
    with pytest.raises(ValueError, match="tensor-parallel"):
        S.speculative_sampling_queue_grammar([x], None, tp, 2, None, 4, grammar=g)
    with pytest.raises(ValueError, match="grammar: 2 entries for 1 streams"):
        S.speculative_sampling_batch([x], None, None, 2, None, 4, grammar=[g, None])
    with pytest.raises(ValueError, match="grammar: stream 0: a TokenGrammar or None"):
        S.autoregressive_sampling_batch([x], None, 4, 2, grammar=["json"])
    with pytest.raises(ValueError, match="one TokenGrammar for all prompts"):
        S.speculative_sampling_queue_grammar([x], None, None, 2, None, 4, grammar=[g])
    assert G.grammar_list(3, "stream", None) is None and G.grammar_list(3, "stream", [None] * 3) is None
    assert G.grammar_list(2, "stream", g) == [g, g] and G.grammar_list(2, "stream", [None, g]) == [None, g]
    with pytest.raises(ValueError, match="built for a vocabulary of 8, the model's is 512"):
        G.check_grammar_vocab([None, g], "stream", 512)


# ----------------------------------------------------------------------------- the builder
def test_token_grammar_validates_on_the_host():
    V = 10
    cls = np.arange(V) % 3
    nxt = np.array([[1, -1, 0], [-1, 2, -1], [0, 0, 0], [-1, -1, -1]])    # state 3 allows nothing and nothing leads to it: fine
    g = TokenGrammar(nxt, 0, 2, V, classes=cls)
    assert (g.n_states, g.n_classes, g.start, g.vocab_size) == (4, 3, 0, V) and g.masks.shape == (4, 1) and g.masks.dtype == np.uint32
    assert g.next.dtype == np.int32 and g.classes.dtype == np.int32
    for s in range(4):                                             # masks is next >= 0, bit for bit; the bits past V are clear
        assert [bool((int(g.masks[s, 0]) >> t) & 1) for t in range(32)] == [t < V and nxt[s, cls[t]] >= 0 for t in range(32)]
        assert g.allowed_ids(s).tolist() == [t for t in range(V) if nxt[s, cls[t]] >= 0]
    for tables in (torch.from_numpy(nxt), nxt.astype(np.int32), nxt.tolist()):
        assert np.array_equal(TokenGrammar(tables, 0, 2, V, classes=torch.from_numpy(cls)).masks, g.masks)
    reach = nxt.copy()
    reach[1, 1] = 3                                                # now state 3 is reachable: 0 -c0-> 1 -c1-> 3
    with pytest.raises(ValueError, match="state 3 is reachable from start 0 and allows no token"):
        TokenGrammar(reach, 0, 2, V, classes=cls)
    with pytest.raises(ValueError, match="state 3 is reachable from start 3"):
        TokenGrammar(nxt, 3, 2, V, classes=cls)
    # a class no token has does not make its target reachable
    lone = np.array([[0, 0, 0, 1], [-1, -1, -1, -1]])
    TokenGrammar(lone, 0, 2, V, classes=cls)
    for bad, text in ((4, r"state 0, class 0: 4 lies outside \[-1, 4\)"), (-2, r"-2 lies outside \[-1, 4\)")):
        broken = nxt.copy()
        broken[0, 0] = bad
        with pytest.raises(ValueError, match=text):
            TokenGrammar(broken, 0, 2, V, classes=cls)
    for bad, text in ((3, r"token 4: class 3 lies outside \[0, 3\)"), (-1, r"token 4: class -1 lies outside")):
        c = cls.copy()
        c[4] = bad
        with pytest.raises(ValueError, match=text):
            TokenGrammar(nxt, 0, 2, V, classes=c)
    with pytest.raises(ValueError, match="classes: 9 entries for a vocabulary of 10"):
        TokenGrammar(nxt, 0, 2, V, classes=cls[:9])
    with pytest.raises(ValueError, match="without a class table next has one column per token id, 10, not 3"):
        TokenGrammar(nxt, 0, 2, V)
    for start in (4, -1, True, 0.0):
        with pytest.raises(ValueError, match="start: a state in"):
            TokenGrammar(nxt, start, 2, V, classes=cls)
    with pytest.raises(ValueError, match="next: an integer table"):
        TokenGrammar(nxt.astype(np.float32), 0, 2, V, classes=cls)
    with pytest.raises(ValueError, match="next: a \\(n_states >= 1"):
        TokenGrammar(np.zeros(3, dtype=np.int64), 0, 2, V, classes=cls)


# ----------------------------------------------------------------------------- the definition
def test_from_choices_on_nested_and_prefix_sharing_choices():
    V, EOS = 40, 2
    choices = [[5, 6, 7], [5, 6], [5, 9, 9, 9], [11]]              # [5, 6] is a prefix of [5, 6, 7]; three share their first token
    g = TokenGrammar.from_choices(choices, V, EOS)
    assert g.classes is None and g.n_classes == V and g.start == 0
    assert g.allowed_ids(0).tolist() == [5, 11]
    assert g.allowed_ids(g.state_after([5])).tolist() == [6, 9]
    assert g.allowed_ids(g.state_after([5, 6])).tolist() == [EOS, 7]             # the end of a choice that a longer one continues
    assert g.allowed_ids(g.state_after([5, 6, 7])).tolist() == [EOS] and g.allowed_ids(g.state_after([11])).tolist() == [EOS]
    assert g.allowed_ids(g.state_after([5, 9, 9])).tolist() == [9]
    free = g.state_after([11, EOS])
    assert g.allowed_ids(free).tolist() == list(range(V)) and g.state_after([11, EOS, 3, EOS, 39]) == free   # behind EOS everything goes
    for c in choices:
        assert g.accepts_prefix(c) and g.accepts_prefix(c + [EOS]) and all(g.accepts_prefix(c[:k]) for k in range(len(c)))
    for bad in ([6], [5, 7], [5, 6, 7, 7], [5, 9, EOS], [EOS], [5, 6, 6], [V], [-1]):
        assert not g.accepts_prefix(bad), bad
    assert g.state_after([5, 7, 6]) == -1 and g.step(-1, 5) == -1 and g.step(g.n_states, 5) == -1 and g.step(0, V) == -1
    for bad, text in (([[5, EOS]], "is EOS"), ([[5], []], "choice 1 is empty"), ([], "at least one choice"), ([[V]], "outside")):
        with pytest.raises(ValueError, match=text):
            TokenGrammar.from_choices(bad, V, EOS)


def _plain_apply(row, masks_row, state, n_states):
    """apply_grammar restated element by element."""
    out = row.clone()
    if 0 <= state < n_states:
        for t in range(row.shape[0]):
            if not (int(masks_row[t >> 5]) >> (t & 31)) & 1:
                out[t] = float("-inf")
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_apply_grammar_against_a_plain_python_restatement(dtype):
    V = 130                                                        # 4 full words and a last word 2 bits wide
    rng = np.random.default_rng(3)
    cls = rng.integers(0, 7, size=V)
    nxt = rng.integers(-1, 6, size=(6, 7))
    nxt[:, 0] = np.arange(6)                                       # every state allows class 0 ...
    nxt[:, 1] = -1                                                 # ... and none class 1
    g = TokenGrammar(nxt, 2, 1, V, classes=cls)
    row = torch.from_numpy(rng.standard_normal(V).astype(np.float32) * 8).to(dtype)
    row[[3, 4, 5, 6, 129]] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")]).to(dtype)
    bits = lambda t: t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    for state in (-1, 0, 1, 2, 5, 6, 99):
        got = apply_grammar(row, g, state)
        want = _plain_apply(row, g.masks[state] if 0 <= state < 6 else None, state, 6)
        assert got.dtype == dtype and torch.equal(bits(got), bits(want)), state
        if not 0 <= state < 6:
            assert torch.equal(bits(got), bits(row))               # a dead row keeps every bit
        else:
            dropped = set(range(V)) - set(g.allowed_ids(state).tolist())
            assert dropped and all(float(got[t]) == float("-inf") for t in dropped)
    assert torch.equal(bits(row), bits(row.clone()))               # (the argument is not written)


# ----------------------------------------------------------------------------- the loop reference
def grammar_a(V, eos=None):
    """A 5-state cycle over cls = id mod 5: state s allows classes s, s + 1 (and s + 3 for even s) and moves on to s + 1, so
    every state keeps 40 - 60 % of the vocabulary."""
    nxt = np.full((5, 5), -1, dtype=np.int64)
    for s in range(5):
        for c in [s, (s + 1) % 5] + ([(s + 3) % 5] if s % 2 == 0 else []):
            nxt[s, c] = (s + 1) % 5
    return TokenGrammar(nxt, 0, eos, V, classes=np.arange(V) % 5)


def test_the_oracle_on_wrapped_models_emits_only_what_the_grammar_accepts():
    cfg = load_config("tiny-llama-target")
    dsd = make_state_dict(cfg, 21)
    od, ot = oracle.RefCausalLM(cfg, dsd), oracle.RefCausalLM(cfg, perturb_state_dict(dsd, 22, 0.12))
    V, EOS = cfg.vocab_size, 2
    prompt = torch.from_numpy(np.random.default_rng(5).integers(3, V, size=(1, 9)))
    L = prompt.shape[1]
    ga = grammar_a(V, EOS)
    gb = TokenGrammar.from_choices([[7, 300, 41], [7, 300], [7, 8, 8, 9]], V, EOS)
    torch.manual_seed(11)
    plain = oracle.speculative_sampling(prompt, od, ot, EOS, None, 16, gamma=4, top_k=20, top_p=0.9)
    assert not ga.accepts_prefix(plain[0, L:].tolist())            # (else the test shows nothing)
    for seed in (11, 12, 13):
        torch.manual_seed(seed)
        out = oracle.speculative_sampling(prompt, GrammarModel(od, L, EOS, ga), GrammarModel(ot, L, EOS, ga), EOS, None, 16, gamma=4,
                                          top_k=20, top_p=0.9)
        new = out[0, L:].tolist()
        assert len(new) >= 1 and ga.accepts_prefix(new), new
        torch.manual_seed(seed)
        out = oracle.speculative_sampling(prompt, GrammarModel(od, L, EOS, gb), GrammarModel(ot, L, EOS, gb), EOS, None, 16, gamma=4,
                                          top_k=20, top_p=0.9)
        new = out[0, L:].tolist()
        assert new in ([7, 300, 41, EOS], [7, 300, EOS], [7, 8, 8, 9, EOS]), new
        torch.manual_seed(seed)
        out = oracle.autoregressive_sampling(prompt, GrammarModel(ot, L, EOS, gb), 16, EOS, 1, 20, 0.9)
        assert out[0, L:].tolist() in ([7, 300, 41, EOS], [7, 300, EOS], [7, 8, 8, 9, EOS])
