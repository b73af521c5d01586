"""Per-request repetition / frequency / presence penalties: what needs no GPU - the ABI (one symbol, three structs; the
loops take the block as member penalties of sd_loop_opts; sd_version() 7), the keywords on the four free functions and the new
queue function, the refusals that come
before a model is touched, the refusals of sd_penalize_rows (all before a launch), sampling.utils.apply_penalties against a
hand-computed example (and HF's RepetitionPenaltyLogitsProcessor where transformers imports), and the wrapped oracle model
(tests/penalised_model.py) against a forward without a cache."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
import torch

import abi_header
import oracle
import penalised_model as PM
import llmspeculativesampling_amd.sampling as S
from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.config import load_config
from llmspeculativesampling_amd.sampling.utils import apply_penalties
from llmspeculativesampling_amd.synth import make_state_dict

NEW = ("sd_penalize_rows",)
REMOVED = ("sd_spec_generate_penalties", "sd_spec_batch_generate_penalties", "sd_spec_queue_generate_penalties",
           "sd_ar_batch_generate_penalties")                                    # ABI 7: member penalties of sd_loop_opts
SYM = {name: (res, args) for name, res, args in _lib.SYMBOLS}
PROTOS, STRUCTS = abi_header.parse()
KEYWORDS = {"repetition_penalty": 1.0, "frequency_penalty": 0.0, "presence_penalty": 0.0}
FREE = ["speculative_sampling", "speculative_sampling_batch", "autoregressive_sampling", "autoregressive_sampling_batch"]


def test_new_symbols_are_declared_bound_and_exported():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in PROTOS and name in SYM, name
        assert hasattr(raw, name), name
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(SYM[name][1])
    for name in REMOVED:
        assert name not in PROTOS and name not in SYM and not hasattr(raw, name), name
    assert _lib.lib.sd_version() == 7


def test_new_structs_match_the_header():
    for name, cls, size, fields in (
            ("sd_penalty", _lib.SdPenalty, 12, ["repetition", "frequency", "presence"]),
            ("sd_penalty_item", _lib.SdPenaltyItem, 72, ["in", "out", "ld_in", "ld_out", "rows", "seq", "hist0", "prompt_len", "pen"]),
            ("sd_penalty_block", _lib.SdPenaltyBlock, 32, ["rows", "ld", "max_rows", "params"])):
        assert _lib.C_STRUCTS[name] is cls
        assert C.sizeof(cls) == size == STRUCTS[name][1]
        assert [f for f, _ in cls._fields_] == fields
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == STRUCTS[name][0]
    # what the existing entries must keep
    assert C.sizeof(_lib.SdLogprobItem) == 48 and C.sizeof(_lib.SdLogprobBlock) == 24 and C.sizeof(_lib.SdAcceptResult) == 208


@pytest.mark.parametrize("name", FREE + ["speculative_sampling_queue_requests"])
def test_keywords_are_keyword_only_and_neutral_by_default(name):
    params = inspect.signature(getattr(S, name)).parameters
    for k, v in KEYWORDS.items():
        assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default == v, (name, k)


def test_queue_requests_has_queue_shared_s_positional_parameters():
    assert "speculative_sampling_queue_requests" in S.__all__
    a = inspect.signature(S.speculative_sampling_queue_shared).parameters
    b = inspect.signature(S.speculative_sampling_queue_requests).parameters
    positional = [k for k in b if b[k].kind is not inspect.Parameter.KEYWORD_ONLY]
    assert positional == list(a)
    assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    assert [k for k in b if b[k].kind is inspect.Parameter.KEYWORD_ONLY] == ["logprobs"] + list(KEYWORDS)
    assert b["logprobs"].default is False
    for f in (S.speculative_sampling_queue, S.speculative_sampling_queue_shared, S.speculative_sampling_queue_logprobs):
        assert not set(KEYWORDS) & set(inspect.signature(f).parameters)      # pinned by their own tests: no new keyword


X = torch.zeros((1, 3), dtype=torch.int64)
CALLS = {
    "speculative_sampling": lambda **kw: S.speculative_sampling(X, kw.pop("model", None), kw.pop("model2", None), 2, None, 4,
                                                                  **dict(dict(rng="device"), **kw)),
    "autoregressive_sampling": lambda **kw: S.autoregressive_sampling(X, kw.pop("model2", None), 4, 2, **dict(dict(rng="device"), **kw)),
    "speculative_sampling_batch": lambda **kw: S.speculative_sampling_batch([X, X], None, kw.pop("model2", None), 2, None, 4, **kw),
    "autoregressive_sampling_batch": lambda **kw: S.autoregressive_sampling_batch([X, X], kw.pop("model2", None), 4, 2, **kw),
    "speculative_sampling_queue_requests": lambda **kw: S.speculative_sampling_queue_requests([X, X], None, kw.pop("model2", None), 2,
                                                                                              None, 4, **kw),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_bad_values_refuse_before_a_model_is_touched(name):
    call = CALLS[name]
    for bad in (0.0, -1.5):
        with pytest.raises(ValueError, match="repetition_penalty"):
            call(repetition_penalty=bad)
    for k in KEYWORDS:
        for bad in (float("nan"), float("inf"), -float("inf"), "1", None, True):
            with pytest.raises(ValueError, match=k):
                call(**{k: bad})
    with pytest.raises(ValueError, match="tensor-parallel"):
        call(model2=types.SimpleNamespace(tp_group=object()), presence_penalty=0.5)
    if name in ("speculative_sampling", "autoregressive_sampling"):
        return
    for k in KEYWORDS:
        with pytest.raises(ValueError, match=f"{k}: 3 entries for 2"):
            call(**{k: [1.0, 1.0, 1.0]})
        with pytest.raises(ValueError, match=k):
            call(**{k: [1.0, float("nan")]})
    with pytest.raises(ValueError, match="repetition_penalty: (stream|prompt) 1"):
        call(repetition_penalty=[1.0, 0.0])


def test_interpreter_paths_refuse_before_a_model_is_touched():
    for pen in (dict(repetition_penalty=1.2), dict(frequency_penalty=0.1), dict(presence_penalty=-0.1)):
        for kw in (dict(), dict(rng="host"), dict(rng="device", verbose=True)):
            with pytest.raises(ValueError, match='penalties need the native loop: rng="device"'):
                S.speculative_sampling(X, None, None, 2, None, 4, **pen, **kw)
        for kw in (dict(rng="device", _native=False), dict(), dict(rng="host")):
            with pytest.raises(ValueError, match='penalties need the native loop: rng="device"'):
                S.autoregressive_sampling(X, None, 4, 2, **pen, **kw)


def _one(n_items=1, V=8, mode=0, pen=(1.2, 0.5, 0.5), **over):
    buf, out, seq = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_int32 * 32)()
    fields = dict(out=C.addressof(out), ld_in=V, ld_out=V, rows=1, seq=C.addressof(seq), hist0=4, prompt_len=2, pen=_lib.SdPenalty(*pen))
    fields["in"] = C.addressof(buf)
    fields.update(over)
    items = (_lib.SdPenaltyItem * 16)()
    for it in items:
        for k, v in fields.items():
            setattr(it, k, v)
    return _lib.lib.sd_penalize_rows(items, n_items, V, mode, None)


def test_penalize_rows_refusals_come_before_any_launch():
    """Host memory throughout: a call that got as far as a launch would fail another way."""
    err = lambda: _lib.lib.sd_last_error().decode()
    assert _lib.lib.sd_penalize_rows(None, 1, 8, 0, None) == _lib.SD_ERR_INVALID
    for n in (0, 17, -1):
        assert _one(n_items=n) == _lib.SD_ERR_INVALID and "n_items" in err()
    for rows in (0, 18):
        assert _one(rows=rows) == _lib.SD_ERR_INVALID and "rows" in err()
    for ld in ("ld_in", "ld_out"):
        assert _one(**{ld: 7}) == _lib.SD_ERR_INVALID and "ld" in err()
    for null in ("in", "out", "seq"):
        assert _one(**{null: None}) == _lib.SD_ERR_INVALID and "item 0" in err()
    for V in (0, 65537):
        assert _one(V=V, ld_in=70000, ld_out=70000) == _lib.SD_ERR_INVALID
    assert _one(mode=3) == _lib.SD_ERR_INVALID and _one(mode=3 | _lib.SD_NORM_DT_BF16) == _lib.SD_ERR_INVALID
    assert _one(hist0=0) == _lib.SD_ERR_INVALID and "hist0" in err()
    assert _one(prompt_len=-1) == _lib.SD_ERR_INVALID and "prompt_len" in err()
    for pen in ((0.0, 0, 0), (-1.0, 0, 0), (float("nan"), 0, 0), (1.0, float("inf"), 0), (1.0, 0, float("-inf")), (float("inf"), 0, 0)):
        assert _one(pen=pen) == _lib.SD_ERR_INVALID and "item 0" in err(), pen


def test_apply_penalties_on_a_hand_computed_example():
    """V = 8, history [5, 2, 2 | 7, 2, 0, 9] with a prompt of 3 (the 9 is outside [0, V) and ignored): c_all = {5: 1, 2: 3, 7: 1,
    0: 1}, c_out = {7: 1, 2: 1, 0: 1}.  theta = 2, f = 0.5, pi = 0.25; every value below is exact in fp32 (and in bf16)."""
    x = torch.tensor([4.0, 1.0, -3.0, 0.5, float("-inf"), 6.0, float("nan"), -0.0])
    hist = [5, 2, 2, 7, 2, 0, 9]
    want = torch.tensor([4.0 / 2 - 0.5 - 0.25,       # 0: in the output once
                         1.0,                        # 1: not in the history
                         -3.0 * 2 - 0.5 - 0.25,      # 2: negative logit, three times in all, once in the output
                         0.5, float("-inf"),         # 3, 4: not in the history
                         6.0 / 2,                    # 5: in the prompt only - no frequency / presence
                         float("nan"),               # 6: not in the history
                         -0.0 * 2 - 0.5 - 0.25])     # 7: in the output once
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        got = apply_penalties(x.to(dtype), hist, 3, 2.0, 0.5, 0.25)
        assert got.dtype == dtype
        assert torch.equal(got.float().nan_to_num(nan=77.0), want.nan_to_num(nan=77.0)), (dtype, got)
    # frequency scales with the count: token 2 three times in the output
    got = apply_penalties(x, [5, 2, 2, 2], 1, 1.0, 0.5, 0.0)
    assert float(got[2]) == -3.0 - 1.5 and float(got[5]) == 6.0
    # a prompt-only history: frequency and presence do nothing; neutral parameters: the row itself
    assert torch.equal(apply_penalties(x[:6], hist[:3], 3, 1.0, 9.0, 9.0), x[:6])
    assert torch.equal(apply_penalties(x[:6], hist, 3), x[:6])
    # 16-bit rows round after every operation: 1.0 / 1.2 in bf16, then minus bf16(0.3 * 1)
    r = apply_penalties(torch.tensor([1.0, 1.0], dtype=torch.bfloat16), [0, 0], 1, 1.2, 0.3, 0.0)
    one = torch.tensor(1.0)
    a = (one / torch.tensor(1.2)).to(torch.bfloat16).float()
    b = (torch.tensor(0.3) * 1.0).to(torch.bfloat16).float()
    assert float(r[0]) == float((a - b).to(torch.bfloat16)) and float(r[1]) == 1.0


def test_repetition_part_equals_the_hf_processor():
    tr = pytest.importorskip("transformers")
    proc = tr.RepetitionPenaltyLogitsProcessor(1.3)
    g = torch.Generator().manual_seed(3)
    scores = torch.randn(1, 500, generator=g) * 6
    ids = torch.randint(0, 500, (1, 120), generator=g)
    want = proc(ids, scores.clone())[0]
    got = apply_penalties(scores[0], ids[0], 40, 1.3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_wrapped_oracle_model_equals_a_forward_without_a_cache():
    """The wrapper follows the prefix through prefill, cached steps of 1 and 3 rows and a rollback of the cache."""
    cfg = load_config("tiny-llama-draft")
    om = oracle.RefCausalLM(cfg, make_state_dict(cfg, 3))
    ids = torch.from_numpy(np.random.default_rng(5).integers(0, 12, size=(1, 14)))     # a small alphabet: plenty of repeats
    pen = (1.7, 0.6, -0.4)
    want = PM.full_forward(om, ids, 4, *pen)
    assert not torch.equal(want, om(ids, use_cache=False).logits[0])
    wm = PM.PenalisedModel(om, 4, *pen)
    out = wm(ids[:, :6])
    rows = [out.logits[0]]
    out = wm(ids[:, 6:7], past_key_values=out.past_key_values)
    rows.append(out.logits[0])
    out = wm(ids[:, 7:10], past_key_values=out.past_key_values)
    rows.append(out.logits[0])
    back = [(k[:, :, :8], v[:, :, :8]) for k, v in out.past_key_values]               # positions 8, 9 are fed again
    out = wm(ids[:, 8:14], past_key_values=back)
    got = torch.cat(rows + [out.logits[0][2:]])
    assert torch.allclose(got, want, rtol=0, atol=1e-5)
    assert torch.allclose(out.logits[0][:2], rows[2][1:], rtol=0, atol=1e-5)           # (the two rows fed twice)
    assert wm.tokens == ids[0].tolist()
