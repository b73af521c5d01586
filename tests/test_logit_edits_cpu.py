"""Per-request logit_bias / allowed_token_ids / banned_token_ids / min_tokens: what needs no GPU - the ABI (one symbol, three
structs; the loops take the block as member edits of sd_loop_opts; sd_version() 7), sampling.utils.apply_logit_edits against a
plain per-element loop in the
five rounding / dtype modes, the composition order with apply_penalties, the mask builder, every refusal that comes before a
model is touched, the refusals of sd_edit_rows (all before a launch), and which members of sd_loop_opts a call sets."""
import ctypes as C
import importlib
import inspect
import math
import types

import numpy as np
import pytest
import torch

import abi_header
import edited_model as EM
import llmspeculativesampling_amd.sampling as S
from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.sampling import _loop_common as LC
from llmspeculativesampling_amd.sampling.utils import apply_logit_edits, apply_penalties

AR = importlib.import_module("llmspeculativesampling_amd.sampling.autoregressive_sampling")   # (the package exports the function)
NEW = ("sd_edit_rows",)
REMOVED = ("sd_spec_generate_edits", "sd_spec_batch_generate_edits", "sd_spec_queue_generate_edits",
           "sd_ar_batch_generate_edits")                                        # ABI 7: member edits of sd_loop_opts
SYM = {name: (res, args) for name, res, args in _lib.SYMBOLS}
PROTOS, STRUCTS = abi_header.parse()
KEYWORDS = {"logit_bias": None, "allowed_token_ids": None, "banned_token_ids": None, "min_tokens": 0}
FREE = ["speculative_sampling", "speculative_sampling_batch", "autoregressive_sampling", "autoregressive_sampling_batch"]
ROUND_BF16, DT_BF16, DT_F16 = 1, 16, 32
MODES = {"fp32": 0, "round_bf16": ROUND_BF16, "dt_bf16": DT_BF16, "dt_f16": DT_F16, "round_bf16_dt_bf16": ROUND_BF16 | DT_BF16}


# ----------------------------------------------------------------------------- the ABI
def test_new_symbols_are_declared_bound_and_exported():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in PROTOS and name in SYM, name
        assert hasattr(raw, name), name
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(SYM[name][1])
        assert PROTOS[name][1] == [abi_header.ctypes_class(t) for t in SYM[name][1]], name
    for name in REMOVED:
        assert name not in PROTOS and name not in SYM and not hasattr(raw, name), name
    assert _lib.lib.sd_version() == 7
    assert "#define SD_EDIT_MAX_BIAS 1024" in open(abi_header.HEADER).read() and _lib.SD_EDIT_MAX_BIAS == 1024


def test_new_structs_match_the_header():
    for name, cls, size, fields in (
            ("sd_logit_edit", _lib.SdLogitEdit, 40, ["bias_ids", "bias_vals", "n_bias", "allowed", "min_tokens"]),
            ("sd_logit_edit_item", _lib.SdLogitEditItem, 120,
             ["in", "out", "ld_in", "ld_out", "rows", "seq", "hist0", "prompt_len", "pen", "edit", "eos_token_id"]),
            ("sd_logit_edit_block", _lib.SdLogitEditBlock, 32, ["rows", "ld", "max_rows", "params"])):
        assert _lib.C_STRUCTS[name] is cls
        assert C.sizeof(cls) == size == STRUCTS[name][1]
        assert [f for f, _ in cls._fields_] == fields
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == STRUCTS[name][0]
    # an edit item starts with a penalty item, field for field; what the existing entries take keeps its size
    n = len(_lib.SdPenaltyItem._fields_)
    assert STRUCTS["sd_logit_edit_item"][0][:n] == STRUCTS["sd_penalty_item"][0]
    assert C.sizeof(_lib.SdPenaltyItem) == 72 and C.sizeof(_lib.SdPenaltyBlock) == 32 and C.sizeof(_lib.SdPenalty) == 12


@pytest.mark.parametrize("name", FREE + ["speculative_sampling_queue_edits"])
def test_keywords_are_keyword_only_and_neutral_by_default(name):
    params = inspect.signature(getattr(S, name)).parameters
    for k, v in KEYWORDS.items():
        assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default == v, (name, k)


def test_queue_edits_has_queue_requests_parameters_and_the_four_keywords():
    """speculative_sampling_queue_requests' parameter list is pinned by test_penalties_cpu, so the queue takes the four keywords
    through a function of its own, with that function's parameters, kinds and defaults in front of them."""
    assert "speculative_sampling_queue_edits" in S.__all__
    a = inspect.signature(S.speculative_sampling_queue_requests).parameters
    b = inspect.signature(S.speculative_sampling_queue_edits).parameters
    assert list(b) == list(a) + list(KEYWORDS)
    assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    for f in (S.speculative_sampling_queue, S.speculative_sampling_queue_shared, S.speculative_sampling_queue_logprobs,
              S.speculative_sampling_queue_requests):
        assert not set(KEYWORDS) & set(inspect.signature(f).parameters)      # pinned by their own tests: no new keyword


# ----------------------------------------------------------------------------- the definition
def _as_read(x, mode):
    """The row as the sampler reads it (pending rounding applied), in the dtype the definitions are to work in."""
    if mode & 3:
        x = x.to(torch.bfloat16).float()
    dt = {DT_BF16: torch.bfloat16, DT_F16: torch.float16}.get(mode & 48)
    return x.to(dt) if dt else x


def _loop_definition(row, j, eos, bias, mask, m):
    """include/specdec.h's three steps, one element at a time, on python / numpy scalars."""
    V, dt = row.shape[0], row.dtype
    out = row.clone()
    for t in range(V):
        y = np.float32(row[t].float().item())
        if bias and t in bias:
            with np.errstate(invalid="ignore", over="ignore"):
                y = np.float32(y + np.float32(bias[t]))
            y = np.float32(torch.tensor(float(y), dtype=torch.float32).to(dt).float().item())
        if mask is not None and not (int(mask[t >> 5]) >> (t & 31)) & 1:
            y = np.float32(-np.inf)
        if eos >= 0 and t == eos and m > 0 and j < m:
            y = np.float32(-np.inf)
        out[t] = float(y)
    return out


def _bits(x):
    return x.float().view(torch.int32)


@pytest.mark.parametrize("mode", list(MODES))
def test_apply_logit_edits_equals_a_per_element_loop(mode):
    V = 77                                                        # a partial last mask word
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal(V).astype(np.float32)) * 8
    special = [0.0, -0.0, float("inf"), float("-inf"), float("nan")]
    for i, v in enumerate(special * 3):
        x[3 * i] = v                                              # ids 0, 3, ..., 42: five specials, three times
    row = _as_read(x, MODES[mode])
    # biases on every special of the first two rounds, on plain ids, one far above the 16-bit grids' spacing, one outside [0, V)
    bias = {3 * i: b for i, b in enumerate([1.5, -0.0, 2.0, 3.0, 1.0, -1e-3, 0.0, -7.25, 9.0, 0.5])}
    bias.update({50: 0.1, 51: -1234.567, 76: 3.3, V + 4: 5.0})
    allowed = [t for t in range(V) if t % 3 != 1 or t > 60] + []
    mask = LC.allowed_mask_words(V, allowed, [0, 33, 76])
    dm = MODES[mode] & 48
    # (j < 0: a row inside the prompt - below any min_tokens > 0, and left alone by min_tokens 0)
    for eos, j, m in ((6, 2, 3), (6, 3, 3), (-1, 0, 9), (50, 0, 1), (6, -4, 0), (6, -4, 2)):
        for b, k in ((bias, mask), (bias, None), (None, mask), (None, None)):
            got = apply_logit_edits(row, j, eos, b, k, m)
            want = _loop_definition(row, j, eos, b, k, m)
            assert got.dtype == row.dtype and got is not row
            nan = want.float().isnan()
            assert torch.equal(got.float().isnan(), nan) and torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (mode, eos, j, m)
            # the explicit dtype mode on an fp32 copy of the row says the same
            again = apply_logit_edits(row.float(), j, eos, b, k, m, dtype_mode=dm)
            assert torch.equal(_bits(again)[~nan], _bits(want)[~nan])
            if b is None and k is None and not (0 <= eos and 0 < m and j < m):
                assert torch.equal(_bits(got), _bits(row))        # neutral: the row's own bits, -0 and NaN payloads included
    assert torch.equal(_bits(apply_logit_edits(row, -4, 6, None, None, 0)), _bits(row)) and float(row[6]) == math.inf
    assert float(apply_logit_edits(row, -4, 6, None, None, 2)[6]) == -math.inf
    # ids in no list keep their bits, -0 included; a masked NaN / +inf is -inf
    got = apply_logit_edits(row, 0, -1, bias, mask, 0)
    for t in range(V):
        if t not in bias and (int(mask[t >> 5]) >> (t & 31)) & 1:
            assert int(_bits(got)[t]) == int(_bits(row)[t]), t
    assert float(got[1]) == -math.inf and float(got[0]) == -math.inf and float(got[33]) == -math.inf


def test_penalties_come_first_then_bias_then_the_masks():
    """Token 1 has logit 2 and sits in the history: repetition 2, bias +3.  Penalty first: 2 / 2 + 3 = 4; bias first would give
    (2 + 3) / 2 = 2.5.  Token 2 is biased by +100 and banned: the mask wins.  Token 3 (EOS) is biased and below min_tokens."""
    x = torch.tensor([0.5, 2.0, 1.0, 1.0, -1.0])
    hist, P = [1, 4, 1], 2
    bias = {1: 3.0, 2: 100.0, 3: 50.0}
    mask = LC.allowed_mask_words(5, None, [2])
    y = apply_logit_edits(apply_penalties(x, hist, P, 2.0), len(hist) - P, 3, bias, mask, 2)
    assert y.tolist() == [0.5, 4.0, -math.inf, -math.inf, -2.0]
    other = apply_penalties(apply_logit_edits(x, len(hist) - P, 3, bias, mask, 2), hist, P, 2.0)
    assert other.tolist()[1] == 2.5
    y = apply_logit_edits(apply_penalties(x, hist, P, 2.0), 2, 3, bias, mask, 2)       # output token number 2: EOS is free again
    assert y.tolist()[3] == 51.0
    om = types.SimpleNamespace(config=types.SimpleNamespace(vocab_size=5), device="cpu")
    wm = EM.EditedModel(om, P, 3, (2.0, 0.0, 0.0), bias, None, [2], 2)
    wm.tokens = hist
    assert wm.row(x, 3).tolist() == [0.5, 4.0, -math.inf, -math.inf, -2.0]


def test_mask_builder():
    V = 77
    w = LC.allowed_mask_words(V, [0, 31, 32, V - 1, 40], [40])
    assert w.dtype == np.uint32 and w.shape == (3,)
    assert w.tolist() == [1 | 1 << 31, 1, 1 << (76 - 64)]
    w = LC.allowed_mask_words(V, None, [31, 32])
    assert w.tolist() == [0x7FFFFFFF, 0xFFFFFFFE, (1 << 13) - 1]                          # bits of ids >= V stay clear
    assert LC.allowed_mask_words(64, None, []).tolist() == [0xFFFFFFFF] * 2
    assert LC.allowed_mask_words(V, [5], [5]).tolist() == [0, 0, 0]


# ----------------------------------------------------------------------------- the helper and its refusals
def test_neutral_arguments_return_none():
    for kw in (dict(), dict(logit_bias={}), dict(logit_bias=[None, {}, None]), dict(allowed_token_ids=[None, None, None]),
               dict(banned_token_ids=[[], None, []]), dict(min_tokens=[0, 0, 0]), dict(min_tokens=np.zeros(3, dtype=np.int64))):
        assert LC.logit_edits(3, "prompt", 100, 2, **kw) is None, kw
        assert LC.logit_edits(3, "prompt", None, 2, **kw) is None, kw


def test_records():
    r = LC.logit_edits(3, "prompt", 100, 2, logit_bias=[{7: 1.0, 3: -2}, None, None], allowed_token_ids=[None, [5, 2, 99], None],
                       banned_token_ids=[4], min_tokens=[0, 0, 6])
    assert r[0]["bias_ids"].tolist() == [3, 7] and r[0]["bias_vals"].tolist() == [-2.0, 1.0] and r[0]["bias_ids"].dtype == np.int32
    assert r[0]["mask"].tolist() == LC.allowed_mask_words(100, None, [4]).tolist() and r[0]["min_tokens"] == 0
    assert r[1]["mask"].tolist() == LC.allowed_mask_words(100, [2, 5, 99], []).tolist() and len(r[1]["bias_ids"]) == 0
    assert r[2]["min_tokens"] == 6
    one = LC.logit_edits(2, "stream", 100, 2, logit_bias={9: 0.5}, allowed_token_ids=np.array([1, 2, 3]))
    assert all(x["bias_ids"].tolist() == [9] and x["mask"].tolist() == [0b1110, 0, 0, 0] for x in one)


X = torch.zeros((1, 3), dtype=torch.int64)
CALLS = {
    "helper": lambda **kw: LC.logit_edits(2, "stream", 5000, 2, **{k: v for k, v in kw.items() if k != "model2"}),
    "speculative_sampling": lambda **kw: S.speculative_sampling(X, None, kw.pop("model2", None), 2, None, 4, **dict(dict(rng="device"), **kw)),
    "autoregressive_sampling": lambda **kw: S.autoregressive_sampling(X, kw.pop("model2", None), 4, 2, **dict(dict(rng="device"), **kw)),
    "speculative_sampling_batch": lambda **kw: S.speculative_sampling_batch([X, X], None, kw.pop("model2", None), 2, None, 4, **kw),
    "autoregressive_sampling_batch": lambda **kw: S.autoregressive_sampling_batch([X, X], kw.pop("model2", None), 4, 2, **kw),
    "speculative_sampling_queue_edits": lambda **kw: S.speculative_sampling_queue_edits([X, X], None, kw.pop("model2", None), 2, None, 4,
                                                                                        **kw),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_bad_values_refuse_before_a_model_is_touched(name):
    call = CALLS[name]
    single = name in ("speculative_sampling", "autoregressive_sampling")
    for bad in (math.nan, math.inf, -math.inf, "1", None, True):
        with pytest.raises(ValueError, match="logit_bias"):
            call(logit_bias={5: bad})
    with pytest.raises(ValueError, match="logit_bias.*1025 entries"):
        call(logit_bias={i: 0.5 for i in range(1025)})
    call_ok = LC.logit_edits(1, "stream", 5000, 2, logit_bias={i: 0.5 for i in range(1024)})
    assert len(call_ok[0]["bias_ids"]) == 1024
    for k, bad in (("logit_bias", {-1: 1.0}), ("logit_bias", {1.5: 1.0}), ("logit_bias", {"7": 1.0}), ("logit_bias", {True: 1.0}),
                   ("logit_bias", 3.0), ("allowed_token_ids", [3, -2]), ("allowed_token_ids", [3, 2.0]), ("allowed_token_ids", 7),
                   ("banned_token_ids", [True]), ("banned_token_ids", ["a"]), ("min_tokens", -1), ("min_tokens", 1.5),
                   ("min_tokens", None), ("min_tokens", True)):
        with pytest.raises(ValueError, match=k):
            call(**{k: bad})
    with pytest.raises(ValueError, match="allowed_token_ids: (stream|prompt) 0: no token id is left"):
        call(allowed_token_ids=[4, 9], banned_token_ids=[9, 4, 11])
    with pytest.raises(ValueError, match="allowed_token_ids: (stream|prompt) 0: no token id is left"):
        call(allowed_token_ids=[])
    with pytest.raises(ValueError, match="allowed_token_ids: (stream|prompt) 0: only EOS"):
        call(allowed_token_ids=[2, 8], banned_token_ids=[8], min_tokens=1)
    if name != "helper":
        with pytest.raises(ValueError, match="tensor-parallel"):
            call(model2=types.SimpleNamespace(tp_group=object()), min_tokens=3)
    if single:
        return
    for k, three in (("logit_bias", [None, {1: 1.0}, None]), ("allowed_token_ids", [[1], [2], None]), ("banned_token_ids", [[1], None, None]),
                     ("min_tokens", [1, 2, 3])):
        with pytest.raises(ValueError, match=f"{k}: 3 entries for 2"):
            call(**{k: three})
    with pytest.raises(ValueError, match="logit_bias: (stream|prompt) 1"):
        call(logit_bias=[None, {3: math.nan}])
    with pytest.raises(ValueError, match="banned_token_ids: (stream|prompt) 1"):
        call(banned_token_ids=[None, [-4]])
    with pytest.raises(ValueError, match="min_tokens: (stream|prompt) 1"):
        call(min_tokens=[0, -2])
    with pytest.raises(ValueError, match="allowed_token_ids: (stream|prompt) 1: only EOS"):
        call(allowed_token_ids=[None, [2]], min_tokens=[0, 4])


def test_bind_finishes_the_records_of_a_parse_without_the_vocabulary():
    """The wrappers parse before a model is touched (V None) and bind once V is known: the same records as one call with V,
    requests that share their lists share one mask, and the refusals that need V come from the bind."""
    kw = dict(logit_bias=[{7: 1.0, 3: -2}, None, {99: 0.5}], allowed_token_ids=[None, [5, 2, 99], None], banned_token_ids=[4], min_tokens=[0, 0, 6])
    whole = LC.logit_edits(3, "prompt", 100, 2, **kw)
    early = LC.logit_edits(3, "prompt", None, 2, **kw)
    assert all(r["mask"] is None for r in early)
    late = LC.bind_logit_edits(early, "prompt", 100, 2)
    assert late is early
    for a, b in zip(whole, late):
        assert a["bias_ids"].tolist() == b["bias_ids"].tolist() and a["bias_vals"].tolist() == b["bias_vals"].tolist()
        assert a["mask"].tolist() == b["mask"].tolist() and a["min_tokens"] == b["min_tokens"]
    assert late[0]["mask"] is late[2]["mask"] and late[0]["mask"] is not late[1]["mask"]
    for name, bad in (("logit_bias", dict(logit_bias={100: 1.0})), ("allowed_token_ids", dict(allowed_token_ids=[1, 100])),
                      ("banned_token_ids", dict(banned_token_ids=[None, [3, 100]]))):
        early = LC.logit_edits(2, "stream", None, 2, **bad)
        with pytest.raises(ValueError, match=name + r": stream [01]: token id 100 outside \[0, 100\)"):
            LC.bind_logit_edits(early, "stream", 100, 2)
    early = LC.logit_edits(1, "stream", None, 2, banned_token_ids=[0, 1, 3], min_tokens=2)
    with pytest.raises(ValueError, match="only EOS"):
        LC.bind_logit_edits(early, "stream", 4, 2)
    assert LC.bind_logit_edits(early, "stream", 5, 2)[0]["mask"].tolist() == [0b10100]


def test_ids_outside_the_vocabulary_refuse_once_it_is_known():
    for kw in (dict(logit_bias={100: 1.0}), dict(allowed_token_ids=[1, 100]), dict(banned_token_ids=[[100], None])):
        with pytest.raises(ValueError, match=r"token id 100 outside \[0, 100\)"):
            LC.logit_edits(2, "stream", 100, 2, **kw)
        assert LC.logit_edits(2, "stream", 101, 2, **kw) is not None
    with pytest.raises(ValueError, match="no token id is left"):
        LC.logit_edits(1, "stream", 4, 2, banned_token_ids=[0, 1, 2, 3])
    with pytest.raises(ValueError, match="only EOS"):
        LC.logit_edits(1, "stream", 4, 2, banned_token_ids=[0, 1, 3], min_tokens=2)


def test_interpreter_paths_refuse_before_a_model_is_touched():
    for ed in (dict(logit_bias={1: 1.0}), dict(allowed_token_ids=[1, 2]), dict(banned_token_ids=[1]), dict(min_tokens=2)):
        for kw in (dict(), dict(rng="host"), dict(rng="device", verbose=True)):
            with pytest.raises(ValueError, match='min_tokens need the native loop: rng="device"'):
                S.speculative_sampling(X, None, None, 2, None, 4, **ed, **kw)
        for kw in (dict(rng="device", _native=False), dict(), dict(rng="host")):
            with pytest.raises(ValueError, match='min_tokens need the native loop: rng="device"'):
                S.autoregressive_sampling(X, None, 4, 2, **ed, **kw)


# ----------------------------------------------------------------------------- sd_edit_rows' refusals
def _one(n_items=1, V=8, mode=0, pen=(1.2, 0.5, 0.5), edit=None, **over):
    buf, out, seq = (C.c_float * 64)(), (C.c_float * 64)(), (C.c_int32 * 32)()
    fields = dict(out=C.addressof(out), ld_in=V, ld_out=V, rows=1, seq=C.addressof(seq), hist0=4, prompt_len=2, pen=_lib.SdPenalty(*pen),
                  edit=_lib.SdLogitEdit(*(edit or (None, None, 0, None, 0))), eos_token_id=2)
    fields["in"] = C.addressof(buf)
    fields.update(over)
    items = (_lib.SdLogitEditItem * 16)()
    for it in items:
        for k, v in fields.items():
            setattr(it, k, v)
    return _lib.lib.sd_edit_rows(items, n_items, V, mode, None)


def test_edit_rows_refusals_come_before_any_launch():
    """Host memory throughout: a call that got as far as a launch would fail another way."""
    err = lambda: _lib.lib.sd_last_error().decode()
    ids, vals = (C.c_int32 * 4)(), (C.c_float * 4)()
    assert _lib.lib.sd_edit_rows(None, 1, 8, 0, None) == _lib.SD_ERR_INVALID
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
    for pen in ((0.0, 0, 0), (float("nan"), 0, 0), (1.0, float("inf"), 0)):
        assert _one(pen=pen) == _lib.SD_ERR_INVALID and "item 0" in err(), pen
    a, b = C.addressof(ids), C.addressof(vals)
    for edit, word in (((a, b, -1, None, 0), "n_bias"), ((a, b, 1025, None, 0), "n_bias"), ((None, b, 2, None, 0), "null array"),
                       ((a, None, 2, None, 0), "null array"), ((None, None, 0, None, -1), "min_tokens")):
        assert _one(edit=edit) == _lib.SD_ERR_INVALID and "item 0" in err() and word in err(), (edit, err())


# ----------------------------------------------------------------------------- which members of sd_loop_opts a call sets
class _Called(Exception):
    pass


class _RecordingLib:
    """Stands in for the module's `lib`: sd_ar_block_bytes answers, every loop entry says its name, its argument count and the
    set of non-NULL members of its last argument, the sd_loop_opts (an empty set: opts was NULL), and stops the call."""

    def sd_ar_block_bytes(self, n):
        return 8 * n

    def __getattr__(self, name):
        def entry(*args):
            opts = args[-1]
            assert opts is None or isinstance(opts, _lib.SdLoopOpts), opts
            raise _Called(name, len(args), {f for f, _ in _lib.SdLoopOpts._fields_ if opts is not None and getattr(opts, f)})
        return entry


def _fake_run(monkeypatch):
    """An ArRun of two streams on the CPU, with stand-ins for what generate() reads of a model, a session and a noise object."""
    monkeypatch.setattr(AR, "lib", _RecordingLib())
    monkeypatch.setattr(AR, "_stream", lambda: None)
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    V = 64
    model = types.SimpleNamespace(device="cpu", cfg=types.SimpleNamespace(vocab_size=V), norm_mode=0)
    run = AR.ArRun(model, 1.0, 20, 0.9, 2)
    for i in range(2):
        ses = types.SimpleNamespace(handle=None, cache_len=0, max_rows=8, logits=torch.zeros(8, V), model=model)
        kv = types.SimpleNamespace(_session=ses, _probs=torch.zeros(8, V), _norm_ws=torch.zeros(16))
        run.add(kv, torch.zeros(16, dtype=torch.int32), np.array([3, 4, 5], dtype=np.int32), 8, types.SimpleNamespace(seed=1, draw=0))
    return run


def test_neutral_calls_take_the_entry_they_took_before(monkeypatch):
    """generate() - behind autoregressive_sampling and autoregressive_sampling_batch - with the records logit_edits returns: None
    (every neutral spelling) makes the call that was made before the keywords existed - a NULL sd_loop_opts, or the members
    logprobs and penalties alone ask for; records set member edits, with and without a penalty block.  The whole set of non-NULL
    members is compared, and a call that sets none passes NULL, not an empty block."""
    run = _fake_run(monkeypatch)
    neutral = LC.logit_edits(2, "stream", 64, 2, logit_bias=[None, {}], allowed_token_ids=None, banned_token_ids=[[], None], min_tokens=[0, 0])
    assert neutral is None
    pens = [(1.0, 0.0, 0.5), (1.0, 0.0, 0.0)]
    recs = LC.logit_edits(2, "stream", 64, 2, logit_bias=[{5: 1.0}, None], min_tokens=3, banned_token_ids=[7])
    for kw, want in ((dict(edits=neutral), set()), (dict(edits=neutral, logprobs=True), {"logprobs"}),
                     (dict(edits=neutral, penalties=pens), {"penalties"}),
                     (dict(edits=neutral, penalties=pens, logprobs=True), {"logprobs", "penalties"}),
                     (dict(edits=recs), {"edits"}), (dict(edits=recs, penalties=pens), {"penalties", "edits"}),
                     (dict(edits=recs, penalties=pens, logprobs=True), {"logprobs", "penalties", "edits"})):
        with pytest.raises(_Called) as e:
            run.generate(**kw)
        assert e.value.args == ("sd_ar_batch_generate", 10, want), (kw, e.value.args)


def test_edit_block_uploads_one_tensor_per_kind():
    recs = LC.logit_edits(3, "prompt", 70, 2, logit_bias=[{7: 1.0, 3: -2.0}, None, {69: 0.25}], allowed_token_ids=[None, [5, 2, 69], None],
                          min_tokens=[0, 0, 6])
    eb = LC.LogitEditBlock("cpu", recs, 70, 5)
    assert eb.rows.shape == (5, 72) and eb.block.ld == 72 and eb.block.max_rows == 5
    assert eb._ids.tolist() == [3, 7, 69] and eb._vals.tolist() == [-2.0, 1.0, 0.25] and eb._masks.numel() == 3
    p = eb._params
    assert [x.n_bias for x in p] == [2, 0, 1] and [x.min_tokens for x in p] == [0, 0, 6]
    assert p[0].bias_ids == eb._ids.data_ptr() and p[2].bias_ids == eb._ids.data_ptr() + 8 and p[1].bias_ids is None
    assert p[2].bias_vals == eb._vals.data_ptr() + 8 and p[1].bias_vals is None
    assert p[1].allowed == eb._masks.data_ptr() and p[0].allowed is None and p[2].allowed is None
    shared = torch.zeros(5, 72)
    assert LC.LogitEditBlock("cpu", recs, 70, 5, shared).block.rows == shared.data_ptr()
