"""Token scoring (sd_score_rows, sd_score_sequence, quality.score_tokens): what needs no GPU - the ABI (two symbols, two structs),
the refusals that come before a launch (those of sd_score_sequence that read the session - ld_slab, max_seq, a tensor-parallel
group - need a session and so a device: tests/test_gpu_score.py has them), quality.score_rows_torch against the numpy truth of
tests/score_rows.py, and score_tokens' refusals before a model is touched."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import abi_header
import score_rows as SR
from llmspeculativesampling_amd import _lib, quality
from llmspeculativesampling_amd.engine import SpecDecModel

NEW = ("sd_score_rows", "sd_score_sequence")
SYM = {name: (res, args) for name, res, args in _lib.SYMBOLS}
PROTOS, STRUCTS = abi_header.parse()
INVALID = _lib.SD_ERR_INVALID


def _err():
    return _lib.lib.sd_last_error().decode()


def test_symbols_are_declared_bound_and_exported():
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in PROTOS and name in SYM, name
        assert hasattr(raw, name), name
        fn = getattr(_lib.lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(SYM[name][1])
        assert PROTOS[name][0] == "i32" and PROTOS[name][1] == [abi_header.ctypes_class(a) for a in SYM[name][1]]
    assert _lib.lib.sd_version() == 7
    text = open(abi_header.HEADER).read()
    assert "#define SD_SCORE_MAX_TOP 20\n" in text and "#define SD_SCORE_MAX_ROWS 80\n" in text
    assert (_lib.SD_SCORE_MAX_TOP, _lib.SD_SCORE_MAX_ROWS) == (20, 80) == (SR.MAX_TOP, 80)


def test_structs_match_the_header():
    for name, cls, size in (("sd_score_item", _lib.SdScoreItem, 64), ("sd_score_out", _lib.SdScoreOut, 32)):
        assert _lib.C_STRUCTS[name] is cls
        assert C.sizeof(cls) == size == STRUCTS[name][1]
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == STRUCTS[name][0]
    assert [f for f, _ in _lib.SdScoreItem._fields_] == ["logits", "ld", "rows", "tokens", "logprob", "rank", "top_ids", "top_logprobs"]
    assert [f for f, _ in _lib.SdScoreOut._fields_] == ["logprob", "rank", "top_ids", "top_logprobs"]
    # what the existing entries must keep
    assert C.sizeof(_lib.SdLogprobItem) == 48 and C.sizeof(_lib.SdLogprobBlock) == 24 and C.sizeof(_lib.SdLoopOpts) == 32


def _rows(n_items=1, V=8, top_n=2, mode=0, **over):
    buf, tok, lp, rk = (C.c_float * 64)(), (C.c_int32 * 80)(), (C.c_float * 80)(), (C.c_int32 * 80)()
    ti, tl = (C.c_int32 * 1600)(), (C.c_float * 1600)()
    fields = dict(logits=C.addressof(buf), ld=V, rows=1, tokens=C.addressof(tok), logprob=C.addressof(lp), rank=C.addressof(rk),
                  top_ids=C.addressof(ti), top_logprobs=C.addressof(tl))
    fields.update(over)
    items = (_lib.SdScoreItem * 17)(*[_lib.SdScoreItem(**fields) for _ in range(17)])
    return _lib.lib.sd_score_rows(items, n_items, V, top_n, mode, None)


def test_score_rows_refusals_come_before_any_launch():
    """Host memory throughout: a call that got as far as a launch would fail another way."""
    assert _lib.lib.sd_score_rows(None, 1, 8, 0, 0, None) == INVALID
    for n in (0, 17, -1):
        assert _rows(n_items=n) == INVALID and "n_items" in _err()
    assert _rows(V=0, ld=4) == INVALID and "V 0" in _err()
    assert _rows(mode=3) == INVALID and "mode" in _err()
    for top in (-1, 21):
        assert _rows(top_n=top) == INVALID and "top_n" in _err()
    for rows in (0, 81):
        assert _rows(n_items=3, rows=rows) == INVALID and "item 0: rows" in _err()
    assert _rows(ld=7) == INVALID and "item 0: ld" in _err()
    for null in ("logits", "tokens", "logprob"):
        assert _rows(**{null: None}) == INVALID and "item 0: null" in _err()
    for null in ("top_ids", "top_logprobs"):
        assert _rows(**{null: None}) == INVALID and "item 0: top_n 2" in _err()
    # the item is named: the second of two
    buf = (C.c_float * 64)()
    good = dict(logits=C.addressof(buf), ld=8, rows=1, tokens=C.addressof(buf), logprob=C.addressof(buf), rank=None, top_ids=None,
                top_logprobs=None)
    items = (_lib.SdScoreItem * 2)(_lib.SdScoreItem(**good), _lib.SdScoreItem(**dict(good, ld=7)))
    assert _lib.lib.sd_score_rows(items, 2, 8, 0, 0, None) == INVALID and "item 1: ld" in _err()


def _seq(ses=0x1000, n=8, first=1, top_n=2, slab_rows=4, **over):
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    fields = dict(logprob=p, rank=p, top_ids=p, top_logprobs=p)
    args = dict(tokens=p, slab=p, out=True)
    for k, v in over.items():
        (args if k in args else fields)[k] = v
    out = _lib.SdScoreOut(**fields)
    return _lib.lib.sd_score_sequence(ses, args["tokens"], n, first, top_n, args["slab"], 8, slab_rows,
                                      C.byref(out) if args["out"] else None, None)


def test_score_sequence_refusals_that_do_not_read_the_session():
    """The session pointer is a placeholder: each of these is refused before the session is read (and so before any launch)."""
    assert _seq(ses=None) == INVALID and "null" in _err()
    for null in ("tokens", "slab", "out", "logprob"):
        assert _seq(**{null: None}) == INVALID and "null" in _err(), null
    for null in ("top_ids", "top_logprobs"):
        assert _seq(**{null: None}) == INVALID and "top_n 2" in _err(), null
    for top in (-1, 21):
        assert _seq(top_n=top) == INVALID and "top_n" in _err()
    for n in (1, 0, -3):
        assert _seq(n=n) == INVALID and "n %d" % n in _err()
    for first in (0, 8, -1):
        assert _seq(first=first) == INVALID and "first" in _err()
    for rows in (0, -1):
        assert _seq(slab_rows=rows) == INVALID and "slab_rows" in _err()


# ------------------------------------------------------------------------------------------- the definition in torch
def _same(got, want):
    return (math.isnan(got) and math.isnan(want)) or SR.within_bar(got, want)


@pytest.mark.parametrize("dt", [0, 1, 2], ids=["fp32", "bf16_round", "f16_round"])
@pytest.mark.parametrize("V", [7, 257, 8192])
def test_score_rows_torch_against_the_numpy_truth(V, dt):
    """Every row kind at every top_n in {0, 1, 5, 20}: ids and ranks exactly, values within logprob_rows.BAR."""
    for top_n in (0, 1, 5, 20):
        cases = [(kind, x, tr, t) for kind, x, tr in SR.pool(V, dt) for t in SR.tokens(kind, x, tr, top_n)]
        logits = torch.stack([x for _, x, _, _ in cases])
        toks = torch.tensor([t for *_, t in cases], dtype=torch.int32)
        lp, rank, ids, tlp = quality.score_rows_torch(logits, toks, top_n, dt)
        assert lp.dtype == tlp.dtype == torch.float32 and rank.dtype == ids.dtype == torch.int32
        assert tuple(lp.shape) == tuple(rank.shape) == (len(cases),) and tuple(ids.shape) == tuple(tlp.shape) == (len(cases), top_n)
        for r, (kind, x, tr, t) in enumerate(cases):
            what = (kind, V, dt, top_n, t)
            assert int(rank[r]) == tr.rank[t], what
            assert _same(float(lp[r]), float(tr.logp[t])), what
            want_ids, want_lp = tr.top(top_n)
            assert ids[r].tolist() == want_ids, what
            assert all(_same(float(g), w) for g, w in zip(tlp[r], want_lp)), what
            for j, i in enumerate(want_ids):
                if i == t:                                        # the same float where the token is listed
                    assert float(tlp[r, j]) == float(lp[r]) or math.isnan(float(lp[r])), what
    kinds = {k for k, *_ in SR.pool(V, dt)}
    assert kinds == set(SR.KINDS)


def test_rows_are_what_they_are_named_for():
    V = 257
    assert len(set(SR.row("ties", 1, V).tolist())) == 7
    z = SR.row("signed_zero", 1, V)
    signs = torch.signbit(z[z == 0])
    assert bool(signs.any()) and not bool(signs.all()) and int((z > 0).sum()) == 3
    tr = SR.Truth(z, 0)
    zeros = [i for i in tr.order[3:]]
    assert zeros == sorted(zeros)                                 # -0.0 == +0.0: the zeros follow the positives in id order
    assert int(SR.row("ascending", 1, V).argmax()) == V - 1 and int(SR.row("descending", 1, V).argmax()) == 0
    assert sorted(SR.Truth(SR.row("ends", 1, V), 0).order[:6]) == [0, 1, 2, V - 3, V - 2, V - 1]
    ff = SR.Truth(SR.row("few_finite", 1, V), 0)
    assert int(torch.isfinite(SR.row("few_finite", 1, V)).sum()) == 3 and ff.order[3:] == sorted(ff.order[3:])
    assert ff.top(5)[1][3] == -math.inf
    # under bf16 rounding a Gaussian row has ties inside its first 21 places
    g = SR.as_dtype(SR.row("gauss", 140, 8192), 1).float()
    assert g.unique().numel() < g.numel()
    # the cut of the ties row falls inside a tie group at every top_n
    t = SR.row("ties", 147, V)
    tt = SR.Truth(t, 0)
    assert all(float(t[tt.order[k - 1]]) == float(t[tt.order[k]]) for k in (1, 5, 20))
    s = SR.stripes(1, 4096, lanes=2)
    hot = torch.nonzero(s >= 10.0)[:, 0]
    assert hot.numel() == 2 * 4 * 4 and float(s[s < 10.0].max()) < 10.0 and set(((hot // 4) % 256).tolist()) == {0, 1}


def test_score_rows_torch_void_rows_and_tokens_out_of_range():
    V, top_n = 257, 5
    rows = [SR.void_row(k, 3, V) for k in SR.VOID_KINDS] + [SR.row("gauss", 5, V)] * 3
    lp, rank, ids, tlp = quality.score_rows_torch(torch.stack(rows), torch.tensor([3, 4, 5, -1, V, 6]), top_n)
    for r in range(3):
        assert math.isnan(float(lp[r])) and int(rank[r]) == 0 and ids[r].tolist() == [-1] * top_n and bool(torch.isnan(tlp[r]).all())
    tr = SR.Truth(rows[3], 0)
    for r in (3, 4):                                              # out of range: NaN and 0, the top list is still there
        assert math.isnan(float(lp[r])) and int(rank[r]) == 0 and ids[r].tolist() == tr.top(top_n)[0]
    assert int(rank[5]) == tr.rank[6] and ids[5].tolist() == tr.top(top_n)[0]
    # V < top_n: the tail is -1 / NaN
    lp, rank, ids, tlp = quality.score_rows_torch(torch.tensor([[0.5, 2.0, 2.0]]), torch.tensor([2]), 5)
    assert ids[0].tolist() == [1, 2, 0, -1, -1] and int(rank[0]) == 2 and bool(torch.isnan(tlp[0, 3:]).all())
    assert float(tlp[0, 1]) == float(lp[0])


# ------------------------------------------------------------------------------------------- score_tokens
def _fake_model(**over):
    m = SpecDecModel.__new__(SpecDecModel)                        # (no handle: nothing native is behind it)
    m.cfg = m.config = types.SimpleNamespace(vocab_size=100, is_encoder_decoder=False)
    m.tp_group = None
    for k, v in over.items():
        setattr(m, k, v)
    return m


def test_score_tokens_refuses_before_a_model_is_touched():
    x = torch.arange(6, dtype=torch.int64)[None]
    for bad in (0, 6, -1, 7):
        with pytest.raises(ValueError, match="input_len"):
            quality.score_tokens(x, None, bad)
    for bad in (-1, 21):
        with pytest.raises(ValueError, match="top_n"):
            quality.score_tokens(x, None, 1, bad)
    with pytest.raises(ValueError, match="input_len"):
        quality.score_tokens(x[:, :1], None)                      # one token: nothing to score
    with pytest.raises(ValueError, match=r"\(1, S\)"):
        quality.score_tokens(x[0], None)
    with pytest.raises(IndexError, match="outside"):
        quality.score_tokens(x + 95, _fake_model(), 1)
    with pytest.raises(ValueError, match="is not available with a tensor-parallel target model"):
        quality.score_tokens(x, _fake_model(tp_group=object()), 1)
    enc = _fake_model()
    enc.cfg.is_encoder_decoder = True
    with pytest.raises(NotImplementedError, match="encoder-decoder"):
        quality.score_tokens(x, enc, 1)
    assert quality.TokenScores._fields == ("logprobs", "ranks", "top_ids", "top_logprobs")
    assert np.isclose(float(quality.score_from_logprobs(torch.tensor([[-1.0, -2.0]]))), -1.5)   # (stays as it is)
