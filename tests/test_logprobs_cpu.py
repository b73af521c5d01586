"""Per-token target log-probabilities from the native decode loops: what needs no GPU - the ABI (one symbol, two structs; the loops
take the block as member logprobs of sd_loop_opts), the keyword on the four free functions, the queue function's parameter list, the refusals that come before a
model is touched, the refusals of sd_token_logprobs (all before a launch), the helper's float64 truth and the score."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import abi_header
import logprob_rows as LR
import llmspeculativesampling_amd.sampling as S
from llmspeculativesampling_amd import _lib, quality

NEW = ("sd_token_logprobs",)
REMOVED = ("sd_spec_generate_logprobs", "sd_spec_batch_generate_logprobs", "sd_spec_queue_generate_logprobs",
           "sd_ar_batch_generate_logprobs")                                     # ABI 7: member logprobs of sd_loop_opts
SYM = {name: (res, args) for name, res, args in _lib.SYMBOLS}
PROTOS, STRUCTS = abi_header.parse()


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
    for name, cls, size in (("sd_logprob_item", _lib.SdLogprobItem, 48), ("sd_logprob_block", _lib.SdLogprobBlock, 24)):
        assert _lib.C_STRUCTS[name] is cls
        assert C.sizeof(cls) == size == STRUCTS[name][1]
        assert [(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_] == STRUCTS[name][0]
    # what the existing entries must keep
    assert C.sizeof(_lib.SdAcceptResult) == 208 == STRUCTS["sd_accept_result"][1]
    assert [_lib.lib.sd_ar_block_bytes(n) for n in (0, 1, 2, 3, 16, 17)] == [0, 16, 16, 32, 128, 0]


@pytest.mark.parametrize("name", ["speculative_sampling", "speculative_sampling_batch", "autoregressive_sampling",
                                  "autoregressive_sampling_batch"])
def test_keyword_is_keyword_only_and_off_by_default(name):
    p = inspect.signature(getattr(S, name)).parameters["logprobs"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_queue_logprobs_has_queue_shared_s_parameters():
    assert "speculative_sampling_queue_logprobs" in S.__all__
    a = inspect.signature(S.speculative_sampling_queue_shared).parameters
    b = inspect.signature(S.speculative_sampling_queue_logprobs).parameters
    assert list(a) == list(b)
    assert all(a[k].default == b[k].default and a[k].kind == b[k].kind for k in a)
    assert b["shared_prefix"].default == 0
    for f in (S.speculative_sampling_queue, S.speculative_sampling_queue_shared):     # pinned by their own tests: no new keyword
        assert "logprobs" not in inspect.signature(f).parameters


def test_interpreter_paths_refuse_before_a_model_is_touched():
    x = torch.zeros((1, 3), dtype=torch.int64)
    for kw in (dict(), dict(rng="host"), dict(rng="device", verbose=True)):
        with pytest.raises(ValueError, match='rng="device"'):
            S.speculative_sampling(x, None, None, 2, None, 4, logprobs=True, **kw)
    for kw in (dict(rng="device", _native=False), dict(), dict(rng="host")):
        with pytest.raises(ValueError, match='rng="device"'):
            S.autoregressive_sampling(x, None, 4, 2, logprobs=True, **kw)


def _one(n_items=1, V=8, mode=0, **over):
    buf, tok, out = (C.c_float * 64)(), (C.c_int32 * 17)(), (C.c_float * 17)()
    fields = dict(logits=C.addressof(buf), ld=V, rows=1, tokens=C.addressof(tok), res=None, out=C.addressof(out))
    fields.update(over)
    items = (_lib.SdLogprobItem * 16)(*[_lib.SdLogprobItem(**fields) for _ in range(16)])
    return _lib.lib.sd_token_logprobs(items, n_items, V, mode, None)


def test_token_logprobs_refusals_come_before_any_launch():
    """Host memory throughout: a call that got as far as a launch would fail another way."""
    assert _lib.lib.sd_token_logprobs(None, 1, 8, 0, None) == _lib.SD_ERR_INVALID
    for n in (0, 17, -1):
        assert _one(n_items=n) == _lib.SD_ERR_INVALID
        assert "n_items" in _lib.lib.sd_last_error().decode()
    for rows in (0, 18):
        assert _one(rows=rows) == _lib.SD_ERR_INVALID
        assert "rows" in _lib.lib.sd_last_error().decode()
    assert _one(ld=7) == _lib.SD_ERR_INVALID and "ld" in _lib.lib.sd_last_error().decode()
    for null in ("logits", "tokens", "out"):
        assert _one(**{null: None}) == _lib.SD_ERR_INVALID
    assert _one(V=0, ld=4) == _lib.SD_ERR_INVALID
    assert _one(mode=3) == _lib.SD_ERR_INVALID


def test_helper_truth_against_a_direct_float64_computation():
    V = 257
    for dt in (0, 1, 2):
        for kind, x, tok, want in LR.pool(V, dt):
            xs = x.to(LR.as_dtype(x, dt).dtype).double().numpy()
            assert LR.truth(x, tok, dt) == want
            if np.isinf(xs[tok]):
                assert want == -math.inf, kind
                continue
            m = xs[np.isfinite(xs)].max()
            direct = xs[tok] - (m + math.log(np.exp(xs - m).sum()))
            assert abs(direct - want) <= 1e-12 * max(1.0, abs(want)), (kind, tok, dt)
            if kind == "equal":
                assert abs(want + math.log(V)) <= 1e-12
    kinds = {k for k, *_ in LR.pool(V, 0)}
    assert kinds == set(LR.KINDS)
    # the rows are what they are named for
    assert float(LR.row("max_last", 1, V).argmax()) == V - 1
    assert set(LR.row("pm80", 1, V).tolist()) == {80.0, -80.0}
    sp = LR.row("spike", 1, V).sort().values
    assert float(sp[-1] - sp[-2]) >= 59.9
    assert int(torch.isinf(LR.row("neg_inf", 1, V)).sum()) >= 2
    assert LR.within_bar(-1.0 - LR.BAR, -1.0) and not LR.within_bar(-1.0 - 2.5 * LR.BAR, -1.0)
    assert LR.within_bar(-100.0 - 99 * LR.BAR, -100.0) and LR.within_bar(-math.inf, -math.inf) and not LR.within_bar(-1e30, -math.inf)


def test_score_from_logprobs_is_the_mean():
    lp = torch.tensor([[-1.0, -2.5, -0.25, -4.25]])
    assert float(quality.score_from_logprobs(lp)) == -2.0
    assert float(quality.score_from_logprobs(lp.double()[:, :1])) == -1.0
