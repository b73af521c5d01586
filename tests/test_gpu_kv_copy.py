"""The session-to-session KV copy alone (`pytest -m gpu`): sd_session_copy_kv through ctypes on arenas of random bytes -
every byte of every destination is either the source's (inside the range) or the sentinel it held (outside) - its refusals,
which launch nothing, and a sequence continued on copied rows against the session that computed them."""
import numpy as np
import pytest
import torch

from test_gpu_native_parity import _st
from test_gpu_parity import MID_CFGS
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu

SRC_SEQ, DST_SEQ, SENTINEL = 48, 80, 0xA5                          # arenas of different sizes: the plane strides differ
CASES = [  # (id, config, dtype, kv_dtype)
    ("fp32_tiny", "tiny-llama-target", torch.float32, None),
    ("bf16_d64_gqa", "llama_d64_gqa", torch.bfloat16, None),
    ("bf16_d128", "llama_d128", torch.bfloat16, None),
    ("fp8_d64_gqa", "llama_d64_gqa", torch.bfloat16, "fp8"),
]
RANGES = [(0, 1), (0, 17), (3, 40), (5, 5), (0, 48)]


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine
    return types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine)


def _model(hip, name, dtype, seed=31):
    cfg = ModelConfig(**MID_CFGS[name]) if name in MID_CFGS else load_config(name)
    return cfg, hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, seed, dtype=dtype), dtype=dtype)


def _bytes(ses):
    """The arena as [layers][2][H_kv][max_seq][row bytes] uint8 (random bytes in an fp32 arena include NaNs: compare bytes)."""
    return ses.kv.view(torch.uint8)


def _items(hip, triples):
    items = (hip.L.SdKvCopyItem * len(triples))()
    for it, (dst, lo, hi) in zip(items, triples):
        it.dst, it.lo, it.hi = dst.handle, lo, hi
    return items


def _arenas(m, kv_dtype, n_dst=3):
    gen = torch.Generator(device="cuda").manual_seed(5)
    src = m.new_session(SRC_SEQ, kv_dtype=kv_dtype)
    _bytes(src).copy_(torch.randint(0, 256, _bytes(src).shape, generator=gen, dtype=torch.uint8, device="cuda"))
    dsts = [m.new_session(DST_SEQ, kv_dtype=kv_dtype) for _ in range(n_dst)]
    for d in dsts:
        _bytes(d).fill_(SENTINEL)
    return src, dsts


def _want(src, dst, lo, hi):
    want = torch.full_like(_bytes(dst), SENTINEL)
    want[:, :, :, lo:hi] = _bytes(src)[:, :, :, lo:hi]
    return want


@pytest.mark.parametrize("name,cfg_name,dtype,kv_dtype", CASES, ids=[c[0] for c in CASES])
def test_copy_kv_moves_the_range_of_every_plane_and_nothing_else(hip, name, cfg_name, dtype, kv_dtype):
    cfg, m = _model(hip, cfg_name, dtype)
    src, dsts = _arenas(m, kv_dtype)
    assert src.max_seq == SRC_SEQ and dsts[0].max_seq == DST_SEQ and src.kv_fp8 == (kv_dtype == "fp8")
    keep = _bytes(src).clone()
    for lo, hi in RANGES:
        d = dsts[0]
        _bytes(d).fill_(SENTINEL)
        hip.L.check(hip.lib.sd_session_copy_kv(src.handle, _items(hip, [(d, lo, hi)]), 1, _st()), "sd_session_copy_kv")
        torch.cuda.synchronize()
        assert torch.equal(_bytes(d), _want(src, d, lo, hi)), (lo, hi)
        assert torch.equal(_bytes(src), keep), (lo, hi)
    # one call, three destinations, each with a range of its own (the grid is sized by the longest)
    for d in dsts:
        _bytes(d).fill_(SENTINEL)
    triples = [(dsts[0], 0, 48), (dsts[1], 7, 8), (dsts[2], 3, 40)]
    hip.L.check(hip.lib.sd_session_copy_kv(src.handle, _items(hip, triples), 3, _st()), "sd_session_copy_kv")
    torch.cuda.synchronize()
    for d, lo, hi in triples:
        assert torch.equal(_bytes(d), _want(src, d, lo, hi)), (lo, hi)
    assert torch.equal(_bytes(src), keep)
    # ... and with an empty item among them
    for d in dsts:
        _bytes(d).fill_(SENTINEL)
    triples = [(dsts[0], 5, 5), (dsts[1], 0, 17), (dsts[2], 47, 48)]
    hip.L.check(hip.lib.sd_session_copy_kv(src.handle, _items(hip, triples), 3, _st()), "sd_session_copy_kv")
    torch.cuda.synchronize()
    for d, lo, hi in triples:
        assert torch.equal(_bytes(d), _want(src, d, lo, hi)), (lo, hi)
    # the Python wrapper: the same bytes, and no cache length moves
    d = dsts[0]
    _bytes(d).fill_(SENTINEL)
    d.copy_kv_from(src, 3, 40)
    torch.cuda.synchronize()
    assert torch.equal(_bytes(d), _want(src, d, 3, 40)) and d.cache_len == 0 and src.cache_len == 0


def test_copy_kv_refusals_launch_nothing(hip):
    cfg, m = _model(hip, "llama_d64_gqa", torch.bfloat16)
    _, other = _model(hip, "llama_d64_gqa", torch.bfloat16)         # the same shapes, another model
    src, (d0, d1) = _arenas(m, None, n_dst=2)
    big = m.new_session(DST_SEQ)                                  # a source LARGER than a destination: hi past the destination's end
    small = m.new_session(SRC_SEQ)
    _bytes(small).fill_(SENTINEL)
    f8 = m.new_session(DST_SEQ, kv_dtype="fp8")
    _bytes(f8).fill_(SENTINEL)
    foreign = other.new_session(DST_SEQ)
    _bytes(foreign).fill_(SENTINEL)
    f = hip.lib.sd_session_copy_kv
    null_dst = (hip.L.SdKvCopyItem * 1)()
    null_dst[0].lo, null_dst[0].hi = 0, 4
    cases = [
        ("null", lambda: f(None, _items(hip, [(d0, 0, 4)]), 1, _st())),
        ("null", lambda: f(src.handle, None, 1, _st())),
        ("null", lambda: f(src.handle, null_dst, 1, _st())),
        ("n_items 0 outside", lambda: f(src.handle, _items(hip, [(d0, 0, 4)]), 0, _st())),
        ("n_items 17 outside", lambda: f(src.handle, _items(hip, [(d0, 0, 4)] * 17), 17, _st())),
        ("another model", lambda: f(src.handle, _items(hip, [(foreign, 0, 4)]), 1, _st())),
        ("one session", lambda: f(src.handle, _items(hip, [(src, 0, 4)]), 1, _st())),
        ("fp8", lambda: f(src.handle, _items(hip, [(f8, 0, 4)]), 1, _st())),
        ("fp8", lambda: f(f8.handle, _items(hip, [(d0, 0, 4)]), 1, _st())),
        ("positions", lambda: f(src.handle, _items(hip, [(d0, -1, 4)]), 1, _st())),
        ("positions", lambda: f(src.handle, _items(hip, [(d0, 5, 4)]), 1, _st())),
        ("positions", lambda: f(src.handle, _items(hip, [(d0, 0, SRC_SEQ + 1)]), 1, _st())),       # past the source's end
        ("positions", lambda: f(big.handle, _items(hip, [(small, 0, SRC_SEQ + 1)]), 1, _st())),    # past the destination's end
        # a good item ahead of a bad one: the call is refused as a whole, before any launch
        ("item 1", lambda: f(src.handle, _items(hip, [(d0, 0, 4), (d1, 0, SRC_SEQ + 1)]), 2, _st())),
    ]
    keep = _bytes(src).clone()
    for word, call in cases:
        assert call() == hip.L.SD_ERR_INVALID, word
        msg = hip.lib.sd_last_error().decode()
        assert msg.startswith("sd_session_copy_kv:") and word in msg, (word, msg)
    torch.cuda.synchronize()
    for ses in (d0, d1, small, f8, foreign):
        assert bool((_bytes(ses) == SENTINEL).all())
    assert torch.equal(_bytes(src), keep)
    # the wrapper answers for the fp8 scale tables
    a, b = m.new_session(SRC_SEQ, kv_dtype="fp8"), m.new_session(DST_SEQ, kv_dtype="fp8")
    b.copy_kv_from(a, 0, 4)
    b.kv_scale[0, 0, 0] = 2.0
    with pytest.raises(ValueError, match="scale tables"):
        b.copy_kv_from(a, 0, 4)
    with pytest.raises(ValueError, match="sd_session_copy_kv"):
        d0.copy_kv_from(src, 0, SRC_SEQ + 1)


CONT = [("fp32_llama", "tiny-llama-target", torch.float32), ("fp32_opt", "tiny-opt-pre", torch.float32),
        ("bf16_d64_gqa", "llama_d64_gqa", torch.bfloat16)]


@pytest.mark.parametrize("name,cfg_name,dtype", CONT, ids=[c[0] for c in CONT])
def test_a_sequence_continues_on_copied_rows(hip, name, cfg_name, dtype):
    """Session A forwards 23 prompt rows, then rows 23..30.  Session B (a larger arena) copies positions [0, 23) from A and
    forwards rows 23..30 at pos0 = 23.  fp32: the logits and the new K / V rows are bit-equal (OPT's learned positions make a
    wrong pos0 visible).  bf16: held to the method and bar of test_batch_forward_verify_rows_plus_prompt_rows_without_logits
    (0.03 of the largest logit, K / V within 0.05)."""
    cfg, m = _model(hip, cfg_name, dtype)
    seq = torch.from_numpy(np.random.default_rng(9).integers(3, cfg.vocab_size, size=(31,)).astype(np.int32)).cuda()
    A, B = m.new_session(SRC_SEQ), m.new_session(DST_SEQ)
    A.forward(seq[:23], 0)
    want = A.forward(seq[23:31], 8).clone()
    B.copy_kv_from(A, 0, 23)
    assert B.cache_len == 0                                       # the lengths live with the caller
    got = B.forward(seq[23:31], 8, pos0=23).clone()
    assert A.cache_len == B.cache_len == 31 and got.shape == want.shape == (8, cfg.vocab_size)
    assert torch.equal(_bytes(A)[:, :, :, :23], _bytes(B)[:, :, :, :23])
    diff = float((got - want).abs().max())
    print(name, "max |logit difference|", diff, "of", float(want.abs().max()))
    if dtype == torch.float32:
        assert torch.equal(got, want)
    else:
        assert diff <= 0.03 * float(want.abs().max())
    for (ka, va), (kb, vb) in zip(A.past_key_values(), B.past_key_values()):
        for x, y in ((ka, kb), (va, vb)):
            x, y = x[:, :, 23:31], y[:, :, 23:31]
            assert torch.equal(x, y) if dtype == torch.float32 else float((x.float() - y.float()).abs().max()) < 0.05
