"""Host side of the grouped-query decode attention (no GPU): the new symbols, sd_grouped_attn_plan and the route
sd_forward_route - plan_forward itself - answers under SD_ATTN_GROUPED = 0, 1 (default) and 2."""
import ctypes as C
import os
import re

import pytest
import torch

from llmspeculativesampling_amd import _lib, engine
from llmspeculativesampling_amd.config import ModelConfig
from sd_env import tunables

lib = _lib.lib
# the 70b layer shape (64 query heads over 8 KV heads) and its TP = 8 shard's attention (8 over 1), and an MHA model
GQA70 = dict(arch="llama", vocab_size=512, hidden_size=8192, intermediate_size=1024, num_hidden_layers=1,
             num_attention_heads=64, num_key_value_heads=8, max_position_embeddings=200000, rms_norm_eps=1e-5)
MHA = dict(GQA70, hidden_size=4096, num_attention_heads=32, num_key_value_heads=32)


def _plan(D, Hq, Hkv, s_max, groups, cus=256):
    ns, ck, lds = C.c_int(), C.c_int(), C.c_long()
    _lib.check(lib.sd_grouped_attn_plan(D, Hq, Hkv, s_max, groups, cus, C.byref(ns), C.byref(ck), C.byref(lds)), "sd_grouped_attn_plan")
    return ns.value, ck.value, lds.value


def _route(kw, n, pos0, env):
    c = engine.c_model_config(ModelConfig(**kw), torch.bfloat16)
    p = _lib.SdPassDesc(n_rows=n, pos0=pos0, n_logit_rows=n, kv_fp8=0, tp=0, max_rows=16, cus=256)
    out = _lib.SdForwardRouteInfo()
    with tunables(env):
        _lib.check(lib.sd_forward_route(C.byref(c), C.byref(p), C.byref(out)), "sd_forward_route")
    return out.attn, out.nsplit, out.chunk_keys, out.attn_lds


def test_new_symbols_are_exported_and_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "specdec.h")).read()
    names = {s[0] for s in _lib.SYMBOLS}
    for sym in ("sd_grouped_attn_plan", "sd_session_grouped_attn_launches"):
        assert sym in names and callable(getattr(lib, sym)) and re.search(rf"\b{sym}\(", header), sym
    assert _lib.SD_ATTN_GROUPED == 3 and "SD_ATTN_GROUPED = 3" in header and lib.sd_version() == 7
    assert lib.sd_session_grouped_attn_launches(None) == 0 and callable(engine.Session.grouped_attn_launches)


@pytest.mark.parametrize("D,Hq,Hkv", [(128, 64, 8), (128, 8, 1), (64, 4, 2)])
def test_plan_fills_the_device_within_the_partial_buffer_and_a_fixed_lds(D, Hq, Hkv):
    for groups in (1, 2, 16, 32):
        for s_max in (1, 64, 257, 5909, 1_000_000):
            ns, ck, lds = _plan(D, Hq, Hkv, s_max, groups)
            assert 1 <= ns and ns * groups <= 64 and ck % 64 == 0 and (ns - 1) * ck < s_max <= ns * ck, (groups, s_max, ns, ck)
            assert (ns - 1) * Hkv * groups < 256 and (ns == 1 or ck >= 256)   # no split past the CU count, none under 256 keys
            assert lds == _plan(D, Hq, Hkv, 64, 1)[2] <= 160 * 1024
    none = [None] * 3
    for bad in ((32, Hq, Hkv, 64, 1, 0), (D, Hkv, Hkv, 64, 1, 0), (D, 16 * Hkv, Hkv, 64, 1, 0), (D, Hq, Hkv, 0, 1, 0),
                (D, Hq, Hkv, 64, 0, 0), (D, Hq, Hkv, 64, 33, 0), (D, Hq, Hkv, 64, 1, -1)):
        assert lib.sd_grouped_attn_plan(*bad, *none) == _lib.SD_ERR_INVALID and b"sd_grouped_attn_plan" in lib.sd_last_error(), bad


def test_forward_route_takes_the_grouped_kernel_only_where_the_tunable_says():
    before = _route(GQA70, 5, 300, {"SD_ATTN_GROUPED": None})
    assert before[0] != _lib.SD_ATTN_GROUPED and before == _route(GQA70, 5, 300, {"SD_ATTN_GROUPED": 0})
    got = _route(GQA70, 5, 300, {"SD_ATTN_GROUPED": 2})
    assert got == (_lib.SD_ATTN_GROUPED,) + _plan(128, 64, 8, 305, 1)
    for env in (None, 0, 2):                                       # an MHA model: no setting moves it
        assert _route(MHA, 5, 300, {"SD_ATTN_GROUPED": env}) == _route(MHA, 5, 300, {})
    # past attn_kernel's LDS (9 rows = 2 groups): the default takes the grouped kernel, = 0 keeps the plan launch_attn refuses
    s_max, lds = 150000, C.c_long()
    assert lib.sd_attn_split(128, s_max, 2, None, None, None, C.byref(lds)) == _lib.SD_OK and lds.value > 160 * 1024 - 512
    assert _route(GQA70, 9, s_max - 9, {})[0] == _lib.SD_ATTN_GROUPED
    off = _route(GQA70, 9, s_max - 9, {"SD_ATTN_GROUPED": 0})
    assert off[0] == _lib.SD_ATTN_KERNEL and off[3] == lds.value
