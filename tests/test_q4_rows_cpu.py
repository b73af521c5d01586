"""The balanced record GEMM without a GPU: every refusal of sd_gemm_q4_rows and sd_model_set_q4_rows, and the values
SpecDecModel(q4=...) takes - all of it decided on the host before anything is launched or allocated."""
import ctypes as C

import pytest
import torch

from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.engine import SpecDecModel
from test_gemm_routes_cpu import _model_handle
from test_gpu_w12 import CFG

lib = _lib.lib
P = 0x1000                                                         # (aligned, never read: every call below is refused)
OK = dict(records=P, x=P, M=40, N=1024, K=2816, slabs=0, part=P, floats=1 << 30)


@pytest.mark.parametrize("change,word", [
    (dict(N=1032), b"N % 16"), (dict(N=0), b"N % 16"), (dict(K=2784), b"K % 128"), (dict(K=0), b"K % 128"),
    (dict(M=0), b"M out of range"), (dict(M=81), b"M out of range"),
    (dict(records=None), b"null"), (dict(x=None), b"null"), (dict(part=None), b"null"),
    (dict(records=P + 64), b"128-byte aligned"),
    (dict(floats=4 * 48 * 1024 - 1, slabs=4), b"part_floats too small"),
    (dict(slabs=-1), b"slabs"), (dict(slabs=3), b"no record plan"), (dict(slabs=2, K=128), b"no record plan"),
])
def test_gemm_q4_rows_refuses(change, word):
    a = dict(OK, **change)
    splits = C.c_int(-7)
    rc = lib.sd_gemm_q4_rows(a["records"], a["x"], a["M"], a["N"], a["K"], a["slabs"], a["part"], a["floats"], None,
                             C.byref(splits), None)
    assert rc == _lib.SD_ERR_INVALID and splits.value == -7
    err = lib.sd_last_error()
    assert b"sd_gemm_q4_rows" in err and word in err


def test_model_set_q4_rows_refusals():
    assert lib.sd_model_set_q4_rows(None, 1) == _lib.SD_ERR_INVALID and b"sd_model_set_q4_rows" in lib.sd_last_error()
    h, keep = _model_handle(("llama", 1024, 2816, 8, 8, 128, 4096, None))
    assert lib.sd_model_set_q4_rows(h, 1) == _lib.SD_OK and lib.sd_model_set_q4_rows(h, 0) == _lib.SD_OK
    lib.sd_model_destroy(h)
    c = _lib.SdModelConfig(arch=0, dtype=_lib.SD_F16, vocab=4096, hidden=1024, inter=2816, n_layers=2, n_heads=8, n_kv_heads=8,
                           head_dim=128, max_pos=2048, opt_pre_ln=1, opt_proj_dim=1024, norm_eps=1e-5, logits_bf16_round=1, fused_layout=1)
    arrays = [(C.c_void_p * 2)(P, P) for _ in range(12)]
    w = _lib.SdModelWeights()
    w.embed = w.lm_head = w.final_norm_w = w.pos_embed = w.rope_cos = w.rope_sin = P
    (w.wqkv, w.bqkv, w.wo, w.bo, w.w_gate_up, w.b_fc1, w.w_down, w.b_fc2, w.norm1_w, w.norm1_b, w.norm2_w,
     w.norm2_b) = (C.cast(a, C.POINTER(C.c_void_p)) for a in arrays)
    h = C.c_void_p()
    assert lib.sd_model_create(C.byref(c), C.byref(w), C.byref(h)) == _lib.SD_OK
    assert lib.sd_model_set_q4_rows(h, 1) == _lib.SD_ERR_INVALID and b"bf16" in lib.sd_last_error()
    lib.sd_model_destroy(h)


@pytest.mark.parametrize("q4,ok", [("rows", True), (("rows", lambda n: None), True), ("row", False), ("Rows", False),
                                   (("rows", None), False), (("rows",), False), (("cols", len), False)])
def test_q4_values(monkeypatch, q4, ok):
    """a good value gets past validation to the GPU check (RuntimeError here: no device), a bad one is a ValueError; either
    way before a tensor is asked for.  SD_Q4=rows is the string."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    asked = []
    with pytest.raises(RuntimeError if ok else ValueError, match="needs a GPU" if ok else "q4"):
        SpecDecModel(CFG, asked.append, dtype=torch.bfloat16, q4=q4)
    if q4 == "rows":
        monkeypatch.setenv("SD_Q4", "rows")
        with pytest.raises(ValueError, match="q4"):           # (the environment's value is read: fp16 cannot hold records)
            SpecDecModel(CFG, asked.append, dtype=torch.float16)
    assert asked == []
