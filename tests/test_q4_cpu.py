"""4-bit weight records without a GPU: the size query and every refusal of the C entry points and of SpecDecModel(q4=...)."""
import ctypes as C

import pytest
import torch

from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.engine import SpecDecModel
from test_gemm_routes_cpu import _model_handle

lib = _lib.lib
P = 0x1000                                                         # (aligned, never read: every call below is refused or host-only)


@pytest.mark.parametrize("N,K,want", [(16, 128, 1088), (5120, 13824, 320 * 108 * 1088), (16, 96, None), (24, 128, None), (0, 128, None)])
def test_q4_bytes(N, K, want):
    nb = C.c_size_t(7)
    rc = lib.sd_q4_bytes(N, K, C.byref(nb))
    assert (rc, nb.value) == ((_lib.SD_OK, want) if want else (_lib.SD_ERR_INVALID, 7))
    assert want or b"sd_q4_bytes" in lib.sd_last_error()
    assert want is None or want * 8 <= 4.5 * N * K


def test_entry_points_refuse():
    assert lib.sd_q4_bytes(16, 128, None) == _lib.SD_ERR_INVALID
    for N, K, args in ((16, 96, [P] * 5), (24, 128, [P] * 5)) + tuple((16, 128, [P] * i + [None] + [P] * (4 - i)) for i in range(5)):
        assert lib.sd_pack_weight_q4(*args, N, K, None) == _lib.SD_ERR_INVALID and b"sd_pack_weight_q4" in lib.sd_last_error()
    for N, K, args in ((16, 96, [P, P]), (24, 128, [P, P]), (16, 128, [None, P]), (16, 128, [P, None])):
        assert lib.sd_unpack_weight_q4(*args, N, K, None) == _lib.SD_ERR_INVALID and b"sd_unpack_weight_q4" in lib.sd_last_error()
    assert lib.sd_session_q4_launches(None) == 0


def test_model_set_q4_refusals():
    h, keep = _model_handle(("llama", 1024, 2816, 8, 8, 128, 4096, None))
    Q, D = _lib.SD_W12_QKV, _lib.SD_W12_DOWN
    assert lib.sd_model_set_q4(None, Q, 1, P) == _lib.SD_ERR_INVALID
    assert lib.sd_model_set_q4(h, 3, 1, P) == _lib.SD_ERR_INVALID and lib.sd_model_set_q4(h, Q, 2, P) == _lib.SD_ERR_INVALID
    assert lib.sd_model_set_q4(h, Q, 1, P + 64) == _lib.SD_ERR_INVALID and b"aligned" in lib.sd_last_error()
    # one kind of records per matrix, either way round; NULL unregisters
    assert lib.sd_model_set_q4(h, Q, 1, P) == _lib.SD_OK
    assert lib.sd_model_set_w12(h, Q, 1, P, P) == _lib.SD_ERR_INVALID and b"4-bit" in lib.sd_last_error()
    assert lib.sd_model_set_w12(h, D, 0, P, P) == _lib.SD_OK
    assert lib.sd_model_set_q4(h, D, 0, P) == _lib.SD_ERR_INVALID and b"12-bit" in lib.sd_last_error()
    assert lib.sd_model_set_q4(h, Q, 1, None) == _lib.SD_OK and lib.sd_model_set_w12(h, Q, 1, P, P) == _lib.SD_OK
    lib.sd_model_destroy(h)


def test_model_set_q4_refuses_fp16():
    c = _lib.SdModelConfig(arch=0, dtype=_lib.SD_F16, vocab=4096, hidden=1024, inter=2816, n_layers=2, n_heads=8, n_kv_heads=8,
                           head_dim=128, max_pos=2048, opt_pre_ln=1, opt_proj_dim=1024, norm_eps=1e-5, logits_bf16_round=1, fused_layout=1)
    arrays = [(C.c_void_p * 2)(P, P) for _ in range(12)]
    w = _lib.SdModelWeights()
    w.embed = w.lm_head = w.final_norm_w = w.pos_embed = w.rope_cos = w.rope_sin = P
    (w.wqkv, w.bqkv, w.wo, w.bo, w.w_gate_up, w.b_fc1, w.w_down, w.b_fc2, w.norm1_w, w.norm1_b, w.norm2_w,
     w.norm2_b) = (C.cast(a, C.POINTER(C.c_void_p)) for a in arrays)
    h = C.c_void_p()
    assert lib.sd_model_create(C.byref(c), C.byref(w), C.byref(h)) == _lib.SD_OK
    assert lib.sd_model_set_q4(h, _lib.SD_W12_QKV, 1, P) == _lib.SD_ERR_INVALID and b"bf16" in lib.sd_last_error()
    lib.sd_model_destroy(h)


@pytest.mark.parametrize("dtype,inter", [(torch.float16, 2816), (torch.float32, 2816), (torch.bfloat16, 2784)])
def test_model_refuses_before_allocating(dtype, inter):
    """fp16 / fp32 weights and a K that is no multiple of 128: ValueError before a tensor is asked for (or a GPU looked for)"""
    cfg = ModelConfig(arch="llama", vocab_size=4096, hidden_size=1024, intermediate_size=inter, num_hidden_layers=2,
                      num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=512, rms_norm_eps=1e-5)
    asked = []
    with pytest.raises(ValueError, match="q4"):
        SpecDecModel(cfg, asked.append, dtype=dtype, q4=True)
    assert asked == []
