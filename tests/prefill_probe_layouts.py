"""Planted-key layouts for the matrix-core prefill attention (attn_prefill_kernel<T, D, KV8>, prefill_attn.h): helper of
test_prefill_probe_cpu.py and test_gpu_prefill_attention_variants.py; needs no GPU.

attn_probe.prefill_layouts() - one call of 81, 200 and 256 rows at pos0 0 and 37 - plus, for (n, pos0) in {(81, 37), (200, 0),
(256, 37)} (S = pos0 + n keys), the edges of the kernel's own tiling:

  * the marker at keys 63, 64, 127 and 128 (where the call has them), probed from the last row: the last and the first key
    of a 64-key V chunk (PA_VCH), which are also edges of the 16-key score tiles and of the 32-key P.V steps;
  * for r in {n - 64, n - 17, n - 16, n - 1} - the first row of the 64-row logit tail, and the last / first row of a 16-row
    group inside it - the marker at pos0 + r probed from row r (`own`: the last key the row may see) and at pos0 + r + 1
    probed from row r (`forbidden`: a later row of the call, so it exists for r < n - 1 only; the stale slot behind the
    last row is in attn_probe.prefill_layouts()).

81 rows is the smallest contiguous call (more than SD_MAX_ROWS = 80 rows) and leaves a ragged last group of 1 row; 256 rows
at pos0 = 37 give the longest score rows, 293 keys.  Logits come out for the last 64 rows of a call, so every probed row lies
there."""
from typing import List

import numpy as np
import pytest
import torch

import attn_probe as P
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict

# The probe models of attn_probe at hidden 512.  A call of more than 64 rows needs gemm_bf16_mm for every GEMM of a layer, which
# takes k >= 512 and n a multiple of 128: at attn_probe's hidden 256 sd_model_max_rows is 64, Session.forward cuts an 81-row
# call into 64 + 17 rows, no pass is contiguous and attn_prefill_kernel is never reached.  Same construction otherwise
# (attn_probe.probe_state_dict works from the config): one layer, vocab 512, filler / marker / query tokens.
WIDE_MODELS = {
    "llama_d128_h512": dict(P.MODELS["llama_d128"], hidden_size=512, num_attention_heads=4, num_key_value_heads=4),
    "llama_gqa_d64_h512": dict(P.MODELS["llama_gqa_d64"], hidden_size=512, num_attention_heads=8, num_key_value_heads=2),
    "llama_d32_h512": dict(P.MODELS["llama_d32"], hidden_size=512, intermediate_size=512, num_attention_heads=16,
                           num_key_value_heads=16),                # head_dim 32: outside the kernel's gate
}


@pytest.fixture
def wide_models(monkeypatch):
    """WIDE_MODELS in attn_probe's registry for the length of one test (attn_probe's helpers and the runner of
    test_gpu_attention_edges take a model by name and look it up when they are constructed); the registry is as it was
    afterwards, so what other test files see in it does not depend on this module."""
    for name, kw in WIDE_MODELS.items():
        monkeypatch.setitem(P.MODELS, name, kw)

EDGE_CALLS = [(81, 37), (200, 0), (256, 37)]
V_CHUNK_EDGES = (63, 64, 127, 128)
TAIL = 64                                                          # logit rows per call


def edge_layouts() -> List[P.Layout]:
    out = []
    for n, pos0 in EDGE_CALLS:
        S = pos0 + n
        for key in V_CHUNK_EDGES:
            if key < S:
                out.append(P.Layout(S, n, key, n - 1, "chunk_edge"))
        for r in (n - 64, n - 17, n - 16, n - 1):
            out.append(P.Layout(S, n, pos0 + r, r, "own"))
            if r + 1 < n:
                out.append(P.Layout(S, n, pos0 + r + 1, r, "forbidden"))
    return out


def layouts() -> List[P.Layout]:
    return P.prefill_layouts() + edge_layouts()


# (model, dtype name, kv_quant) of the kernel's new instances: fp8 arena at D = 128, D = 64 with either arena - and of the
# restructured <T, 128, false> one: at attn_probe's hidden 256 no call reaches the kernel (above), so these two are what holds
# the 16-bit D = 128 instance to the planted keys
CASES = [("llama_d128_h512", "bf16", "fp8"), ("llama_d128_h512", "fp16", "fp8"), ("llama_gqa_d64_h512", "bf16", None),
         ("llama_gqa_d64_h512", "fp16", None), ("llama_gqa_d64_h512", "bf16", "fp8"), ("llama_gqa_d64_h512", "fp16", "fp8"),
         ("llama_d128_h512", "bf16", None), ("llama_d128_h512", "fp16", None)]
CASE_IDS = [f"{n}-{d}{'-fp8kv' if k else ''}" for n, d, k in CASES]


# ----------------------------------------------------------------------------- batched prefill, one scale tensor per stream
# (two layers: layer 1's K / V rows depend on layer 0's attention output, so a forward AFTER the prefill sees what the prefill
#  attention computed; random weights, every value a bf16 number)
TWO_LAYER = dict(WIDE_MODELS["llama_gqa_d64_h512"], num_hidden_layers=2, max_position_embeddings=128)
BATCH_ROWS = (40, 33, 90)


def stream_scales(i, cfg):
    """[L, k|v, Hkv]: streams 0 and 2 carry attn_probe's scales in every layer, stream 1 the same with K's and V's swapped."""
    k, v = (P.FP8_V_SCALE, P.FP8_K_SCALE) if i == 1 else (P.FP8_K_SCALE, P.FP8_V_SCALE)
    hkv = cfg.num_key_value_heads
    return torch.tensor([[[k[h % 2] for h in range(hkv)], [v[h % 2] for h in range(hkv)]]] * cfg.num_hidden_layers)


def fold_scales(cfg, sd, sc):
    """attn_probe.fp8_scaled_sd for every layer and for the scales given: the weights with which the oracle's scale-1 arena
    emulation computes what an arena with scales `sc` holds and yields (powers of two: exact)."""
    D, rep = cfg.head_dim, cfg.num_attention_heads // cfg.num_key_value_heads
    out = {k: v.clone() for k, v in sd.items()}
    for l in range(cfg.num_hidden_layers):
        p = f"model.layers.{l}.self_attn."
        for h in range(cfg.num_key_value_heads):
            ks, vs = float(sc[l, 0, h]), float(sc[l, 1, h])
            out[p + "k_proj.weight"][h * D:(h + 1) * D] /= ks
            out[p + "v_proj.weight"][h * D:(h + 1) * D] /= vs
            out[p + "q_proj.weight"][h * rep * D:(h + 1) * rep * D] *= ks
            out[p + "o_proj.weight"][:, h * rep * D:(h + 1) * rep * D] *= vs
    return out


def batch_model():
    """(config, fp32 state dict of bf16 numbers, token ids [1, n + 1] per stream: n prefill rows and the row fed after them)."""
    cfg = ModelConfig(**TWO_LAYER)
    sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 31, head_gain=2.0).items()}
    rng = np.random.default_rng(9)
    ids = [torch.from_numpy(rng.integers(3, cfg.vocab_size, size=(1, n + 1))) for n in BATCH_ROWS]
    return cfg, sd, ids
