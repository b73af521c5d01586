"""Bit-level record of the forward pass on every route it can take: tests/golden/forward_routes.json.

    python tests/golden/make_forward_routes.py [out.json]        # on the GPU, at the commit whose behaviour is the record

Every case runs seeded synthetic weights (2 layers, vocab 4096) through the public Python API only - SpecDecModel,
Session.forward, batch_forward, batch_prefill, the tree forward, Session.profile / profile_read - and stores

    logits   SHA-256 of the fp32 logit rows of the measured pass(es)
    kv       SHA-256 of the written range [:, :, :, :cache_len] of every session's KV arena ("" where the API hides them)
    counts   launches per profile class of the measured pass (profile_read)
    prefill  [attn_prefill launches, of which blocked] of the case's first session

tests/test_gpu_forward_routes.py recomputes each case with run_case() and compares; a refactor of the host code that keeps
every launch (kernel, grid, arguments) keeps every digest and every count.  main() also asserts from the counts that each
case took the route it is named for (EXPECT) and that a second run of every case gives the same record.
"""
import ctypes as C
import hashlib
import json
import os
import sys
import threading

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from llmspeculativesampling_amd import _lib, tp                                   # noqa: E402
from llmspeculativesampling_amd.config import ModelConfig                         # noqa: E402
from llmspeculativesampling_amd.engine import SpecDecModel, batch_forward, batch_prefill   # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "forward_routes.json")
V, L = 4096, 2
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32

LLAMA_1K = dict(arch="llama", vocab_size=V, hidden_size=1024, intermediate_size=2048, num_hidden_layers=L,
                num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=256, rms_norm_eps=1e-5)
LLAMA_4K = dict(arch="llama", vocab_size=V, hidden_size=4096, intermediate_size=2048, num_hidden_layers=L,
                num_attention_heads=32, num_key_value_heads=8, max_position_embeddings=256, rms_norm_eps=1e-5)
OPT_1K = dict(arch="opt", vocab_size=V, hidden_size=1024, ffn_dim=2048, num_hidden_layers=L, num_attention_heads=8,
              max_position_embeddings=256)
CONFIGS = {
    "llama1k": LLAMA_1K,
    "llama4k": LLAMA_4K,
    "opt1k": OPT_1K,
    "opt1k_proj": dict(OPT_1K, word_embed_proj_dim=512),
    "opt1k_post": dict(OPT_1K, do_layer_norm_before=False),
}
_MODELS = {}


def model(name, dtype=BF16):
    """One model per (config, dtype) for the whole process: weights from numpy's seeded generator, tensor by tensor."""
    if (name, dtype) not in _MODELS:
        seed = 40 + sorted(CONFIGS).index(name)
        _MODELS[name, dtype] = SpecDecModel.synthetic(ModelConfig(**CONFIGS[name]), seed=seed, dtype=dtype, method="numpy")
    return _MODELS[name, dtype]


def tokens(n, seed=3):
    return torch.from_numpy(np.random.default_rng(seed).integers(3, V, size=(n,))).to(torch.int32).cuda()


def sha(t):
    t = t.detach().contiguous().cpu()
    if t.dtype in (torch.bfloat16, torch.float16):
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def kv_sha(sessions):
    h = hashlib.sha256()
    for s in sessions:
        h.update(sha(s.kv[:, :, :, :s.cache_len]).encode())
    return h.hexdigest()


def record(sessions, logits, counts):
    s0 = sessions[0]
    return {"logits": sha(logits), "kv": kv_sha(sessions), "counts": counts,
            "prefill": [s0.prefill_attn_launches(), s0.prefill_attn_blocked_launches()]}


def measured(ses, fn):
    """fn() with the session's profile on: (what fn returned, {class: launches})."""
    ses.profile(True)
    out = fn()
    counts = {k: v[1] for k, v in ses.profile_read().items()}
    ses.profile(False)
    return out, counts


def decode(name, rows, dtype=BF16, ctx=12, kv_dtype=None, env=None):
    """A `ctx`-token context pass, then the measured pass: `rows` new rows, logits for all of them."""
    def run():
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            ses = model(name, dtype).new_session(256, kv_dtype=kv_dtype)        # (tunables are sampled here)
        finally:
            for k in env or {}:
                os.environ.pop(k, None)
        ids = tokens(ctx + rows)
        if ctx:
            ses.forward(ids[:ctx], 0)
        n_logits = min(rows, 64) if rows <= 64 else 1
        logits, counts = measured(ses, lambda: ses.forward(ids[ctx:], n_logits).clone())
        return record([ses], logits, counts)
    return run


def native_loop(name):
    """The native speculative loop, model `name` drafting for itself (gamma 3, top-k sampling on the device's Philox stream):
    its forwards carry a head request, so the head of the draft's 1-row steps and of the 4-row verify passes leaves raw
    logits, tile maxima and cleared probability rows.  The loop owns its sessions: the record is the token sequence."""
    def run():
        from llmspeculativesampling_amd.noise import DeviceNoise
        from llmspeculativesampling_amd.sampling import speculative_sampling
        m = model(name)
        out = speculative_sampling(tokens(10).long()[None], m, m, -1, None, 24, gamma=3, top_k=20, top_p=0.9, rng=DeviceNoise(seed=5))
        assert out.shape[1] == 34
        return {"logits": sha(out.to(torch.int32)), "kv": "", "counts": {}, "prefill": [0, 0]}
    return run


def batched(n_streams, rows):
    def run():
        m = model("llama1k")
        sess = [m.new_session(64, max_rows=80) for _ in range(n_streams)]
        seqs = [tokens(6 + rows, seed=10 + i) for i in range(n_streams)]
        for s, q in zip(sess, seqs):
            s.forward(q[:6], 0)
        big = torch.empty((n_streams * rows, V), dtype=torch.float32, device="cuda")
        logits, counts = measured(sess[0], lambda: batch_forward(sess, seqs, [rows] * n_streams, [rows] * n_streams, big).clone())
        return record(sess, logits, counts)
    return run


def batched_prefill():
    m = model("llama1k")
    sess = [m.new_session(128) for _ in range(2)]
    seqs = [tokens(40, seed=20), tokens(88, seed=21)]
    _, counts = measured(sess[0], lambda: batch_prefill(sess, seqs, [40, 88]))
    # the logits of one more row per stream read every K / V row the batched pass wrote
    logits = torch.cat([s.forward(tokens(1, seed=22), 1).clone() for s in sess])
    return record(sess, logits, counts)


def tree():
    """A 7-node draft tree (two branches under a root, as beam search builds them) behind a 6-token prefix."""
    m = model("llama1k")
    ses = m.new_session(64)
    ids = tokens(13)
    ses.forward(ids[:6], 0)
    parent = [-1, 0, 0, 1, 1, 2, 2]
    masks, depth = [], []
    for i, p in enumerate(parent):
        masks.append((1 << i) | (masks[p] if p >= 0 else 0))
        depth.append(depth[p] + 1 if p >= 0 else 0)
    pos = (C.c_int32 * 7)(*[6 + d for d in depth])
    msk = (C.c_uint64 * 7)(*masks)
    logits = torch.empty((7, V), dtype=torch.float32, device="cuda")

    def go():
        _lib.check(_lib.lib.sd_session_forward_tree(ses.handle, ids[6:].data_ptr(), pos, msk, 7, 6, logits.data_ptr(), logits.stride(0),
                                                    torch.cuda.current_stream().cuda_stream), "sd_session_forward_tree")
        ses.cache_len = 13
        return logits
    out, counts = measured(ses, go)
    return record([ses], out, counts)


def tensor_parallel():
    """Two Megatron shards of llama1k on one GPU through the loopback group: each rank on its own thread and stream."""
    from llmspeculativesampling_amd.synth import make_state_dict
    cfg = ModelConfig(**LLAMA_1K)
    sd = make_state_dict(cfg, 47, dtype=BF16)
    groups = tp.TPGroup.loopback(2)
    sess = [tp.shard_model(cfg, sd, r, 2, group=groups[r], dtype=BF16).new_session(64) for r in range(2)]
    ids = tokens(17)
    out, errs = [None, None], []

    def work(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                sess[r].forward(ids[:12], 0)
                out[r] = measured(sess[r], lambda: sess[r].forward(ids[12:], 5).clone())
                torch.cuda.current_stream().synchronize()
        except Exception as e:                                   # noqa: BLE001
            errs.append((r, repr(e)))
    ts = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
    assert not errs and all(not t.is_alive() for t in ts), errs
    assert out[0][1] == out[1][1]
    return record(sess, torch.cat([out[0][0], out[1][0]]), out[0][1])


CASES = {
    # bf16 small-model path: <= 4 rows at hidden <= 2048
    "small_llama_1row": decode("llama1k", 1),
    "small_llama_4rows": decode("llama1k", 4),
    "small_opt_1row": decode("opt1k", 1),
    "small_opt_4rows": decode("opt1k", 4),
    "small_llama_head_request": native_loop("llama1k"),
    "small_opt_head_request": native_loop("opt1k"),
    # bf16, hidden 1024: fused attention + O with both norm-on-load seams / with two row groups / separate launches
    "llama1k_5rows": decode("llama1k", 5),
    "llama1k_8rows": decode("llama1k", 8),
    "llama1k_9rows": decode("llama1k", 9),
    "llama1k_16rows": decode("llama1k", 16),
    "llama1k_17rows": decode("llama1k", 17),
    # the large-model decode route: no embed + QKV launch, no small path
    "llama4k_1row": decode("llama4k", 1),
    "llama4k_4rows": decode("llama4k", 4),
    "fp16_5rows": decode("llama1k", 5, dtype=F16),
    "fp32_5rows": decode("llama1k", 5, dtype=F32),
    "opt_proj_5rows": decode("opt1k_proj", 5),
    "opt_post_ln_5rows": decode("opt1k_post", 5),
    "batch_8x5": batched(8, 5),
    "batch_13x5": batched(13, 5),
    "batch_prefill_40_88": batched_prefill,
    "prefill_128": decode("llama1k", 128, ctx=0),
    "prefill_128_fp8kv": decode("llama1k", 128, ctx=0, kv_dtype="fp8"),
    "prefill_128_blocked": decode("llama1k", 128, ctx=0, env={"SD_PREFILL_ATTN_BLOCK": "64"}),
    "tree_7nodes": tree,
    "tp2_loopback_5rows": tensor_parallel,
}

# What the launch counts of the measured pass must say for the route a case is named for (2 layers).  Per layer the per-op
# chain makes 4 GEMMs, 1 attention launch and 2 residual+norm launches; + 1 embedding launch and the head's GEMM + logits.
#   fused attention + O: the O projection is no GEMM launch (7 GEMMs);  norm on load: the attention seam keeps no norm launch,
#   the down seam only the last layer's;  small path: the embedding rides layer 0's QKV and only the final norm has a launch.
PER_OP = {"embed": 1, "gemm": 9, "attention": 2, "norm_residual": 4, "logits": 1}
FUSED_AO = dict(PER_OP, gemm=7)
SMALL = {"gemm": 9, "attention": 2, "norm_residual": 1, "logits": 1}
PREFILL = dict(PER_OP)
EXPECT = {
    "small_llama_1row": SMALL, "small_llama_4rows": SMALL, "small_opt_1row": SMALL, "small_opt_4rows": SMALL,
    "small_llama_head_request": {}, "small_opt_head_request": {},      # (the loop's sessions are its own: no counts)
    "llama1k_5rows": dict(FUSED_AO, norm_residual=1), "llama1k_8rows": dict(FUSED_AO, norm_residual=1),
    "llama1k_9rows": FUSED_AO, "llama1k_16rows": FUSED_AO, "llama1k_17rows": PER_OP,
    "llama4k_1row": dict(FUSED_AO, norm_residual=1), "llama4k_4rows": dict(FUSED_AO, norm_residual=1),
    "fp16_5rows": dict(FUSED_AO, norm_residual=1),
    "fp32_5rows": dict(PER_OP, qkv_rope_append=2, activation=2),
    # project_in / project_out: 2 more GEMMs, embedding + add-positions, the first pre-norm, a fold launch in front of the head
    "opt_proj_5rows": {"embed": 2, "gemm": 9, "attention": 2, "norm_residual": 5, "logits": 2},
    "opt_post_ln_5rows": dict(FUSED_AO, norm_residual=5),          # (+ the operand-layout copy of the embedded rows)
    "batch_8x5": PER_OP, "batch_13x5": PER_OP,
    "batch_prefill_40_88": {"embed": 1, "gemm": 8, "attention": 2, "norm_residual": 4},
    "prefill_128": PREFILL, "prefill_128_fp8kv": PREFILL, "prefill_128_blocked": PREFILL,
    "tree_7nodes": dict(PER_OP, norm_residual=3),                   # (7 rows: the down seam opens, the attention seam needs the fused launch)
    "tp2_loopback_5rows": dict(PER_OP, other=4),                    # (two all-reduces per layer)
}
EXPECT_PREFILL = {"batch_prefill_40_88": [2, 0], "prefill_128": [2, 0], "prefill_128_fp8kv": [2, 0], "prefill_128_blocked": [2, 2]}


def run_case(name):
    with torch.no_grad():
        rec = CASES[name]()
    torch.cuda.synchronize()
    return rec


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    recs, bad = {}, []
    for name in CASES:
        rec = run_case(name)
        again = run_case(name)
        print(name, json.dumps(rec), flush=True)
        if rec != again:
            bad.append(f"{name}: not reproducible: {again}")
        if rec["counts"] != EXPECT[name] or rec["prefill"] != EXPECT_PREFILL.get(name, [0, 0]):
            bad.append(f"{name}: route: counts {rec['counts']} prefill {rec['prefill']}, expected {EXPECT[name]} "
                       f"{EXPECT_PREFILL.get(name, [0, 0])}")
        recs[name] = rec
    with open(out, "w") as f:
        json.dump(recs, f, indent=1, sort_keys=True)
        f.write("\n")
    assert not bad, "\n".join(bad)
    print("wrote", out)


if __name__ == "__main__":
    main()
