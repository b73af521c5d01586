#!/usr/bin/env python3
"""Attention of one verify pass (gamma = 4: 5 rows per stream) of a GQA model, attn_grouped_kernel (SD_ATTN_GROUPED=2: one
workgroup per KV head, row group and key split, both products on the matrix cores) against attn_kernel (SD_ATTN_GROUPED=0: one
workgroup per query head; the parent's device code, i.e. the baseline), on

    (a) llama-2-70b's layer shape cut to 4 layers          64 query heads over 8 KV heads, D = 128
    (b) its TP = 8 shard's shape, 4 layers                  8 query heads over 1 KV head (a whole model of that shape: no group)

with the 16-bit and the fp8 KV arena, at contexts of 512 / 2048 / 4096 keys and 1 / 8 / 16 lock-step streams
(engine.batch_forward), random-init bf16 weights.

    python tools/grouped_attn_bench.py [out.txt]        # MODELS=a,b  ARENAS=bf16,fp8  CTXS=512,2048,4096  STREAMS=1,8,16

Per shape and setting, RUNS alternating runs in one process after warm-up (the runs give the spread; call no difference
inside it a win): the attention class of Session.profile_read() - the median over PROF profiled passes, all layers - and the
event-timed pass.  The tunable is sampled when a session is created, so every measurement makes its own sessions on one
model, and asserts the route it took from Session.grouped_attn_launches().  The K / V bytes are the algorithmic ones - every
visible K and V element of every stream and KV head once per layer - and the share is of the 8 TB/s HBM peak; attn_kernel
reads them through G query heads, so its share says how far the caches carry the re-reads.

Kernel times come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/grouped_attn_bench.py"""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmspeculativesampling_amd import engine  # noqa: E402
from llmspeculativesampling_amd.config import load_config  # noqa: E402

GAMMA, REPS, RUNS, PROF, PEAK = 4, 10, 3, 5, 8e12
ROWS = GAMMA + 1
MODELS = {
    "a": ("llama-2-70b layer shape x 4 layers (64 heads over 8 KV heads)", {}),
    "b": ("TP = 8 shard shape x 4 layers (8 heads over 1 KV head)",
          dict(num_attention_heads=8, num_key_value_heads=1, head_dim_=128, intermediate_size=28672 // 8)),
}


def env_list(name, default, conv=str):
    return [conv(v) for v in os.environ.get(name, default).split(",")]


def kv_bytes(cfg, ctx, streams, kv_dtype):
    """K and V of every visible key, every KV head, stream and layer, once (the last row sees ctx + ROWS keys)."""
    return 2 * (ctx + ROWS) * cfg.num_key_value_heads * cfg.head_dim * (1 if kv_dtype else 2) * streams * cfg.num_hidden_layers


def measure(m, toks, ctx, streams, kv_dtype, flag):
    os.environ["SD_ATTN_GROUPED"] = str(flag)
    sess = [m.new_session(ctx + ROWS + 3, kv_dtype=kv_dtype) for _ in range(streams)]
    sess[0].forward(toks[:ctx], 0)
    for ses in sess[1:]:                                            # the streams share the prompt: one prefill, copied rows
        ses.copy_kv_from(sess[0], 0, ctx)

    def one():
        for ses in sess:
            ses.cache_len = ctx
        if streams == 1:
            sess[0].forward(toks[ctx:ctx + ROWS], ROWS)
        else:
            engine.batch_forward(sess, [toks] * streams, [ROWS] * streams, [ROWS] * streams)
    for _ in range(3):
        one()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        one()
    e1.record()
    torch.cuda.synchronize()
    n0 = sess[0].grouped_attn_launches()
    sess[0].profile(True)
    att = []
    for _ in range(PROF):
        one()
        att.append(sess[0].profile_read()["attention"][0])           # (reads and resets)
    sess[0].profile(False)
    launches = (sess[0].grouped_attn_launches() - n0) / PROF
    assert launches == (m.config.num_hidden_layers if flag else 0), (flag, launches)
    return float(np.median(att)), e0.elapsed_time(e1) / REPS


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    ctxs, streams_l = env_list("CTXS", "512,2048,4096", int), env_list("STREAMS", "1,8,16", int)
    say(f"one verify pass of {ROWS} rows per stream, bf16, random-init weights; attention = the class's time per pass (all layers), "
        f"median of {PROF} profiled passes; pass = mean of {REPS} event-timed passes; {RUNS} alternating runs each (min .. max); "
        f"share = algorithmic K/V bytes / attention time / {PEAK / 1e12:.0f} TB/s")
    for key in env_list("MODELS", "a,b"):
        label, over = MODELS[key]
        cfg = dataclasses.replace(load_config("llama-2-70b"), num_hidden_layers=4, max_position_embeddings=max(ctxs) + 64, **over)
        m = engine.SpecDecModel.synthetic(cfg, seed=1, dtype=torch.bfloat16)
        toks = torch.from_numpy(np.random.default_rng(0).integers(3, cfg.vocab_size, size=max(ctxs) + ROWS)).to(torch.int32).cuda()
        say(f"({key}) {label}")
        for arena in env_list("ARENAS", "bf16,fp8"):
            kv_dtype = "fp8" if arena == "fp8" else None
            for ctx in ctxs:
                for streams in streams_l:
                    res = {0: [], 2: []}
                    for _ in range(RUNS):
                        for flag in (0, 2):
                            res[flag].append(measure(m, toks, ctx, streams, kv_dtype, flag))
                    nbytes = kv_bytes(cfg, ctx, streams, kv_dtype)
                    cols = []
                    for flag, name in ((0, "attn_kernel"), (2, "attn_grouped_kernel")):
                        att, ms = [r[0] for r in res[flag]], [r[1] for r in res[flag]]
                        cols.append(f"{name} attention {min(att):7.3f} .. {max(att):7.3f} ms ({nbytes / (np.mean(att) * 1e-3) / PEAK:6.1%} of peak), "
                                    f"pass {min(ms):7.3f} .. {max(ms):7.3f} ms")
                    ratio = np.mean([r[0] for r in res[0]]) / np.mean([r[0] for r in res[2]])
                    say(f"    {arena:4s} KV, {ctx:4d} keys, {streams:2d} streams ({nbytes / 1e6:7.1f} MB of K/V): " + "; ".join(cols) + f"; means {ratio:.2f}x")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
