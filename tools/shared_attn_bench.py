#!/usr/bin/env python3
"""One target verify pass (gamma = 4: 5 rows per stream) of streams that all hold copies of one prompt prefix:
attn_shared_kernel (SD_ATTN_SHARED=2: the prefix's K / V read from the donor arena once per 64-row query tile of the pass)
against the per-stream routes (SD_ATTN_SHARED=0: the launches sd_batch_forward makes, i.e. the parent's), on

    (a) llama-2-13b's layer shape cut to 4 layers           40 heads, MHA, D = 128, 16-bit KV arena
    (b) llama-2-70b's layer shape cut to 4 layers           64 query heads over 8 KV heads, D = 128, fp8 KV arena

at prefixes of 256 / 512 / 1024 / 2048 / 3840 tokens with 64 keys of its own per stream, 8 and 16 lock-step streams
(engine.batch_forward(shared=...)), random-init bf16 weights.

    python tools/shared_attn_bench.py [out.txt]        # MODELS=a,b  PREFIXES=256,...  STREAMS=8,16

Per shape and setting, RUNS alternating runs in one process after warm-up (the runs give the spread; call no difference
inside it a win): the attention class of Session.profile_read() - the median over PROF profiled passes, all layers - and the
event-timed pass.  The tunable is sampled when a session is created, so every measurement makes its own sessions on one
model, and asserts the route it took from Session.shared_attn_launches().  The K / V bytes are the algorithmic ones per pass:
per-stream routes read prefix + own keys of every stream, the shared route the prefix once and every stream's own keys."""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmspeculativesampling_amd import engine  # noqa: E402
from llmspeculativesampling_amd.config import load_config  # noqa: E402

GAMMA, OWN, REPS, RUNS, PROF = 4, 64, 10, 3, 5
ROWS = GAMMA + 1
MODELS = {"a": ("llama-2-13b layer shape x 4 layers (MHA, 16-bit KV)", "llama-2-13b", None),
          "b": ("llama-2-70b layer shape x 4 layers (64 heads over 8 KV heads, fp8 KV)", "llama-2-70b", "fp8")}


def env_list(name, default, conv=str):
    return [conv(v) for v in os.environ.get(name, default).split(",")]


def kv_bytes(cfg, prefix, streams, kv_dtype, shared):
    row = 2 * cfg.num_key_value_heads * cfg.head_dim * (1 if kv_dtype else 2) * cfg.num_hidden_layers
    return row * ((prefix if shared else prefix * streams) + (OWN + ROWS) * streams)


def measure(m, toks, prefix, streams, kv_dtype, flag):
    os.environ["SD_ATTN_SHARED"] = str(flag)
    donor = m.new_session(prefix, kv_dtype=kv_dtype)
    sess = [m.new_session(prefix + OWN + ROWS + 3, kv_dtype=kv_dtype) for _ in range(streams)]
    donor.forward(toks[:prefix], 0)
    for ses in sess:
        ses.copy_kv_from(donor, 0, prefix)
        ses.cache_len = prefix
        ses.forward(toks[prefix:prefix + OWN], 0)
    ctx = prefix + OWN

    def one():
        for ses in sess:
            ses.cache_len = ctx
        engine.batch_forward(sess, [toks] * streams, [ROWS] * streams, [ROWS] * streams, shared=(donor, prefix))
    for _ in range(3):
        one()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        one()
    e1.record()
    torch.cuda.synchronize()
    n0 = sess[0].shared_attn_launches()
    sess[0].profile(True)
    att = []
    for _ in range(PROF):
        one()
        att.append(sess[0].profile_read()["attention"][0])           # (reads and resets)
    sess[0].profile(False)
    launches = (sess[0].shared_attn_launches() - n0) / PROF
    assert launches == (m.config.num_hidden_layers if flag else 0), (flag, launches)
    return float(np.median(att)), e0.elapsed_time(e1) / REPS


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    prefixes, streams_l = env_list("PREFIXES", "256,512,1024,2048,3840", int), env_list("STREAMS", "8,16", int)
    say(f"one verify pass of {ROWS} rows per stream behind a shared prefix + {OWN} own keys, bf16, random-init weights; attention = the "
        f"class's time per pass (all layers), median of {PROF} profiled passes; pass = mean of {REPS} event-timed passes; {RUNS} "
        f"alternating runs each (min .. max); MB = algorithmic K/V bytes of the pass")
    for key in env_list("MODELS", "a,b"):
        label, name, kv_dtype = MODELS[key]
        cfg = dataclasses.replace(load_config(name), num_hidden_layers=4, max_position_embeddings=max(prefixes) + OWN + 64)
        m = engine.SpecDecModel.synthetic(cfg, seed=1, dtype=torch.bfloat16)
        toks = torch.from_numpy(np.random.default_rng(0).integers(3, cfg.vocab_size, size=max(prefixes) + OWN + ROWS)).to(torch.int32).cuda()
        say(f"({key}) {label}")
        for prefix in prefixes:
            for streams in streams_l:
                res = {0: [], 2: []}
                for _ in range(RUNS):
                    for flag in (0, 2):
                        res[flag].append(measure(m, toks, prefix, streams, kv_dtype, flag))
                cols = []
                for flag, who in ((0, "per-stream"), (2, "shared")):
                    att, ms = [r[0] for r in res[flag]], [r[1] for r in res[flag]]
                    cols.append(f"{who} ({kv_bytes(cfg, prefix, streams, kv_dtype, flag) / 1e6:7.1f} MB) attention {min(att):7.3f} .. "
                                f"{max(att):7.3f} ms, pass {min(ms):7.3f} .. {max(ms):7.3f} ms")
                ra = np.median([r[0] for r in res[0]]) / np.median([r[0] for r in res[2]])
                rp = np.median([r[1] for r in res[0]]) / np.median([r[1] for r in res[2]])
                say(f"    prefix {prefix:4d}, {streams:2d} streams: " + "; ".join(cols) + f"; medians: attention {ra:.2f}x, pass {rp:.2f}x")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
