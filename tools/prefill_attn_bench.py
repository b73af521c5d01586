#!/usr/bin/env python3
"""Attention of one 256-row prefill pass at a 37-token context, attn_prefill_kernel (16-row groups, both products on the
matrix cores) against attn_kernel (8-row groups; SD_PREFILL_ATTN=0 - the route such passes took before the kernel covered
them), for the instances beyond head_dim 128 with a 16-bit arena:

    (a) llama-2-70b's layer shape cut to 4 layers, fp8 KV arena      fp8, D = 128
    (b) opt-125m, 16-bit arena                                       D = 64
    (c) llama-68m, fp8 KV arena                                      fp8 + D = 64

    python tools/prefill_attn_bench.py [out.txt]        # MODELS=a,b,c selects; random-init bf16 weights

Per model and setting, twice (the two runs give the spread): the whole pass event-timed over 5 repetitions, and 5 profiled
passes for the per-class times, each class the median over the passes (Session.profile: event pairs around every launch
class; `attention` is the class of both kernels; a draft model's attention launch is about 15 us, where one event pair's
jitter shows - the median keeps a single late event out of the figure).  The tunable is sampled when a session is created, so every measurement makes its own session on one model."""
import dataclasses
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmspeculativesampling_amd.config import load_config  # noqa: E402
from llmspeculativesampling_amd.engine import SpecDecModel  # noqa: E402

CTX, ROWS, REPS, RUNS, PROF = 37, 256, 5, 2, 5
MODELS = {
    "a": ("llama-2-70b layer shape x 4 layers, fp8 KV (D = 128)", "llama-2-70b", 4, "fp8"),
    "b": ("opt-125m, 16-bit KV (D = 64)", "opt-125m", None, None),
    "c": ("llama-68m, fp8 KV (D = 64)", "llama-68m", None, "fp8"),
}


def measure(m, toks, kv_dtype, flag):
    os.environ["SD_PREFILL_ATTN"] = str(flag)
    ses = m.new_session(CTX + ROWS + 3, kv_dtype=kv_dtype)
    ses.forward(toks[:CTX], 0)

    def one():
        ses.rollback(CTX)
        ses.forward(toks[CTX:CTX + ROWS], 1)
    for _ in range(2):
        one()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        one()
    e1.record()
    torch.cuda.synchronize()
    n0 = ses.prefill_attn_launches()
    ses.profile(True)
    profs = []
    for _ in range(PROF):
        one()
        profs.append(ses.profile_read())                           # (reads and resets)
    ses.profile(False)
    prof = {k: (float(np.median([p[k][0] for p in profs])), profs[0][k][1]) for k in profs[0]}
    return e0.elapsed_time(e1) / REPS, prof, (ses.prefill_attn_launches() - n0) / PROF     # launches per profiled pass


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    say(f"one {ROWS}-row prefill pass at a {CTX}-token context, bf16, random-init weights; SD_PREFILL_ATTN=1: attn_prefill_kernel, "
        f"=0: attn_kernel; {RUNS} runs of each, pass = mean of {REPS} event-timed passes, classes = median of {PROF} profiled passes")
    for key in os.environ.get("MODELS", "a,b,c").split(","):
        label, name, layers, kv_dtype = MODELS[key]
        cfg = load_config(name)
        if layers:
            cfg = dataclasses.replace(cfg, num_hidden_layers=layers)
        m = SpecDecModel.synthetic(cfg, seed=1, dtype=torch.bfloat16)
        toks = torch.from_numpy(np.random.default_rng(0).integers(3, cfg.vocab_size, size=CTX + ROWS)).to(torch.int32).cuda()
        say(f"({key}) {label}: {cfg.num_hidden_layers} layers, {cfg.num_attention_heads} heads on {cfg.num_key_value_heads} KV heads")
        res = {1: [], 0: []}
        for run in range(RUNS):
            for flag in (1, 0):
                ms, prof, launches = measure(m, toks, kv_dtype, flag)
                assert launches == (cfg.num_hidden_layers if flag else 0), (key, flag, launches)
                att = prof["attention"]
                res[flag].append((att[0], ms))
                say(f"    SD_PREFILL_ATTN={flag} run {run}: attention {att[0]:7.3f} ms in {att[1]} launches, pass {ms:7.3f} ms;  "
                    + ", ".join(f"{k} {v[0]:.2f}" for k, v in prof.items() if k != "attention"))
        for what, col in (("attention", 0), ("pass", 1)):
            new, old = [r[col] for r in res[1]], [r[col] for r in res[0]]
            say(f"    {what:9s}: attn_prefill_kernel {min(new):7.3f} .. {max(new):7.3f} ms, attn_kernel {min(old):7.3f} .. {max(old):7.3f} ms "
                f"(means {sum(old) / len(old) / (sum(new) / len(new)):.2f}x)")
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
