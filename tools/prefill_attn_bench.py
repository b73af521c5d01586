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
jitter shows - the median keeps a single late event out of the figure).  The tunable is sampled when a session is created, so every measurement makes its own session on one model.

    python tools/prefill_attn_bench.py --sweep [out.txt]

The context sweep: the same pass of models (a) and (b), and of four synthetic Llama layer shapes (d)-(g) that separate the head
dim from the launch's workgroup count (heads x 16 row groups), at contexts of 37, 1792, 2304 and 3840 tokens (3840 + 256 = the 4096
positions of both Llama-2 configs; the position tables are lengthened to hold them, the weights are random anyway), under the
default route (attn_prefill_kernel while its score tile fits the LDS - 2048 keys at D = 128, 2176 at D = 64; past that
attn_prefill_blocked_kernel for launches of at least two workgroups per CU and attn_kernel for smaller ones - the route
sd_prefill_attn_route states, which every measurement is asserted to have taken), under SD_PREFILL_ATTN=0 (attn_kernel, keys split over workgroups + the combine
launch: the route passes past the tile limit took before) and under SD_PREFILL_ATTN_BLOCK = 256, 512, 1024 (the blocked kernel
at every context, blocks of that many keys).  profiles/prefill_attn_long_context.txt is this output."""
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
# (sweep only) synthetic Llama layer shapes that separate the head dim from the workgroup count of a 256-row pass (heads x 16 row groups)
SHAPES = {
    "d": ("64 heads of D = 64 (hidden 4096) x 2 layers, 16-bit KV: 1024 workgroups", 4096, 64, 2),
    "e": ("32 heads of D = 64 (hidden 2048) x 2 layers, 16-bit KV: 512 workgroups", 2048, 32, 2),
    "f": ("8 heads of D = 128 (hidden 1024) x 4 layers, 16-bit KV: 128 workgroups", 1024, 8, 4),
    "g": ("16 heads of D = 128 (hidden 2048) x 4 layers, 16-bit KV: 256 workgroups", 2048, 16, 4),
}


def measure(m, toks, kv_dtype, flag, ctx=CTX, block=0):
    os.environ["SD_PREFILL_ATTN"] = str(flag)
    os.environ["SD_PREFILL_ATTN_BLOCK"] = str(block)
    ses = m.new_session(ctx + ROWS + 3, kv_dtype=kv_dtype)
    ses.forward(toks[:ctx], 0)

    def one():
        ses.rollback(ctx)
        ses.forward(toks[ctx:ctx + ROWS], 1)
    for _ in range(2):
        one()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        one()
    e1.record()
    torch.cuda.synchronize()
    n0, b0 = ses.prefill_attn_launches(), ses.prefill_attn_blocked_launches()
    ses.profile(True)
    profs = []
    for _ in range(PROF):
        one()
        profs.append(ses.profile_read())                           # (reads and resets)
    ses.profile(False)
    prof = {k: (float(np.median([p[k][0] for p in profs])), profs[0][k][1]) for k in profs[0]}
    # (launches per profiled pass: either matrix-core kernel, the blocked one)
    return e0.elapsed_time(e1) / REPS, prof, (ses.prefill_attn_launches() - n0) / PROF, (ses.prefill_attn_blocked_launches() - b0) / PROF


SWEEP_CTX = (37, 1792, 2304, 3840)
SWEEP_SETTINGS = [("default", 1, 0), ("SD_PREFILL_ATTN=0", 0, 0), ("SD_PREFILL_ATTN_BLOCK=256", 1, 256),
                  ("SD_PREFILL_ATTN_BLOCK=512", 1, 512), ("SD_PREFILL_ATTN_BLOCK=1024", 1, 1024)]


KERNELS = {0: "attn_kernel", 1: "attn_prefill_kernel", 2: "attn_prefill_blocked_kernel"}


def route(cfg, s_max, block):
    """sd_prefill_attn_route for one ROWS-row pass on this device: 0 attn_kernel, 1 single tile, 2 blocked."""
    import ctypes as C
    from llmspeculativesampling_amd._lib import lib
    k = C.c_int(-1)
    assert lib.sd_prefill_attn_route(cfg.head_dim, cfg.num_attention_heads, ROWS, s_max, block, 0, C.byref(k)) == 0
    return k.value


def sweep(say):
    say(f"one {ROWS}-row prefill pass at contexts of {', '.join(map(str, SWEEP_CTX))} tokens, bf16, random-init weights; attention = the class's "
        f"time per pass (all layers), median of {PROF} profiled passes, {RUNS} alternating runs; pass = mean of {REPS} event-timed passes; "
        f"kernels = matrix-core launches per pass (of which blocked)")
    for key in os.environ.get("MODELS", "a,b,d,e,f,g").split(","):
        if key in SHAPES:
            label, hidden, heads, layers = SHAPES[key]
            kv_dtype = None
            cfg = dataclasses.replace(load_config("llama-2-13b"), hidden_size=hidden, num_attention_heads=heads, num_key_value_heads=heads,
                                      intermediate_size=4096, vocab_size=4096)
        else:
            label, name, layers, kv_dtype = MODELS[key]
            cfg = load_config(name)
        cfg = dataclasses.replace(cfg, max_position_embeddings=max(SWEEP_CTX) + ROWS + 256)
        if layers:
            cfg = dataclasses.replace(cfg, num_hidden_layers=layers)
        m = SpecDecModel.synthetic(cfg, seed=1, dtype=torch.bfloat16)
        toks = torch.from_numpy(np.random.default_rng(0).integers(3, cfg.vocab_size, size=max(SWEEP_CTX) + ROWS)).to(torch.int32).cuda()
        say(f"({key}) {label}: {cfg.num_hidden_layers} layers, {cfg.num_attention_heads} heads on {cfg.num_key_value_heads} KV heads")
        for ctx in SWEEP_CTX:
            res = {s[0]: [] for s in SWEEP_SETTINGS}
            for run in range(RUNS):
                for tag, flag, block in SWEEP_SETTINGS:
                    ms, prof, launches, blocked = measure(m, toks, kv_dtype, flag, ctx, block)
                    # the route the library states for this pass on this device is the route the session took
                    kernel = route(cfg, ctx + ROWS, block) if flag else 0
                    L = cfg.num_hidden_layers
                    assert (launches, blocked) == {0: (0, 0), 1: (L, 0), 2: (L, L)}[kernel], (key, ctx, tag, kernel, launches, blocked)
                    assert not block or kernel == 2, (key, ctx, tag, kernel)
                    res[tag].append((prof["attention"][0], ms, launches, blocked, KERNELS[kernel]))
            say(f"  context {ctx} ({ctx + ROWS} keys)")
            base = np.mean([r[0] for r in res["SD_PREFILL_ATTN=0"]])
            for tag, _, _ in SWEEP_SETTINGS:
                att, ms = [r[0] for r in res[tag]], [r[1] for r in res[tag]]
                say(f"    {tag:27s}: attention {att[0]:8.3f} / {att[1]:8.3f} ms ({base / np.mean(att):5.2f}x of SD_PREFILL_ATTN=0), pass {ms[0]:8.3f} / {ms[1]:8.3f} ms, "
                    f"kernels {res[tag][0][2]:.0f} ({res[tag][0][3]:.0f}): {res[tag][0][4]}")
        del m
        torch.cuda.empty_cache()


def main():
    args = [a for a in sys.argv[1:] if a != "--sweep"]
    out = open(args[0], "w") if args else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if "--sweep" in sys.argv[1:]:
        return sweep(say)
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
                ms, prof, launches, blocked = measure(m, toks, kv_dtype, flag)
                assert blocked == 0 and launches == (cfg.num_hidden_layers if flag else 0), (key, flag, launches)
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
