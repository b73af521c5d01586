#!/usr/bin/env python3
"""Times autoregressive sampling - the baseline every speed-up of this project is quoted against - on the models bench.py
uses (random-init weights through synth.py, bf16, device RNG, top_k 20 / top_p 0.9).

    python tools/ar_baseline.py --model llama-68m [--streams 1,8,16 --prompt-len 128 --max-len 128 --reps 5]
                                [--json-out profiles/ar_baseline.json]

Per stream count B two arms, alternated rep by rep so that both see the same machine:
  native       B = 1: autoregressive_sampling(rng=DeviceNoise) - one sd_ar_batch_generate call with one stream;
               B > 1: autoregressive_sampling_batch - B lock-step streams sharing every pass over the weights
  python_loop  B sequential autoregressive_sampling(..., _native=False) calls: the interpreter loop (two ctypes calls and
               three blocking device reads per token), which is all there was before the native loop
Every rep is a whole call (prompt prefill included) between two device synchronisations on the host clock; EOS is off, so
every stream generates --max-len tokens.  Whether both arms returned the same ids on the warm-up rep is recorded (they do with
one stream; a bf16 pass over B rows need not round like B passes over one row).
The result - tokens/s per rep and their median, per model / stream count / arm - is merged into --json-out under the model's
name, so one invocation per model builds the file; a caller that wants a time limit per step runs one model (or one
--streams value) per invocation under its own limit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmspeculativesampling_amd.config import load_config  # noqa: E402
from llmspeculativesampling_amd.engine import SpecDecModel  # noqa: E402
from llmspeculativesampling_amd.noise import DeviceNoise  # noqa: E402
from llmspeculativesampling_amd.sampling import autoregressive_sampling, autoregressive_sampling_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama-68m", help="a config name (bench.py: llama-68m draft, llama-2-13b target)")
    ap.add_argument("--streams", default="1,8,16")
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--max-len", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    cfg = load_config(a.model)
    max_pos = min(cfg.max_position_embeddings, a.prompt_len + a.max_len + 8)
    m = SpecDecModel.synthetic(cfg, seed=2, dtype=torch.bfloat16, max_pos=max_pos)
    kw = dict(top_k=20, top_p=0.9)
    out = {"config": {k: v for k, v in vars(a).items() if k != "json_out"}, "dtype": "bfloat16", "streams": {}}
    for B in [int(b) for b in a.streams.split(",")]:
        prompts = [torch.from_numpy(np.random.default_rng(100 + i).integers(3, cfg.vocab_size, size=(1, a.prompt_len))).cuda()
                   for i in range(B)]

        def native(seed0):
            if B == 1:
                return [autoregressive_sampling(prompts[0], m, a.max_len, -1, rng=DeviceNoise(seed0), **kw)]
            return autoregressive_sampling_batch(prompts, m, a.max_len, -1, seeds=[seed0 + i for i in range(B)], **kw)

        def python_loop(seed0):
            return [autoregressive_sampling(p, m, a.max_len, -1, rng=DeviceNoise(seed0 + i), _native=False, **kw)
                    for i, p in enumerate(prompts)]

        arms = {"native": native, "python_loop": python_loop}
        warm = {name: fn(1000) for name, fn in arms.items()}              # warm-up of every shape; the ids are compared
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(warm["native"], warm["python_loop"]))
        rates = {name: [] for name in arms}
        for r in range(a.reps):
            for name, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs = fn(2000 + 100 * r)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rates[name].append(sum(o.shape[1] - a.prompt_len for o in outs) / dt)
        res = {name: {"tokens_per_s_reps": v, "tokens_per_s_median": float(np.median(v))} for name, v in rates.items()}
        res["same_ids_native_and_python_loop"] = bool(same)
        res["native_over_python_loop"] = res["native"]["tokens_per_s_median"] / res["python_loop"]["tokens_per_s_median"]
        out["streams"][str(B)] = res
        print(json.dumps({a.model: {str(B): res}}), flush=True)
    if a.json_out:
        merged = {}
        if os.path.exists(a.json_out):
            with open(a.json_out) as f:
                merged = json.load(f)
        merged.setdefault(a.model, {"streams": {}})
        merged[a.model]["streams"].update(out["streams"])
        merged[a.model].update({k: v for k, v in out.items() if k != "streams"})
        with open(a.json_out, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
