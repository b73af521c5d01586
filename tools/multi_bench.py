#!/usr/bin/env python3
"""Times multi_speculative_sampling(strategy="iid") on the headline pair (random-init weights, device RNG).

    python tools/multi_bench.py --widths 2,4,8 --reps 5 --host-loop
        [--draft llama-68m --target llama-2-13b --gamma 4 --prompt-len 128 --max-len 64 --json-out FILE]

By default only the native loop (sd_spec_multi_generate) is timed per width; --host-loop adds the Python-orchestrated
loop (SD_MULTI_NATIVE=0) as a second arm.  Every rep is timed on its own and ends with a device synchronisation, so
"ms_per_iteration" here is not the figure of the same name that earlier versions of this tool printed (one clock around
all reps, one synchronisation at the end); the per-rep list shows the rep-to-rep spread.
Prints one JSON line: per width and arm tokens/s of the whole calls (prefills included), ms per iteration (all reps and
their median), iterations, mean accepted length; "single" is speculative_sampling on the same pair.
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
from llmspeculativesampling_amd.sampling import multi_speculative_sampling, speculative_sampling  # noqa: E402


def _time_arm(fn, reps, prompt_len):
    fn(0)
    torch.cuda.synchronize()
    toks = iters = 0
    accs, per_rep = [], []
    t_all = time.perf_counter()
    for r in range(reps):
        t0 = time.perf_counter()
        o, d = fn(10 + r)
        torch.cuda.synchronize()
        per_rep.append((time.perf_counter() - t0) / max(1, d["target_call_times"]) * 1e3)
        toks += o.shape[1] - prompt_len
        iters += d["target_call_times"]
        accs += d["acc_len"]
    dt = time.perf_counter() - t_all
    return {"tokens_per_s": toks / dt, "ms_per_iteration": dt / iters * 1e3, "ms_per_iteration_reps": per_rep,
            "ms_per_iteration_median": float(np.median(per_rep)), "iterations": iters, "mean_accept_len": float(np.mean(accs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draft", default="llama-68m")
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--width", type=int, default=4)
    ap.add_argument("--widths", default=None, help="comma-separated widths (default: --width)")
    ap.add_argument("--host-loop", action="store_true", help="also time the Python-orchestrated loop (SD_MULTI_NATIVE=0)")
    ap.add_argument("--gamma", type=int, default=4)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--max-len", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(",")] if a.widths else [a.width]
    dcfg, tcfg = load_config(a.draft), load_config(a.target)
    dm = SpecDecModel.synthetic(dcfg, seed=0, dtype=torch.bfloat16)
    tm = SpecDecModel.synthetic(tcfg, seed=1, dtype=torch.bfloat16)
    prompt = torch.from_numpy(np.random.default_rng(3).integers(3, dcfg.vocab_size, size=(1, a.prompt_len))).cuda()
    out = {"single": _time_arm(lambda s: speculative_sampling(prompt, dm, tm, 2, None, a.max_len, gamma=a.gamma, top_k=20, top_p=0.9,
                                                              details=True, rng=DeviceNoise(s)), a.reps, a.prompt_len)}
    for w in widths:
        def run(s, w=w):
            return multi_speculative_sampling(prompt, dm, tm, 2, None, a.max_len, gamma=a.gamma, width=w, strategy="iid",
                                              top_k=20, top_p=0.9, details=True, rng=DeviceNoise(s))
        arms = {}
        for arm in (["native", "host_loop"] if a.host_loop else ["native"]):
            if arm == "host_loop":
                os.environ["SD_MULTI_NATIVE"] = "0"
            else:
                os.environ.pop("SD_MULTI_NATIVE", None)
            arms[arm] = _time_arm(run, a.reps, a.prompt_len)
        os.environ.pop("SD_MULTI_NATIVE", None)
        out["width_%d" % w] = arms
    out["config"] = vars(a)
    line = json.dumps(out)
    print(line)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
