#!/usr/bin/env python3
"""What per-token target log-probabilities from the native loops cost and save, on the pair bench.py uses (llama-68m ->
llama-2-13b, random-init weights through synth.py, bf16, device RNG, top_k 20 / top_p 0.9, gamma 4, EOS off).

    python tools/logprobs_bench.py --part off [--tree DIR]        # one JSON line: the paths without scores, of the tree at DIR
    python tools/logprobs_bench.py --part onoff                   # one JSON line: (b) and (c) below
    python tools/logprobs_bench.py --part trace                   # one short run with scores on, to be traced from outside
    python tools/logprobs_bench.py --part merge --lines FILE [--bench-lines FILE --kernel-stats CSV] --json-out profiles/logprobs_ab.json

  off    the three paths a caller without scores takes, reps alternated: one stream (speculative_sampling, 128-token prompt,
         max_len 128), the uniform 8-stream queue (8 prompts of 128 tokens through 8 slots, max_len 128) and the
         autoregressive baseline (the target alone, one stream).  --tree runs them on another checkout's package and library
         (the parent commit's), so that a caller can alternate processes of the two trees in one visit: (a).
  onoff  (b) scores on against off, alternated rep by rep in this process: the one stream and the 8-slot queue; (c) per
         prompt of the queue workload, generation followed by quality.get_score of every output against generation with
         scores (speculative_sampling_queue_logprobs), and the largest difference between the two scores.
  trace  both loops once with scores on; run it under `rocprofv3 --kernel-trace --stats` for token_logprob_kernel's time.
  merge  the JSON lines of all runs of a visit (each tagged with its tree) into one file with per-arm medians and spreads.
A rep is a whole call, prefill included, between two device synchronisations on the host clock, after one warm-up rep of
every arm.  Rates count the tokens each prompt asked for."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

GAMMA, SLOTS, L, M = 4, 8, 128, 128


def _rate(fn, lens, budgets):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return sum(min(o.shape[1] - n, m) for o, n, m in zip(outs, lens, budgets)) / dt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["off", "onoff", "trace", "merge"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="branch")
    ap.add_argument("--draft", default="llama-68m")
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lines", default=None)
    ap.add_argument("--bench-lines", default=None, help="merge: tagged bench.py / `off` lines of further visits, the trees in both orders")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    if a.part == "merge":
        return merge(a)
    sys.path.insert(0, a.tree)
    import torch
    from llmspeculativesampling_amd import quality
    from llmspeculativesampling_amd import sampling as S
    from llmspeculativesampling_amd.config import load_config
    from llmspeculativesampling_amd.engine import SpecDecModel
    from llmspeculativesampling_amd.noise import DeviceNoise
    dcfg, tcfg = load_config(a.draft), load_config(a.target)
    max_pos = L + M + GAMMA + 8
    dm = SpecDecModel.synthetic(dcfg, seed=1, dtype=torch.bfloat16, max_pos=max_pos)
    tm = SpecDecModel.synthetic(tcfg, seed=2, dtype=torch.bfloat16, max_pos=max_pos)
    kw = dict(gamma=GAMMA, top_k=20, top_p=0.9)
    prompts = [torch.from_numpy(np.random.default_rng(100 + i).integers(3, tcfg.vocab_size, size=(1, L))).cuda() for i in range(SLOTS)]
    seeds = lambda s0: [s0 + i for i in range(SLOTS)]

    def single(s0, **more):
        r = S.speculative_sampling(prompts[0], dm, tm, -1, None, M, rng=DeviceNoise(s0), **more, **kw)
        return list(r) if isinstance(r, tuple) else [r]

    def queue(s0):
        return S.speculative_sampling_queue(prompts, dm, tm, -1, None, M, seeds=seeds(s0), slots=SLOTS, **kw)

    def queue_lp(s0):
        return S.speculative_sampling_queue_logprobs(prompts, dm, tm, -1, None, M, seeds=seeds(s0), slots=SLOTS, **kw)

    def ar(s0):
        return [S.autoregressive_sampling(prompts[0], tm, M, -1, top_k=20, top_p=0.9, rng=DeviceNoise(s0))]

    def queue_then_get_score(s0):
        outs = queue(s0)
        return outs, [float(quality.get_score(o, tm, L)) for o in outs]

    if a.part == "trace":
        single(1000, logprobs=True)
        queue_lp(1000)
        torch.cuda.synchronize()
        return
    one, eight = ([L], [M]), ([L] * SLOTS, [M] * SLOTS)
    if a.part == "off":
        arms = {"one_stream": (lambda s0: single(s0)[:1], one), "queue_uniform_8": (queue, eight), "ar_one_stream": (ar, one)}
    else:
        arms = {"one_stream_off": (lambda s0: single(s0)[:1], one), "one_stream_on": (lambda s0: single(s0, logprobs=True)[:1], one),
                "queue_uniform_8_off": (queue, eight), "queue_uniform_8_on": (lambda s0: queue_lp(s0)[0], eight),
                "queue_then_get_score": (lambda s0: queue_then_get_score(s0)[0], eight)}
    for fn, _ in arms.values():                                   # warm-up of every shape
        fn(1000)
    rates = {k: [] for k in arms}
    secs = {k: [] for k in arms}
    for r in range(a.reps):
        for k, (fn, (lens, budgets)) in arms.items():
            rate, dt = _rate(lambda: fn(2000 + 100 * r), lens, budgets)
            rates[k].append(rate)
            secs[k].append(dt)
    line = {"part": a.part, "tag": a.tag, "tokens_per_s": rates, "seconds_per_call": secs}
    if a.part == "onoff":
        # the same seeds: the tokens must not move, and the two scores are one quantity computed twice
        outs, want = queue_then_get_score(3000)
        outs2, lps = queue_lp(3000)
        got = [float(quality.score_from_logprobs(lp)) for lp in lps]
        line["queue_tokens_identical_on_and_off"] = bool(all(torch.equal(x, y) for x, y in zip(outs, outs2)))
        o1, o2 = single(3000), single(3000, logprobs=True)
        line["one_stream_tokens_identical_on_and_off"] = bool(torch.equal(o1[0], o2[0]))
        line["scores_get_score"], line["scores_from_loop"] = want, got
        line["largest_score_difference"] = max(abs(x - y) for x, y in zip(want, got))
        line["per_prompt_seconds"] = {"generation_plus_get_score": float(np.median(secs["queue_then_get_score"])) / SLOTS,
                                      "generation_with_logprobs": float(np.median(secs["queue_uniform_8_on"])) / SLOTS,
                                      "generation_alone": float(np.median(secs["queue_uniform_8_off"])) / SLOTS}
    print(json.dumps(line), flush=True)


def merge(a):
    runs = [json.loads(ln) for ln in open(a.lines) if ln.startswith("{")]
    out = {"what": "llama-68m -> llama-2-13b, bf16, gamma 4, device RNG, top_k 20 / top_p 0.9, EOS off; 128-token prompts, max_len 128; "
                   "--lines: one visit to one MI355X, the parent commit's tree and this tree alternated process by process, then "
                   "the on / off run; --bench-lines: further visits, the two trees in both orders",
           "order": [r.get("tag", "?") + ":" + r.get("part", "bench_py" if "metric" in r else "?") for r in runs]}
    ab = {}
    for r in runs:
        if r.get("part") == "off":
            for k, v in r["tokens_per_s"].items():
                ab.setdefault(k, {}).setdefault(r["tag"], []).append(float(np.median(v)))
        elif "metric" in r and "tag" in r:                        # a bench.py result line, tagged by the caller
            ab.setdefault("bench_py", {}).setdefault(r["tag"], []).append(float(r["value"]))
    for k, v in ab.items():
        if "parent" in v and "branch" in v:
            spread = max(v["parent"]) - min(v["parent"])
            v.update(unit="tok/s", parent_spread=spread, difference_of_means=float(np.mean(v["branch"]) - np.mean(v["parent"])),
                     inside_parent_spread=bool(abs(np.mean(v["branch"]) - np.mean(v["parent"])) <= spread))
    out["a_logprobs_off_branch_against_parent"] = ab
    if a.bench_lines:
        more = [json.loads(ln) for ln in open(a.bench_lines) if ln.startswith("{")]
        both = {"order": [r["tag"] for r in more], "unit": "tok/s", "bench_py_steps": [r["steps"] for r in more if "steps" in r][:1]}
        for r in more:                                            # bench.py lines and `off` lines (their reps' medians), by arm
            for k, v in ({"bench_py": r["value"]} if "metric" in r else {k: float(np.median(v)) for k, v in r["tokens_per_s"].items()}).items():
                both.setdefault(k, {}).setdefault(r["tag"], []).append(float(v))
        for k, v in both.items():
            if isinstance(v, dict):
                v["mean"] = {t: float(np.mean(x)) for t, x in v.items()}
        out["a_further_visits_both_orders"] = both
    for r in runs:
        if r.get("part") == "onoff":
            med = {k: float(np.median(v)) for k, v in r["tokens_per_s"].items()}
            out["b_logprobs_on_against_off"] = dict(tokens_per_s_reps=r["tokens_per_s"], tokens_per_s_median=med,
                                                    one_stream_on_over_off=med["one_stream_on"] / med["one_stream_off"],
                                                    queue_on_over_off=med["queue_uniform_8_on"] / med["queue_uniform_8_off"],
                                                    one_stream_tokens_identical=r["one_stream_tokens_identical_on_and_off"],
                                                    queue_tokens_identical=r["queue_tokens_identical_on_and_off"])
            out["c_per_prompt_of_the_queue_workload"] = dict(seconds=r["per_prompt_seconds"], scores_get_score=r["scores_get_score"],
                                                             scores_from_loop=r["scores_from_loop"],
                                                             largest_score_difference=r["largest_score_difference"])
    if a.kernel_stats:
        for row in csv.DictReader(open(a.kernel_stats)):
            if "token_logprob_kernel" in row.get("Name", ""):
                out.setdefault("b_kernel_trace", []).append({k: row[k] for k in row if k in ("Name", "Calls", "TotalDurationNs", "AverageNs",
                                                                                                "MinNs", "MaxNs", "Percentage")})
    with open(a.json_out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
