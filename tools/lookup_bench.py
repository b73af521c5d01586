#!/usr/bin/env python3
"""What prompt-lookup drafting costs and gives: the proposer alone, the iteration beside the speculative iteration and the plain
step, the lock-step loop, and tokens/s where drafts are accepted.

    python tools/lookup_bench.py [--target llama-2-13b] [--draft llama-68m] --json-out profiles/lookup_bench.json

  proposer   lookup_propose_kernel per launch between two device events around `--launches` launches after a warm-up: L = 128 /
             1024 / 4096, 1 and 16 streams, gamma 4, V 32000, with a match (the last 3 tokens planted mid-sequence) and without
             (distinct tokens).  It replaces gamma draft steps of the draft model.
  iteration  prompt_lookup_sampling on the target (random-init weights through synth.py, bf16), speculative_sampling with the
             draft and autoregressive_sampling, all at the same context (`--context` random tokens: nothing matches, nothing
             is accepted, an iteration emits one token).  Per arm the host clock between two device synchronisations around a
             short and a long call (after a warm-up of both); (t_long - t_short) / (iterations_long - iterations_short) is the
             steady iteration, the prefill cancels.  Arms alternated rep by rep, medians and min-max spread.
  lockstep   prompt_lookup_sampling_batch with 8 and 16 streams on random prompts (acceptance 0): new tokens per second, the
             same difference of a long and a short call.
  dial       prompt_lookup_sampling on a prompt that repeats a block of tokens, top_k 20, at falling temperatures: a random-init
             target repeats itself only where the sampling is nearly greedy and its output falls into a cycle, so the
             temperature is the dial.  tokens/s, mean accepted length, mean match length per point.
Acceptance on real text is not measured here: the weights are random."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, V_PROPOSER = 4, 32000


def _events_us(fn, launches):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def proposer_part(launches):
    import torch
    from llmspeculativesampling_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    out = {"V": V_PROPOSER, "gamma": GAMMA, "ngram_max": 3, "ngram_min": 1, "launches_per_figure": launches, "unit": "us per launch",
           "points": []}
    for L in (128, 1024, 4096):
        for n in (1, 16):
            for match in (True, False):
                keep, items = [], (_lib.SdLookupItem * n)()
                for it in items:
                    s = np.arange(10, 10 + L)
                    if match:
                        s[L // 2 - 3:L // 2] = s[L - 3:]
                    seq = torch.zeros(L + GAMMA, dtype=torch.int32)
                    seq[:L] = torch.from_numpy(s.astype(np.int32))
                    seq = seq.cuda()
                    rows = torch.empty((GAMMA, V_PROPOSER), dtype=torch.float32, device="cuda")
                    info = torch.zeros(2, dtype=torch.int32, device="cuda")
                    it.seq, it.L, it.info = seq.data_ptr(), L, info.data_ptr()
                    it.q_hist = rows.data_ptr() - (L - 1) * V_PROPOSER * 4      # rows L-1 .. L+gamma-2 are the buffer's
                    keep.append((seq, rows, info))
                us = _events_us(lambda: _lib.check(_lib.lib.sd_lookup_propose(items, n, V_PROPOSER, V_PROPOSER, GAMMA, 3, 1, st),
                                                   "sd_lookup_propose"), launches)
                torch.cuda.synchronize()
                assert keep[0][2].tolist() == ([3, L // 2] if match else [0, L - 1]), keep[0][2].tolist()
                out["points"].append({"L": L, "streams": n, "match": match, "us": us})
    return out


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def _steady(arms, reps, short, long_):
    """arms: name -> fn(max_len) -> (iterations, new tokens).  -> name -> per-iteration ms and tokens/s of the steady state."""
    for fn in arms.values():
        fn(short), fn(long_)
    per = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ts, (its, toks) = _timed(lambda: fn(short))
            tl, (itl, tokl) = _timed(lambda: fn(long_))
            per[k].append(((tl - ts) / max(1, itl - its) * 1e3, (tokl - toks) / (tl - ts), itl - its, tokl - toks))
    out = {}
    for k, v in per.items():
        ms, tps = [x[0] for x in v], [x[1] for x in v]
        out[k] = {"iteration_ms": statistics.median(ms), "iteration_ms_min_max": [min(ms), max(ms)],
                  "tokens_per_s": statistics.median(tps), "tokens_per_s_min_max": [min(tps), max(tps)],
                  "iterations_in_window": v[-1][2], "tokens_in_window": v[-1][3]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--draft", default="llama-68m")
    ap.add_argument("--context", type=int, default=256)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--short", type=int, default=16)
    ap.add_argument("--long", type=int, default=80)
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("lookup_bench.py measures on the GPU; none is visible")
    from llmspeculativesampling_amd.config import load_config
    from llmspeculativesampling_amd.engine import SpecDecModel
    from llmspeculativesampling_amd.noise import DeviceNoise
    from llmspeculativesampling_amd import sampling as S

    result = {"device": torch.cuda.get_device_name(0), "target": args.target, "draft": args.draft, "dtype": "bf16, random-init",
              "gamma": GAMMA, "sampling": "temperature 1, top_k 20, top_p 0.9", "context": args.context,
              "real_text_acceptance": "not measured: the weights are random"}
    result["proposer"] = proposer_part(args.launches)
    tcfg, dcfg = load_config(args.target), load_config(args.draft)
    max_pos = args.context * 2 + args.long + 64
    tm = SpecDecModel.synthetic(tcfg, seed=2, dtype=torch.bfloat16, max_pos=max_pos)
    dm = SpecDecModel.synthetic(dcfg, seed=1, dtype=torch.bfloat16, max_pos=max_pos)
    V = tcfg.vocab_size
    rng = np.random.default_rng(4)
    prompt = torch.from_numpy(rng.permutation(V - 3)[:args.context][None] + 3).cuda()        # distinct tokens: nothing matches
    kw = dict(gamma=GAMMA, temperature=1, top_k=20, top_p=0.9)
    L0 = prompt.shape[1]

    def lookup(n):
        out, d = S.prompt_lookup_sampling(prompt, tm, -1, None, n, details=True, rng=DeviceNoise(7), **kw)
        return d["target_call_times"], out.shape[1] - L0

    def spec(n):
        out, d = S.speculative_sampling(prompt, dm, tm, -1, None, n, details=True, rng=DeviceNoise(7), **kw)
        return d["target_call_times"], out.shape[1] - L0

    def ar(n):
        out = S.autoregressive_sampling(prompt, tm, n, -1, 1, 20, 0.9, rng=DeviceNoise(7))
        return n, out.shape[1] - L0
    result["iteration"] = _steady({"prompt_lookup_sampling": lookup, "speculative_sampling": spec, "autoregressive_sampling": ar},
                                  args.reps, args.short, args.long)
    it = result["iteration"]
    it["hopeless_iteration_over_plain_step"] = it["prompt_lookup_sampling"]["iteration_ms"] / it["autoregressive_sampling"]["iteration_ms"]

    result["lockstep"] = {}
    for B in (8, 16):
        prompts = [torch.from_numpy(rng.permutation(V - 3)[:128][None] + 3).cuda() for _ in range(B)]

        def batch(n, prompts=prompts):
            outs, ds = S.prompt_lookup_sampling_batch(prompts, tm, -1, None, n, details=True, seeds=list(range(50, 50 + len(prompts))), **kw)
            return max(d["target_call_times"] for d in ds), sum(o.shape[1] - 128 for o in outs)
        r = _steady({"b": batch}, max(2, args.reps // 2), args.short, args.long)["b"]
        r["mean_accept_len"] = 0.0
        result["lockstep"][f"{B}_streams"] = r

    block = rng.permutation(V - 3)[:32] + 3
    rep = torch.from_numpy(np.tile(block, 8)[None]).cuda()
    points = []
    for T in (1.0, 0.5, 0.2, 0.05):
        def dial(n, T=T):
            out, d = S.prompt_lookup_sampling(rep, tm, -1, None, n, gamma=GAMMA, temperature=T, top_k=20, top_p=0.9, details=True,
                                              rng=DeviceNoise(9))
            dial.last = d
            return d["target_call_times"], out.shape[1] - rep.shape[1]
        r = _steady({"d": dial}, max(2, args.reps // 2), args.short, 2 * args.long)["d"]
        d = dial.last
        r.update(temperature=T, mean_accept_len=float(np.mean(d["acc_len"])), mean_match_len=float(np.mean(d["match_len"])))
        points.append(r)
    result["dial"] = {"prompt": "a block of 32 distinct tokens, 8 times", "points": points}
    line = json.dumps(result)
    print(line)
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
