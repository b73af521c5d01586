#!/usr/bin/env python3
"""What token scoring costs: the kernel beside token_logprob_kernel, and quality.score_tokens against quality.get_score.

    python tools/score_bench.py [--target llama-2-13b] [--tokens 1024] [--reps 5] --json-out profiles/score_tokens.json

  kernel  score_rows_kernel per launch at 80 rows x V (the target's vocabulary, 32000), bf16-round mode, top_n 0 / 5 / 20 - with
          and without the rank - beside token_logprob_kernel on the same rows (5 items x 16 rows: it takes 17 rows per item),
          each between two device events around `--launches` launches after a warm-up; and the 80-row pass of the target
          (random-init weights through synth.py, bf16) that such a launch follows in sd_score_sequence, timed the same way.
  e2e     score_tokens(top_n=0) against get_score on one `--tokens`-token sequence, arms alternated rep by rep in this one
          process, a rep between two device synchronisations on the host clock after one warm-up of every arm; medians, each
          arm's min-max spread, and each arm's peak device memory over its own allocations (torch.cuda.max_memory_allocated
          less what was allocated when the arm started).  The same run once more with top_n = 20.
The rows of the kernel part are Gaussian at scale 3 rounded through bf16 by the kernel's mode; the tokens are seeded."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 80


def _events_us(fn, launches):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernel_part(tm, V, launches):
    import torch
    from llmspeculativesampling_amd import _lib
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(7)
    slab = (torch.randn((ROWS, V), generator=g) * 3.0).cuda()
    tok = torch.randint(0, V, (ROWS,), generator=g, dtype=torch.int32).cuda()
    lp = torch.empty(ROWS, dtype=torch.float32, device="cuda")
    rank = torch.empty(ROWS, dtype=torch.int32, device="cuda")
    ids = torch.empty((ROWS, 20), dtype=torch.int32, device="cuda")
    tlp = torch.empty((ROWS, 20), dtype=torch.float32, device="cuda")
    mode = _lib.SD_NORM_ROUND_BF16
    out = {"rows": ROWS, "V": V, "mode": "bf16 round", "launches_per_figure": launches, "unit": "us per launch"}

    def score(top_n, with_rank):
        it = (_lib.SdScoreItem * 1)()
        it[0].logits, it[0].ld, it[0].rows, it[0].tokens, it[0].logprob = slab.data_ptr(), V, ROWS, tok.data_ptr(), lp.data_ptr()
        it[0].rank = rank.data_ptr() if with_rank else None
        it[0].top_ids, it[0].top_logprobs = (ids.data_ptr(), tlp.data_ptr()) if top_n else (None, None)
        return lambda: _lib.check(lib.sd_score_rows(it, 1, V, top_n, mode, st), "sd_score_rows")

    old = (_lib.SdLogprobItem * 5)()
    for i, it in enumerate(old):
        it.logits, it.ld, it.rows = slab.data_ptr() + 4 * 16 * i * V, V, 16
        it.tokens, it.res, it.out = tok.data_ptr() + 4 * 16 * i, None, lp.data_ptr() + 4 * 16 * i
    out["token_logprob_kernel"] = _events_us(lambda: _lib.check(lib.sd_token_logprobs(old, 5, V, mode, st), "sd_token_logprobs"), launches)
    for top_n in (0, 5, 20):
        out[f"score_rows_kernel_top_{top_n}"] = _events_us(score(top_n, True), launches)
        out[f"score_rows_kernel_top_{top_n}_no_rank"] = _events_us(score(top_n, False), launches)
    # the pass a launch follows: 80 rows, all of them logit rows, behind a 512-token context
    ses = tm.new_session(1024)
    ctx = torch.randint(3, V, (512 + ROWS,), generator=g, dtype=torch.int32).cuda()
    ses.forward(ctx[:512], 1)
    rows = min(ROWS, ses.max_pass_rows)

    def one_pass():
        _lib.check(lib.sd_session_forward(ses.handle, ctx.data_ptr() + 4 * 512, rows, 512, rows, ses.logits.data_ptr(),
                                          ses.logits.stride(0), st), "sd_session_forward")
    out["pass_rows"] = rows
    out["target_pass_of_those_rows"] = _events_us(one_pass, max(10, launches // 10))
    for top_n in (0, 5, 20):
        out[f"score_rows_kernel_top_{top_n}_share_of_the_pass"] = out[f"score_rows_kernel_top_{top_n}"] / out["target_pass_of_those_rows"]
    return out


def e2e_part(tm, V, tokens, reps):
    import torch
    from llmspeculativesampling_amd import quality
    seq = torch.from_numpy(np.random.default_rng(11).integers(3, V, size=(1, tokens))).cuda()
    arms = {"get_score": lambda: quality.get_score(seq, tm, 1),
            "score_tokens_top_0": lambda: quality.score_tokens(seq, tm, 1, 0).logprobs.mean(),
            "score_tokens_top_20": lambda: quality.score_tokens(seq, tm, 1, 20).logprobs.mean()}
    secs, peak, value = {k: [] for k in arms}, {}, {}
    for k, fn in arms.items():                                    # warm-up of every arm, and its peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        value[k] = float(fn())
        torch.cuda.synchronize()
        peak[k] = int(torch.cuda.max_memory_allocated() - base)
    for _ in range(reps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in secs.items()}
    spread = {k: float(max(v) - min(v)) for k, v in secs.items()}
    return {"tokens": tokens, "reps": reps, "unit": "s per call", "seconds": secs, "median": med, "min_max_spread": spread,
            "score": value, "peak_bytes_over_the_arm": peak,
            "native_minus_get_score": med["score_tokens_top_0"] - med["get_score"],
            "native_within_get_scores_spread": bool(med["score_tokens_top_0"] - med["get_score"] <= spread["get_score"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--tokens", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("score_bench.py measures on the GPU: no device found")
    from llmspeculativesampling_amd.config import load_config
    from llmspeculativesampling_amd.engine import SpecDecModel
    cfg = load_config(a.target)
    tm = SpecDecModel.synthetic(cfg, seed=2, dtype=torch.bfloat16, max_pos=max(a.tokens, 1024) + 8)
    out = {"what": f"{a.target} layer shape, random-init weights, bf16; one MI355X, one process",
           "kernel": kernel_part(tm, cfg.vocab_size, a.launches),
           "end_to_end": e2e_part(tm, cfg.vocab_size, a.tokens, a.reps)}
    text = json.dumps(out, indent=1, sort_keys=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
