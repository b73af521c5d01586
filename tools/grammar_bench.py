#!/usr/bin/env python3
"""Measures what grammar-constrained decoding costs, on the pair bench.py uses (llama-68m -> llama-2-13b, random-init weights
through synth.py, bf16, device RNG, top_k 20 / top_p 0.9, gamma 4, 8 slots).

    python tools/grammar_bench.py --json-out profiles/grammar_ab.json [--parent-root DIR --reps 5]

Three measurements:
  kernel   grammar_rows_kernel (sd_grammar_rows) beside edit_rows_kernel (sd_edit_rows) on the same rows of 32000 logits with
           the same allowed mask: 8 items x 1 row (a draft step of 8 streams: 1 transition per row), 8 items x 5 rows (their
           verify: up to 5 transitions) and 8 items x 17 rows (up to 17 transitions, the launch's limit).  Device-event time
           per launch; the two kernels alternate in blocks of LAUNCHES launches, ROUNDS times, and each reports its median
           block.  The difference is what the walk and the second mask cost inside the launch - the number that decides
           whether the walk stays in the launch or moves to a prologue launch (which would cost a launch of its own, ~5 us).
  queue    the 8-slot queue on 8 prompts of 128 tokens, max_len 128, EOS off, one speculative_sampling_queue_grammar call per
           arm: `plain` (no block at all), `edited` (the edited pass without a grammar: min_tokens = 1 with no EOS id floors
           nothing but keeps the edit block on), `free_grammar` (one state that allows every id: the edited pass plus the
           walk, the same tokens as `edited`) and `grammar_a` (a 5-state cycle over id mod 5 that allows 2 - 3 classes per
           state).  Arms alternate rep by rep after one warm-up rep each; a rep is the whole call, prefill included, between
           two device synchronisations on the host clock.  Per arm tokens/s per rep, their median, iterations and ms per
           iteration.
  parent   (with --parent-root DIR, a checkout of the parent commit with its library built) the `plain` arm alone in fresh
           processes that alternate between DIR's package and this tree's, PROCS of each: a call without a grammar and without a
           block runs the parent's device code, so the two must lie inside each other's run-to-run spread.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS, GAMMA = 8, 4
LAUNCHES, ROUNDS, PROCS = 50, 5, 2


def grammar_a(V):
    """tests/test_grammar_cpu.py's grammar A: state s allows classes s, s + 1 (and s + 3 for even s) of id mod 5."""
    from llmspeculativesampling_amd.sampling import TokenGrammar
    nxt = np.full((5, 5), -1, dtype=np.int64)
    for s in range(5):
        for c in [s, (s + 1) % 5] + ([(s + 3) % 5] if s % 2 == 0 else []):
            nxt[s, c] = (s + 1) % 5
    return TokenGrammar(nxt, 0, None, V, classes=np.arange(V) % 5)


def kernel_bench(V=32000, hist=512, shapes=((8, 1), (8, 5), (8, 17))):
    """sd_grammar_rows beside sd_edit_rows: [{items, rows_per_item, rows, transitions, edit_rows_us, grammar_rows_us, walk_us}]."""
    from llmspeculativesampling_amd._lib import lib, check, SdGrammarItem, SdLogitEdit, SdLogitEditItem, SdPenalty
    from llmspeculativesampling_amd.engine import _stream
    g = grammar_a(V)
    dg = g.to_device("cuda")
    rows_max = max(n * r for n, r in shapes)
    x = torch.randn(rows_max, V, device="cuda")
    y = torch.empty_like(x)
    mask = torch.full(((V + 31) // 32,), 0x77777777, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(3)
    P = hist // 2
    j0 = hist - P                                                  # the first row's output number: a cached state in front of it
    seqs, states = [], []
    for i in range(max(n for n, _ in shapes)):
        out, s = [], g.start
        for _ in range(j0 + 32):                                   # a live path: every transition of the walk is taken
            t = int(rng.choice(g.allowed_ids(s)))
            out.append(t)
            s = g.step(s, t)
        seqs.append(torch.tensor(rng.integers(0, V, size=P).tolist() + out, dtype=torch.int32, device="cuda"))
        st = torch.zeros(j0 + 32, dtype=torch.int32, device="cuda")
        st[j0 - 1] = g.state_after(out[:j0 - 1])
        states.append(st)
    res = []
    for n, r in shapes:
        plain, gram = (SdLogitEditItem * n)(), (SdGrammarItem * n)()
        for i in range(n):
            for it in (plain[i], gram[i].row):
                setattr(it, "in", x[i * r].data_ptr())
                it.out, it.ld_in, it.ld_out, it.rows = y[i * r].data_ptr(), V, V, r
                it.seq, it.hist0, it.prompt_len, it.pen = seqs[i].data_ptr(), hist, P, SdPenalty(1.0, 0.0, 0.0)
                it.edit, it.eos_token_id = SdLogitEdit(None, None, 0, mask.data_ptr(), 0), -1
            gram[i].grammar, gram[i].states = dg.pointer(), states[i].data_ptr()
        calls = {"edit_rows": lambda: check(lib.sd_edit_rows(plain, n, V, 1, _stream()), "sd_edit_rows"),
                 "grammar_rows": lambda: check(lib.sd_grammar_rows(gram, n, V, 1, _stream()), "sd_grammar_rows")}
        for fn in calls.values():                                  # warm-up: loads both kernels
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(LAUNCHES):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
        e, gr = float(np.median(us["edit_rows"])), float(np.median(us["grammar_rows"]))
        res.append(dict(items=n, rows_per_item=r, rows=n * r, transitions=r, edit_rows_us=e, grammar_rows_us=gr, walk_us=gr - e,
                        edit_rows_us_blocks=us["edit_rows"], grammar_rows_us_blocks=us["grammar_rows"]))
    return dict(V=V, history=hist, launches_per_block=LAUNCHES, blocks=ROUNDS, shapes=res,
                walk_us_per_iteration_8_streams=GAMMA * res[0]["walk_us"] + res[1]["walk_us"])


def models(a):
    from llmspeculativesampling_amd.config import load_config
    from llmspeculativesampling_amd.engine import SpecDecModel
    dcfg, tcfg = load_config(a.draft), load_config(a.target)
    max_pos = min(dcfg.max_position_embeddings, tcfg.max_position_embeddings, 128 + 128 + GAMMA + 8)
    dm = SpecDecModel.synthetic(dcfg, seed=1, dtype=torch.bfloat16, max_pos=max_pos)
    tm = SpecDecModel.synthetic(tcfg, seed=2, dtype=torch.bfloat16, max_pos=max_pos)
    prompts = [torch.from_numpy(np.random.default_rng(100 + i).integers(3, tcfg.vocab_size, size=(1, 128))).cuda() for i in range(8)]
    return dm, tm, prompts, tcfg.vocab_size


def run_arms(arms, prompts, budgets, reps):
    lens = [int(p.shape[1]) for p in prompts]
    stats = {arm: fn(1000)[1] for arm, fn in arms.items()}         # warm-up of every shape
    torch.cuda.synchronize()
    rates = {arm: [] for arm in arms}
    for r in range(reps):
        for arm, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs, st = fn(2000 + 100 * r)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates[arm].append(sum(min(o.shape[1] - L, m) for o, L, m in zip(outs, lens, budgets)) / dt)
            stats[arm] = st
    res = {}
    for arm, v in rates.items():
        med = float(np.median(v))
        res[arm] = dict(stats[arm], tokens_per_s_reps=v, tokens_per_s_median=med,
                        ms_per_iteration=1e3 * sum(budgets) / med / stats[arm]["iterations"])
    return res


def plain_only(a):
    """The `plain` arm through speculative_sampling_queue (what the parent commit has too)."""
    from llmspeculativesampling_amd.sampling import speculative_sampling_queue
    dm, tm, prompts, _ = models(a)
    budgets = [128] * len(prompts)

    def plain(seed0):
        t = {}
        outs = speculative_sampling_queue(prompts, dm, tm, -1, None, budgets, gamma=GAMMA, top_k=20, top_p=0.9,
                                          seeds=[seed0 + i for i in range(len(prompts))], slots=SLOTS, _timing=t)
        return outs, dict(iterations=t["iterations"], target_passes=t["target_passes"])
    return run_arms({"plain": plain}, prompts, budgets, a.reps)["plain"]


def queue_bench(a):
    from llmspeculativesampling_amd.sampling import TokenGrammar, speculative_sampling_queue_grammar
    dm, tm, prompts, V = models(a)
    budgets = [128] * len(prompts)
    free = TokenGrammar(np.zeros((1, 1), dtype=np.int64), 0, None, V, classes=np.zeros(V, dtype=np.int64))
    A = grammar_a(V)

    def arm(**more):
        def fn(seed0):
            t = {}
            outs = speculative_sampling_queue_grammar(prompts, dm, tm, -1, None, budgets, gamma=GAMMA, top_k=20, top_p=0.9,
                                                      seeds=[seed0 + i for i in range(len(prompts))], slots=SLOTS, _timing=t, **more)
            return outs, dict(iterations=t["iterations"], target_passes=t["target_passes"],
                              mean_streams=float(np.mean([v[2] for v in t["verify"]])))
        return fn
    res = run_arms({"plain": arm(), "edited": arm(min_tokens=1), "free_grammar": arm(grammar=free), "grammar_a": arm(grammar=A)},
                   prompts, budgets, a.reps)
    for k in ("edited", "free_grammar", "grammar_a"):
        res[f"{k}_over_plain_tokens_per_s"] = res[k]["tokens_per_s_median"] / res["plain"]["tokens_per_s_median"]
    res["walk_ms_per_iteration"] = res["free_grammar"]["ms_per_iteration"] - res["edited"]["ms_per_iteration"]
    res["prompt_lens"], res["max_len"] = [int(p.shape[1]) for p in prompts], budgets
    return res


def parent_ab(a):
    """The plain queue in fresh processes, the parent's package and this tree's in turn."""
    runs = []
    for k in range(2 * PROCS):
        tree, root = ("parent", a.parent_root) if k % 2 == 0 else ("this", HERE)
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--package-root", root, "--reps", str(a.reps),
               "--draft", a.draft, "--target", a.target]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"{tree}: {p.stderr[-2000:]}")
        runs.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), tree=tree, order=k + 1))
        print(json.dumps(runs[-1]), flush=True)
    spread = {t: [min(min(r["tokens_per_s_reps"]) for r in runs if r["tree"] == t), max(max(r["tokens_per_s_reps"]) for r in runs if r["tree"] == t)]
              for t in ("parent", "this")}
    med = {t: float(np.median([r["tokens_per_s_median"] for r in runs if r["tree"] == t])) for t in ("parent", "this")}
    return dict(runs=runs, tokens_per_s_spread=spread, tokens_per_s_median=med,
                this_median_within_parent_spread=bool(spread["parent"][0] <= med["this"] <= spread["parent"][1]),
                parent_median_within_this_spread=bool(spread["this"][0] <= med["parent"] <= spread["this"][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draft", default="llama-68m")
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--package-root", default=HERE, help="where llmspeculativesampling_amd is imported from")
    ap.add_argument("--plain-only", action="store_true", help="the plain queue alone, one JSON line (what --parent-root spawns)")
    ap.add_argument("--skip", default="", help="comma list of kernel,queue")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    if a.plain_only:
        print(json.dumps(plain_only(a)), flush=True)
        return
    out = {"config": {k: v for k, v in vars(a).items() if k not in ("json_out", "package_root", "parent_root", "plain_only")},
           "dtype": "bfloat16", "slots": SLOTS, "gamma": GAMMA}
    if a.parent_root:                                              # first: no model of this process competes with the children's
        out["plain_queue_against_parent"] = parent_ab(a)
    if "kernel" not in a.skip:
        out["grammar_rows_device_events"] = kernel_bench()
        print(json.dumps({"grammar_rows_device_events": out["grammar_rows_device_events"]}), flush=True)
    if "queue" not in a.skip:
        out["queue"] = queue_bench(a)
        print(json.dumps({"queue": out["queue"]}), flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
