#!/usr/bin/env python3
"""Times continuous batching (speculative_sampling_queue) against the calls of speculative_sampling_batch it replaces, on the
pair bench.py uses (llama-68m -> llama-2-13b, random-init weights through synth.py, bf16, device RNG, top_k 20 / top_p 0.9,
gamma 4, 8 slots).

    python tools/queue_bench.py [--workloads ragged,uniform --reps 5 --json-out profiles/queue_bench.json]
    python tools/queue_bench.py --workloads shared --json-out profiles/queue_bench_shared_prefix.json
    python tools/queue_bench.py --workloads mixed --json-out profiles/queue_bench_mixed_params.json

Decoding workloads, EOS off (every prompt generates its max_len):
  ragged   32 prompts with the lengths of harness.synthetic_prompts (bench.py --prompt-lens synthetic-c3), cut to what a
           slot's arenas hold, max_len alternating 32 / 128.  queue: one call, 8 slots.  batch: four calls of
           speculative_sampling_batch with 8 prompts each, in list order - each call runs until its slowest stream is done.
  uniform  8 prompts of 128 tokens, max_len 128: one queue call against one batch call.  The queue has nothing to admit
           after the start and must cost nothing: its median has to lie within the min-max spread of the batch reps.
  shared   (--workloads shared) 32 prompts, each one fixed 256-token prefix followed by the first <= 256 tokens of a ragged
           prompt, max_len alternating 32 / 128, 8 slots.  Both arms are speculative_sampling_queue_shared: shared_prefix=0 (every prompt forwards all
           its rows) against shared_prefix=256 (the prefix goes through the models once, the prompts copy its K / V rows).
           Per arm also the target rows forwarded for prompts.
  mixed    (--workloads mixed) the ragged prompts and budgets, but prompt i samples with class (i // 2) % 4 of MIXED_CLASSES - four
           different (temperature, top_k, top_p), one of them with top_k == 0; the budgets alternate with i, so every class
           holds four prompts of each budget (i % 4 would hand two classes the short budgets and two the long ones, and the
           per-class arm calls without a straggler that no real load gives it).  mixed_queue: ONE speculative_sampling_queue call
           with per-prompt parameter lists, 8 slots.  per_class_queues: what a caller had to do before the lists existed - four
           queue calls, one per class, each with that class's 8 prompts and scalar parameters, 8 slots.
  copy     (--workloads copy) no decoding: sd_session_copy_kv alone at the target's KV shape, 256 and 512 rows to 1 and 8
           destinations - device-event time per launch over 20 launches after 3 warm-up launches, and the bytes read plus
           the bytes written over that time.
  penalties (--workloads penalties --json-out profiles/penalties_ab.json) the uniform prompts through ONE
           speculative_sampling_queue_requests call per arm, 8 slots: penalties off, on for every prompt (repetition 1.2,
           frequency 0.5, presence 0.5) and on for every second prompt - in that arm every pass is a penalised pass (no tile
           maxima for anyone) but only half the rows are edited, which separates what the lost tile maxima cost from what the
           edit costs.  Also sd_penalize_rows alone at V = 32000 with 512-token histories, 8 items x 1 row (a draft step of 8
           streams) and 8 items x 5 rows (their verify): device-event time per launch, and gamma x the first + the second as
           the penalty launches' time per iteration.
  edits    (--workloads edits --json-out profiles/logit_edits_ab.json) the penalties workload's prompts and call, through
           speculative_sampling_queue_edits: off; every prompt edited (300 bias entries, an allowed mask of half the vocabulary,
           min_tokens 8); every prompt penalised (the `all` arm above); both at once - which is still ONE launch per pass.
           Also sd_edit_rows alone at the shapes above, with the edits, and with the edits and the penalties, next to
           sd_penalize_rows.
Both arms run in this process, alternated rep by rep after one warm-up rep of each (which also loads every kernel); a rep is
the whole call or calls, prefill included, between two device synchronisations on the host clock.  Per arm: tokens/s per rep
and their median, iterations, passes over the target weights (verify passes plus prompt-only passes; for the batch arm the
prefill passes engine.batch_prefill packs plus one verify pass per iteration - 8 streams x 5 rows fit one) and the mean number
of streams per iteration.  The pass counts depend on the tokens alone (on how often a draft is accepted), not on the clock.
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
from llmspeculativesampling_amd.engine import SpecDecModel, MAX_PREFILL_ROWS  # noqa: E402
from llmspeculativesampling_amd.harness import synthetic_prompts  # noqa: E402
from llmspeculativesampling_amd.sampling import (speculative_sampling_batch, speculative_sampling_queue,  # noqa: E402
                                                 speculative_sampling_queue_edits, speculative_sampling_queue_requests,
                                                 speculative_sampling_queue_shared)

SLOTS, GAMMA = 8, 4
SHARED = 256                                                      # tokens of the `shared` workload's common prefix
PENALTY = (1.2, 0.5, 0.5)                                         # (repetition, frequency, presence) of `penalties`
EDIT_BIAS, EDIT_MIN_TOKENS = 300, 8                               # bias entries and min_tokens of `edits`; the mask allows every second id
MIXED_CLASSES = [(1.0, 20, 0.9), (0.7, 50, 0.95), (1.0, 0, 0.9), (1.3, 5, 0.0)]   # (temperature, top_k, top_p) of `mixed`


def prefill_passes(lens):
    """Passes engine.batch_prefill needs for prompts of these lengths (its greedy packing: 256 rows, 32 groups of 8 rows)."""
    passes = rows = groups = 0
    for n in (L - 1 for L in lens):
        if n <= 0:
            continue
        g = (n + 7) // 8
        if n > MAX_PREFILL_ROWS or g > 32:
            passes += (rows > 0) + (n + MAX_PREFILL_ROWS - 1) // MAX_PREFILL_ROWS
            rows = groups = 0
            continue
        if rows + n > MAX_PREFILL_ROWS or groups + g > 32:
            passes, rows, groups = passes + 1, 0, 0
        rows, groups = rows + n, groups + g
    return passes + (rows > 0)


def copy_bench(model, rows_list=(256, 512), dst_counts=(1, 8), warmup=3, launches=20):
    """sd_session_copy_kv alone: [{rows, destinations, us, bytes_moved, read_plus_write_GB_per_s}]."""
    import ctypes as C
    from llmspeculativesampling_amd._lib import lib, check, SdKvCopyItem
    from llmspeculativesampling_amd.engine import _stream
    cap = max(rows_list)
    src = model.new_session(cap)
    src.kv.normal_()
    dsts = [model.new_session(cap) for _ in range(max(dst_counts))]
    out = []
    for rows in rows_list:
        for n in dst_counts:
            items = (SdKvCopyItem * n)()
            for it, d in zip(items, dsts):
                it.dst, it.lo, it.hi = d.handle, 0, rows
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for i in range(warmup + launches):
                if i == warmup:
                    e0.record()
                check(lib.sd_session_copy_kv(src.handle, items, n, _stream()), "sd_session_copy_kv")
            e1.record()
            torch.cuda.synchronize()
            assert all(torch.equal(d.kv[:, :, :, :rows], src.kv[:, :, :, :rows]) for d in dsts[:n])
            us = e0.elapsed_time(e1) * 1e3 / launches
            moved = 2 * n * src.kv[:, :, :, :rows].numel() * src.kv.element_size()
            out.append(dict(rows=rows, destinations=n, us=us, bytes_moved=moved, read_plus_write_GB_per_s=moved / us * 1e-3))
    return out


def penalty_bench(V=32000, hist=512, shapes=((8, 1), (8, 5)), warmup=3, launches=50):
    """sd_penalize_rows alone: [{items, rows_per_item, rows, us}] (fp32 rows with the bf16 rounding pending, as a bf16 head
    leaves them) and the launches of one iteration of 8 streams at gamma GAMMA."""
    from llmspeculativesampling_amd._lib import lib, check, SdPenalty, SdPenaltyItem
    from llmspeculativesampling_amd.engine import _stream
    rows_max = max(n * r for n, r in shapes)
    x = torch.randn(rows_max, V, device="cuda")
    y = torch.empty_like(x)
    seqs = [torch.randint(0, V, (hist + 32,), dtype=torch.int32, device="cuda") for _ in range(max(n for n, _ in shapes))]
    out = []
    for n, r in shapes:
        items = (SdPenaltyItem * n)()
        for i, it in enumerate(items):
            setattr(it, "in", x[i * r].data_ptr())
            it.out, it.ld_in, it.ld_out, it.rows = y[i * r].data_ptr(), V, V, r
            it.seq, it.hist0, it.prompt_len, it.pen = seqs[i].data_ptr(), hist, hist // 2, SdPenalty(*PENALTY)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(warmup + launches):
            if i == warmup:
                e0.record()
            check(lib.sd_penalize_rows(items, n, V, 1, _stream()), "sd_penalize_rows")
        e1.record()
        torch.cuda.synchronize()
        out.append(dict(items=n, rows_per_item=r, rows=n * r, us=e0.elapsed_time(e1) * 1e3 / launches))
    return dict(V=V, history=hist, launches=out, us_per_iteration_8_streams=GAMMA * out[0]["us"] + out[1]["us"])


def edit_bench(V=32000, hist=512, shapes=((8, 1), (8, 5)), warmup=3, launches=50):
    """sd_edit_rows alone at penalty_bench's shapes: {arm: [{items, rows_per_item, rows, us}]} for the `edits` workload's
    edits alone and for edits and penalties together, and the launches of one iteration of 8 streams at gamma GAMMA."""
    from llmspeculativesampling_amd._lib import lib, check, SdLogitEdit, SdLogitEditItem, SdPenalty
    from llmspeculativesampling_amd.engine import _stream
    rows_max = max(n * r for n, r in shapes)
    x = torch.randn(rows_max, V, device="cuda")
    y = torch.empty_like(x)
    seqs = [torch.randint(0, V, (hist + 32,), dtype=torch.int32, device="cuda") for _ in range(max(n for n, _ in shapes))]
    ids = torch.arange(0, V, V // EDIT_BIAS, dtype=torch.int32, device="cuda")[:EDIT_BIAS].contiguous()
    vals = torch.randn(EDIT_BIAS, device="cuda")
    mask = torch.full(((V + 31) // 32,), 0x55555555, dtype=torch.int32, device="cuda")
    out = {}
    for arm, pen in (("edits", (1.0, 0.0, 0.0)), ("both", PENALTY)):
        res = []
        for n, r in shapes:
            items = (SdLogitEditItem * n)()
            for i, it in enumerate(items):
                setattr(it, "in", x[i * r].data_ptr())
                it.out, it.ld_in, it.ld_out, it.rows = y[i * r].data_ptr(), V, V, r
                it.seq, it.hist0, it.prompt_len, it.pen = seqs[i].data_ptr(), hist, hist // 2, SdPenalty(*pen)
                it.edit, it.eos_token_id = SdLogitEdit(ids.data_ptr(), vals.data_ptr(), EDIT_BIAS, mask.data_ptr(), hist), 2
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for i in range(warmup + launches):
                if i == warmup:
                    e0.record()
                check(lib.sd_edit_rows(items, n, V, 1, _stream()), "sd_edit_rows")
            e1.record()
            torch.cuda.synchronize()
            res.append(dict(items=n, rows_per_item=r, rows=n * r, us=e0.elapsed_time(e1) * 1e3 / launches))
        out[arm] = dict(launches=res, us_per_iteration_8_streams=GAMMA * res[0]["us"] + res[1]["us"])
    return dict(V=V, history=hist, bias_entries=EDIT_BIAS, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draft", default="llama-68m")
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--workloads", default="ragged,uniform")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-prompt", type=int, default=512, help="prompts are cut to this many tokens")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    dcfg, tcfg = load_config(a.draft), load_config(a.target)
    max_pos = min(dcfg.max_position_embeddings, tcfg.max_position_embeddings, a.max_prompt + 128 + GAMMA + 8)
    cut = max_pos - 128 - GAMMA - 8                               # a prompt and its slot fit
    dm = SpecDecModel.synthetic(dcfg, seed=1, dtype=torch.bfloat16, max_pos=max_pos)
    tm = SpecDecModel.synthetic(tcfg, seed=2, dtype=torch.bfloat16, max_pos=max_pos)
    kw = dict(gamma=GAMMA, top_k=20, top_p=0.9)
    work = {}
    if "ragged" in a.workloads:
        ps = [p[:, :cut].cuda() for p in synthetic_prompts(100, tcfg.vocab_size, seed=5)[:32]]
        work["ragged"] = (ps, [32 if i % 2 == 0 else 128 for i in range(32)])
    if "uniform" in a.workloads:
        ps = [torch.from_numpy(np.random.default_rng(100 + i).integers(3, tcfg.vocab_size, size=(1, 128))).cuda() for i in range(8)]
        work["uniform"] = (ps, [128] * 8)
    if "shared" in a.workloads:
        head = torch.from_numpy(np.random.default_rng(77).integers(3, tcfg.vocab_size, size=(1, SHARED)))
        ps = [torch.cat([head, p[:, :min(256, cut - SHARED)]], 1).cuda() for p in synthetic_prompts(100, tcfg.vocab_size, seed=5)[:32]]
        work["shared"] = (ps, [32 if i % 2 == 0 else 128 for i in range(32)])
    if "mixed" in a.workloads:
        ps = [p[:, :cut].cuda() for p in synthetic_prompts(100, tcfg.vocab_size, seed=5)[:32]]
        work["mixed"] = (ps, [32 if i % 2 == 0 else 128 for i in range(32)])
    out = {"config": {k: v for k, v in vars(a).items() if k != "json_out"}, "dtype": "bfloat16", "slots": SLOTS, "gamma": GAMMA,
           "workloads": {}}
    if "penalties" in a.workloads:
        ps = [torch.from_numpy(np.random.default_rng(100 + i).integers(3, tcfg.vocab_size, size=(1, 128))).cuda() for i in range(8)]
        work["penalties"] = (ps, [128] * 8)
        out["penalize_rows"] = penalty_bench()
        print(json.dumps({"penalize_rows": out["penalize_rows"]}), flush=True)
    if "edits" in a.workloads:
        ps = [torch.from_numpy(np.random.default_rng(100 + i).integers(3, tcfg.vocab_size, size=(1, 128))).cuda() for i in range(8)]
        work["edits"] = (ps, [128] * 8)
        out["penalize_rows"], out["edit_rows"] = penalty_bench(), edit_bench()
        print(json.dumps({"penalize_rows": out["penalize_rows"], "edit_rows": out["edit_rows"]}), flush=True)
    if "copy" in a.workloads:
        out["copy_kv"] = copy_bench(tm)
        print(json.dumps({"copy_kv": out["copy_kv"]}), flush=True)
    for name, (prompts, budgets) in work.items():
        lens = [int(p.shape[1]) for p in prompts]
        lens_b = budgets                                          # (the tokens a rep generates: every prompt its budget)

        def queue(seed0, **more):
            t = {}
            fn = speculative_sampling_queue_shared if more else speculative_sampling_queue
            outs = fn(prompts, dm, tm, -1, None, budgets, seeds=[seed0 + i for i in range(len(prompts))], slots=SLOTS, _timing=t,
                      **more, **kw)
            return outs, dict(iterations=t["iterations"], target_passes=t["target_passes"], extra_passes=t["extra_passes"],
                              mean_streams=float(np.mean([v[2] for v in t["verify"]])), prompt_rows=t["prompt_rows"])

        def batch(seed0):
            outs, iters, passes, streams = [], 0, 0, []
            for c in range(0, len(prompts), SLOTS):
                t = {}
                # a call takes one max_len: the longest budget of its prompts, every output cut to its own budget afterwards
                got = speculative_sampling_batch(prompts[c:c + SLOTS], dm, tm, -1, None, max(budgets[c:c + SLOTS]),
                                                 seeds=[seed0 + c + i for i in range(len(prompts[c:c + SLOTS]))], _timing=t, **kw)
                outs += [o[:, :L + m] for o, L, m in zip(got, lens[c:], budgets[c:])]
                iters += len(t["verify"])
                passes += len(t["verify"]) + prefill_passes(lens[c:c + SLOTS])
                streams += [v[2] for v in t["verify"]]
            return outs, dict(iterations=iters, target_passes=passes, extra_passes=None, mean_streams=float(np.mean(streams)))

        def mixed_queue(seed0):
            t = {}
            cls = [MIXED_CLASSES[(i // 2) % 4] for i in range(len(prompts))]
            outs = speculative_sampling_queue(prompts, dm, tm, -1, None, budgets, gamma=GAMMA, temperature=[c[0] for c in cls],
                                              top_k=[c[1] for c in cls], top_p=[c[2] for c in cls],
                                              seeds=[seed0 + i for i in range(len(prompts))], slots=SLOTS, _timing=t)
            return outs, dict(iterations=t["iterations"], target_passes=t["target_passes"], extra_passes=t["extra_passes"],
                              mean_streams=float(np.mean([v[2] for v in t["verify"]])), calls=1)

        def per_class_queues(seed0):
            outs, iters, passes, extra, streams = [None] * len(prompts), 0, 0, 0, []
            for c, (T, k, pp) in enumerate(MIXED_CLASSES):
                ids = [i for i in range(len(prompts)) if (i // 2) % 4 == c]
                t = {}
                got = speculative_sampling_queue([prompts[i] for i in ids], dm, tm, -1, None, [budgets[i] for i in ids], gamma=GAMMA,
                                                 temperature=T, top_k=k, top_p=pp, seeds=[seed0 + i for i in ids], slots=SLOTS, _timing=t)
                for i, o in zip(ids, got):
                    outs[i] = o
                iters, passes, extra = iters + t["iterations"], passes + t["target_passes"], extra + t["extra_passes"]
                streams += [v[2] for v in t["verify"]]
            return outs, dict(iterations=iters, target_passes=passes, extra_passes=extra, mean_streams=float(np.mean(streams)),
                              calls=len(MIXED_CLASSES))

        def requests(seed0, on):
            t = {}
            cols = [[PENALTY[j] if i in on else (1.0, 0.0, 0.0)[j] for i in range(len(prompts))] for j in range(3)]
            pen = dict(repetition_penalty=cols[0], frequency_penalty=cols[1], presence_penalty=cols[2]) if on else {}
            outs = speculative_sampling_queue_requests(prompts, dm, tm, -1, None, budgets, seeds=[seed0 + i for i in range(len(prompts))],
                                                       slots=SLOTS, _timing=t, **pen, **kw)
            return outs, dict(iterations=t["iterations"], target_passes=t["target_passes"], extra_passes=t["extra_passes"],
                              mean_streams=float(np.mean([v[2] for v in t["verify"]])), penalised_prompts=len(on))

        def edited(seed0, edits, pens):
            t = {}
            V = tcfg.vocab_size
            more = dict(repetition_penalty=PENALTY[0], frequency_penalty=PENALTY[1], presence_penalty=PENALTY[2]) if pens else {}
            if edits:
                rng = np.random.default_rng(9)
                more.update(logit_bias={int(i): float(b) for i, b in zip(rng.choice(V, size=EDIT_BIAS, replace=False), rng.standard_normal(EDIT_BIAS))},
                            allowed_token_ids=list(range(0, V, 2)), min_tokens=EDIT_MIN_TOKENS)
            outs = speculative_sampling_queue_edits(prompts, dm, tm, -1, None, budgets, seeds=[seed0 + i for i in range(len(prompts))],
                                                    slots=SLOTS, _timing=t, **more, **kw)
            return outs, dict(iterations=t["iterations"], target_passes=t["target_passes"], extra_passes=t["extra_passes"],
                              mean_streams=float(np.mean([v[2] for v in t["verify"]])), edited=bool(edits), penalised=bool(pens))

        arms = {"queue": queue, "batch": batch}
        if name == "edits":
            arms = {"off": lambda seed0: edited(seed0, False, False), "edits": lambda seed0: edited(seed0, True, False),
                    "penalties": lambda seed0: edited(seed0, False, True), "both": lambda seed0: edited(seed0, True, True)}
        if name == "penalties":
            arms = {"off": lambda seed0: requests(seed0, ()), "all": lambda seed0: requests(seed0, range(len(prompts))),
                    "half": lambda seed0: requests(seed0, range(0, len(prompts), 2))}
        if name == "mixed":
            arms = {"mixed_queue": mixed_queue, "per_class_queues": per_class_queues}
        if name == "shared":
            arms = {"shared_prefix_0": lambda seed0: queue(seed0, shared_prefix=0),
                    f"shared_prefix_{SHARED}": lambda seed0: queue(seed0, shared_prefix=SHARED)}
        stats = {}
        for arm, fn in arms.items():                               # warm-up of every shape
            stats[arm] = fn(1000)[1]
        torch.cuda.synchronize()
        rates = {arm: [] for arm in arms}
        for r in range(a.reps):
            for arm, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs, st = fn(2000 + 100 * r)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                # the useful tokens: what each prompt asked for (an iteration may overshoot max_len by up to gamma)
                rates[arm].append(sum(min(o.shape[1] - L, m) for o, L, m in zip(outs, lens, budgets)) / dt)
                stats[arm] = st
        res = {arm: dict(stats[arm], tokens_per_s_reps=v, tokens_per_s_median=float(np.median(v))) for arm, v in rates.items()}
        if name == "mixed":
            res["classes"] = [dict(temperature=T, top_k=k, top_p=pp) for T, k, pp in MIXED_CLASSES]
            res["mixed_over_per_class_tokens_per_s"] = res["mixed_queue"]["tokens_per_s_median"] / \
                res["per_class_queues"]["tokens_per_s_median"]
        elif name == "penalties":
            res["penalty"] = dict(zip(("repetition", "frequency", "presence"), PENALTY))
            for arm in ("all", "half"):
                res[f"{arm}_over_off_tokens_per_s"] = res[arm]["tokens_per_s_median"] / res["off"]["tokens_per_s_median"]
                res[f"{arm}_ms_per_iteration_over_off"] = 1e3 * sum(lens_b) * (
                    1 / res[arm]["tokens_per_s_median"] / res[arm]["iterations"] - 1 / res["off"]["tokens_per_s_median"] / res["off"]["iterations"])
        elif name == "edits":
            res["penalty"] = dict(zip(("repetition", "frequency", "presence"), PENALTY))
            res["edit"] = dict(bias_entries=EDIT_BIAS, allowed="every second id", min_tokens=EDIT_MIN_TOKENS)
            for arm in ("edits", "penalties", "both"):
                res[f"{arm}_over_off_tokens_per_s"] = res[arm]["tokens_per_s_median"] / res["off"]["tokens_per_s_median"]
                res[f"{arm}_ms_per_iteration"] = 1e3 * sum(lens_b) / res[arm]["tokens_per_s_median"] / res[arm]["iterations"]
            res["off_ms_per_iteration"] = 1e3 * sum(lens_b) / res["off"]["tokens_per_s_median"] / res["off"]["iterations"]
        elif name == "shared":
            res["shared_over_plain_tokens_per_s"] = res[f"shared_prefix_{SHARED}"]["tokens_per_s_median"] / \
                res["shared_prefix_0"]["tokens_per_s_median"]
        else:
            res["queue_over_batch_tokens_per_s"] = res["queue"]["tokens_per_s_median"] / res["batch"]["tokens_per_s_median"]
            res["queue_median_within_batch_spread"] = bool(min(rates["batch"]) <= res["queue"]["tokens_per_s_median"] <= max(rates["batch"]))
        res["prompt_lens"], res["max_len"] = lens, budgets
        out["workloads"][name] = res
        print(json.dumps({name: res}), flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
