#!/usr/bin/env python3
"""A/B of 4-bit weight records on the flagship benchmark: `python bench.py --gpus 1 --steps 20 --warmup 5` with SD_Q4=1 (the
quantised target streams records in its <= 8-row passes) against SD_Q4=dequantised (the same model, bf16 copy only),
alternated --rounds times in one visit to one GPU, each run a fresh process.  --rows adds a third arm, SD_Q4=rows (records
in the 9..80-row passes too, gemm_q4_rows), and --streams N runs every arm with N lock-step streams per step (bench.py
--batch-streams N: N x (gamma + 1) rows per verify pass).  Writes profiles/q4_ab.json: every run's tokens/s and verify
time, the medians, their ratios to the dequantised arm and that arm's own spread.

    python tools/q4_bench.py [--rows] [--streams 8] [--rounds 3] [--steps 20] [--warmup 5] [--timeout 600] [--out profiles/q4_ab.json]

A run that fails or exceeds its time limit ends the script: nothing more is started on the GPU."""
import argparse, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(env_q4, a):
    env = dict(os.environ)
    env.pop("SD_Q4", None)
    if env_q4:
        env["SD_Q4"] = env_q4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    if a.streams > 1:
        cmd += ["--batch-streams", str(a.streams)]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=a.timeout)
    if out.returncode != 0:
        sys.exit(f"bench.py (SD_Q4={env_q4}) exit {out.returncode}:\n{out.stderr[-2000:]}")
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    return {"value": r["value"], **{k: r["roofline"].get(k) for k in ("avg_launch_ms", "draft_step_avg_ms")}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--streams", type=int, default=1, help="lock-step streams per step (bench.py --batch-streams)")
    ap.add_argument("--rows", action="store_true", help="a third arm: SD_Q4=rows (records in the 9..80-row passes too)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q4_ab.json"))
    ap.add_argument("--default-arm", action="store_true", help="also run once with SD_Q4 unset (the bf16 model, 12-bit records)")
    a = ap.parse_args()
    arms = (("dequantised", "dequantised"), ("q4", "1")) + ((("rows", "rows"),) if a.rows else ())
    res = {"what": f"llama-68m -> Llama-2-13b (synthetic weights, 4-bit group-quantised at load), gamma 4, {a.streams} stream(s): "
                   "records (SD_Q4=1" + (", SD_Q4=rows" if a.rows else "") + ") against the same model on its bf16 copy "
                   "(SD_Q4=dequantised), alternated in one visit to one MI355X",
           "command": f"python bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}" + (f" --batch-streams {a.streams}" if a.streams > 1 else ""),
           "order": [], **{arm: [] for arm, _ in arms}}
    for i in range(a.rounds):
        for arm, env_q4 in arms:
            res["order"].append(f"{arm}_{i + 1}")
            res[arm].append(bench(env_q4, a))
            print(res["order"][-1], res[arm][-1], flush=True)
    if a.default_arm:
        res["SD_Q4_unset"] = bench(None, a)
        print("SD_Q4 unset", res["SD_Q4_unset"], flush=True)
    med = {arm: statistics.median(r["value"] for r in res[arm]) for arm, _ in arms}
    res["median_value"] = med
    res["ratio_of_medians"] = med["q4"] / med["dequantised"]
    if a.rows:
        res["rows_ratio_of_medians"] = med["rows"] / med["dequantised"]
        res["rows_lead_tok_s"] = med["rows"] - med["dequantised"]
    res["verify_ms"] = {arm: statistics.median(r["avg_launch_ms"] for r in res[arm]) for arm, _ in arms}
    res["dequantised_spread_tok_s"] = max(r["value"] for r in res["dequantised"]) - min(r["value"] for r in res["dequantised"])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["median_value"]), res["ratio_of_medians"], res.get("rows_ratio_of_medians"))
