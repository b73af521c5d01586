#!/usr/bin/env python3
"""What token-tree speculative sampling costs and gives: its two kernels alone, a tree iteration beside the chain iteration of
the same node count, and tokens/s with the mean accepted depth over the acceptance dial.

    python tools/tree_bench.py [--target llama-2-13b] [--draft llama-68m] --json-out profiles/tree_bench.json

  kernels    tree_draw_kernel (1 and 8 parent rows, b = 1 / 3 / 8) and tree_accept_kernel (the (3, 2, 1) and (7, 8) trees, device
             Philox, random rows and tokens; the accept tests made and the depth reached are recorded) at V = 32000, per launch
             between two device events around `--launches` launches after a warm-up.
  iteration  tree_speculative_sampling(branching=(3, 2, 1)), 16 nodes, beside speculative_sampling(gamma=15), 16 verify rows,
             on the random-init pair (nothing is accepted: an iteration emits one token).  tools/lookup_bench.py's protocol: host
             clock around a short and a long call, (t_long - t_short) / (iterations_long - iterations_short), arms alternated,
             medians and min-max spread.
  dial       synth.py's acceptance-dial pair (one target, one draft per sigma): tokens/s and mean accepted depth of the shapes
             (3, 2, 1), (2, 2, 2) and (4, 1, 1, 1) against the chain gamma = 4, same protocol.
Acceptance on real text is not measured here: the weights are random."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lookup_bench import _events_us, _steady  # noqa: E402

V_KERNEL = 32000
SHAPES = [(3, 2, 1), (2, 2, 2), (4, 1, 1, 1)]


def kernels_part(launches):
    import ctypes as C
    import torch
    from llmspeculativesampling_amd import _lib
    st, V = torch.cuda.current_stream().cuda_stream, V_KERNEL
    rows = torch.softmax(torch.randn((2, 64, V), device="cuda") * 2, -1)
    out = {"V": V, "launches_per_figure": launches, "unit": "us per launch", "draw": [], "accept": []}
    tok = torch.zeros((64, 8), dtype=torch.int32, device="cuda")
    for n_rows in (1, 8):
        for b in (1, 3, 8):
            us = _events_us(lambda: _lib.check(_lib.lib.sd_tree_draw(rows[1].data_ptr(), n_rows, V, V, b, None, None, 0, 5, 0,
                                                                     tok.data_ptr(), 8, st), "sd_tree_draw"), launches)
            out["draw"].append({"rows": n_rows, "b": b, "us": us})
    work, res = torch.empty(2 * V, device="cuda"), torch.zeros(C.sizeof(_lib.SdTreeResult), dtype=torch.uint8, device="cuda")
    for shape in ((3, 2, 1), (7, 8)):
        topo = _lib.SdTreeTopology()
        _lib.check(_lib.lib.sd_tree_topology_fill((C.c_int32 * len(shape))(*shape), len(shape), topo), "sd_tree_topology_fill")
        toks = torch.randint(0, V, (64,), dtype=torch.int32, device="cuda")
        us = _events_us(lambda: _lib.check(_lib.lib.sd_tree_accept(topo, toks.data_ptr(), rows[0].data_ptr(), rows[1].data_ptr(), V, V,
                                                                   work.data_ptr(), None, None, 5, 0, 99, res.data_ptr(), None, None,
                                                                   None, 0, st), "sd_tree_accept"), launches)
        torch.cuda.synchronize()
        r = _lib.SdTreeResult.from_buffer_copy(res.cpu().numpy().tobytes())
        out["accept"].append({"branching": list(shape), "us": us, "accept_tests": r.n_uniform, "accepted_depth": r.depth})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-2-13b")
    ap.add_argument("--draft", default="llama-68m")
    ap.add_argument("--context", type=int, default=128)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--short", type=int, default=16)
    ap.add_argument("--long", type=int, default=80)
    ap.add_argument("--sigmas", default="0.0,0.1,0.3")
    ap.add_argument("--json-out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        sys.exit("tree_bench.py measures on the GPU; none is visible")
    from llmspeculativesampling_amd.config import load_config
    from llmspeculativesampling_amd.engine import SpecDecModel
    from llmspeculativesampling_amd.noise import DeviceNoise
    from llmspeculativesampling_amd.synth import dial_draft_transform, dial_target_transform
    from llmspeculativesampling_amd import sampling as S

    result = {"device": torch.cuda.get_device_name(0), "target": args.target, "draft": args.draft, "dtype": "bf16, random-init",
              "sampling": "temperature 1, top_k 20, top_p 0.9", "context": args.context,
              "real_text_acceptance": "not measured: the weights are random"}
    result["kernels"] = kernels_part(args.launches)
    tcfg, dcfg = load_config(args.target), load_config(args.draft)
    max_pos = args.context + 2 * args.long + 128
    V = tcfg.vocab_size
    prompt = torch.from_numpy(np.random.default_rng(4).integers(3, V, size=(1, args.context))).cuda()
    L0, kw = prompt.shape[1], dict(temperature=1, top_k=20, top_p=0.9, details=True)

    def arms(dm, tm, shapes, gamma):
        def tree(shape):
            def fn(n):
                out, d = S.tree_speculative_sampling(prompt, dm, tm, -1, None, n, branching=shape, rng=DeviceNoise(7), **kw)
                fn.acc = d["acc_len"]
                return d["target_call_times"], out.shape[1] - L0
            return fn

        def chain(n):
            out, d = S.speculative_sampling(prompt, dm, tm, -1, None, n, gamma=gamma, rng=DeviceNoise(7), **kw)
            chain.acc = d["acc_len"]
            return d["target_call_times"], out.shape[1] - L0
        return {**{f"tree {s}": tree(s) for s in shapes}, f"chain gamma={gamma}": chain}

    tm = SpecDecModel.synthetic(tcfg, seed=2, dtype=torch.bfloat16, max_pos=max_pos)
    dm = SpecDecModel.synthetic(dcfg, seed=1, dtype=torch.bfloat16, max_pos=max_pos)
    result["iteration"] = _steady(arms(dm, tm, [(3, 2, 1)], 15), args.reps, args.short, args.long)
    del tm
    base = SpecDecModel.synthetic(dcfg, seed=11, dtype=torch.bfloat16, max_pos=max_pos, transform=dial_draft_transform(0.0, 11))
    tgt = SpecDecModel.synthetic(tcfg, seed=12, dtype=torch.bfloat16, max_pos=max_pos,
                                 transform=dial_target_transform(base._synth_get, dcfg.hidden_size, tcfg.hidden_size))
    result["dial"] = []
    for sg in [float(x) for x in args.sigmas.split(",")]:
        drf = base if sg == 0.0 else SpecDecModel.synthetic(dcfg, seed=11, dtype=torch.bfloat16, max_pos=max_pos,
                                                            transform=dial_draft_transform(sg, 11))
        a = arms(drf, tgt, SHAPES, 4)
        r = _steady(a, args.reps, args.short, args.long)
        for k, fn in a.items():
            r[k]["mean_accepted_depth"] = float(np.mean(fn.acc))
        result["dial"].append({"sigma": sg, "arms": r})
    print(json.dumps(result))
    if args.json_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.json_out)), exist_ok=True)
        with open(args.json_out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
