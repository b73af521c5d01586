#!/usr/bin/env python3
"""Workload for a kernel trace of the per-layer GEMMs of a many-row pass on a q4 model: two layers of Llama-2-13b's widths
(hidden 5120, intermediate 13824, 40 heads; synthetic weights, quantised at load), one 8-row prefill, then --reps passes of
--rows rows at the same positions.  SD_Q4 picks the arm: `dequantised` (gemm_bf16_rows / gemm_bf16_mm on the bf16 copy) or
`rows` (gemm_q4_rows on the records).  Run it under the tracer, one process per (arm, row count):

    SD_Q4=rows rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/q4_rows_trace.py --rows 40
    python tools/trace_by_grid.py DIR/.../t_kernel_trace.csv 60
"""
import argparse, os, sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llmspeculativesampling_amd.config import ModelConfig  # noqa: E402
from llmspeculativesampling_amd.engine import SpecDecModel  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    cfg = ModelConfig(arch="llama", vocab_size=4096, hidden_size=5120, intermediate_size=13824, num_hidden_layers=2,
                      num_attention_heads=40, num_key_value_heads=40, max_position_embeddings=512, rms_norm_eps=1e-5)
    m = SpecDecModel.synthetic(cfg, seed=5, dtype=torch.bfloat16, max_pos=256)
    ses = m.new_session(256)
    ids = torch.from_numpy(np.random.default_rng(1).integers(3, cfg.vocab_size, size=256)).to(torch.int32).cuda()
    ses.forward(ids[:8], 1)
    for _ in range(a.reps):
        ses.rollback(8)
        ses.forward(ids[8:8 + a.rows], 1)
    torch.cuda.synchronize()
    print("q4", m.q4, "rows route", m.q4_rows, "record launches", ses.q4_launches())
