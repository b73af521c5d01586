"""Planted-key layouts at the block edges of the key-blocked matrix-core prefill attention (attn_prefill_blocked_kernel<T, D,
KV8>, prefill_attn.h) under SD_PREFILL_ATTN_BLOCK=128: helper of test_prefill_blocked_cpu.py and
test_gpu_prefill_attention_blocked.py; needs no GPU.  Models, cases and the registry fixture are prefill_probe_layouts'.

One call of n rows at pos0 (S = pos0 + n keys, logits of the last 64 rows), blocks of BLOCK = 128 keys:

  (256, 37)   S = 293: two whole blocks and a partial one of 37 keys; the edge 255 | 256 lies inside the logit tail;
  (256, 700)  S = 956: seven whole blocks and a partial one of 60 keys - the early row groups stop five blocks short of the
              last group; the edge 895 | 896 lies inside the logit tail;
  (200, 0)    S = 200: one whole block and a partial one of 72 keys with a ragged last V chunk;
  (256, 0)    S = 256: two whole blocks exactly - the stale slot behind the call is the first key of a block that is never
              visited, the last row's own key the last key of a block.

Classes: `block_edge` - the marker at the last / first key of a block (the first key of the last, partial block among them),
probed from the last row; `own` - the marker at a row's own position where that is a block's last or first key (the last key
the row may see); `forbidden` - its successor, probed from the row in front (a later row of the call, or the stale arena slot
behind the call): the rows up to the probed one must be bit-identical to the filler run."""
from typing import List

import attn_probe as P
from prefill_probe_layouts import CASES, CASE_IDS, TAIL, wide_models  # noqa: F401  (shared with the GPU file)

BLOCK = 128
CALLS = [(256, 37), (256, 700), (200, 0), (256, 0)]


def block_edges(S: int) -> List[int]:
    """Last and first key of every block edge inside 0 .. S - 1."""
    return [k for b in range(BLOCK, S, BLOCK) for k in (b - 1, b)]


def layouts() -> List[P.Layout]:
    out = []
    for n, pos0 in CALLS:
        S = pos0 + n
        for key in block_edges(S):
            out.append(P.Layout(S, n, key, n - 1, "block_edge"))
        for key in block_edges(S + 1):                             # (S + 1: the call's last key may be a block's last)
            r = key - pos0                                         # the row whose own position the edge key is
            if n - TAIL <= r < n:
                out.append(P.Layout(S, n, key, r, "own"))
            if n - TAIL <= r - 1 < n - 1:
                out.append(P.Layout(S, n, key, r - 1, "forbidden"))
        out.append(P.Layout(S, n, S, n - 1, "forbidden"))          # the stale arena slot behind the call's last row
    return out
