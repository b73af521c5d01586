"""Adversarial logit rows for sd_score_rows and their truth in numpy (CPU only, no GPU needed).

Shared by tests/test_score_cpu.py (quality.score_rows_torch against this truth) and tests/test_gpu_score.py (the kernel against
it).  Nothing here comes from the kernel: rows are seeded (logprob_rows.row and the kinds below), the order is
np.lexsort((ids, -x)) of the row after the rounding the kernel's mode names (sampler_rows.as_dtype) - value descending, ties to
the lower id, -0.0 == +0.0 - the rank is read from that order and the log-probabilities are a float64 log-softmax."""
import functools
import math

import numpy as np
import torch

import logprob_rows as LR
from golden_io import logits_row
from sampler_rows import NEG, as_dtype

MAX_TOP = 20
KINDS = LR.KINDS + ("ties", "signed_zero", "ascending", "descending", "ends", "few_finite")
VOID_KINDS = ("nan", "pos_inf", "all_neg_inf")
BAR, within_bar = LR.BAR, LR.within_bar


def row(kind, seed, V):
    """One fp32 row of V logits (1-D)."""
    if kind in LR.KINDS:
        return LR.row(kind, seed, V)
    rng = np.random.default_rng([seed, V, 53])
    if kind == "ties":                                            # 7 distinct values: the cut at every top_n falls inside a tie group
        vals = np.array([-3.0, -1.5, -0.25, 0.0, 0.75, 2.0, 2.5], dtype=np.float32)
        return torch.from_numpy(vals[rng.integers(0, 7, size=V)])
    if kind == "signed_zero":                                     # +0.0 and -0.0 mixed under a few positives
        x = np.where(rng.random(V) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        x[rng.choice(V, size=min(3, V - 1), replace=False)] = np.float32([1.5, 0.5, 2.25][:min(3, V - 1)])
        return torch.from_numpy(x)
    if kind == "ascending":                                       # the top sits in the scalar tail ...
        return logits_row(seed, V, 3.0)[0].sort().values.contiguous()
    if kind == "descending":                                      # ... or in the scalar head
        return logits_row(seed, V, 3.0)[0].sort(descending=True).values.contiguous()
    if kind == "ends":                                            # the largest entries split between the first 3 and the last 3 columns
        x = logits_row(seed, V, 2.0)[0].clamp(max=5.0)
        cols = [c for c in (0, V - 1, 1, V - 2, 2, V - 3) if 0 <= c < V]
        for j, c in enumerate(dict.fromkeys(cols)):
            x[c] = 9.0 + 0.5 * j
        return x
    if kind == "few_finite":                                      # the list runs into the -inf entries, ordered by id
        x = torch.full((V,), NEG)
        x[torch.from_numpy(rng.choice(V, size=min(3, V), replace=False))] = torch.tensor([0.5, -1.0, 2.0])[:min(3, V)]
        return x
    raise KeyError(kind)


def void_row(kind, seed, V):
    """A row whose log-sum is not finite."""
    x = logits_row(seed, V, 3.0)[0]
    if kind == "nan":
        x[V // 2] = float("nan")
    elif kind == "pos_inf":
        x[V // 3] = float("inf")
    elif kind == "all_neg_inf":
        x[:] = NEG
    else:
        raise KeyError(kind)
    return x


def stripes(seed, V, lanes=19):
    """A row that crowds the stripes of `lanes` of the kernel's 256 lanes (16-byte group g of a 16-byte-aligned row is read by
    lane g % 256): every entry of those stripes lies above every other entry, so with top_n > lanes the kernel's first threshold
    keeps all lanes * V / 256 of them."""
    rng = np.random.default_rng([seed, V, 59])
    x = rng.standard_normal(V, dtype=np.float32)
    hot = np.nonzero((np.arange(V) // 4) % 256 < lanes)[0]
    x[hot] = np.float32(10.0) + rng.permutation(hot.size).astype(np.float32) * np.float32(2.0 ** -10)
    return torch.from_numpy(x)


class Truth:
    """Of one row under rounding mode dt: the first MAX_TOP + 1 ids of the order, every id's rank and float64 log-probability."""

    def __init__(self, x, dt):
        xs = as_dtype(x, dt).to(torch.float32).numpy()
        V = xs.size
        order = np.lexsort((np.arange(V), -xs))
        self.V = V
        self.order = order[:MAX_TOP + 1].tolist()
        self.rank = np.empty(V, dtype=np.int64)
        self.rank[order] = np.arange(1, V + 1)
        x64 = xs.astype(np.float64)
        m = x64[np.isfinite(x64)].max()
        with np.errstate(divide="ignore"):
            self.logp = x64 - (m + math.log(np.exp(x64 - m).sum()))

    def top(self, top_n):
        """-> (ids, log-probabilities) of the top list, padded with -1 / NaN past V."""
        ids = self.order[:top_n]
        pad = top_n - len(ids)
        return ids + [-1] * pad, [float(self.logp[i]) for i in ids] + [math.nan] * pad

    def cut_tokens(self, top_n):
        """the id at the cut of the top list and the id just below it"""
        return [self.order[j] for j in (top_n - 1, top_n) if 0 <= j < min(self.V, len(self.order))]


def tokens(kind, x, tr, top_n):
    """Where a row is scored: the two ids at the cut first, then logprob_rows.tokens' columns."""
    return list(dict.fromkeys(tr.cut_tokens(top_n) + [t % x.numel() for t in LR.tokens(kind, x)]))


@functools.lru_cache(maxsize=None)
def pool(V, dt):
    """Every (kind, row, Truth) of one vocabulary and rounding mode, computed once; under dt = 1 a second Gaussian row, whose
    bf16 rounding makes ties."""
    kinds = list(enumerate(KINDS)) + ([(len(KINDS), "gauss")] if dt == 1 else [])
    out = []
    for seed, kind in kinds:
        x = row(kind, 140 + seed, V)
        out.append((kind, x, Truth(x, dt)))
    return out
