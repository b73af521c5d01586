"""Adversarial logit rows for sd_token_logprobs and their float64 truth (CPU only, no GPU needed).

Shared by tests/test_logprobs_cpu.py (the truth against a direct float64 computation) and tests/test_gpu_logprobs.py (the
kernel and the loops against it).  Nothing here comes from the kernel: rows are seeded, the truth is torch.log_softmax in
float64 of the row after the rounding to the dtype the kernel's mode names (sampler_rows.as_dtype)."""
import functools

import numpy as np
import torch

from golden_io import logits_row
from sampler_rows import NEG, as_dtype

KINDS = ("gauss", "equal", "max_last", "pm80", "spike", "neg_inf")
BAR = 2.0 ** -17          # |got - want| <= BAR * max(1, |want|): twice a fast exp's error within 32 of the maximum (the issue's derivation)


def row(kind, seed, V):
    """One fp32 row of V logits (1-D)."""
    rng = np.random.default_rng([seed, V, 31])
    if kind == "gauss":                                           # Gaussian at scale 3
        return logits_row(seed, V, 3.0)[0]
    if kind == "equal":                                           # the truth is -log V at every token
        return torch.full((V,), 1.25)
    if kind == "max_last":                                        # the maximum in the last column
        x = logits_row(seed, V, 3.0)[0]
        x[V - 1] = x.max() + 2.0
        return x
    if kind == "pm80":                                            # a sum without the running maximum overflows
        return torch.from_numpy(np.where(rng.random(V) < 0.5, np.float32(80.0), np.float32(-80.0)).astype(np.float32))
    if kind == "spike":                                           # one entry 60 above the rest
        x = logits_row(seed, V, 1.0)[0]
        x[int(rng.integers(1, V - 1))] = x.max() + 60.0
        return x
    if kind == "neg_inf":                                         # some entries carry no mass
        x = logits_row(seed, V, 3.0)[0]
        x[torch.from_numpy(rng.choice(np.arange(1, V - 1), size=max(2, V // 7), replace=False))] = NEG
        return x
    raise KeyError(kind)


def tokens(kind, x):
    """Where a row of this kind is scored: column 0, the last column, the column before it (inside the scalar tail of every
    row whose tail has two entries), column 1 (inside a misaligned row's scalar head), the row's maximum, a column beside it -
    and, in a row with -inf entries, one of those."""
    V = x.numel()
    top = int(torch.argmax(x))
    toks = [0, V - 1, V - 2, 1, top, (top + 1) % V]
    if kind == "neg_inf":
        toks.append(int(torch.nonzero(torch.isinf(x))[0]))
    return toks


def truth(x, tok, dt):
    """float64 log-softmax at `tok` of the row as the kernel's rounding mode dt (0 fp32, 1 bf16, 2 f16) sees it."""
    return float(torch.log_softmax(as_dtype(x, dt).double(), dim=-1)[tok])


@functools.lru_cache(maxsize=None)
def pool(V, dt):
    """Every (kind, row, token, truth) of one vocabulary and rounding mode, computed once."""
    out = []
    for seed, kind in enumerate(KINDS):
        x = row(kind, 40 + seed, V)
        lsm = torch.log_softmax(as_dtype(x, dt).double(), dim=-1)
        out += [(kind, x, t, float(lsm[t])) for t in tokens(kind, x)]
    return out


def within_bar(got, want):
    if np.isinf(want):
        return got == want
    return abs(got - want) <= BAR * max(1.0, abs(want))
