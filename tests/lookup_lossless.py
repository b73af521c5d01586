"""Losslessness of the prompt-lookup loops, as tests/lossless.py states it for the speculative ones: the first M tokens a loop
emits are distributed as M tokens of the TARGET's own sampling, whatever the lookup proposes.  Tree, pearson, ALPHA, the fixed
seed list and the bars are tests/lossless.py's (M = 4, gamma = 2); this helper adds what a drafter without a model needs:

  prompts    The existing prompts will not do - their proposals fall outside a top-3 support and nothing would ever be accepted.
             plant() writes an earlier occurrence of the prompt's last token into the prompt, followed by the target's most
             likely next token and the most likely token after that, and repeats until the planted tokens ARE those of the
             planted prompt (planting changes the target's conditionals).  condition() then computes exactly, from the tree's
             tables and the reference proposer, the probability that the first iteration accepts at least one draft and that it
             accepts both; a case is admissible at >= 0.25 and >= 0.05 (tests/test_lookup_cpu.py prints them).
  simulate   a numpy simulator of the lookup loop on the tree's tables with lossless.simulate's defect switch, to SIZE the tests;
             the GPU tests never compare against it.

Expected cells and bars come from the oracle only, never from the engine."""
import functools
import types

import numpy as np
import torch

import lookup_reference as R
import lossless as LL

GAMMA, M_TOKENS, NGRAM_MAX, NGRAM_MIN = LL.GAMMA, LL.M_TOKENS, 3, 1
DEFECTS = ("resample_p", "resample_abs", "bonus_prev_row")
P_ANY, P_BOTH = 0.25, 0.05

CASES = {
    #  name                          models  prompt (seed, len)  T    k   N
    "lookup_batch_fp32_filtered": dict(models="fp32", prompt=(2, 13), temperature=2.0, top_k=3, N=8000),
    "lookup_batch_bf16_plain": dict(models="bf16", prompt=(2, 24), temperature=1.0, top_k=0, N=8000),
    "lookup_single_fp32_filtered": dict(models="fp32", prompt=(2, 13), temperature=2.0, top_k=3, N=4000),
}
# the planted defects every case claims to catch: the simulator's X2 exceeds the bar at the case's N (test_lookup_cpu.py asserts
# it and prints the figures).  Not claimed, because a lookup loop has no such step or the case cannot see it: shared_uniform
# (as in lossless.py at these N), early_p and same_noise (no draft rows to read early, no draft noise to reuse).
CLAIMS = {name: DEFECTS for name in CASES}


def _target_logits(kind, prompt):
    _, _, tc, tsd = LL.models(kind)
    up = {k: v.float() for k, v in tsd.items()}
    return LL.logits_fn(tc, up, prompt), (LL.logits_fn(tc, tsd, prompt) if kind != "fp32" else None)


def plant(kind, prompt_key, temperature, top_k, rounds=6):
    """-> the planted prompt (1, L): prompt[1] = the last token, prompt[2], prompt[3] = the target's two most likely next
    tokens GIVEN the planted prompt (a fixed point of planting), or None if `rounds` plantings do not reach one."""
    _, _, tc, _ = LL.models(kind)
    prompt = LL.make_prompt(tc, *prompt_key).clone()
    prompt[0, 1] = prompt[0, -1]
    for _ in range(rounds):
        lf, _ = _target_logits(kind, prompt)
        pf = LL.probs_fn(lf, temperature, top_k)
        x1 = int(np.argmax(pf(())))
        x2 = int(np.argmax(pf((x1,))))
        if (int(prompt[0, 2]), int(prompt[0, 3])) == (x1, x2):
            return prompt
        prompt = prompt.clone()
        prompt[0, 2], prompt[0, 3] = x1, x2
    return None


def condition(tree, prompt):
    """Exact, from the tree's tables and the reference proposer: (P[first iteration accepts >= 1 draft], P[it accepts both])."""
    d, k, c = R.propose(prompt[0].numpy(), GAMMA, NGRAM_MAX, NGRAM_MIN)
    p1 = float(tree.P[0][d[0]])
    nxt = tree.child[0][d[0]]
    p2 = float(tree.P[nxt][d[1]]) if nxt >= 0 else 0.0
    return p1, p1 * p2, (d.tolist(), k, c)


def simulate(tree, prompt, N, rng, defect=None):
    """N runs of the lookup loop on the tree's tables: per iteration the reference proposer on prompt + emitted tokens, gamma
    accept tests (reject iff r > p[x] / 1), the residual norm(max(p - onehot_x, 0)) at the first reject or the bonus token from
    the next row.  defect: None, resample_p (the residual is p), resample_abs (|p - onehot|), bonus_prev_row.  -> (N, M) tokens,
    LL.OTHER behind a token that left the tree."""
    assert defect is None or defect in DEFECTS
    M, base = tree.M, [int(t) for t in prompt[0].tolist()]
    out = np.full((N, M), LL.OTHER, dtype=np.int64)
    # every run is at a tree node at an iteration's start; runs at the same node share the proposal
    work = [(0, np.arange(N), 0)]                                  # (node, run ids, tokens emitted so far)
    while work:
        node, idx, cnt = work.pop()
        drafted, _, _ = R.propose(base + list(tree.prefixes[node]), GAMMA, NGRAM_MAX, NGRAM_MIN)
        nd, alive = node, idx
        prev = tree.parent[node] if tree.parent[node] >= 0 else node   # the row before the current one (the root: itself)
        ended = []                                                # (run ids, token, node they emitted at, count before)
        for i in range(GAMMA):
            if len(alive) == 0 or cnt + i >= M:
                break
            x, p = int(drafted[i]), tree.P[nd]
            rej = rng.random(len(alive)) > p[x]
            if rej.any():
                onehot = np.zeros_like(p)
                onehot[x] = 1.0
                res = p.copy() if defect == "resample_p" else np.abs(p - onehot) if defect == "resample_abs" else np.maximum(p - onehot, 0.0)
                if res.sum() <= 0.0:
                    res = p.copy()
                ended.append((alive[rej], LL._draw(res, rng.random(int(rej.sum()))), nd, cnt + i))
            alive = alive[~rej]
            out[alive, cnt + i] = x                               # accepted: the drafted token is emitted
            nxt = tree.child[nd][x]
            if nxt < 0:                                           # it left the tree (or M tokens are out): the cell is decided
                alive = alive[:0]
                break
            prev, nd = nd, nxt
        else:
            if len(alive) and cnt + GAMMA < M:                    # all gamma accepted: the bonus token
                row = tree.P[prev] if defect == "bonus_prev_row" else tree.P[nd]
                ended.append((alive, LL._draw(row, rng.random(len(alive))), nd, cnt + GAMMA))
        for ids, toks, at, pos in ended:
            out[ids, pos] = toks
            if pos + 1 >= M:
                continue
            for t in np.unique(toks):
                nxt = tree.child[at][t]
                if nxt >= 0:
                    work.append((int(nxt), ids[toks == t], pos + 1))
    return out


@functools.lru_cache(maxsize=None)
def case(name, N=None):
    """Everything a test of CASES[name] needs, as lossless.case gives it: tree, planted prompt, dof, bar, lambda_ref."""
    c = dict(CASES[name])
    N = N or c["N"]
    T, k, kind = c["temperature"], c["top_k"], c["models"]
    prompt = plant(kind, c["prompt"], T, k)
    assert prompt is not None, (name, "planting did not reach a fixed point")
    tl, same = _target_logits(kind, prompt)
    tree = LL.Tree(LL.probs_fn(tl, T, k), None, M_TOKENS, filtered=k > 0)
    dof = LL._dof(tree.prob, N)
    lam, prob_same = 0.0, None
    if same is not None:
        prob_same = tree.cell_probs(LL.probs_fn(same, T, k))
        lam = LL.lambda_ref(tree.prob, prob_same, N)
    bar = LL.bar_fp32(dof) if same is None else LL.bar_16bit(dof, lam)
    return types.SimpleNamespace(name=name, N=N, tree=tree, prompt=prompt, dof=dof, bar=bar, lam=lam, prob_same=prob_same,
                                 temperature=T, top_k=k, kind=kind, gamma=GAMMA, M=M_TOKENS)
