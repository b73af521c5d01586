"""What "speculative sampling is lossless" means, as something a test can hold a decode loop to: the first M tokens a loop
emits are distributed exactly as M tokens of the TARGET model's own sampling, whatever the draft proposes.  This helper (in
the style of seam_probe.py / attn_probe.py; needs no GPU) holds

  Tree        the target's conditional next-token distributions on every prefix of fewer than M generated tokens, from the fp32
              oracle (oracle.RefCausalLM + oracle.norm_logits), evaluated lazily and cached; the exact probability of every
              cell is the product along its path.  Two cell schemes:
                filtered (top_k = k > 0)       a cell is the token M-tuple: at most k^M cells; any other tuple has mass 0
                plain    (top_k = 0, top_p = 0) a cell is a path of ranks {0, 1, 2} under the target's conditional that ends
                                                early in an absorbing "other" cell at the first token outside the top 3
  pearson     Pearson's X2 over the cells whose expected count is >= 8, the others pooled into one cell; a sample in a cell
              of expected mass 0 is reported apart (fp32: fails outright)
  simulate    a numpy speculative-sampling simulator over the same tables with a switch for planted defects.  It exists to
              SIZE the tests (which N shows which defect); the GPU tests never compare against it.
  CASES       every free choice of the GPU tests (prompt, temperature, k, gamma, M, N, seeds), fixed here and justified by
              tests/test_lossless_cpu.py on the oracle alone before any GPU run.

The expected cells always come from the fp32 oracle; for a 16-bit engine it runs on the 16-bit-rounded weights, and the
allowance for the engine's own rounding is lambda_ref below, measured on the oracle in that dtype - never on the engine.

Out of scope: multi_speculative_sampling(strategy="iid") and the beam variant.  The reference's "longest accepted replica
wins" rule is not distribution-preserving, so token parity with the oracle stays their check."""
import functools

import numpy as np
import torch

import oracle
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

MIN_EXPECTED = 8.0
ALPHA = 1e-9
RANKS = 3
OTHER = -1                                   # the absorbing cell of the plain scheme, as a token id in a cell's path
DEFECTS = ("resample_p", "resample_abs", "shared_uniform", "bonus_prev_row", "early_p", "same_noise")

# BF16_CFG of tests/test_gpu_native_parity.py (a test module cannot be imported from a helper without its GPU fixtures)
CFG16 = dict(arch="llama", vocab_size=8192, hidden_size=256, intermediate_size=704, num_hidden_layers=2,
             num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-6)


# ------------------------------------------------------------------------------------------------------------ models
def fp32_pair():
    """The tiny correlated pair of tests/test_gpu_native_parity.py:_pair("corr")."""
    cfg = load_config("tiny-llama-target")
    dsd = make_state_dict(cfg, 11)
    return cfg, dsd, cfg, perturb_state_dict(dsd, 12, 0.12)


def pair16(dtype):
    """BF16_CFG's pair as test_native_bf16_iteration_bit_equals_python_loop builds it, in bf16 or fp16."""
    cfg = ModelConfig(**CFG16)
    dsd = make_state_dict(cfg, 5, dtype=dtype)
    tsd = {k: v.to(dtype) for k, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    return cfg, dsd, cfg, tsd


def make_prompt(cfg, seed, length):
    return torch.from_numpy(np.random.default_rng(seed).integers(3, cfg.vocab_size, size=(1, length)))


def logits_fn(cfg, sd, prompt):
    """prefix (tuple of generated tokens) -> the model's last logit row as float64, through the oracle in sd's dtype."""
    model = oracle.RefCausalLM(cfg, sd)

    @functools.lru_cache(maxsize=None)
    def f(prefix):
        ids = torch.cat([prompt, torch.tensor([list(prefix)], dtype=prompt.dtype)], dim=1) if prefix else prompt
        return model(ids).logits[:, -1, :].float()
    return f


def probs_fn(lf, temperature, top_k, top_p=0.0):
    @functools.lru_cache(maxsize=None)
    def f(prefix):
        p = oracle.norm_logits(lf(prefix), temperature, top_k, top_p)[0].double().numpy()
        return p / p.sum()                           # the fp32 softmax sums to 1 within 1e-7; the cells must sum to exactly 1
    return f


# ------------------------------------------------------------------------------------------------------------ the tree
class Tree:
    """p_fn / q_fn: prefix tuple -> float64 probability vector over V (target / draft).  filtered: the cell scheme."""

    def __init__(self, p_fn, q_fn, M, filtered):
        self.p_fn, self.q_fn, self.M, self.filtered = p_fn, q_fn, M, filtered
        self.prefixes, self.index = [], {}
        self.tokens, self.child, self.parent = [], [], []
        self._add((), -1)
        i = 0
        while i < len(self.prefixes):                                  # breadth first: a node's id is below its children's
            pre = self.prefixes[i]
            p = p_fn(pre)
            if filtered:
                toks = np.flatnonzero(p > 0)
            else:
                toks = np.argsort(-p, kind="stable")[:RANKS]
            self.tokens.append(toks)
            ch = np.full(len(p), -1, dtype=np.int64)
            if len(pre) + 1 < M:
                for t in toks:
                    ch[t] = self._add(pre + (int(t),), i)
            self.child.append(ch)
            i += 1
        self.P = [p_fn(pre) for pre in self.prefixes]
        self.Q = [q_fn(pre) for pre in self.prefixes] if q_fn is not None else None
        self.cells, self.cell_index = [], {}
        self._enumerate((), 0)
        self.prob = self.cell_probs(p_fn)

    def _add(self, prefix, parent):
        self.index[prefix] = len(self.prefixes)
        self.prefixes.append(prefix)
        self.parent.append(parent)
        return len(self.prefixes) - 1

    def _enumerate(self, path, node):
        for t in self.tokens[node]:
            nxt = path + (int(t),)
            if len(nxt) == self.M:
                self._cell(nxt)
            else:
                self._enumerate(nxt, self.index[nxt])
        if not self.filtered:
            self._cell(path + (OTHER,))

    def _cell(self, path):
        self.cell_index[path] = len(self.cells)
        self.cells.append(path)

    def cell_probs(self, p_fn):
        """Exact cell probabilities when the conditionals are p_fn's (the cells stay this tree's)."""
        out = np.zeros(len(self.cells))
        for ci, path in enumerate(self.cells):
            pr = 1.0
            for d, t in enumerate(path):
                pre = path[:d]
                p = p_fn(pre)
                pr *= (1.0 - p[self.tokens[self.index[pre]]].sum()) if t == OTHER else p[t]
            out[ci] = pr
        return np.maximum(out, 0.0)

    def classify(self, samples):
        """samples: (N, >= M) token ids -> (counts per cell, number of samples in no cell [expected mass 0])."""
        counts, outside = np.zeros(len(self.cells), dtype=np.int64), 0
        member = [set(int(t) for t in toks) for toks in self.tokens]
        for row in np.asarray(samples)[:, :self.M].tolist():
            node, path = 0, ()
            for d, t in enumerate(row):
                if t not in member[node]:
                    path = None if self.filtered else path + (OTHER,)
                    break
                path = path + (t,)
                if d + 1 < self.M:
                    node = self.child[node][t]
            if path is None:
                outside += 1
            else:
                counts[self.cell_index[path]] += 1
        return counts, outside


# ------------------------------------------------------------------------------------------------------------ statistic
def pooled(prob, N):
    """(ids of the cells kept apart, ids of the pooled ones): expected count >= MIN_EXPECTED or not."""
    big = N * prob >= MIN_EXPECTED
    return np.flatnonzero(big), np.flatnonzero(~big)


def pool_vector(x, prob, N):
    keep, rest = pooled(prob, N)
    v = np.asarray(x, dtype=np.float64)
    return np.append(v[keep], v[rest].sum()) if len(rest) else v[keep]


def pearson(counts, outside, prob, N):
    """(X2, dof).  Cells with expected count >= 8 stand alone, the rest is one cell; samples in no cell (expected mass 0)
    count in that pooled cell, and X2 is inf when it has no expected mass to set them against."""
    keep, rest = pooled(prob, N)
    e, o = N * prob[keep], np.asarray(counts, dtype=np.float64)[keep]
    e_pool, o_pool = N * prob[rest].sum(), float(np.asarray(counts)[rest].sum() + outside)
    assert int(round(o.sum() + o_pool)) == N, (o.sum(), o_pool, N)
    if e_pool > 0.0:
        e, o = np.append(e, e_pool), np.append(o, o_pool)
    elif o_pool > 0:
        return float("inf"), len(e) - 1
    return float(((o - e) ** 2 / e).sum()), len(e) - 1


def _dof(prob, N):
    keep, rest = pooled(prob, N)
    return len(keep) + (1 if prob[rest].sum() > 0 else 0) - 1


def lambda_ref(prob, prob_same, N):
    """N * sum (p_same-dtype-oracle - p_fp32)^2 / p_fp32 over the statistic's cells: the noncentrality the same-dtype
    oracle's own rounding would give X2."""
    e, s = pool_vector(prob, prob, N), pool_vector(prob_same, prob, N)
    ok = e > 0
    return float(N * ((s[ok] - e[ok]) ** 2 / e[ok]).sum())


def bar_fp32(dof):
    from scipy import stats
    return float(stats.chi2.isf(ALPHA, dof))


def bar_16bit(dof, lam):
    """The 1 - 1e-9 quantile of the noncentral chi-square with noncentrality 2.25 * lambda_ref (the project's 1.5x error
    rule, squared)."""
    from scipy import stats
    return float(stats.ncx2.isf(ALPHA, dof, 2.25 * lam))


def independence(a, b, n_classes):
    """Pearson X2 of the n_classes x n_classes contingency table of two class sequences, on the table's own dof."""
    tab = np.zeros((n_classes, n_classes))
    np.add.at(tab, (np.asarray(a), np.asarray(b)), 1)
    tab = tab[tab.sum(1) > 0][:, tab.sum(0) > 0]
    e = np.outer(tab.sum(1), tab.sum(0)) / tab.sum()
    return float(((tab - e) ** 2 / e).sum()), (tab.shape[0] - 1) * (tab.shape[1] - 1), float(e.min())


# ------------------------------------------------------------------------------------------------------------ simulator
def _draw(prob_rows, u):
    """Inverse-CDF draw: prob_rows (V,) shared by all samples, u (n,) uniforms."""
    c = np.cumsum(prob_rows)
    return np.minimum(np.searchsorted(c / c[-1], u, side="right"), len(c) - 1)


def simulate(tree, gamma, N, rng, defect=None):
    """N runs of speculative sampling on the tree's tables: draft gamma tokens, accept-test each (reject iff r > p / q),
    resample the residual norm(max(p - q, 0)) at the first reject or draw the bonus token from the next row.  Returns the
    (N, M) emitted tokens (OTHER behind a token that left the tree: its cell is decided) and the accept-test counts
    (tests, accepts).  defect: None or one of DEFECTS
      resample_p       the residual is p itself
      resample_abs     the residual is |p - q|
      shared_uniform   one uniform serves the gamma accept tests of an iteration
      bonus_prev_row   the bonus token is drawn from the previous row's distribution
      early_p          the accept ratio reads p one history row early (the parent prefix's row)
      same_noise       the residual sample reuses the exponential noise the rejected draft token was drawn with"""
    assert defect is None or defect in DEFECTS
    M = tree.M
    out = np.full((N, M), OTHER, dtype=np.int64)
    cnt = np.zeros(N, dtype=np.int64)
    node = np.zeros(N, dtype=np.int64)
    done = np.zeros(N, dtype=bool)
    tests = accepts = 0

    def emit(idx, tok):
        """append tok to samples idx (all at the same node); returns nothing, updates node / cnt / done"""
        out[idx, cnt[idx]] = tok
        cnt[idx] += 1
        nxt = tree.child[node[idx[0]]][tok]
        # M tokens, or a token outside the tree: the cell is decided (plain: "other"; filtered: no cell at all)
        done[idx[(cnt[idx] >= M) | (nxt < 0)]] = True
        node[idx] = np.where(nxt < 0, node[idx], nxt)

    while not done.all():
        alive = ~done
        par = np.asarray(tree.parent)[node]
        prev = np.where(par >= 0, par, node)                              # the row before the current one (the root: itself)
        r_shared = rng.random(N)
        for _ in range(gamma):
            for nd in np.unique(node[alive]):
                idx = np.flatnonzero(alive & (node == nd))
                p, q = tree.P[nd], tree.Q[nd]
                if defect == "same_noise":
                    E = rng.exponential(size=(len(idx), len(q)))
                    x = np.argmax(q[None, :] / E, axis=1)
                else:
                    x = _draw(q, rng.random(len(idx)))
                p_use = tree.P[prev[idx[0]]] if defect == "early_p" else p
                ratio = p_use[x] / q[x]
                r = r_shared[idx] if defect == "shared_uniform" else rng.random(len(idx))
                rej = r > ratio
                tests += len(idx)
                accepts += int((~rej).sum())
                # --- rejected: residual resample, the iteration ends
                if rej.any():
                    ri = idx[rej]
                    res = p.copy() if defect == "resample_p" else np.abs(p - q) if defect == "resample_abs" else np.maximum(p - q, 0.0)
                    if res.sum() <= 0.0:
                        res = p.copy()
                    if defect == "same_noise":
                        t = np.argmax(res[None, :] / E[rej], axis=1)
                    else:
                        t = _draw(res, rng.random(len(ri)))
                    alive[ri] = False
                    emit(ri, t)
                # --- accepted: the drafted token is emitted, the scan goes on one row later
                ai = idx[~rej]
                if len(ai):
                    prev[ai] = nd
                    emit(ai, x[~rej])
                    alive[ai] &= ~done[ai]
        for nd in np.unique(node[alive]):                                 # all gamma accepted: the bonus token
            idx = np.flatnonzero(alive & (node == nd))
            row = tree.P[prev[idx[0]]] if defect == "bonus_prev_row" else tree.P[nd]
            emit(idx, _draw(row, rng.random(len(idx))))
    return out, (tests, accepts)


def simulate_ar(tree, N, rng):
    """The control: the target's own sampling on the same tables."""
    out = np.full((N, tree.M), OTHER, dtype=np.int64)
    node = np.zeros(N, dtype=np.int64)
    live = np.ones(N, dtype=bool)
    for d in range(tree.M):
        for nd in np.unique(node[live]):
            idx = np.flatnonzero(live & (node == nd))
            t = _draw(tree.P[nd], rng.random(len(idx)))
            nxt = tree.child[nd][t]
            out[idx, d] = t
            live[idx[nxt < 0]] = False
            node[idx] = np.where(nxt < 0, nd, nxt)
    return out


# ------------------------------------------------------------------------------------------------------------ the cases
# Every free choice of tests/test_gpu_lossless.py.  random_seed stays None in all of them: with a seed the reference
# reseeds before every uniform, so the gamma uniforms of an iteration are equal - that quirk IS the shared-uniform defect,
# and such runs do not preserve the distribution by design.  M >= gamma + 2 in all of them: the all-accept bonus token
# (position gamma + 1) and the first token of the next iteration (gamma + 2) are both observed.
GAMMA, M_TOKENS = 2, 4
SEED_BASE = 0x5EED0000                       # sample i of a case runs on Philox stream seed_base + i
HIGH_SEED_STEP = 1 << 32                     # the case whose seeds differ in the high word only: seed = 77 + i * 2^32

CASES = {
    #  name              models   prompt (seed, len)  T     k   N
    "fp32_filtered": dict(models="fp32", prompt=(5, 13), temperature=2.0, top_k=3, N=20000),
    "fp32_plain":    dict(models="fp32", prompt=(5, 13), temperature=1.0, top_k=0, N=20000),
    "bf16_plain":    dict(models="bf16", prompt=(3, 24), temperature=1.0, top_k=0, N=8000),
    "fp16_plain":    dict(models="fp16", prompt=(3, 24), temperature=1.0, top_k=0, N=8000),
    # one queue call with per-prompt parameters alternating between two requests (row_params): _a even, _b odd prompts
    "rows_fp32_a": dict(models="fp32", prompt=(5, 13), temperature=2.0, top_k=3, N=10000),
    "rows_fp32_b": dict(models="fp32", prompt=(5, 13), temperature=1.3, top_k=0, N=10000),
    "rows_bf16_a": dict(models="bf16", prompt=(3, 24), temperature=1.0, top_k=0, N=8000),
    "rows_bf16_b": dict(models="bf16", prompt=(3, 24), temperature=0.8, top_k=0, N=8000),
    "fp32_filtered_high_seeds": dict(models="fp32", prompt=(5, 13), temperature=2.0, top_k=3, N=4000),
    # 16 lock-step streams x N / 16 calls (speculative_sampling_batch and the autoregressive control)
    "batch_fp32_filtered": dict(models="fp32", prompt=(5, 13), temperature=2.0, top_k=3, N=8000),
    "batch_bf16_plain":    dict(models="bf16", prompt=(3, 24), temperature=1.0, top_k=0, N=8000),
    # one call per run (sd_spec_generate)
    "single_fp32_filtered": dict(models="fp32", prompt=(5, 13), temperature=2.0, top_k=3, N=4000),
    "single_bf16_plain":    dict(models="bf16", prompt=(3, 24), temperature=1.0, top_k=0, N=8000),
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=None)
def models(kind):
    """(cfg_d, sd_d, cfg_t, sd_t) in the engine's dtype."""
    return fp32_pair() if kind == "fp32" else pair16(DTYPES[kind])


@functools.lru_cache(maxsize=None)
def _logit_fns(kind, prompt_key):
    """(draft fp32-oracle logits, target fp32-oracle logits, target same-dtype-oracle logits or None, prompt)."""
    dc, dsd, tc, tsd = models(kind)
    prompt = make_prompt(tc, *prompt_key)
    up = lambda sd: {k: v.float() for k, v in sd.items()}                 # noqa: E731  (the 16-bit-rounded weights, in fp32)
    same = logits_fn(tc, tsd, prompt) if kind != "fp32" else None
    return logits_fn(dc, up(dsd), prompt), logits_fn(tc, up(tsd), prompt), same, prompt


@functools.lru_cache(maxsize=None)
def case(name, N=None):
    """Everything a test of CASES[name] needs: tree, prompt, dof, bar, lambda_ref (0 in fp32)."""
    import types
    c = dict(CASES[name])
    N = N or c["N"]
    dl, tl, same, prompt = _logit_fns(c["models"], c["prompt"])
    T, k = c["temperature"], c["top_k"]
    tree = Tree(probs_fn(tl, T, k), probs_fn(dl, T, k), M_TOKENS, filtered=k > 0)
    dof = _dof(tree.prob, N)
    lam, prob_same = 0.0, None
    if same is not None:
        prob_same = tree.cell_probs(probs_fn(same, T, k))
        lam = lambda_ref(tree.prob, prob_same, N)
    bar = bar_fp32(dof) if same is None else bar_16bit(dof, lam)
    return types.SimpleNamespace(name=name, N=N, tree=tree, prompt=prompt, dof=dof, bar=bar, lam=lam, prob_same=prob_same,
                                 temperature=T, top_k=k, kind=c["models"], gamma=GAMMA, M=M_TOKENS,
                                 logits=(dl, tl, same))


def x2_of(cs, samples):
    counts, outside = cs.tree.classify(samples)
    x2, dof = pearson(counts, outside, cs.tree.prob, len(samples))
    return x2, dof, outside


def kth_gap(kind, prompt_key, temperature, top_k):
    """For a 16-bit filtered case: (smallest gap between the k-th and (k+1)-th scaled logit over the tree's prefixes, the
    same-dtype oracle's worst scaled-logit error on those prefixes, the same-dtype oracle's mass outside the fp32 support at
    the worst prefix).  Admissible when gap >= 8 * error: rounding then cannot move the k-th token."""
    dl, tl, same, _ = _logit_fns(kind, prompt_key)
    tree = Tree(probs_fn(tl, temperature, top_k), None, M_TOKENS, filtered=True)
    same_p = probs_fn(same, temperature, top_k)
    gap, err, leak = np.inf, 0.0, 0.0
    for pre, toks in zip(tree.prefixes, tree.tokens):
        z = tl(pre)[0].double().numpy() / temperature
        zs = np.sort(z)[::-1]
        gap = min(gap, zs[top_k - 1] - zs[top_k])
        err = max(err, float(np.abs(same(pre)[0].double().numpy() / temperature - z).max()))
        leak = max(leak, 1.0 - float(same_p(pre)[toks].sum()))
    return float(gap), err, leak


# The planted defects each case CLAIMS to catch: the simulator's X2 is >= 2 x the bar at the case's N
# (tests/test_lossless_cpu.py asserts it and prints the rest of the table).  What is not listed, the case cannot see:
#   shared_uniform  needs N >= 20000 on the fp32 pair and is invisible on the 16-bit pair at any N the time allows (its
#                   acceptance rate is 73 %: a shared uniform rarely changes the outcome);
#   same_noise      only the filtered fp32 cases of N >= 10000; not simulated on the 16-bit pair (V = 8192 noise per draw).
_GROSS = ("resample_p", "resample_abs", "bonus_prev_row", "early_p")
CLAIMS = {
    "fp32_filtered": _GROSS + ("shared_uniform", "same_noise"),
    "fp32_plain": _GROSS + ("shared_uniform",),
    "bf16_plain": _GROSS, "fp16_plain": _GROSS,
    "rows_fp32_a": _GROSS + ("same_noise",), "rows_fp32_b": _GROSS,
    "rows_bf16_a": _GROSS, "rows_bf16_b": _GROSS,
    "fp32_filtered_high_seeds": _GROSS,
    "batch_fp32_filtered": _GROSS, "batch_bf16_plain": _GROSS,
    "single_fp32_filtered": _GROSS, "single_bf16_plain": _GROSS,
}
