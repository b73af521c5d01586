"""Prompt-lookup drafting as a reference: the proposer's definition (include/specdec.h, sd_lookup_propose) as a direct numpy
loop over every continuation index c and every length k, and the whole decode loop on the oracle's norm_logits / sample /
max_fn with the Philox draw layout of sd_lookup_generate.  Nothing here shares code with sampling.utils.lookup_propose or the
kernel.  Needs no GPU: CpuPhiloxNoise draws from tests/philox_reference.py; the GPU tests pass philox_replay.PhiloxOracleNoise
(the device's own variates) instead.

Draw layout of one iteration, d = the stream's position on entry: d .. d+gamma reserved and unread, d+gamma+1 .. d+2*gamma the
accept uniforms (all gamma indices reserved even when the scan stops early), d+2*gamma+1 the residual / bonus sample."""
import numpy as np
import torch

import oracle
import philox_reference as PR
from oracle.kvcache_ref import RefKVCacheModel
from oracle.sampling_ref import max_fn, sample

MAX_NGRAM = 8


def propose(seq, gamma, ngram_max=3, ngram_min=1):
    """-> (drafted tokens [gamma], match length, c).  Every c in 1 .. L-1 and every k in 1 .. min(N, c) is tried."""
    seq = np.asarray(seq).reshape(-1)
    L = len(seq)
    assert L >= 1 and 1 <= gamma <= 16 and 1 <= ngram_min <= ngram_max <= MAX_NGRAM
    best_k, best_c = 0, L - 1
    for c in range(1, L):
        kc = 0
        for k in range(1, min(ngram_max, c) + 1):
            if np.array_equal(seq[c - k:c], seq[L - k:L]):
                kc = k
        if kc >= ngram_min and (kc > best_k or (kc == best_k and c > best_c)):
            best_k, best_c = kc, c
    out = list(seq[:L])
    for i in range(gamma):                                        # the sequential copy, which may run into its own output
        out.append(out[best_c + i])
    return np.asarray(out[L:], dtype=np.int64), best_k, best_c


def onehot_rows(drafted, V):
    """The gamma rows the proposer leaves in q_hist: float32 zeros, 1.0 at the drafted token (an id outside [0, V): all zero)."""
    rows = np.zeros((len(drafted), V), dtype=np.float32)
    for i, t in enumerate(drafted):
        if 0 <= t < V:
            rows[i, int(t)] = 1.0
    return rows


class CpuPhiloxNoise:
    """philox_replay.PhiloxOracleNoise's interface and bookkeeping with the variates of tests/philox_reference.py."""

    def __init__(self, seed, gamma):
        self.seed, self.gamma = int(seed) & 0xFFFFFFFFFFFFFFFF, gamma
        self.c = 0
        self.uni_start = None

    def exponential(self, like):
        if self.uni_start is not None:
            self.c = self.uni_start + self.gamma
            self.uni_start = None
        out = torch.from_numpy(PR.exponential(self.seed, self.c, like.numel()).astype(np.float32))
        self.c += 1
        return out.reshape(like.shape)

    def uniform(self):
        if self.uni_start is None:
            self.uni_start = self.c
        out = torch.tensor([PR.uniform(self.seed, self.c)[0]], dtype=torch.float32)
        self.c += 1
        return out


def run(target_model, prompt, eos_token_id, max_len, gamma=4, temperature=1, top_k=0, top_p=0, ngram_max=3, ngram_min=1, noise=None):
    """prompt: (1, L) int64.  -> (tokens (1, len), dict(acc_len, match_len, src, wraps, draws)); `noise` has exponential /
    uniform and the draw counter `c` (PhiloxOracleNoise, CpuPhiloxNoise)."""
    eos_in_prompt = int((prompt == eos_token_id).sum())
    T = prompt.shape[1] + max_len
    target = RefKVCacheModel(target_model, temperature, top_k, top_p, noise)
    prefix = out = prompt
    acc_len, match_len, srcs, wraps = [], [], [], []
    while prefix.shape[1] < T:
        noise.c += gamma + 1                                      # no draft samples, no discarded target sample
        L = prefix.shape[1]
        drafted, k, c = propose(prefix[0].numpy(), gamma, ngram_max, ngram_min)
        match_len.append(k); srcs.append(c); wraps.append(c + gamma > L)
        x = torch.cat((prefix, torch.from_numpy(drafted)[None]), dim=1)
        target._forward_with_kvcache(x)
        p_hist = target._prob_history
        n, accepted = L + gamma - 1, 0
        for i in range(gamma):
            r = noise.uniform()
            j = int(x[0, L + i])
            if bool(r > p_hist[0, L + i - 1, j].item() / 1.0):     # q is one-hot: q[j] = 1
                n = L + i - 1
                break
            accepted += 1
        acc_len.append(accepted)
        prefix = x[:, :n + 1]
        if n < L + gamma - 1:
            q = torch.zeros_like(p_hist[:, n, :])
            q[0, int(x[0, n + 1])] = 1
            try:
                t = sample(max_fn(p_hist[:, n, :] - q), noise)
            except Exception:
                t = sample(max_fn(p_hist[:, n, :]), noise)
            target.rollback(n + 1)
        else:
            t = sample(p_hist[:, -1, :], noise)
            target.rollback(n + 2)
        prefix = out = torch.cat((prefix, t), dim=1)
        hit = out == eos_token_id
        if int(hit.sum()) > eos_in_prompt:                        # the EOS rule of speculative_sampling
            keep = torch.cumsum(hit.float(), dim=1) < eos_in_prompt + 1
            end = int(keep.sum())
            if end < keep.size(1):
                keep[:, end] = True
            out = out[keep][None, :]
            break
    return out, dict(acc_len=acc_len, match_len=match_len, src=srcs, wraps=wraps, draws=noise.c)


def admissible(det, gamma, ngram_max):
    """What a parity case must contain (test_lookup_cpu.py checks it on the CPU run, the GPU tests on theirs): an iteration with
    all gamma accepted, one with 0, one with a partial count, a match of length 0, one of length ngram_max, a continuation that
    wraps behind a real match (match length > 0 and c + gamma > L).  -> the names of the missing ones."""
    a, m = det["acc_len"], det["match_len"]
    have = {"all accepted": gamma in a, "none accepted": 0 in a, "partial": any(0 < v < gamma for v in a),
            "match 0": 0 in m, "match ngram_max": ngram_max in m, "wrap": any(w and k > 0 for w, k in zip(det["wraps"], m))}
    return [k for k, v in have.items() if not v]


# ---- the fixed choices of tests/test_gpu_lookup_parity.py, found by search on this file alone (test_lookup_cpu.py re-checks them)
PARITY_CFG, PARITY_WEIGHT_SEED = "tiny-llama-target", 12
PARITY_GAMMA, PARITY_NGRAM_MAX, PARITY_NGRAM_MIN, PARITY_MAX_LEN = 4, 3, 1, 40
# case -> (prompt seed, Philox seed, top_k); temperature 1, top_p 0.  (a) top_k 1: the sampling is deterministic, which isolates
# the proposer and the accept logic; (b) top_k 4: stochastic.  Greedy runs of the tiny random model fall into cycles, which gives
# the long matches and the all-accept iterations.
PARITY_CASES = {"a_top1": (0, 1000, 1), "b_top4": (3, 1002, 4)}
# the lock-step test: three streams of different prompt lengths (prompt seed, length, Philox seed), top_k 4
PARITY_BATCH = [(0, 12, 1000), (3, 12, 1002), (5, 9, 1001)]


def parity_model():
    from llmspeculativesampling_amd.config import load_config
    from llmspeculativesampling_amd.synth import make_state_dict
    cfg = load_config(PARITY_CFG)
    sd = make_state_dict(cfg, PARITY_WEIGHT_SEED)
    return cfg, sd, oracle.RefCausalLM(cfg, sd)


def parity_prompt(cfg, prompt_seed, length=12):
    return torch.from_numpy(np.random.default_rng(prompt_seed).integers(3, cfg.vocab_size, size=(1, length)))
