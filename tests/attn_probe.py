"""Planted-key probes for the attention kernels (helper of test_attn_probe_cpu.py and test_gpu_attention_edges.py; needs
no GPU).

A probe model has ONE layer: its layer-0 K / V rows depend on the token, the position and RoPE alone, never on an
attention result, so the cache is the same however it was filled and any difference in the logits of the rows under
test comes from the attention of those rows.

Weights start from synth.make_state_dict (every value rounded to bf16, so one dict serves fp32, bf16 and fp16) and are
overwritten so that three tokens play fixed parts:

  * the filler token F fills the context.  Its key scores exactly 0 (Llama: K is exactly 0) or one small constant (OPT: the
    learned position table is zeroed, so every filler key is the same row) against any query - a uniform softmax row;
  * the marker token M has a key that the query token Q (and M itself) scores `MARGIN` above F: hidden channel 0 carries
    "asks" (Q, M), channel 1 "is the marker" (M); q_proj reads channel 0 and k_proj channel 1 into ONE head dimension - for
    Llama the slowest RoPE pair, whose phase turns by < 0.35 rad over 1040 positions, so the margin survives RoPE;
  * M's value row is F's plus +-2 per dimension times the marker channel (v_proj's column 1).

One planted marker therefore owns > 99 % of the softmax row of every query that may see it, and a kernel that loses it
(or lets a query see one it may not) moves the logits by whole units where the bars are 1e-3 (fp32) or a few hundredths
(16-bit).  `discrimination` measures exactly that on the oracle alone.

A layout is a filler context with M planted at one key; `Layout.cls` names the class of position, `branches` the
dispatch branches of launch_attn / attn_body the shape sits on (plain Python mirrors of the launch arithmetic below).
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Dict, List, Optional

import numpy as np
import torch

import oracle
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict

Q_TOK, M_TOK, F_TOK = 5, 6, 7
MARGIN = 12.0                     # score of the marker's key above a filler's: e^12 / (e^12 + 1039) > 0.993 of the row
MAX_SEQ = 1040                    # arena slots of a probe session (1025 keys + the stale slot behind them, 16-aligned)
ATT_TQ = 8                        # rows of one attention group (model_kernels.h)

MODELS: Dict[str, dict] = {
    "llama_d128": dict(arch="llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=1,
                       num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=MAX_SEQ, rms_norm_eps=1e-5),
    "llama_gqa_d64": dict(arch="llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=1,
                          num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=MAX_SEQ, rms_norm_eps=1e-5),
    "opt_d32": dict(arch="opt", vocab_size=512, hidden_size=128, ffn_dim=256, num_hidden_layers=1, num_attention_heads=4,
                    max_position_embeddings=MAX_SEQ, do_layer_norm_before=True),
    "llama_d32": dict(arch="llama", vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=1,
                      num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=MAX_SEQ, rms_norm_eps=1e-5),
    "llama_d16": dict(arch="llama", vocab_size=512, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                      num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=MAX_SEQ, rms_norm_eps=1e-5),
}


def probe_config(name: str) -> ModelConfig:
    return ModelConfig(**MODELS[name])


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


def probe_state_dict(name: str, seed: int = 41, margin: float = MARGIN) -> Dict[str, torch.Tensor]:
    """fp32 tensors whose values are all bf16 numbers (cast with .to(dtype) for a 16-bit model)."""
    cfg = probe_config(name)
    sd = {k: _bf16(v) for k, v in make_state_dict(cfg, seed, head_gain=2.0).items()}
    H, D, Hq, Hkv = cfg.hidden_size, cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads
    llama = cfg.arch == "llama"
    emb_name = "model.embed_tokens.weight" if llama else "model.decoder.embed_tokens.weight"
    emb = sd[emb_name]
    if not llama:
        emb.mul_(0.25)                                             # tied head: keeps the logits at a few units (exact in bf16)
        sd["model.decoder.embed_positions.weight"].zero_()
    emb[:, 0:2] = 0.0
    emb[Q_TOK, 0] = 2.0
    emb[M_TOK, 0] = 2.0
    emb[M_TOK, 1] = 2.0
    p = "model.layers.0." if llama else "model.decoder.layers.0."
    if llama:
        sd[p + "input_layernorm.weight"].fill_(1.0)
        x = emb[[Q_TOK, M_TOK]]
        hn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.rms_norm_eps)
        dim = D // 2 - 1                                           # the slowest RoPE pair is (D/2 - 1, D - 1)
    else:
        sd[p + "self_attn_layer_norm.weight"].fill_(1.0)
        sd[p + "self_attn_layer_norm.bias"].zero_()
        sd[p + "self_attn.q_proj.bias"].zero_()
        sd[p + "self_attn.k_proj.bias"].zero_()
        x = emb[[Q_TOK, M_TOK]]
        hn = torch.nn.functional.layer_norm(x, (H,), eps=cfg.layer_norm_eps)
        dim = 0
    hq, hm = float(hn[0, 0]), float(hn[1, 1])                     # normed "asks" channel of Q, "marker" channel of M
    B = 4.0
    A = float(_bf16(torch.tensor(margin * math.sqrt(D) / (B * hq * hm))))
    wq, wk, wv = (sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv")
    wq.zero_()
    wk.zero_()
    for h in range(Hq):
        wq[h * D + dim, 0] = A
    for h in range(Hkv):
        wk[h * D + dim, 1] = B
    sign = torch.from_numpy(np.random.default_rng([seed, 99]).choice([-2.0, 2.0], size=wv.shape[0]).astype(np.float32))
    wv[:, 1] = sign
    if not llama:
        sd["lm_head.weight"] = emb
    return sd


# Scales of the fp8 arena, per KV head (cycled): powers of two, K's and V's different in every head, heads different.
FP8_K_SCALE = (0.5, 2.0)
FP8_V_SCALE = (2.0, 0.5)


def fp8_scales(name: str) -> torch.Tensor:
    """[1 layer, k|v, Hkv] as Session.kv_scale holds them: the arena stores fp8(x / scale)."""
    hkv = probe_config(name).num_key_value_heads
    return torch.tensor([[[FP8_K_SCALE[h % 2] for h in range(hkv)], [FP8_V_SCALE[h % 2] for h in range(hkv)]]])


def fp8_scaled_sd(name: str, sd):
    """Weights with which the oracle's scale-1 arena emulation (models_ref._kv_fp8 on every new K / V row) computes what an
    arena with the scales of fp8_scales holds and yields: k_proj / v_proj rows of KV head h divided by its scale, so the
    oracle quantises x / s; q_proj rows of the query heads on h multiplied by the K scale (scores are bilinear, RoPE is
    linear) and o_proj's columns of those heads by the V scale.  Powers of two: every product is exact in every dtype, so
    this IS quant(x / s) * s folded into the oracle's K / V rows."""
    cfg = probe_config(name)
    assert cfg.arch == "llama"
    D, rep = cfg.head_dim, cfg.num_attention_heads // cfg.num_key_value_heads
    sc = fp8_scales(name)[0]
    out = {k: v.clone() for k, v in sd.items()}
    p = "model.layers.0.self_attn."
    for h in range(cfg.num_key_value_heads):
        ks, vs = float(sc[0, h]), float(sc[1, h])
        out[p + "k_proj.weight"][h * D:(h + 1) * D] /= ks
        out[p + "v_proj.weight"][h * D:(h + 1) * D] /= vs
        out[p + "q_proj.weight"][h * rep * D:(h + 1) * rep * D] *= ks
        out[p + "o_proj.weight"][:, h * rep * D:(h + 1) * rep * D] *= vs
    return out


def cast_sd(sd, dtype):
    out = {k: v.to(dtype) for k, v in sd.items()}
    if "model.decoder.embed_tokens.weight" in out:
        out["lm_head.weight"] = out["model.decoder.embed_tokens.weight"]
    return out


# ----------------------------------------------------------------------------- launch_attn's arithmetic, mirrored
def in_register_limit(nr: int) -> int:
    """Keys up to which a group's score rows stay in registers (s_hi <= 8 * LW).  attn_body's `half = nr > 4`: groups of 5..8
    rows run the HALF-wave softmax (one half-wave per row, LW = 32): 256 keys; groups of 4 or fewer rows the FULL-wave
    softmax (one wave per row, LW = 64): 512 keys."""
    return 256 if nr > 4 else 512


def nsplit_for(s_all: int, n_groups: int = 1, split_keys: int = 384, keys_per: int = 256) -> int:
    ns = 1
    if s_all > split_keys:
        ns = min(8, (s_all + max(16, keys_per) - 1) // max(16, keys_per))
        while ns > 1 and ns * n_groups > 64:
            ns -= 1
    return ns


def chunk_keys(s_all: int, nsplit: int) -> int:
    return (((s_all + nsplit - 1) // nsplit + 15) & ~15) if nsplit > 1 else s_all


def chunk_edges(s_all: int, nsplit: int) -> List[int]:
    """First and last key of every chunk that holds a key at all (s_all: the keys the LAST row of a group sees - every
    group of a launch cuts its own range into the launch's nsplit chunks)."""
    ck = chunk_keys(s_all, nsplit)
    out = []
    for c in range(nsplit):
        lo, hi = c * ck, min(s_all, (c + 1) * ck)
        if lo < hi:
            out += [lo, hi - 1]
    return out


def v_prefetch_keys(D: int) -> int:
    return 16 * 256 // (D // 8)


def groups_of(n: int) -> List[int]:
    return [min(ATT_TQ, n - r) for r in range(0, n, ATT_TQ)]


def pv_width(nr: int) -> int:
    """The P.V step is instantiated for 1, 3, 5 and 8 rows: a group takes the smallest that holds it."""
    return next(w for w in (1, 3, 5, 8) if nr <= w)


def branches(D: int, S: int, n: int, split_keys: int = 384, keys_per: int = 256) -> List[str]:
    gs = groups_of(n)
    ns = nsplit_for(S, len(gs), split_keys, keys_per)
    ck = chunk_keys(S, ns)
    out = []
    for nr in sorted(set(gs)):
        out.append(("register" if ck <= in_register_limit(nr) else "lds") + "-softmax")
        out.append("half-wave" if nr > 4 else "full-wave")
        out.append(f"pv{pv_width(nr)}")
    if ck > v_prefetch_keys(D):
        out.append("prefetch-tail")
    if ck > 256:
        out.append("mfma-batch2")
    if ns > 1:
        out.append("split")
        if (ns - 1) * ck >= S - n + 1:                             # a chunk wholly past row 0's causal range
            out.append("chunk-past-causal-range")
    return out


# ----------------------------------------------------------------------------- layouts
Layout = namedtuple("Layout", "S n marker probe cls")
# S keys in all, the last n are the new rows (token Q; F or M where the marker sits); `marker` is the key index of M (None:
# no marker; == S: the stale arena slot behind the last key); `probe` the index (0..n-1) of the row the class is about.

CAUSAL_S = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 383, 384, 385, 511, 512, 513, 1025]
CAUSAL_N = [1, 2, 3, 4, 5, 8, 9, 16]
CLASSES = ["key0", "last_cached", "own", "forbidden", "chunk_edge", "past_prefetch", "key255", "key256"]


def _place(cls: str, S: int, n: int, D: int, k: int, split_keys: int, keys_per: int) -> Optional[Layout]:
    """The layout of class `cls` at (S, n), or None where the class does not exist there.  k varies the choice between
    the candidates of a class (which chunk edge, which row)."""
    pos0 = S - n
    last = n - 1
    if cls == "key0":
        return Layout(S, n, 0, last, cls) if pos0 >= 1 else None
    if cls == "last_cached":
        return Layout(S, n, pos0 - 1, k % n, cls) if pos0 >= 1 else None
    if cls == "own":                                               # the marker is row `probe`'s own token
        r = k % n
        return Layout(S, n, pos0 + r, r, cls)
    if cls == "forbidden":                                         # the key just after row `probe`; past the last row it
        r = (k % n) if k % 3 else last                             # is the stale arena slot S
        return Layout(S, n, pos0 + r + 1, r, cls)
    if cls == "key255":
        return Layout(S, n, 255, last, cls) if pos0 > 255 else None
    if cls == "key256":
        return Layout(S, n, 256, last, cls) if pos0 > 256 else None
    ns = nsplit_for(S, len(groups_of(n)), split_keys, keys_per)
    if cls == "chunk_edge":
        if ns == 1:
            return None
        edges = sorted({e for r0 in range(0, n, ATT_TQ) for e in chunk_edges(pos0 + min(n, r0 + ATT_TQ), ns) if e < pos0})
        return Layout(S, n, edges[k % len(edges)], last, cls) if edges else None
    if cls == "past_prefetch":
        w = v_prefetch_keys(D)
        ck = chunk_keys(S, ns)
        if ck <= w:
            return None
        key = (k % ns) * ck + w                                    # first key past the window of chunk k
        if key >= min(S, (k % ns + 1) * ck):
            key = w
        return Layout(S, n, key, last, cls) if key < pos0 else None
    raise ValueError(cls)


def causal_layouts(D: int, s_list=CAUSAL_S, n_list=CAUSAL_N, split_keys: int = 384, keys_per: int = 256,
                   max_s: Optional[int] = None, per_s: int = 1) -> List[Layout]:
    """The thinned S x n x class table: every S meets every class (where the class exists at that S) with `per_s` values
    of n, walking n round-robin so that every n meets every class too; a second pass adds, for every (n, class) pair the
    walk missed, the smallest S at which it exists.  Deterministic."""
    out, seen = [], set()
    k = 0
    for ci, cls in enumerate(CLASSES):
        for si, S in enumerate(s_list):
            if max_s and S > max_s:
                continue
            got = 0
            for step in range(len(n_list)):
                n = n_list[(si + ci + step) % len(n_list)]
                if n > S:
                    continue
                lay = _place(cls, S, n, D, k, split_keys, keys_per)
                k += 1
                if lay is not None and lay not in seen:
                    out.append(lay)
                    seen.add(lay)
                    got += 1
                    if got >= per_s:
                        break
    have = {(l.n, l.cls) for l in out}
    for cls in CLASSES:
        for n in n_list:
            if (n, cls) in have:
                continue
            for S in s_list:
                if n > S or (max_s and S > max_s):
                    continue
                lay = _place(cls, S, n, D, k, split_keys, keys_per)
                k += 1
                if lay is not None:
                    out.append(lay)
                    break
    return out


def layout_tokens(lay: Layout) -> np.ndarray:
    """Tokens of keys 0 .. S (S + 1 entries: the last is the stale arena slot behind the sequence)."""
    t = np.full(lay.S + 1, F_TOK, dtype=np.int64)
    t[lay.S - lay.n:lay.S] = Q_TOK
    if lay.marker is not None:
        t[lay.marker] = M_TOK
    return t


# ----------------------------------------------------------------------------- the oracle on a layout
def kv_rows(lm, ids, lo, hi, chunk=512):
    """K / V rows lo .. hi - 1 of a ONE-layer model: they depend on token and position alone, so they are computed in
    chunks at their own positions (the attention inside a chunk is discarded) instead of by one hi-row causal forward."""
    assert lm.cfg.num_hidden_layers == 1
    ks, vs = [], []
    for a in range(lo, hi, chunk):
        b = min(hi, a + chunk)
        k, v = lm(ids[:, a:b], position_ids=torch.arange(a, b)[None]).past_key_values[0]
        ks.append(k)
        vs.append(v)
    return torch.cat(ks, 2), torch.cat(vs, 2)


class ProbeOracle:
    """oracle.RefCausalLM of a probe model in one dtype, with the K / V rows of F and M at every position tabulated once
    (layer 0's rows are a function of token and position alone), so a layout costs one n-row forward."""

    def __init__(self, name: str, dtype=torch.float32, kv_quant: Optional[str] = None, sd=None, max_seq: int = MAX_SEQ):
        self.name, self.dtype = name, dtype
        self.cfg = probe_config(name)
        sd = sd if sd is not None else probe_state_dict(name)
        if kv_quant == "fp8":                                      # the arena's non-unit scales, folded into the weights
            sd = fp8_scaled_sd(name, sd)
        self.sd = cast_sd(sd, dtype)
        self.lm = oracle.RefCausalLM(self.cfg, self.sd, kv_quant=kv_quant)
        self.tab = {}
        for tok in (F_TOK, M_TOK):
            ids = torch.full((1, max_seq), tok, dtype=torch.long)
            # (a table past MAX_SEQ positions is tabulated in chunks; up to it by the one forward the bars were measured with)
            self.tab[tok] = self.lm(ids).past_key_values[0] if max_seq <= MAX_SEQ else kv_rows(self.lm, ids, 0, max_seq)

    def past(self, tokens: np.ndarray, upto: int):
        if upto == 0:
            return None
        kF, vF = self.tab[F_TOK]
        kM, vM = self.tab[M_TOK]
        is_m = torch.from_numpy(tokens[:upto] == M_TOK)[None, None, :, None]
        return [(torch.where(is_m, kM[:, :, :upto], kF[:, :, :upto]), torch.where(is_m, vM[:, :, :upto], vF[:, :, :upto]))]

    def logits(self, lay: Layout, with_marker: bool = True) -> torch.Tensor:
        """fp32 logits [n, V] of the layout's new rows (the marker replaced by F when with_marker is False)."""
        t = layout_tokens(lay)
        if not with_marker:
            t[t == M_TOK] = F_TOK
        pos0 = lay.S - lay.n
        ids = torch.from_numpy(t[pos0:lay.S])[None]
        return self.lm(ids, past_key_values=self.past(t, pos0)).logits.float()[0]

    def leaked(self, lay: Layout) -> torch.Tensor:
        """Logits of row `probe` of a forbidden-key layout if the kernel DID let it see the key behind it: the marker's
        K / V row (at its own position) joins the cached keys, the rows up to `probe` keep their positions."""
        assert lay.cls == "forbidden"
        t = layout_tokens(lay)
        pos0, r = lay.S - lay.n, lay.probe
        kM, vM = self.tab[M_TOK]
        j = lay.marker
        extra = (kM[:, :, j:j + 1], vM[:, :, j:j + 1])
        past = self.past(t, pos0)
        past = [extra] if past is None else [(torch.cat([past[0][0], extra[0]], 2), torch.cat([past[0][1], extra[1]], 2))]
        ids = torch.from_numpy(t[pos0:pos0 + r + 1])[None]
        pid = torch.arange(pos0, pos0 + r + 1)[None]
        return self.lm(ids, past_key_values=past, position_ids=pid).logits.float()[0, r]


def discrimination(o32: ProbeOracle, lay: Layout) -> float:
    """max-abs change of the probed row's fp32 oracle logits between the marker at work and not: marker against F in its
    place for a key the row may see; for a forbidden key, the key leaked into the row against the oracle proper."""
    if lay.cls == "forbidden":
        return float((o32.leaked(lay) - o32.logits(lay)[lay.probe]).abs().max())
    return float((o32.logits(lay)[lay.probe] - o32.logits(lay, with_marker=False)[lay.probe]).abs().max())


def errors(got: torch.Tensor, ref16: torch.Tensor, truth: torch.Tensor):
    """(e_hip, e_ref, rms_hip, rms_ref) as test_gpu_production_parity._assert_within_reference_error takes them."""
    return (float((got - truth).abs().max()), float((ref16 - truth).abs().max()),
            float((got - truth).pow(2).mean().sqrt()), float((ref16 - truth).pow(2).mean().sqrt()))


FP32_TOL = 1e-3                   # the north_star bar of the fp32 forward tests


def tol16(e_ref: float) -> float:
    """The max-abs side of _assert_within_reference_error (its constants are asserted equal in the CPU test)."""
    return 1.5 * e_ref + 0.02


# ----------------------------------------------------------------------------- other layout tables
def split_layouts(D: int, split_keys: int, keys_per: int, s_list, n_list) -> List[Layout]:
    """Every (S, n) of an alternative split setting with every class that exists there."""
    out, k = [], 0
    for S in s_list:
        for n in n_list:
            for cls in CLASSES:
                lay = _place(cls, S, n, D, k, split_keys, keys_per)
                k += 1
                if lay is not None and lay not in out:
                    out.append(lay)
    return out


# (SD_ATTN_SPLIT_KEYS, SD_ATTN_KEYS_PER_SPLIT), S values, n values of the alternative split settings
SPLIT_SETTINGS = [((64, 32), (65, 96, 97, 250), (1, 5, 8)), ((4096, 256), (512, 513, 600), (1, 4, 5))]


def split_cases(D: int):
    """[((split_keys, keys_per), layouts)] - the one table both the CPU check and the GPU test run."""
    return [(st, split_layouts(D, st[0], st[1], s_list, n_list)) for st, s_list, n_list in SPLIT_SETTINGS]


def prefill_layouts() -> List[Layout]:
    """One call of 81, 200 and 256 rows at pos0 0 and 37; logits come out for the last <= 64 rows, so `probe` lies there."""
    out = []
    for n in (81, 200, 256):
        for pos0 in (0, 37):
            S = pos0 + n
            out.append(Layout(S, n, 0, n - 1, "key0"))             # (at pos0 = 0 key 0 is row 0's own token)
            if pos0:
                out.append(Layout(S, n, pos0 - 1, n - 33, "last_cached"))
            out.append(Layout(S, n, pos0 + n - 10, n - 10, "own"))
            out.append(Layout(S, n, pos0 + n - 20, n - 21, "forbidden"))
            out.append(Layout(S, n, S, n - 1, "forbidden"))        # the stale arena slot behind the call's last row
    return out


BATCH_CACHE = (3, 390, 17, 256)
BATCH_NEW = [(1, 5, 9, 5), (9, 1, 5, 1), (5, 9, 1, 9)]


def batch_layouts(n_new) -> List[Layout]:
    """One layout per stream of a batched pass (cache lengths BATCH_CACHE): key 0 in the 3-key stream, the first key of
    the second chunk in the 390-key stream, the stale slot behind the 17-key stream's last row (forbidden), key 255 = the last
    cached key of stream 3.  The pass splits 2 ways (390 + n > 384) and every group cuts ITS OWN s_all into the launch's 2
    chunks: the 3-key stream (S <= 12) gets one 16-key chunk and an empty second one (s_hi == 0); the 17-key stream (S =
    18..26) gets 16 keys and a second chunk of 2..10 keys (see batch_second_chunk_keys)."""
    s_max = max(c + n for c, n in zip(BATCH_CACHE, n_new))
    ns = nsplit_for(s_max, sum(len(groups_of(n)) for n in n_new))
    assert ns == 2
    out = []
    for i, (c, n) in enumerate(zip(BATCH_CACHE, n_new)):
        S = c + n
        if i == 0:
            out.append(Layout(S, n, 0, n - 1, "key0"))
        elif i == 1:
            out.append(Layout(S, n, chunk_keys(S, ns), n - 1, "chunk_edge"))
        elif i == 2:
            out.append(Layout(S, n, S, n - 1, "forbidden"))
        else:
            out.append(Layout(S, n, 255, 0, "last_cached"))
    return out


def batch_second_chunk_keys(lay: Layout, ns: int = 2) -> int:
    """s_hi of the second chunk of the stream's LAST group (0: an empty chunk)."""
    return max(0, min(lay.S, 2 * chunk_keys(lay.S, ns)) - chunk_keys(lay.S, ns))


# ----------------------------------------------------------------------------- trees
TreeLayout = namedtuple("TreeLayout", "base N marker probe cls")
# N tree nodes behind `base` cached keys; node i sits at arena slot base + i; `marker` is a KEY index (base + node, or a
# cached key); `probe` the node the class is about.
TREE_W = 8


def tree_parent(i: int) -> int:
    """Levels of TREE_W nodes; a node's parent is a fixed node of the level above (-1: a root)."""
    lv = i // TREE_W
    return -1 if lv == 0 else (lv - 1) * TREE_W + (i * 5 + 3) % TREE_W


def tree_ancestors(i: int) -> List[int]:
    out = []
    while i >= 0:
        out.append(i)
        i = tree_parent(i)
    return out                                                     # the node itself first, its root last


def tree_layouts(bases=(0, 1, 150, 380), sizes=(9, 40, 64)) -> List[TreeLayout]:
    out = []
    for base in bases:
        for N in sizes:
            r = N - 1
            anc = tree_ancestors(r)
            out.append(TreeLayout(base, N, base + anc[-1], r, "ancestor"))
            non = next(j for j in range(r - 1, -1, -1) if j not in anc)
            out.append(TreeLayout(base, N, base + non, r, "forbidden"))
            if base:
                out.append(TreeLayout(base, N, base - 1, r, "last_cached"))
            if N == 64:
                out.append(TreeLayout(base, N, base + 63, 63, "node63"))
    return out


def tree_inputs(lay: TreeLayout, with_marker: bool = True, leak: bool = False):
    """(key tokens [base + N], node positions [N], ancestor bit masks [N]); leak: `probe` also sees the marker's node."""
    t = np.full(lay.base + lay.N, F_TOK, dtype=np.int64)
    t[lay.base:] = Q_TOK
    if with_marker:
        t[lay.marker] = M_TOK
    pos = np.array([lay.base + i // TREE_W for i in range(lay.N)], dtype=np.int64)
    bits = [sum(1 << a for a in tree_ancestors(i)) for i in range(lay.N)]
    if leak:
        bits[lay.probe] |= 1 << (lay.marker - lay.base)
    return t, pos, bits


def tree_logits(o: ProbeOracle, lay: TreeLayout, with_marker: bool = True, leak: bool = False) -> torch.Tensor:
    t, pos, bits = tree_inputs(lay, with_marker, leak)
    mask = torch.ones((1, lay.N, lay.base + lay.N), dtype=torch.bool)
    for i, b in enumerate(bits):
        mask[0, i, lay.base:] = torch.tensor([(b >> j) & 1 == 1 for j in range(lay.N)])
    ids = torch.from_numpy(t[lay.base:])[None]
    return o.lm(ids, past_key_values=o.past(t, lay.base), extra_attention_mask=mask,
                position_ids=torch.from_numpy(pos)[None]).logits.float()[0]


def tree_discrimination(o32: ProbeOracle, lay: TreeLayout) -> float:
    if lay.cls == "forbidden":
        return float((tree_logits(o32, lay, leak=True)[lay.probe] - tree_logits(o32, lay)[lay.probe]).abs().max())
    return float((tree_logits(o32, lay)[lay.probe] - tree_logits(o32, lay, with_marker=False)[lay.probe]).abs().max())


# ----------------------------------------------------------------------------- what the GPU tests run
# (test name, model, dtype name, kv_quant, layouts): test_attn_probe_cpu.py checks every row of this table on the oracle
# alone, test_gpu_attention_edges.py runs the same rows on the device.
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CAUSAL_MODELS = [("llama_d128", "fp32"), ("llama_d128", "bf16"), ("llama_d128", "fp16"), ("llama_gqa_d64", "fp32"),
                 ("llama_gqa_d64", "bf16"), ("opt_d32", "fp32"), ("opt_d32", "bf16"), ("llama_d16", "fp32"),
                 ("llama_d16", "bf16")]
SPLIT_MODELS = [("llama_d128", "bf16"), ("llama_gqa_d64", "fp32"), ("llama_gqa_d64", "bf16"), ("opt_d32", "bf16")]
FP8_MODELS = ["llama_d32", "llama_gqa_d64", "llama_d128"]     # (the fp8 arena and its oracle emulation are Llama's)
TREE_MODELS = [("llama_gqa_d64", "fp32", None), ("llama_gqa_d64", "bf16", None), ("llama_gqa_d64", "bf16", "fp8")]


def head_dim(name: str) -> int:
    return probe_config(name).head_dim


def fp8_layouts(D: int) -> List[Layout]:
    return split_layouts(D, 384, 256, (17, 257, 385), (1, 5))


def fused_layouts() -> List[Layout]:
    return causal_layouts(128, max_s=384)


def all_cases():
    """(label, model, dtype name, kv_quant, layouts) of every causal-layout GPU test."""
    out = []
    for name, dt in CAUSAL_MODELS:
        out.append(("causal", name, dt, None, causal_layouts(head_dim(name))))
    for name, dt in SPLIT_MODELS:
        D = head_dim(name)
        for (sk, kp), lays in split_cases(D):
            out.append((f"split{sk}_{kp}", name, dt, None, lays))
    for n_new in BATCH_NEW:
        for dt in ("fp32", "bf16"):
            out.append(("batch", "llama_d128", dt, None, batch_layouts(n_new)))
    for name in FP8_MODELS:
        out.append(("fp8", name, "bf16", "fp8", fp8_layouts(head_dim(name))))
    for dt in ("bf16", "fp16"):
        out.append(("fused", "llama_d128", dt, None, fused_layouts()))
        out.append(("prefill", "llama_d128", dt, None, prefill_layouts()))
    return out
