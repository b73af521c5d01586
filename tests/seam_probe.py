"""Adversarial rows for the layer seams (helper of test_seam_probe_cpu.py and test_gpu_layer_seams.py; needs no GPU).

The seams are the kernels between the GEMMs and attention: embed_kernel / embed_norm_kernel / norm_kernel /
residual_norm_kernel / qkv_epilogue_kernel / act_kernel / reduce_*_kernel / logits_kernel (model_kernels.h), their fused
twins in gemm_epilogue_fold, the residual epilogue + norm-on-load pair (normload_kernels.h), the PRO_EMBED / PRO_RESID
prologues of gemm_small (small_kernels.h) and the 12-bit-record variants.  The whole-model tests feed them i.i.d. rows, on
which a norm that leaves a column out of its statistics moves the scale by 1 / H.  Here a probe model (at most 2 layers,
vocabulary 512, weights from synth.make_state_dict rounded to bf16, so one dict serves fp32, bf16 and fp16) gets token
rows that are NOT like that:

  A. statistics columns: token A_TOK0 + i has ONE embedding column - class i of `stat_columns` - set to `MAG[model]`
     against the synthetic background.  A norm that drops that column from its sum (of squares) rescales the whole row
     by a factor of 1.7 .. 8.  `stat_discrimination` measures, per norm site, how far the fp32 oracle's logits move
     when that one call's statistics leave the column out (models_ref._rms_norm / the F.layer_norm calls of opt_forward
     are patched inside the helper and restored);
  B. degenerate rows: all zero (OPT: the learned positions of the rows that carry them are zero too), all 2^-60 (the
     squares are lost against eps), +m / -m alternating (mean exactly zero), and for LayerNorm 16 + k / 8 (mean^2 ~ 10^3 .. 10^4 x
     the variance).  `degenerate_discrimination`: the same pass with an ordinary token in the row's place;
  C. planted slabs: a split-K GEMM leaves S slabs which its consumer folds - reduce_part4 in residual_norm_kernel and
     PRO_RESID, the scalar reduce_part in reduce_rows_kernel / reduce_addpos_kernel (OPT's project_out / project_in) and
     logits_kernel, gemm_bf16_stream_fin's own fold - in an 8-burst, a 4-burst and a scalar tail.  (qkv_epilogue_kernel and
     act_kernel meet S > 1 nowhere: sd_model_create admits a 16-bit model only with intermediate % 32 == 0 and head_dim in
     {16, 32, 64, 128}, so the engine always gives it the fused layout, and the fp32 GEMM leaves one slab.)  A weight variant is zero except in
     the k-range of ONE slab (times a power of two), so the pass's logits ARE that slab's contribution: a fold that
     skips the slab gives the logits of the all-zero weight (`slab_discrimination`).  (S, ksp) come from sd_gemm_route;
  D. activation columns: ONE intermediate column j (classes: 0, 7 | 8 - the 8-gate / 8-up interleave of the fused layout,
     15 | 16, 255 | 256 - act_kernel's block edge, I - 1) is made decisive: its gate row reads hidden channel 1 alone, its up
     row channel 2 alone, layer 0's o_proj is zero, so both channels reach the second norm as embedded, and its
     down_proj column is scaled up.  Six tokens put the gate pre-activation at about -96 (expf overflows: SiLU is -0),
     -20, -+2^-10 and 20, 96 (the linear tail), with an up value that makes SiLU(gate) * up of order 1 where it is not 0.
     `act_discrimination`: the same weights with the gate row negated (what a column taken from the wrong place, or a
     wrong sign, computes).  OPT (`relu_state_dict`): fc1 row j reads a channel that the second LayerNorm sets to a constant
     (weight 0, bias beta), so the pre-activation A * beta + bias[j] is the same exact number for every token: 2^-12 where a
     dot product rounded to 16 bits BEFORE the bias add gives 0 ("cancel"), and the bias alone at -0.0 and at the
     smallest positive bf16 subnormal, which no logit can show (measured in test_seam_probe_cpu.py, so not run on the GPU);
     Head columns: vocabulary column v (0, 15 | 16, 255 | 256, V - 1) is made every row's maximum by a planted lm_head
     row that reads hidden channel 5 alone, which every token carries at 1 and no projection writes
     (`head_discrimination`: the planted row missing);
  E. (second observable of the same passes) the K / V rows a pass writes: `SeamOracle.run` returns the oracle's
     past_key_values next to the logits.

A pass is (tokens of its rows, pos0); the rows in front of pos0 are ordinary tokens (`prefix_tokens`).  Several plants ride
one pass as its rows: `passes(family, model, n)` cuts the family's plants into passes of n rows (at most 8 plants per
pass, the remaining rows ordinary tokens).

Route mirrors (plain Python restatements of plan_forward, pinned by test_seam_probe_cpu.py): rn_threads,
SMALL_MAX_ROWS, small_path_ok, norm_on_load_ok.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import oracle
from oracle import models_ref
from attn_probe import FP32_TOL, errors, tol16, tree_ancestors, TREE_W  # noqa: F401  (re-exported: the GPU test's bars)
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MAX_POS = 160                      # positions (and arena slots) of the 2-layer probe models: 130 prefill rows + a prefix

MODELS: Dict[str, dict] = {
    # hidden % 1024 == 0: norm on load, the small path, 12-bit records; residual_norm_kernel with 128 threads
    "llama_h1024": dict(arch="llama", vocab_size=512, hidden_size=1024, intermediate_size=1024, num_hidden_layers=2,
                        num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=MAX_POS, rms_norm_eps=1e-5),
    # 64 threads: the second register group starts at column 256 = H and is never on
    "llama_h256": dict(arch="llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                       num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=MAX_POS, rms_norm_eps=1e-5),
    "opt_pre_h256": dict(arch="opt", vocab_size=512, hidden_size=256, ffn_dim=512, num_hidden_layers=2, num_attention_heads=4,
                         max_position_embeddings=MAX_POS, do_layer_norm_before=True),
    # RES_POST, to_operand_kernel in the first norm's place, no final norm (one layer: see A_SITES_DROPPED)
    "opt_post_h128": dict(arch="opt", vocab_size=512, hidden_size=128, ffn_dim=256, num_hidden_layers=1, num_attention_heads=4,
                          max_position_embeddings=MAX_POS, do_layer_norm_before=False),
    # embed_kernel tiled, reduce_addpos_kernel, reduce_rows_kernel
    "opt_proj_h128": dict(arch="opt", vocab_size=512, hidden_size=128, ffn_dim=256, num_hidden_layers=2, num_attention_heads=4,
                          max_position_embeddings=MAX_POS, do_layer_norm_before=True, word_embed_proj_dim=64),
    # hidden % 8 != 0 (fp32 only): embed_norm_kernel's scalar load path; vocabulary 500: logits_kernel's last block partial
    "llama_h96": dict(arch="llama", vocab_size=500, hidden_size=96, intermediate_size=160, num_hidden_layers=2,
                      num_attention_heads=3, num_key_value_heads=3, max_position_embeddings=MAX_POS, rms_norm_eps=1e-5),
    # family C: one layer whose down projection has K = 4096 - up to 16 k-slabs in front of the final residual + norm
    "llama_c": dict(arch="llama", vocab_size=512, hidden_size=256, intermediate_size=4096, num_hidden_layers=1,
                    num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=MAX_POS, rms_norm_eps=1e-5),
    # family C: project_out has K = 4096 (up to 16 slabs in front of reduce_rows_kernel), project_in K = 512 (2 slabs in front
    # of reduce_addpos_kernel) - the scalar reduce_part
    "opt_c": dict(arch="opt", vocab_size=512, hidden_size=4096, ffn_dim=256, num_hidden_layers=1, num_attention_heads=32,
                  max_position_embeddings=16, do_layer_norm_before=True, word_embed_proj_dim=512),
    # the limit sd_model_create admits: 1024 threads, both register groups full, MAXV = 4 of embed_norm_kernel full
    "llama_h8192": dict(arch="llama", vocab_size=512, hidden_size=8192, intermediate_size=32, num_hidden_layers=1,
                        num_attention_heads=64, num_key_value_heads=1, max_position_embeddings=16, rms_norm_eps=1e-5),
}

# magnitude of the planted column (a bf16 number, finite in fp16 after every norm): chosen on the CPU so that every norm
# site of every (model, dtype) that the GPU test runs discriminates >= 20x the bar (test_seam_probe_cpu.py prints the
# floors).  OPT's embedding is scaled by EMB_SCALE first: the tied head otherwise puts the planted tokens' own logit
# columns at hundreds of units, where one bf16 ulp of the logit is already the bar
MAG = {"llama_h1024": 256.0, "llama_h256": 128.0, "opt_pre_h256": 128.0, "opt_post_h128": 16.0, "opt_proj_h128": 16.0,
       "llama_h96": 128.0, "llama_h8192": 256.0, "llama_c": 128.0, "opt_c": 16.0}
EMB_SCALE = 0.25
ALT_M = 2.0                        # the +m / -m row
TINY = 2.0 ** -60                  # its squares, 2^-120, are lost against eps (fp16: the row itself is zero)

A_TOK0, B_TOK0, ORD_TOK0 = 8, 40, 100
B_KINDS = ["zero", "tiny", "alt", "ln"]
N_ZERO_POS = 4                     # OPT: learned positions 0 .. 3 are zero, so the degenerate rows reach the norm as planted
MAX_LOGIT_ROWS = 64                # logit rows of one single-sequence call (engine.MAX_LOGIT_ROWS)
MAX_PLANTS = 8                     # plants of one pass; the other rows are ordinary tokens


def probe_config(name: str) -> ModelConfig:
    return ModelConfig(**MODELS[name])


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------- plan_forward's arithmetic, mirrored
RN_RG = 2                          # register groups of 4 columns per thread of residual_norm_kernel
SMALL_MAX_ROWS = 4
NORM_ON_LOAD_MAX_ROWS = 8


def rn_threads(H: int) -> int:
    """blockDim of residual_norm_kernel: thread t owns columns 4t .. 4t + 3 and 4 (t + rn_threads) .. + 3."""
    per = (H // 4 + RN_RG - 1) // RN_RG
    return min(1024, max(64, (per + 63) // 64 * 64))


def norm_on_load_ok(cfg: ModelConfig, dt: str, n_rows: int, env_norm_on_load: int = 2) -> bool:
    fused = dt != "fp32" and cfg.intermediate_size % 8 == 0 and cfg.head_dim % 4 == 0
    return (dt != "fp32" and env_norm_on_load != 0 and cfg.arch == "llama" and fused and n_rows <= NORM_ON_LOAD_MAX_ROWS
            and cfg.hidden_size % 1024 == 0 and cfg.hidden_size <= 8192)


def small_path_ok(cfg: ModelConfig, dt: str, n_rows: int, env_small_path: int = 1) -> bool:
    """forward_small: bf16, the fused layout, a non-contiguous pass of <= 4 rows, hidden <= 2048, no input projection,
    not post-LN (a pass of <= 80 rows is never contiguous)."""
    fused = cfg.intermediate_size % 8 == 0 and cfg.head_dim % 4 == 0
    if not env_small_path or dt != "bf16" or not fused or n_rows > SMALL_MAX_ROWS:
        return False
    if cfg.hidden_size > 2048 or cfg.hidden_size % 32 or cfg.word_embed_proj_dim not in (0, cfg.hidden_size):
        return False
    return cfg.arch == "llama" or cfg.do_layer_norm_before


def stat_columns(name: str) -> List[int]:
    """Column classes of family A: 0; 3 | 4 (load4's vector group); 7 | 8 (16 bytes of embed_norm_kernel); 15 | 16 (a
    sum-of-squares tile); 4 rn_threads - 1 | 4 rn_threads (first column of residual_norm_kernel's second register
    group, where the row has one); H - 1."""
    H = probe_config(name).hidden_size
    rt = rn_threads(H)
    out = []
    for c in (0, 3, 4, 7, 8, 15, 16, 4 * rt - 1, 4 * rt, H - 1):
        if c < H and c not in out:
            out.append(c)
    return out


# ----------------------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def _probe_state_dict(name: str, seed: int) -> Dict[str, torch.Tensor]:
    cfg = probe_config(name)
    sd = {k: _bf16(v) for k, v in make_state_dict(cfg, seed, head_gain=2.0).items()}
    llama = cfg.arch == "llama"
    emb = sd["model.embed_tokens.weight" if llama else "model.decoder.embed_tokens.weight"]
    if not llama:
        emb.mul_(EMB_SCALE)                                        # (exact in bf16)
        sd["model.decoder.embed_positions.weight"][2:2 + N_ZERO_POS].zero_()
    W = emb.shape[1]
    if W == cfg.hidden_size:                                       # (with an input projection a column is no residual column)
        for i, c in enumerate(stat_columns(name)):
            emb[A_TOK0 + i, c] = MAG[name]
        if not llama:
            # the tied head reads the planted entry back: the LAST norm's weight is 1 / 16 at the class columns, so a planted
            # token's own logit column stays at tens of units and the 16-bit bar at a tenth (the statistics are untouched)
            if cfg.do_layer_norm_before:
                sd["model.decoder.final_layer_norm.weight"][stat_columns(name)] = 1.0 / MAG[name]
    col = torch.arange(W)
    emb[B_TOK0 + 0] = 0.0
    emb[B_TOK0 + 1] = TINY
    # (OPT: the tied head reads these rows back as logit columns 42 and 43, so they are scaled down by powers of two -
    # LayerNorm's result does not depend on the row's scale, the mean^2 : variance ratio of the last row neither)
    s_alt, s_ln = (1.0, 1.0) if llama else (2.0 ** -5, 2.0 ** -6)
    emb[B_TOK0 + 2] = torch.where(col % 2 == 0, ALT_M, -ALT_M) * s_alt
    emb[B_TOK0 + 3] = (16.0 + (col % 8).float() / 8.0) * s_ln
    if not llama:
        sd["lm_head.weight"] = emb
    return sd


def probe_state_dict(name: str, seed: int = 43) -> Dict[str, torch.Tensor]:
    """fp32 tensors whose values are all bf16 numbers (cast with cast_sd for a 16-bit model).  Shared: do not modify."""
    return _probe_state_dict(name, seed)


def cast_sd(sd, dtype):
    out = {k: v.to(dtype) for k, v in sd.items()}
    if "model.decoder.embed_tokens.weight" in out:
        out["lm_head.weight"] = out["model.decoder.embed_tokens.weight"]
    return out


# ----------------------------------------------------------------------------- passes
def ordinary(r: int) -> int:
    return ORD_TOK0 + r % 64


def prefix_tokens(pos0: int) -> List[int]:
    """The ordinary tokens in front of a pass that starts at pos0."""
    return [ORD_TOK0 + 64 + i % 96 for i in range(pos0)]


def plants(family: str, name: str) -> List[int]:
    cfg = probe_config(name)
    if family == "A":
        if cfg.word_embed_proj_dim not in (0, cfg.hidden_size):
            return []
        return [A_TOK0 + i for i in range(len(stat_columns(name)))]
    if family == "B":
        kinds = B_KINDS if cfg.arch == "opt" else B_KINDS[:3]
        return [B_TOK0 + B_KINDS.index(k) for k in kinds]
    raise ValueError(family)


def passes(family: str, name: str, n: int, first_only: bool = False) -> List[Tuple[int, ...]]:
    """The family's plants cut into passes of n rows, up to MAX_PLANTS plants each, the other rows ordinary tokens.

    The plants are the first rows whose logits the call returns (its last 64).  Up to 64 rows that is row 0, where OPT's
    degenerate rows sit on the zeroed positions.  A planted row that attends to many ordinary rows dilutes what its first
    norm does.  first_only: one pass (the many-row routes; every class has been through the kernel at a smaller n)."""
    pl = plants(family, name)
    k = min(n, MAX_PLANTS)
    out = []
    for a in range(0, len(pl), k):
        rows = pl[a:a + k]
        fill = [ordinary(r) for r in range(n - len(rows))]
        first = n - min(n, MAX_LOGIT_ROWS)                         # the first row whose logits the call returns
        out.append(tuple(fill[:first] + rows + fill[first:]))
        if first_only:
            break
    return out


def plant_column(name: str, tok: int) -> int:
    """The planted column of a family-A token; -1 for every other token."""
    i = tok - A_TOK0
    cols = stat_columns(name)
    return cols[i] if 0 <= i < len(cols) and plants("A", name) else -1


# ----------------------------------------------------------------------------- the oracle
class SeamOracle:
    """oracle.RefCausalLM of a probe model in one dtype; `run` caches by (tokens, pos0)."""

    def __init__(self, name: str, dtype=torch.float32, sd=None):
        self.name, self.dtype, self.cfg = name, dtype, probe_config(name)
        self.lm = oracle.RefCausalLM(self.cfg, cast_sd(sd if sd is not None else probe_state_dict(name), dtype))
        self._past, self._runs = {}, {}

    def past(self, pos0: int):
        if pos0 == 0:
            return None
        if pos0 not in self._past:
            self._past[pos0] = self.lm(torch.tensor([prefix_tokens(pos0)])).past_key_values
        return self._past[pos0]

    def forward(self, tokens: Sequence[int], pos0: int = 0):
        o = self.lm(torch.tensor([list(tokens)]), past_key_values=self.past(pos0))
        return o.logits.float()[0], o.past_key_values

    def run(self, tokens: Sequence[int], pos0: int = 0):
        """(fp32 logits [n, V], past_key_values of pos0 + n keys per layer)."""
        key = (tuple(tokens), pos0)
        if key not in self._runs:
            self._runs[key] = self.forward(tokens, pos0)
        return self._runs[key]

    def tree(self, tokens: Sequence[int], base: int, pos: Sequence[int], bits: Sequence[int]):
        N = len(tokens)
        mask = torch.ones((1, N, base + N), dtype=torch.bool)
        for i, b in enumerate(bits):
            mask[0, i, base:] = torch.tensor([(b >> j) & 1 == 1 for j in range(N)])
        o = self.lm(torch.tensor([list(tokens)]), past_key_values=self.past(base), extra_attention_mask=mask,
                    position_ids=torch.tensor([list(pos)]))
        return o.logits.float()[0], o.past_key_values


TREE_BASE, TREE_NODES = 3, 9       # 9 nodes behind 3 cached keys: node 8 is a depth-1 node in slot base + 8
TREE_CASES = [("llama_h256", "fp32"), ("llama_h256", "bf16"), ("opt_pre_h256", "bf16")]


def tree_tokens(name: str) -> Tuple[int, ...]:
    return passes("A", name, TREE_NODES)[0]


def tree_shape(N: int, base: int):
    """Levels of TREE_W nodes (attn_probe's tree): node i sits at arena slot base + i, its position is its depth."""
    pos = [base + i // TREE_W for i in range(N)]
    bits = [sum(1 << a for a in tree_ancestors(i)) for i in range(N)]
    return pos, bits


# ----------------------------------------------------------------------------- discrimination (fp32 oracle alone)
class _DropColumn:
    """Patches ONE norm call (counted over models_ref._rms_norm and F.layer_norm in call order) of the oracle: the mean
    and the variance of row r leave column cols[r] out - what a kernel computes that skips that column in its sums (the
    divisor stays H)."""

    def __init__(self, site: int, cols: Sequence[int]):
        self.site, self.cols, self.calls = site, list(cols), 0

    def _keep(self, x):
        keep = torch.ones(x.shape, dtype=torch.float32)
        for r, c in enumerate(self.cols):
            if c >= 0:
                keep[..., r, c] = 0.0
        return keep

    def __enter__(self):
        self.rms, self.F = models_ref._rms_norm, models_ref.F
        outer = self

        def rms(x, w, eps):
            outer.calls += 1
            if outer.calls - 1 != outer.site:
                return outer.rms(x, w, eps)
            xf = x.to(torch.float32)
            ms = (xf.pow(2) * outer._keep(x)).sum(-1, keepdim=True) / x.shape[-1]
            return w * (xf * torch.rsqrt(ms + eps)).to(x.dtype)

        class FProxy:
            def __getattr__(self, k):
                return getattr(outer.F, k)

            @staticmethod
            def layer_norm(x, shape, w, b, eps):
                outer.calls += 1
                if outer.calls - 1 != outer.site:
                    return outer.F.layer_norm(x, shape, w, b, eps)
                xf, keep, H = x.to(torch.float32), outer._keep(x), x.shape[-1]
                mean = (xf * keep).sum(-1, keepdim=True) / H
                var = ((xf - mean).pow(2) * keep).sum(-1, keepdim=True) / H
                return ((xf - mean) * torch.rsqrt(var + eps) * w.float() + b.float()).to(x.dtype)

        models_ref._rms_norm, models_ref.F = rms, FProxy()
        return self

    def __exit__(self, *exc):
        models_ref._rms_norm, models_ref.F = self.rms, self.F


def norm_sites(name: str) -> List[str]:
    """The norm calls of one forward, in call order."""
    cfg = probe_config(name)
    out = []
    for l in range(cfg.num_hidden_layers):
        out += [f"layer{l}.norm1", f"layer{l}.norm2"]
    if cfg.arch == "llama" or cfg.do_layer_norm_before:
        out.append("final")
    return out


def stat_discrimination(o32: SeamOracle, tokens: Sequence[int], pos0: int = 0) -> Dict[str, float]:
    """Per norm site: the least max-abs movement, over the pass's planted rows, of the fp32 oracle's logits when that
    site's statistics leave each row's planted column out."""
    assert o32.dtype == torch.float32
    cols = [plant_column(o32.name, t) for t in tokens]
    rows = [r for r, c in enumerate(cols) if c >= 0]
    truth, _ = o32.run(tokens, pos0)
    out = {}
    for k, site in enumerate(norm_sites(o32.name)):
        with _DropColumn(k, cols) as patch:
            moved, _ = o32.forward(tokens, pos0)
        assert patch.calls == len(norm_sites(o32.name)), (patch.calls, o32.name)
        out[site] = float((moved - truth)[rows].abs().amax(-1).min())
    return out


def degenerate_discrimination(o32: SeamOracle, tokens: Sequence[int], pos0: int = 0) -> float:
    """The least max-abs movement of a degenerate row's logits when an ordinary token takes its place."""
    truth, _ = o32.run(tokens, pos0)
    worst = float("inf")
    for r, t in enumerate(tokens):
        if B_TOK0 <= t < B_TOK0 + len(B_KINDS):
            other = list(tokens)
            other[r] = ordinary(r + 32)
            moved, _ = o32.forward(other, pos0)
            worst = min(worst, float((moved - truth)[r].abs().max()))
    return worst


# ----------------------------------------------------------------------------- what the GPU test runs
# (route label, environment, w12, model, dtypes, row counts).  The label's route is asserted from the session's profile
# counts and w12_launches() in test_gpu_layer_seams.py; test_seam_probe_cpu.py checks every pass below on the oracle alone.
MANY = (1, 4, 5, 8, 9, 16, 17, 64, 65)
ROUTES = [
    ("fp32", {}, False, "llama_h1024", ("fp32",), (1, 5, 9)),
    ("fp32", {}, False, "llama_h256", ("fp32",), (1, 5, 9)),
    ("fp32", {}, False, "opt_pre_h256", ("fp32",), (1, 5, 9)),
    ("fp32", {}, False, "opt_post_h128", ("fp32",), (1, 5, 9)),
    ("fp32", {}, False, "opt_proj_h128", ("fp32",), (1, 5, 9)),
    ("fp32", {}, False, "llama_h96", ("fp32",), (1, 5, 9)),
    ("default", {}, False, "llama_h1024", ("bf16", "fp16"), MANY),
    ("default", {}, False, "llama_h256", ("bf16", "fp16"), MANY),
    ("default", {}, False, "opt_pre_h256", ("bf16", "fp16"), MANY),
    ("default", {}, False, "opt_post_h128", ("bf16",), MANY),
    ("default", {}, False, "opt_proj_h128", ("bf16",), MANY),
    ("small_off", {"SD_SMALL_PATH": 0}, False, "llama_h1024", ("bf16",), (1, 4)),
    ("small_off", {"SD_SMALL_PATH": 0}, False, "opt_pre_h256", ("bf16",), (1, 4)),
    ("small_all_pro", {"SD_SMALL_PATH": 2}, False, "llama_h1024", ("bf16",), (1, 4)),
    ("small_all_pro", {"SD_SMALL_PATH": 2}, False, "opt_pre_h256", ("bf16",), (1, 4)),
    ("no_embed_pro", {"SD_SMALL_PATH": 0, "SD_FUSE_EMBED_QKV": 0}, False, "llama_h1024", ("bf16",), (1, 4)),
    ("no_embed_pro", {"SD_SMALL_PATH": 0, "SD_FUSE_EMBED_QKV": 0}, False, "opt_pre_h256", ("bf16",), (1, 4)),
    ("norm_on_load0", {"SD_NORM_ON_LOAD": 0}, False, "llama_h1024", ("bf16", "fp16"), (1, 5, 8, 9)),
    ("norm_on_load1", {"SD_NORM_ON_LOAD": 1}, False, "llama_h1024", ("bf16", "fp16"), (1, 5, 8, 9)),
    ("norm_on_load2", {"SD_NORM_ON_LOAD": 2}, False, "llama_h1024", ("bf16", "fp16"), (1, 5, 8, 9)),
    ("two_launch_attn", {"SD_FUSE_ATTN_O": 0}, False, "llama_h1024", ("bf16",), (5,)),
    ("w12", {}, True, "llama_h1024", ("bf16",), (1, 5, 9)),
    ("w12_small_off", {"SD_SMALL_PATH": 0}, True, "llama_h1024", ("bf16",), (1, 4)),
]
PREFILL_ROWS = (130,)              # one call at pos0 = 0 of more than 80 rows: a contiguous pass (64 and 65 rows ride MANY)
PREFILL_MODELS = [("llama_h1024", "bf16"), ("llama_h1024", "fp16"), ("llama_h256", "fp16"), ("opt_pre_h256", "bf16")]
CONTIG_MODELS = ("llama_h1024",)   # every layer GEMM routes 256 rows: the 130 rows are ONE contiguous pass (else chunks of 64)
FAMILIES = ("A", "B")


# Family A where the oracle alone cannot show 20x the 16-bit bar (test_seam_probe_cpu.py measures and prints the factors):
# a norm site that is not claimed (at every row count: None, or at the row counts listed) - at most one per (model, dtype),
# none in fp32.  A first norm acts on the logits through the row's attention result alone, which the keys in front of the
# row dilute (the one ordinary row in front of the planted rows of a 65-row call costs the site half its factor); post-LN
# renormalises the residual stream itself at the next norm, so what its first norm gets wrong survives one sublayer only
A_SITES_DROPPED = {("llama_h256", "bf16"): ("layer0.norm1", None), ("llama_h1024", "bf16"): ("layer1.norm1", (65,)),
                   ("opt_post_h128", "bf16"): ("layer0.norm1", None)}


def route_passes(name: str, dt: str, n: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """(family, tokens) of every pass a route runs at n rows: every plant up to 16 rows, one pass per family beyond."""
    out = []
    for fam in FAMILIES:
        out += [(fam, p) for p in passes(fam, name, n, first_only=n > 16)]
    return out


def all_passes():
    """{(model, dtype name): set of (family, tokens, pos0)} - everything the GPU file feeds, for the CPU check."""
    out: Dict[Tuple[str, str], set] = {}
    for _, _, _, name, dts, ns in ROUTES:
        for dt in dts:
            for n in ns:
                out.setdefault((name, dt), set()).update((f, p, 0) for f, p in route_passes(name, dt, n))
    for name, dt in PREFILL_MODELS:
        for n in PREFILL_ROWS:
            out.setdefault((name, dt), set()).update((f, p, 0) for f, p in route_passes(name, dt, n) if f == "A")
    for name, dt, pos0s, n in KV_CASES:
        for pos0 in pos0s:
            out.setdefault((name, dt), set()).add(kv_pass(name, dt, n) + (pos0,))
    for name, dt in BATCH_MODELS:
        out.setdefault((name, dt), set()).update((f, p, pos0) for f, pos0, p in batch_plan(name, dt))
    out.setdefault(("llama_h8192", "bf16"), set()).add(("A", h8192_pass(), 0))
    return out


def h8192_pass() -> Tuple[int, ...]:
    """The ONE pass of the H = 8192 model: the last 8 column classes (4 .. 16, 4095 | 4096, 8191)."""
    return tuple(plants("A", "llama_h8192")[-MAX_PLANTS:])


# two streams of one sd_batch_forward: (family, cache length, tokens)
BATCH_MODELS = [("llama_h256", "bf16"), ("opt_pre_h256", "fp32")]


def batch_plan(name: str, dt: str):
    a, b = passes("A", name, 5)[0], passes("B", name, 4)[0]
    return [("A", 0, a), ("B", 2, b)]


# E: (model, dtype, pos0 values, rows) of the written-K/V passes: pos0 = max_position - n reads the last row of the RoPE /
# learned-position table
KV_ROWS = 5
KV_CASES = [(name, dt, (0, 1, MAX_POS - KV_ROWS), KV_ROWS)
            for name, dt in (("llama_h256", "fp32"), ("llama_h256", "bf16"), ("llama_h1024", "bf16"), ("opt_pre_h256", "fp32"),
                             ("opt_pre_h256", "bf16"), ("opt_post_h128", "bf16"))]


def kv_pass(name: str, dt: str, n: int) -> Tuple[str, Tuple[int, ...]]:
    """(family, tokens) of a written-K/V pass: Llama - the first family-A pass (K rows of outlier rows, after RoPE); OPT -
    ordinary tokens ("E"), on which a wrong learned position shows best (behind a planted column LayerNorm squeezes the
    position's share of the row)."""
    if probe_config(name).arch == "opt":
        return "E", tuple(ordinary(r) for r in range(n))
    return route_passes(name, dt, n)[0]


KV_SENTINEL = 0x7B                 # finite in every arena format: bf16 / fp16 0x7b7b, fp32 0x7b7b7b7b, e4m3 0x7b


# ----------------------------------------------------------------------------- the launches of a pass, mirrored
def call_chunks(n: int, max_rows: int) -> List[Tuple[int, int]]:
    """(rows, logit rows) of the passes Session.forward cuts a call of n rows into when the logits of its last
    min(n, 64) rows are asked for and one pass carries at most max_rows rows (Session.max_rows)."""
    first_logit, done, out = n - min(n, MAX_LOGIT_ROWS), 0, []
    while done < n:
        m = min(max_rows, n - done)
        lo = max(first_logit, done)
        if done + m - lo > MAX_LOGIT_ROWS:
            m = lo + MAX_LOGIT_ROWS - done
        out.append((m, max(0, done + m - lo)))
        done += m
    return out


def expected_call(name: str, dt: str, n: int, env: Optional[dict], w12, max_rows: int) -> dict:
    """expected_launches summed over the passes of one call (a pass of more than 80 rows is a contiguous one).  w12: False,
    True (every matrix packed) or SpecDecModel.w12_packed (matrix kind -> layers whose records were registered)."""
    tot: Dict[str, int] = {}
    for m, nl in call_chunks(n, max_rows):
        for k, v in expected_launches(name, dt, m, env, w12, contig=m > 80, n_logits=nl).items():
            tot[k] = tot.get(k, 0) + v
    return tot


def expected_launches(name: str, dt: str, n: int, env: Optional[dict] = None, w12=False, contig: bool = False,
                      n_logits: Optional[int] = None) -> dict:
    """{profile class: launches} and "w12" (GEMM launches on 12-bit records) of ONE single-stream pass of n rows with
    n_logits logit rows (default: all of them, at most 64), no key split: forward_small / forward_impl of engine.hip restated.  This is what tells
    the routes apart: the small path has 4 L + 1 GEMM-class launches and one (SD_SMALL_PATH=1) or no norm launch; the
    embedding prologue removes the embed launch; fused attention + O removes the O GEMM; a norm-on-load seam removes a
    residual+norm launch; the 16-bit fused epilogues remove the qkv / activation launches."""
    env = env or {}
    cfg = probe_config(name)
    L, H, D = cfg.num_hidden_layers, cfg.hidden_size, cfg.head_dim
    llama = cfg.arch == "llama"
    pre = llama or cfg.do_layer_norm_before
    is16 = dt != "fp32"
    fused = is16 and cfg.intermediate_size % 8 == 0 and D % 4 == 0
    proj = cfg.word_embed_proj_dim not in (0, H)
    e_small, e_embed = int(env.get("SD_SMALL_PATH", 1)), int(env.get("SD_FUSE_EMBED_QKV", 1))
    e_nol, e_ao = int(env.get("SD_NORM_ON_LOAD", 2)), int(env.get("SD_FUSE_ATTN_O", 1))
    head = 1 if (n if n_logits is None else n_logits) > 0 else 0
    out = {"gemm": 0, "attention": L, "norm_residual": 0, "qkv_rope_append": 0, "activation": 0, "embed": 0, "logits": head, "w12": 0}
    if not contig and small_path_ok(cfg, dt, n, e_small):
        out["gemm"] = 4 * L + head
        out["norm_residual"] = head if e_small == 1 else 0
        return out
    embed_qkv = (dt == "bf16" and e_embed and fused and pre and not proj and not contig and n <= SMALL_MAX_ROWS and H <= 2048
                 and H % 32 == 0)
    qd = cfg.num_attention_heads * D
    oproj = (is16 and e_ao and not contig and D == 128 and n <= 16 and qd // 128 <= 40
             and cfg.num_attention_heads * ((n + 7) // 8) + (H // 16 + 1) // 2 <= 256)
    seams = pre and norm_on_load_ok(cfg, dt, n, e_nol)
    seam_o, seam_d = seams and oproj, seams and e_nol > 1
    if not embed_qkv:
        out["embed"] = 2 if proj else 1
        out["gemm"] += 1 if proj else 0
        out["norm_residual"] += 0 if (not proj and pre) else 1
    for l in range(L):
        xn_q, xn_d = seam_d and l > 0, seam_d and l + 1 < L
        out["gemm"] += 3 + (0 if oproj else 1)
        out["norm_residual"] += (0 if seam_o else 1) + (0 if xn_d else 1)
        if not fused:
            out["qkv_rope_append"] += 1
            out["activation"] += 1
        if w12:
            has = (lambda kind: True) if w12 is True else (lambda kind: l in w12.get(kind, ()))
            out["w12"] += int(xn_q and has("qkv")) + int(seam_o and D == 128 and has("gate_up")) + int(xn_d and has("down"))
    out["gemm"] += head * (2 if proj else 1)
    out["logits"] += head if proj else 0
    return out


# ----------------------------------------------------------------------------- C. planted slabs
def gemm_slabs(N: int, K: int, M: int, env: Optional[dict] = None, small: bool = False) -> Tuple[int, int]:
    """(S, ksp) of the streaming GEMM [N][K] at M rows as sd_gemm_route plans it under the tunables `env`; small: the
    small path's O / down slabs (small_split: the plan at ONE row, at most 16 slabs)."""
    import gemm_route_classes as G
    with G.tunables({k: str(v) for k, v in (env or {}).items() if k.startswith("SD_GEMM") or k.startswith("SD_MM")}):
        r = G.route(N, K, 1 if small else M, 0)
    S, ksp, KS = r.S, r.ksp, K // 32
    if small and S > 16:
        ksp = (KS + 15) // 16
        S = (KS + ksp - 1) // ksp
    return S, ksp


def fold_loops(S: int) -> Dict[str, int]:
    """First slab of each loop of reduce_part / reduce_part4 / logits_kernel that runs at S slabs."""
    out = {}
    if S >= 8:
        out["burst8"] = 0
    if S % 8 >= 4:
        out["burst4"] = S - S % 8
    if S % 4:
        out["tail"] = S - S % 4
    return out


def slab_classes(S: int) -> List[int]:
    return sorted({0, S - 1} | set(fold_loops(S).values()))


# (label, model, dtype, tunables, rows, weight, consumer): the pass runs ordinary tokens; `weight` is the matrix whose slabs
# are planted.  llama_c's down projection [256][4096]: S = 3 (tail alone), 5 (default: 4-burst + tail), 8 (8-burst alone), 13
# (all three loops) in front of residual_norm_kernel (1 row: the small path's streaming slabs, 5 rows: forward_impl) and of
# the head's PRO_RESID prologue (SD_SMALL_PATH=2, gemm_small's slabs); llama_h1024's head [512][1024]: S = 3 in logits_kernel
_DOWN = "model.layers.0.mlp.down_proj.weight"
C_CASES = [(f"down_S{S}_n{n}", "llama_c", "bf16", env, n, _DOWN, "residual_norm_kernel / reduce_part4")
           for S, env in ((3, {"SD_GEMM_UNITS": 48}), (5, {}), (8, {"SD_GEMM_UNITS": 128}), (13, {"SD_GEMM_UNITS": 208}))
           for n in (1, 5)]
C_CASES += [
    ("down_S13_pro", "llama_c", "bf16", {"SD_GEMM_UNITS": 208, "SD_SMALL_PATH": 2}, 1, _DOWN, "PRO_RESID / reduce_part4"),
    ("down_S5_fp16", "llama_c", "fp16", {}, 1, _DOWN, "residual_norm_kernel / reduce_part4"),
    ("head_S3", "llama_h1024", "bf16", {"SD_GEMM_UNITS": 96}, 5, "lm_head.weight", "logits_kernel"),
]
# opt_c's project_out [512][4096] in front of reduce_rows_kernel: S = 3, 5 (default), 8, 13 - every loop of the scalar
# reduce_part; its project_in [4096][512]: S = 2 in front of reduce_addpos_kernel (K = 512 admits no more)
_POUT, _PIN = "model.decoder.project_out.weight", "model.decoder.project_in.weight"
C_CASES += [(f"projout_S{S}", "opt_c", "bf16", env, 5, _POUT, "reduce_rows_kernel / reduce_part")
            for S, env in ((3, {"SD_GEMM_UNITS": 96}), (5, {}), (8, {"SD_GEMM_UNITS": 256}), (13, {"SD_GEMM_UNITS": 416}))]
C_CASES += [("projin_S2", "opt_c", "bf16", {"SD_GEMM_UNITS": 416}, 5, _PIN, "reduce_addpos_kernel / reduce_part"),
            ("projout_S5_fp16", "opt_c", "fp16", {}, 1, _POUT, "reduce_rows_kernel / reduce_part")]
_DOWN1, _O0 = "model.layers.1.mlp.down_proj.weight", "model.layers.0.self_attn.o_proj.weight"
# llama_h1024 (O / down [1024][1024], S = 4: the 4-burst alone) on the routes with their own fold: the 130-row contiguous pass
# (slabs of the many-row kernel), the residual epilogue's own fold (gemm_bf16_stream_fin, norm on load 2; with 12-bit records:
# C_W12), residual_norm_kernel with norm on load 1 / 0, the O projection as its own launch, the small path switched off
_U = {"SD_GEMM_UNITS": 256}
C_CASES += [
    ("down1_S4_prefill130", "llama_h1024", "bf16", {}, 130, _DOWN1, "residual_norm_kernel / reduce_part4"),
    ("down0_S4_fin", "llama_h1024", "bf16", _U, 5, _DOWN, "gemm_bf16_stream_fin's own fold"),
    ("down0_S4_fin_w12", "llama_h1024", "bf16", _U, 5, _DOWN, "gemm_bf16_stream_fin's own fold"),
    ("down0_S4_fin_small_off", "llama_h1024", "bf16", dict(_U, SD_SMALL_PATH=0), 1, _DOWN, "gemm_bf16_stream_fin's own fold"),
    ("down0_S4_nol1", "llama_h1024", "bf16", dict(_U, SD_NORM_ON_LOAD=1), 5, _DOWN, "residual_norm_kernel / reduce_part4"),
    ("o0_S4_nol0_two_launch", "llama_h1024", "fp16", dict(_U, SD_NORM_ON_LOAD=0, SD_FUSE_ATTN_O=0), 5, _O0,
     "residual_norm_kernel / reduce_part4"),
]
C_W12 = {"down0_S4_fin_w12"}       # cases whose model also carries 12-bit records


def c_gain(weight: str) -> float:
    """The planted slab times a power of two: the slab alone decides the logits."""
    return 8.0 if weight.endswith(("down_proj.weight", "o_proj.weight")) else 1.0



def c_slabs(case) -> Tuple[int, int]:
    """(S, ksp) of the planted matrix's GEMM in the case's pass."""
    _, name, dt, env, n, weight, _ = case
    cfg = probe_config(name)
    if weight.endswith(("down_proj.weight", "o_proj.weight")):
        small = small_path_ok(cfg, dt, n, int(env.get("SD_SMALL_PATH", 1)))
        N, K = probe_state_dict(name)[weight].shape
        return gemm_slabs(N, K, n, env, small)
    N, K = probe_state_dict(name)[weight].shape
    return gemm_slabs(N, K, n, env)


def c_tokens(n: int) -> Tuple[int, ...]:
    return tuple(ordinary(r) for r in range(n))


@functools.lru_cache(maxsize=None)
def slab_state_dict(name: str, weight: str, ksp: int, s: Optional[int]) -> Dict[str, torch.Tensor]:
    """The probe weights with `weight` zero outside the k-range of slab s (k-steps of 32 columns, ksp per slab) and times
    c_gain inside; s = None: `weight` all zero (what a fold that skips the slab computes)."""
    sd = dict(probe_state_dict(name))
    w = torch.zeros_like(sd[weight])
    if s is not None:
        lo, hi = s * ksp * 32, min(w.shape[1], (s + 1) * ksp * 32)
        assert lo < hi
        w[:, lo:hi] = sd[weight][:, lo:hi] * c_gain(weight)
    sd[weight] = w
    return sd


def slab_discrimination(name: str, weight: str, ksp: int, s: int, tokens: Sequence[int]) -> float:
    """The least max-abs movement over the rows of the fp32 oracle's logits between the planted slab and none."""
    a = SeamOracle(name, sd=slab_state_dict(name, weight, ksp, s)).forward(tokens)[0]
    b = SeamOracle(name, sd=slab_state_dict(name, weight, ksp, None)).forward(tokens)[0]
    return float((a - b)[-MAX_LOGIT_ROWS:].abs().amax(-1).min())


# ----------------------------------------------------------------------------- D. activation columns
D_TOK0 = 60
D_C0, D_C1 = 1, 2                  # hidden channels that carry the gate / up value of the D tokens (no class of family A)
D_GATES = (-96.0, -20.0, -2.0 ** -10, 2.0 ** -10, 20.0, 96.0)
D_UPS = (1.0, 1.0, 1024.0, 1024.0, 2.0 ** -4, 2.0 ** -6)     # SiLU(gate) * up: -0, -4e-8, -+0.5, 1.25, 1.5
D_A, D_B = 128.0, 1024.0           # the gate row's / up row's one entry
D_GAIN = 16.0                      # on the down_proj column
SILU_OVERFLOW = 88.73              # expf(x) is inf in fp32 from here
D_MODELS = [("llama_h256", "fp32"), ("llama_h256", "bf16"), ("llama_h256", "fp16"), ("llama_h1024", "bf16")]
D_ROWS = {"llama_h256": (1, 4, 9, 17, 64, 65), "llama_h1024": (1, 5)}
# (label, model, dtype, 12-bit records, tunables, rows): every route whose activation seam is its own code.  With records the
# planted gate / up rows (one entry of 128 / 1024 in a row of zeros) put more escapes into a tile than a record holds, so
# the packer leaves layer 0's gate/up matrix in bf16 - asserted from SpecDecModel.w12_packed - and the case runs the
# decisive column next to the record launches of the other matrices
D_CASES = [("default", n, d, False, {}, D_ROWS[n]) for n, d in D_MODELS]
D_CASES += [(lab, "llama_h1024", "bf16", False, env, (1, 5)) for lab, env in (
    ("small_off", {"SD_SMALL_PATH": 0}), ("small_all_pro", {"SD_SMALL_PATH": 2}), ("norm_on_load0", {"SD_NORM_ON_LOAD": 0}),
    ("norm_on_load1", {"SD_NORM_ON_LOAD": 1}), ("two_launch_attn", {"SD_FUSE_ATTN_O": 0}))]
D_CASES += [("small_off", "llama_h256", "bf16", False, {"SD_SMALL_PATH": 0}, (1, 4)),
            ("small_all_pro", "llama_h256", "bf16", False, {"SD_SMALL_PATH": 2}, (1, 4)),
            ("w12", "llama_h1024", "bf16", True, {}, (1, 5)), ("w12_small_off", "llama_h1024", "bf16", True, {"SD_SMALL_PATH": 0}, (1,))]


def act_columns(name: str) -> List[int]:
    I = probe_config(name).intermediate_size
    return [0, 7, 8, 15, 16, 255, 256, I - 1]


@functools.lru_cache(maxsize=None)
def act_state_dict(name: str, j: int, flip: bool = False, swap_up: bool = False) -> Dict[str, torch.Tensor]:
    """The probe weights with intermediate column j of layer 0 made decisive (flip: its gate row negated; swap_up: the up
    rows of columns j and j ^ 8 exchanged - what a fused epilogue computes that pairs gate column j with the up column
    8 away, the offset of the 8-gate / 8-up interleave)."""
    cfg = probe_config(name)
    assert cfg.arch == "llama"
    sd = dict(probe_state_dict(name))
    p = "model.layers.0."
    names = ["model.embed_tokens.weight", p + "self_attn.o_proj.weight", p + "post_attention_layernorm.weight",
             p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", p + "mlp.down_proj.weight"]
    emb, wo, n2, gate, up, down = (sd[k].clone() for k in names)
    emb[:, [D_C0, D_C1]] = 0.0
    wo.zero_()                                                     # layer 0's attention adds nothing: the row reaches the
    n2[[D_C0, D_C1]] = 1.0                                         # second norm as embedded, whatever else rides the pass
    gate[j, :] = 0.0
    up[j, :] = 0.0
    gate[j, D_C0] = -D_A if flip else D_A
    up[j, D_C1] = D_B
    down[:, j] *= D_GAIN
    if swap_up:
        up[[j, j ^ 8]] = up[[j ^ 8, j]]
    toks = torch.arange(D_TOK0, D_TOK0 + len(D_GATES))
    rms = torch.sqrt(emb[toks].pow(2).mean(-1) + cfg.rms_norm_eps)
    emb[toks, D_C0] = _bf16(torch.tensor(D_GATES) * rms / D_A)
    emb[toks, D_C1] = _bf16(torch.tensor(D_UPS) * rms / D_B)
    sd.update(zip(names, (emb, wo, n2, gate, up, down)))
    return sd


def act_passes(n: int) -> List[Tuple[int, ...]]:
    """The six D tokens cut into passes of n rows (all six first from 6 rows on), ordinary tokens behind them."""
    toks = list(range(D_TOK0, D_TOK0 + len(D_GATES)))
    k, first = min(n, len(toks)), n - min(n, MAX_LOGIT_ROWS)
    out = []
    for a in range(0, len(toks), k):
        fill = [ordinary(r) for r in range(n - len(toks[a:a + k]))]
        out.append(tuple(fill[:first] + toks[a:a + k] + fill[first:]))
    return out


class _CaptureSilu:
    """Records column j of what the oracle's first F.silu call is given."""

    def __init__(self, j: int):
        self.j, self.seen = j, None

    def __enter__(self):
        self.F = models_ref.F
        outer = self

        class FProxy:
            def __getattr__(self, k):
                return getattr(outer.F, k)

            @staticmethod
            def silu(x):
                if outer.seen is None:
                    outer.seen = x[0, :, outer.j].float().clone()
                return outer.F.silu(x)

        models_ref.F = FProxy()
        return self

    def __exit__(self, *exc):
        models_ref.F = self.F


def act_gates(o: SeamOracle, j: int, tokens: Sequence[int]) -> torch.Tensor:
    """The gate pre-activations of column j (layer 0) for the pass's rows, as the oracle computes them."""
    with _CaptureSilu(j) as cap:
        o.forward(tokens)
    return cap.seen


def act_discrimination(name: str, j: int, tokens: Sequence[int], swap_up: bool = False) -> float:
    """The least max-abs movement, over the pass's D rows, of the fp32 oracle's logits when column j's gate is negated
    (swap_up: when its up value comes from the column 8 away; only rows whose SiLU(gate) is not 0 can show that)."""
    a = SeamOracle(name, sd=act_state_dict(name, j)).forward(tokens)[0]
    b = SeamOracle(name, sd=act_state_dict(name, j, flip=not swap_up, swap_up=swap_up)).forward(tokens)[0]
    if swap_up:
        rows = [r for r, t in enumerate(tokens) if D_TOK0 + 2 <= t < D_TOK0 + len(D_GATES)]
        return float((a - b)[rows].abs().amax(-1).min()) if rows else float("inf")
    rows = [r for r, t in enumerate(tokens) if D_TOK0 <= t < D_TOK0 + len(D_GATES)]
    return float((a - b)[rows].abs().amax(-1).min())


# ----------------------------------------------------------------------------- D. head columns
H_C2 = 5                           # the hidden channel every token carries at 1 (no class of family A, not D_C0 / D_C1)
H_GAIN = 64.0                      # lm_head[v, H_C2]: the planted logit is 64 / rms(row) - about 50, the others stay under 10
HEAD_MODELS = [("llama_h256", "fp32"), ("llama_h256", "bf16"), ("llama_h256", "fp16"), ("llama_h96", "fp32")]
HEAD_ROWS = (1, 5, 17)


def head_columns(name: str) -> List[int]:
    return [0, 15, 16, 255, 256, probe_config(name).vocab_size - 1]


@functools.lru_cache(maxsize=None)
def head_state_dict(name: str, v: Optional[int]) -> Dict[str, torch.Tensor]:
    """The probe weights with lm_head row v reading channel H_C2 alone (v = None: the channel set up, no row planted)."""
    cfg = probe_config(name)
    assert cfg.arch == "llama"
    sd = dict(probe_state_dict(name))
    emb = sd["model.embed_tokens.weight"].clone()
    emb[:, H_C2] = 1.0
    sd["model.embed_tokens.weight"] = emb
    for l in range(cfg.num_hidden_layers):
        for k in (f"model.layers.{l}.self_attn.o_proj.weight", f"model.layers.{l}.mlp.down_proj.weight"):
            w = sd[k].clone()
            w[H_C2, :] = 0.0                                       # nothing but the embedding writes the channel
            sd[k] = w
    nf = sd["model.norm.weight"].clone()
    nf[H_C2] = 1.0
    head = sd["lm_head.weight"].clone()
    head[:, H_C2] = 0.0
    if v is not None:
        head[v, :] = 0.0
        head[v, H_C2] = H_GAIN
    sd["model.norm.weight"], sd["lm_head.weight"] = nf, head
    return sd


def head_tokens(n: int) -> Tuple[int, ...]:
    return tuple(ordinary(r) for r in range(n))


def head_discrimination(name: str, v: int, tokens: Sequence[int]) -> float:
    a = SeamOracle(name, sd=head_state_dict(name, v)).forward(tokens)[0]
    b = SeamOracle(name, sd=head_state_dict(name, None)).forward(tokens)[0]
    return float((a - b).abs().amax(-1).min())


# ----------------------------------------------------------------------------- D. OPT: fc1 bias edges
R_A = 2.0 * (1.0 + 2.0 ** -7)      # fc1[j, D_C0] and the LayerNorm bias of channel D_C0: A * beta = 4 (1 + 2^-6 + 2^-14) exactly
R_BIAS = -4.0 * (1.0 + 2.0 ** -6)  # fc1.bias[j]: the fp32 sum is 2^-12; with the dot rounded to bf16 first it is 0
R_GAIN = 2.0 ** 16                 # on fc2's column j: ReLU(2^-12) * 2^16 = 16 times the column
R_KINDS = ("cancel", "neg0", "subnormal")
RELU_MODELS = [("opt_pre_h256", "fp32"), ("opt_pre_h256", "bf16"), ("opt_pre_h256", "fp16")]
RELU_ROWS = (1, 5, 17)
RELU_CASES = [("default", n, d, {}, RELU_ROWS) for n, d in RELU_MODELS]
RELU_CASES += [("small_off", "opt_pre_h256", "bf16", {"SD_SMALL_PATH": 0}, (1,)),
               ("small_all_pro", "opt_pre_h256", "bf16", {"SD_SMALL_PATH": 2}, (1,))]


@functools.lru_cache(maxsize=None)
def relu_state_dict(name: str, j: int, kind: Optional[str]) -> Dict[str, torch.Tensor]:
    """OPT probe weights with fc1 row j of layer 0 reading channel D_C0 alone, which the second LayerNorm makes a constant.
    kind: "cancel" (pre-activation 2^-12 = A * beta + bias), "neg0" / "subnormal" (dot 0; bias -0.0 / 2^-133), None (row
    and bias zero: what a kernel computes that loses the column, or rounds the dot before the bias add)."""
    cfg = probe_config(name)
    assert cfg.arch == "opt" and cfg.do_layer_norm_before
    sd = dict(probe_state_dict(name))
    p = "model.decoder.layers.0."
    names = [p + "final_layer_norm.weight", p + "final_layer_norm.bias", p + "fc1.weight", p + "fc1.bias", p + "fc2.weight"]
    nw, nb, w1, b1, w2 = (sd[k].clone() for k in names)
    nw[D_C0], nb[D_C0] = 0.0, R_A
    w1[j, :] = 0.0
    b1[j] = 0.0
    if kind == "cancel":
        w1[j, D_C0], b1[j] = R_A, R_BIAS
    elif kind == "neg0":
        b1[j] = -0.0
    elif kind == "subnormal":
        b1[j] = 2.0 ** -133
    w2[:, j] *= R_GAIN
    sd.update(zip(names, (nw, nb, w1, b1, w2)))
    return sd


def relu_discrimination(name: str, j: int, kind: str, tokens: Sequence[int]) -> float:
    a = SeamOracle(name, sd=relu_state_dict(name, j, kind)).forward(tokens)[0]
    b = SeamOracle(name, sd=relu_state_dict(name, j, None)).forward(tokens)[0]
    return float((a - b).abs().amax(-1).min())
