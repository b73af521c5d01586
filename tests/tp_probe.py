"""Probes for the tensor-parallel forward (helper of test_tp_probe_cpu.py and test_gpu_tp_routes.py; needs no GPU).

A shard's O and down projections are row-parallel GEMMs whose fp32 partials tp_reduce (csrc/engine.hip) sums over the
group: tp_fold_kernel folds the rank's own k-slabs where the GEMM left more than one, tp_sum_kernel adds the ranks' partials
in rank order (the loopback group; RCCL's all-reduce in its place otherwise).  Which GEMM kernel feeds the reduce, and with
how many slabs, depends on (hidden, K / world, rows): the probe models below are the issue's shapes, at which
sd_gemm_route - asked at run time, never trusted from a table - reaches every class of `CLASSES`:

  tp_h1024  hidden 1024, 8 heads x 128, 4 KV heads, intermediate 4096, 2 layers (a layer boundary behind a down reduce)
            world 2: O (1024, 512), down (1024, 2048); world 4: O (1024, 256) - no kernel past 64 rows, the shard's row
            limit drops to 64 - and down (1024, 1024)
  tp_h4096  hidden 4096, 32 heads x 128, 8 KV heads, intermediate 1024, 1 layer, bf16 only on the GPU
            world 2: O (4096, 2048) - one slab only because the one-slab flag forces it up to 16 rows; world 8: O (4096, 512),
            four query heads and one KV head per rank, and down (4096, 128) - intermediate 1024 / 8, which has no kernel
            past 64 rows, so this shard's row limit is 64 as well

(No smaller shape was found that keeps the forced one-slab class: it needs N x K large enough for the planner to split K
at <= 16 rows, which (4096, 2048) is the smallest listed shard shape to do.)  Vocabulary 256: the head has a kernel at
every row count.  Weights are synth.make_state_dict rounded to bf16, so one dict serves fp32 and bf16.

Plants (state dicts derived from the base weights):
  rank plant r   o_proj / down_proj of every layer zero outside rank r's input-column slice and times RANK_GAINS[r] inside:
                 rank r's partial alone decides every reduce, so a sum that drops rank r, reads another rank in its place
                 or stops one rank early returns the logits of zero projections;
  slab plant     for a shard route with S > 1: the weight zero outside ONE k-slab of ONE rank (the slab's k-range in the
                 rank's local k order, i.e. columns rank * K_local + [s * ksp * 32, (s + 1) * ksp * 32) of the full matrix).
Rows: every pass of >= 5 rows carries the all-zero, 2^-60, alternating and large-mean rows of seam_probe's family B in front
of ordinary token rows, so the reduce sees partials of very different magnitude per row.

TpOracle wraps the unsharded oracle.RefCausalLM on the full weights (algebraically the sharded forward, oracle/tp_ref.py)
and, as a second path, runs oracle.tp_ref.llama_forward_tp for all ranks in lock step (one thread per rank, the all-reduce
a rendezvous) with an optional Fault: drop a rank, read one rank over another, or skip one k-slab of a rank's partial.

run_ranks runs one callable per rank, each on its own daemon thread and HIP stream.  A rank that raises or does not come
back poisons the module: a rank parked in TpLoop::barrier holds its stream, and nothing may be started behind it.
"""
from __future__ import annotations

import functools
import threading
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

import oracle
from oracle import tp_ref
from seam_probe import (ALT_M, FP32_TOL, KV_SENTINEL, MAX_LOGIT_ROWS, TINY, call_chunks, cast_sd, errors, slab_classes,  # noqa: F401
                        tol16, tree_shape)
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict
from llmspeculativesampling_amd.tp import shard_config, shard_tensor

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
PREFIX = 150                       # cached rows in front of a pass (0 or PREFIX)
MAX_POS = PREFIX + 256 + 10        # the prefix, one pass of the largest row count, a few rows behind it

MODELS: Dict[str, dict] = {
    "tp_h1024": dict(arch="llama", vocab_size=256, hidden_size=1024, intermediate_size=4096, num_hidden_layers=2,
                     num_attention_heads=8, num_key_value_heads=4, max_position_embeddings=MAX_POS, rms_norm_eps=1e-5),
    "tp_h4096": dict(arch="llama", vocab_size=256, hidden_size=4096, intermediate_size=1024, num_hidden_layers=1,
                     num_attention_heads=32, num_key_value_heads=8, max_position_embeddings=MAX_POS, rms_norm_eps=1e-5),
}
WORLDS = {"tp_h1024": (2, 4), "tp_h4096": (2, 8)}
GPU_DTYPES = {"tp_h1024": ("fp32", "bf16"), "tp_h4096": ("bf16",)}
CASES = [(name, world, dt) for name in MODELS for world in WORLDS[name] for dt in GPU_DTYPES[name]]
ROWS = (1, 5, 16, 17, 64, 65, 144, 145)        # both sides of every class edge of the planner; + the session's max_rows
RANK_GAINS = (8.0, 16.0, 8.0, 16.0, 8.0, 16.0, 8.0, 16.0)       # powers of two (exact in bf16); neighbours always differ


def slab_gain(S: int) -> float:
    """The planted slab times a power of two, so that the slab alone decides the logits: seam_probe.c_gain's 8 up to four
    slabs, 32 beyond (an eighth of the k-range at 8 reaches 13 .. 17x the bf16 bar only)."""
    return 8.0 if S <= 4 else 32.0


B_TOK0, ORD_TOK0, PRE_TOK0 = 40, 64, 160
B_KINDS = ("zero", "tiny", "alt", "mean")


def probe_config(name: str) -> ModelConfig:
    return ModelConfig(**MODELS[name])


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _base(name: str, seed: int) -> Dict[str, torch.Tensor]:
    cfg = probe_config(name)
    sd = {k: _bf16(v) for k, v in make_state_dict(cfg, seed, head_gain=2.0).items()}
    emb = sd["model.embed_tokens.weight"]
    col = torch.arange(emb.shape[1])
    emb[B_TOK0 + 0] = 0.0
    emb[B_TOK0 + 1] = TINY
    # (alternating and large-mean rows at the magnitude of an ordinary row, by powers of two: a row that is 16 times the
    # others drowns what the projections add to it, and with it every fault of the reduce)
    emb[B_TOK0 + 2] = torch.where(col % 2 == 0, ALT_M, -ALT_M) * 0.5
    emb[B_TOK0 + 3] = (16.0 + (col % 8).float() / 8.0) * 2.0 ** -4
    return sd


def base_state_dict(name: str, seed: int = 47) -> Dict[str, torch.Tensor]:
    """fp32 tensors whose values are all bf16 numbers.  Shared: do not modify."""
    return _base(name, seed)


# ----------------------------------------------------------------------------- rows
def ordinary(r: int) -> int:
    return ORD_TOK0 + r % 96


def prefix_tokens(pos0: int) -> List[int]:
    return [PRE_TOK0 + i % 96 for i in range(pos0)]


def tokens(n: int, salt: int = 0) -> Tuple[int, ...]:
    """The rows of a pass of n rows: ordinary tokens, and from 5 rows on the four degenerate rows behind the first row whose
    logits the call returns (its last 64) - behind, because an all-zero row with no key but itself has all-zero partials
    on every rank, which no reduce can get wrong."""
    if n < 5:
        return tuple(ordinary(r + salt) for r in range(n))
    deg = [B_TOK0 + i for i in range(len(B_KINDS))]
    fill = [ordinary(r + salt) for r in range(n - len(deg))]
    first = n - min(n, MAX_LOGIT_ROWS) + 1
    return tuple(fill[:first] + deg + fill[first:])


# ----------------------------------------------------------------------------- the route table
CLASSES = ("stream S=1 natural", "stream S=1 forced", "stream S>1", "rows S=1", "rows S>1", "mm S>1", "none")


def shard_shapes(name: str, world: int) -> Dict[str, Tuple[int, int]]:
    """{"o" | "down": (N, K_local)} of one of `world` shards."""
    cfg = probe_config(name)
    return {"o": (cfg.hidden_size, cfg.num_attention_heads // world * cfg.head_dim),
            "down": (cfg.hidden_size, cfg.intermediate_size // world)}


def _route_pair(N: int, K: int, M: int):
    import gemm_route_classes as G
    return G.route(N, K, M, G.ONE_SLAB), G.route(N, K, M, 0)


def route_class(N: int, K: int, M: int) -> Tuple[str, int, int]:
    """(class, S, ksp) of a shard's row-parallel GEMM [N][K] at M rows: sd_gemm_route with SD_GN_ONE_SLAB, as
    plan_forward asks it for a session bound to a group, and with need 0 to tell a forced single slab from a natural one."""
    import gemm_route_classes as G
    r1, r0 = _route_pair(N, K, M)
    kind = G.KIND_NAMES[r1.kind]
    if kind == "none":
        return "none", 0, 0
    if kind == "stream" and r1.S == 1:
        forced = G.KIND_NAMES[r0.kind] != "none" and r0.S > 1
        return ("stream S=1 forced" if forced else "stream S=1 natural"), 1, r1.ksp
    return f"{kind} S{'=1' if r1.S == 1 else '>1'}", r1.S, r1.ksp


def reduce_routes(name: str, world: int, rows: int) -> Dict[str, Tuple[str, int, int]]:
    """{"o" | "down": (class, S, ksp)} of ONE pass of `rows` rows on a bf16 shard."""
    return {role: route_class(N, K, rows) for role, (N, K) in shard_shapes(name, world).items()}


def shard_handle(name: str, world: int):
    """(sd_model handle of a bf16 shard - no weights behind it, for the planner's queries only -, what keeps it alive)."""
    from test_gemm_routes_cpu import _model_handle
    cfg = shard_config(probe_config(name), world)
    m = ("llama", cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.head_dim,
         cfg.vocab_size, 0)
    handle, keep = _model_handle(m, layers=cfg.num_hidden_layers)
    assert handle is not None, (name, world)
    return handle, keep


@functools.lru_cache(maxsize=None)
def shard_max_rows(name: str, world: int, dt: str = "bf16") -> int:
    """Session.max_rows of a shard: sd_model_max_rows of the bf16 shard (an fp32 model has one GEMM kernel and no limit)."""
    from llmspeculativesampling_amd import _lib
    if dt == "fp32":
        return 256
    handle, keep = shard_handle(name, world)
    try:
        return int(_lib.lib.sd_model_max_rows(handle))
    finally:
        _lib.lib.sd_model_destroy(handle)
        del keep


def probe_rows(name: str, world: int, dt: str = "bf16") -> List[int]:
    """The row counts of the calls to run.  A count past the shard's max_rows is a call that Session.forward cuts into
    passes of at most max_rows rows (seam_probe.call_chunks)."""
    return sorted(set(ROWS) | {shard_max_rows(name, world, dt)})


def call_routes(name: str, world: int, dt: str, n: int) -> List[Tuple[int, int, Dict[str, Tuple[str, int, int]]]]:
    """(rows, logit rows, reduce routes) of every pass of a call of n rows; an fp32 shard has one slab everywhere."""
    out = []
    for m, nl in call_chunks(n, shard_max_rows(name, world, dt)):
        routes = {"o": ("fp32", 1, 0), "down": ("fp32", 1, 0)} if dt == "fp32" else reduce_routes(name, world, m)
        out.append((m, nl, routes))
    return out


def expected_other(name: str, world: int, dt: str, n: int) -> Tuple[int, int]:
    """(tp_fold_kernel launches, tp_sum_kernel launches) of a call of n rows: per layer and projection one sum, and one fold
    where the GEMM left more than one slab.  The profile's class "other" counts their sum."""
    L = probe_config(name).num_hidden_layers
    folds = sums = 0
    for _, _, routes in call_routes(name, world, dt, n):
        for cls, S, _ in routes.values():
            assert cls != "none", (name, world, dt, n)
            folds += L * int(S > 1)
            sums += L
    return folds, sums


# ----------------------------------------------------------------------------- plants
_ROW_PAR = ("self_attn.o_proj.weight", "mlp.down_proj.weight")


def _layers(name: str):
    return range(probe_config(name).num_hidden_layers)


def rank_slice(name: str, key: str, rank: int, world: int) -> Tuple[int, int]:
    """Rank `rank`'s input columns of a row-parallel weight (tp.shard_tensor's cut)."""
    n = base_state_dict(name)[key].shape[1] // world
    return rank * n, (rank + 1) * n


@functools.lru_cache(maxsize=None)
def rank_state_dict(name: str, world: int, rank: int) -> Dict[str, torch.Tensor]:
    sd = dict(base_state_dict(name))
    for l in _layers(name):
        for suffix in _ROW_PAR:
            key = f"model.layers.{l}.{suffix}"
            lo, hi = rank_slice(name, key, rank, world)
            w = torch.zeros_like(sd[key])
            w[:, lo:hi] = sd[key][:, lo:hi] * RANK_GAINS[rank]
            sd[key] = w
    return sd


def slab_range(name: str, key: str, world: int, rank: int, ksp: int, s: int) -> Tuple[int, int]:
    """Columns of the FULL weight that are k-slab s of rank `rank`'s GEMM (k-steps of 32 columns, ksp per slab)."""
    lo, hi = rank_slice(name, key, rank, world)
    a, b = lo + s * ksp * 32, min(hi, lo + (s + 1) * ksp * 32)
    assert lo <= a < b <= hi, (key, world, rank, ksp, s)
    return a, b


@functools.lru_cache(maxsize=None)
def slab_state_dict(name: str, key: str, world: int, rank: int, ksp: int, s: Optional[int], gain: float = 8.0) -> Dict[str, torch.Tensor]:
    """`key` zero outside k-slab s of rank `rank` (times `gain` inside); s = None: all zero."""
    sd = dict(base_state_dict(name))
    w = torch.zeros_like(sd[key])
    if s is not None:
        a, b = slab_range(name, key, world, rank, ksp, s)
        w[:, a:b] = sd[key][:, a:b] * gain
    sd[key] = w
    return sd


def slab_key(name: str, role: str) -> str:
    """The planted matrix of a role: the LAST layer's (its reduce is the one the logits see most directly)."""
    l = probe_config(name).num_hidden_layers - 1
    return f"model.layers.{l}." + ("self_attn.o_proj.weight" if role == "o" else "mlp.down_proj.weight")


def slab_cases(name: str, world: int) -> List[Tuple[str, int, int, int, int, int]]:
    """(role, rows, S, ksp, rank, slab) of the slab plants of a bf16 shard: per role and per distinct (S, ksp) among the
    passes of probe_rows the smallest row count that takes it, one case per slab class of slab_classes(S); the planted rank
    walks over the group with the case number."""
    out, k = [], 0
    for role in ("o", "down"):
        seen = set()
        for n in probe_rows(name, world):
            if n > shard_max_rows(name, world):
                continue
            cls, S, ksp = reduce_routes(name, world, n)[role]
            if S > 1 and (cls, S, ksp) not in seen:
                seen.add((cls, S, ksp))
                for s in slab_classes(S):
                    out.append((role, n, S, ksp, k % world, s))
                    k += 1
    return out


# ----------------------------------------------------------------------------- the oracle
@dataclass(frozen=True)
class Fault:
    """What a wrong reduce computes.  kind "drop": rank a's partial is left out; "dup": rank a's partial is read in rank b's
    place; "slab": columns [lo, hi) of the FULL matrix `key` are missing from their rank's GEMM (a fold that skips the slab)."""
    kind: str
    a: int = 0
    b: int = 0
    key: str = ""
    lo: int = 0
    hi: int = 0


class TpOracle:
    """The unsharded oracle.RefCausalLM of a probe model in one dtype (`run` caches by (tokens, pos0)), and the lock-step
    sharded forward of oracle.tp_ref on the same weights."""

    def __init__(self, name: str, dtype=torch.float32, sd=None):
        self.name, self.dtype, self.cfg = name, dtype, probe_config(name)
        self.sd = cast_sd(sd if sd is not None else base_state_dict(name), dtype)
        self.lm = oracle.RefCausalLM(self.cfg, self.sd)
        self._past, self._runs = {}, {}

    def past(self, pos0: int):
        if pos0 == 0:
            return None
        if pos0 not in self._past:
            self._past[pos0] = self.lm(torch.tensor([prefix_tokens(pos0)])).past_key_values
        return self._past[pos0]

    def forward(self, toks: Sequence[int], pos0: int = 0):
        o = self.lm(torch.tensor([list(toks)]), past_key_values=self.past(pos0))
        return o.logits.float()[0], o.past_key_values

    def run(self, toks: Sequence[int], pos0: int = 0):
        key = (tuple(toks), pos0)
        if key not in self._runs:
            self._runs[key] = self.forward(toks, pos0)
        return self._runs[key]

    def tree(self, toks: Sequence[int], base: int, pos: Sequence[int], bits: Sequence[int]):
        N = len(toks)
        mask = torch.ones((1, N, base + N), dtype=torch.bool)
        for i, b in enumerate(bits):
            mask[0, i, base:] = torch.tensor([(b >> j) & 1 == 1 for j in range(N)])
        o = self.lm(torch.tensor([list(toks)]), past_key_values=self.past(base), extra_attention_mask=mask,
                    position_ids=torch.tensor([list(pos)]))
        return o.logits.float()[0], o.past_key_values

    # -- the sharded path ------------------------------------------------------------------------------------------------
    def _shard_sds(self, world: int, fault: Optional[Fault]):
        out = []
        for r in range(world):
            sd = {k: shard_tensor(self.cfg, k, v, r, world) for k, v in self.sd.items()}
            if fault is not None and fault.kind == "slab":
                n = self.sd[fault.key].shape[1] // world
                if r * n <= fault.lo and fault.hi <= (r + 1) * n:
                    w = sd[fault.key].clone()
                    w[:, fault.lo - r * n:fault.hi - r * n] = 0
                    sd[fault.key] = w
            out.append(sd)
        return out

    def sharded(self, world: int, toks: Sequence[int], pos0: int = 0, fault: Optional[Fault] = None, limit_s: float = 300.0):
        """Logits [n, V] of oracle.tp_ref.llama_forward_tp run for all `world` ranks in lock step; every rank's logits are
        asserted equal.  The all-reduce adds the partials in rank order, as tp_sum_kernel does."""
        cfg_l = shard_config(self.cfg, world)
        sds = self._shard_sds(world, fault)
        ids = torch.tensor([list(toks)])
        full_past = self.past(pos0)
        hk = cfg_l.num_key_value_heads
        pasts = [None if full_past is None else [(k[:, r * hk:(r + 1) * hk], v[:, r * hk:(r + 1) * hk]) for k, v in full_past]
                 for r in range(world)]
        bar = threading.Barrier(world, timeout=limit_s)
        slots: List[Optional[torch.Tensor]] = [None] * world
        out: List[Optional[torch.Tensor]] = [None] * world
        errs = []

        def all_reduce(r: int, t: torch.Tensor, fault: Optional[Fault] = fault) -> torch.Tensor:
            slots[r] = t
            bar.wait()
            parts = list(slots)
            if fault is not None and fault.kind == "drop":
                parts[fault.a] = torch.zeros_like(t)
            elif fault is not None and fault.kind == "dup":
                parts[fault.b] = parts[fault.a]
            total = parts[0].clone()
            for p in parts[1:]:
                total += p
            bar.wait()
            return total

        def work(r: int):
            try:
                with torch.no_grad():
                    out[r] = tp_ref.llama_forward_tp(cfg_l, sds[r], ids, pasts[r], lambda t: all_reduce(r, t))[0][0]
            except BaseException as e:                              # noqa: BLE001
                errs.append((r, repr(e)))
                bar.abort()
        ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(limit_s)
        assert not errs and all(not t.is_alive() for t in ts), errs
        for r in range(1, world):
            assert torch.equal(out[0], out[r]), (self.name, world, r)
        return out[0]


def faults_of(name: str, world: int) -> List[Fault]:
    """Drop each rank; read each rank's right neighbour in its place (what a sum that indexes the buffers one off does;
    with rank world - 1 dropped this is also the sum that stops at world - 1)."""
    return [Fault("drop", a=r) for r in range(world)] + [Fault("dup", a=(r + 1) % world, b=r) for r in range(world)]


def moved(a: torch.Tensor, b: torch.Tensor, nl: int) -> float:
    """The least max-abs movement over the observed logit rows (the last nl) between two forwards."""
    return float((a - b)[-nl:].abs().amax(-1).min())


# ----------------------------------------------------------------------------- the rank runner
_POISON: List[str] = []


def poisoned() -> Optional[str]:
    return _POISON[0] if _POISON else None


def run_ranks(fns: Sequence[Callable[[], object]], limit_s: float):
    """One callable per rank, each on its own daemon thread and HIP stream; returns their results in rank order.  Build and
    validate every argument BEFORE the call: a rank that raises in front of a rendezvous leaves the others waiting in it.
    If a rank raises or the join runs out, the module is poisoned and every later call fails at once, without touching
    the GPU: a rank parked in TpLoop::barrier holds its stream."""
    assert not _POISON, f"an earlier rank run failed ({_POISON[0]}): no further group is opened in this process"
    assert 1 <= len(fns) <= 8, len(fns)
    out, errs = [None] * len(fns), []
    streams = [torch.cuda.Stream() for _ in fns]

    def work(r: int):
        try:
            with torch.cuda.stream(streams[r]):
                out[r] = fns[r]()
                streams[r].synchronize()
        except BaseException as e:                                  # noqa: BLE001
            errs.append((r, repr(e)))
    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(len(fns))]
    for t in ts:
        t.start()
    import time
    deadline = time.monotonic() + limit_s
    for t in ts:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [r for r, t in enumerate(ts) if t.is_alive()]
    if errs or alive:
        _POISON.append(f"errors {errs}, ranks still running after {limit_s} s: {alive}")
        raise AssertionError(_POISON[0])
    return out


# ----------------------------------------------------------------------------- what both test files run
def plant_list(name: str, world: int, dt: str) -> List[Tuple[str, Optional[tuple]]]:
    """(label, spec) of the base weights and every plant of a (probe, world, dtype): spec None - the base weights;
    ("rank", r); ("slab", role, rows, S, ksp, rank, s) - bf16 only, an fp32 shard leaves one slab everywhere."""
    out: List[Tuple[str, Optional[tuple]]] = [("base", None)]
    out += [(f"rank{r}", ("rank", r)) for r in range(world)]
    if dt != "fp32":
        out += [(f"slab-{role}-n{n}-S{S}-rank{r}-s{s}", ("slab", role, n, S, ksp, r, s)) for role, n, S, ksp, r, s in slab_cases(name, world)]
    return out


def plant_state_dict(name: str, world: int, spec: Optional[tuple]) -> Dict[str, torch.Tensor]:
    if spec is None:
        return base_state_dict(name)
    if spec[0] == "rank":
        return rank_state_dict(name, world, spec[1])
    _, role, _, S, ksp, r, s = spec
    return slab_state_dict(name, slab_key(name, role), world, r, ksp, s, slab_gain(S))


def plant_faults(name: str, world: int, spec: Optional[tuple]) -> List[Fault]:
    """The faults a plant must show: the base weights every fault of faults_of; rank plant r the sums that lose rank r;
    a slab plant the fold that skips the planted slab."""
    if spec is None:
        return faults_of(name, world)
    if spec[0] == "rank":
        r = spec[1]
        return [Fault("drop", a=r), Fault("dup", a=(r + 1) % world, b=r)]
    _, role, _, _, ksp, r, s = spec
    key = slab_key(name, role)
    lo, hi = slab_range(name, key, world, r, ksp, s)
    return [Fault("slab", key=key, lo=lo, hi=hi)]


def plant_calls(name: str, world: int, dt: str, spec: Optional[tuple]) -> List[Tuple[int, int]]:
    """(rows, cached prefix) of the calls a plant rides on the GPU: the base weights and the rank plants every probe_rows count
    behind 0 and PREFIX cached rows; a slab plant the row count whose route cuts the slab, behind both."""
    rows = probe_rows(name, world, dt) if spec is None or spec[0] == "rank" else [spec[2]]
    return [(n, pos0) for n in rows for pos0 in (0, PREFIX)]


FACTOR = 20                        # the house condition of test_seam_probe_cpu.py
BASE_FAULT_CALLS = ((1, 0), (5, 0), (65, PREFIX))


def fault_calls(name: str, world: int, dt: str, spec: Optional[tuple]) -> List[Tuple[int, int]]:
    """The calls on which test_tp_probe_cpu.py injects a plant's faults, i.e. the calls on which the plant CLAIMS to show them
    (the fault-free sharded oracle is compared with the unsharded one on every call of plant_calls).  A fault of the reduce is
    elementwise over [rows][hidden]; what a call adds is the route its row count takes, not its prefix.  So: a rank plant, and
    the base weights in fp32, every row count of probe_rows, behind 0 and PREFIX cached rows in turn; a slab plant both of its
    calls; the base weights in bf16 - rejected at every world size, they claim nothing - the three calls their listed
    factor was measured on."""
    calls = plant_calls(name, world, dt, spec)
    if spec is not None and spec[0] == "slab":
        return calls
    if spec is None and dt != "fp32":
        return [c for c in calls if c in BASE_FAULT_CALLS]
    rows = sorted({n for n, _ in calls})
    return [(n, (0, PREFIX)[i % 2]) for i, n in enumerate(rows)]


# Plants that cannot show 20x the bar on the oracle alone, with the factor measured by test_tp_probe_cpu.py (which asserts
# this table): they still run on the GPU against the bars, but claim no discrimination.  In bf16 the BASE weights are
# such a plant at every world size: a dropped or doubled rank moves i.i.d. logits by a few bars only.
REJECTED: Dict[Tuple[str, int, str, str], float] = {
    ("tp_h1024", 2, "bf16", "base"): 18.7, ("tp_h1024", 4, "bf16", "base"): 13.1,
    ("tp_h4096", 2, "bf16", "base"): 19.2, ("tp_h4096", 8, "bf16", "base"): 7.9,
}


def admitted(name: str, world: int, dt: str) -> List[Tuple[str, Optional[tuple]]]:
    return [(lab, spec) for lab, spec in plant_list(name, world, dt) if (name, world, dt, lab) not in REJECTED]
