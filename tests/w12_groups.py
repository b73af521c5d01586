"""Planted escapes for the GEMMs that stream 12-bit weight records (csrc/normload_kernels.h) - host side, no GPU.

The kernels request a wave's weight tiles in bursts - groups of four k-steps and, in the finishing GEMM, a tail of one to
three; the finishing GEMM settles the escapes of a burst behind one branch, the norm-on-load GEMM tile by tile in front of
each MFMA of the group.  This module works out which k-steps form which burst of
which wave, picks bursts whose tiles have no escape of their own (w12_format.pack says so), and plants zeros - a zero under
a tile's exponent window is an escape - so that every burst shape, escape count and escape position the repair handles
occurs with an exact, known count.  The plan is a map tensor name -> flat indices to zero, which `transform` applies to
the tensors of SpecDecModel.synthetic(method="numpy"); the same tensors are regenerated here, so everything is checked
before a GPU sees it."""
import ctypes as C
import functools

import numpy as np

import w12_format as F
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import _scale, param_shapes

SEED = 21


def config(intermediate):
    return ModelConfig(arch="llama", vocab_size=4096, hidden_size=1024, intermediate_size=intermediate, num_hidden_layers=2,
                       num_attention_heads=8, num_key_value_heads=8, max_position_embeddings=512, rms_norm_eps=1e-5)


@functools.lru_cache(maxsize=None)
def _host_tensor(intermediate, name):
    cfg = config(intermediate)
    shapes = {n: (i, s, k) for i, (n, s, k) in enumerate(param_shapes(cfg))}
    idx, shape, kind = shapes[name]
    mean, std = _scale(kind, shape, 1.0, 4.0)
    rng = np.random.default_rng([SEED, idx])
    return rng.standard_normal(size=shape, dtype=np.float32) * np.float32(std) + np.float32(mean)


def host_tensor(cfg, name):
    """The float32 tensor SpecDecModel.synthetic(cfg, SEED, method="numpy") generates for `name` (a copy)."""
    return _host_tensor(cfg.intermediate_size, name).copy()


# ---- the three matrices that are read as records in a 2-layer model, in the layout the engine fuses them to ----------------
def _names(kind):
    if kind == "qkv":
        return [f"model.layers.1.self_attn.{n}_proj.weight" for n in "qkv"]
    if kind == "gate_up":
        return ["model.layers.0.mlp.gate_proj.weight", "model.layers.0.mlp.up_proj.weight"]
    return ["model.layers.0.mlp.down_proj.weight"]


def _fuse(cfg, kind, parts):
    """engine.SpecDecModel._build's row order, on numpy arrays [rows][K] of any dtype."""
    if kind == "qkv":
        q, k, v = parts
        D, K = cfg.head_dim, q.shape[1]
        q = q.reshape(-1, 2, D // 2, K).transpose(0, 2, 1, 3).reshape(-1, K)
        k = k.reshape(-1, 2, D // 2, K).transpose(0, 2, 1, 3).reshape(-1, K)
        return np.concatenate([q, k, v], 0)
    if kind == "gate_up":
        g, u = parts
        K = g.shape[1]
        return np.stack([g.reshape(-1, 8, K), u.reshape(-1, 8, K)], 1).reshape(-1, K)
    return parts[0]


def fused_bits(cfg, kind, plan=None):
    """bf16 bits [N][K] of the fused matrix, with the zeros of `plan` (name -> flat indices) planted."""
    parts = []
    for n in _names(kind):
        t = host_tensor(cfg, n)
        if plan and n in plan:
            t.reshape(-1)[plan[n]] = 0
        parts.append(F.f32_to_bf16(t).reshape(t.shape))
    return _fuse(cfg, kind, parts)


def _source(cfg, kind):
    """[N][K] of (tensor number << 32 | flat index): where each element of the fused matrix comes from."""
    parts = []
    for i, n in enumerate(_names(kind)):
        shape = {m: s for m, s, _ in param_shapes(cfg)}[n]
        parts.append((np.arange(int(np.prod(shape)), dtype=np.int64) + (np.int64(i) << np.int64(32))).reshape(shape))
    return _fuse(cfg, kind, parts)


# ---- which k-steps a wave decodes together ------------------------------------------------------------------------------
def down_split(cfg):
    """(S, ksp) of the down projection's k-split at every row count of a <= 8-row pass (sd_gemm_route: the planner)."""
    from llmspeculativesampling_amd import _lib
    got = set()
    for M in range(1, 9):
        info = _lib.SdGemmRouteInfo()
        assert _lib.lib.sd_gemm_route(cfg.hidden_size, cfg.intermediate_size, M, 0, C.byref(info)) == _lib.SD_OK
        assert info.kind == _lib.SD_GEMM_STREAM
        got.add((info.S, info.ksp))
    assert len(got) == 1, got
    return got.pop()


def bursts(KS, S, ksp):
    """[(slab, wave, [k-steps], is_tail)] of one n-tile, as gemm_bf16_stream_xn (S = 1) and gemm_bf16_stream_fin cut K:
    a workgroup per slab, four waves, each wave its quarter in groups of four k-steps and a tail of what is left."""
    out = []
    for sb in range(S):
        kb0, kb1 = sb * ksp, min(KS, sb * ksp + ksp)
        per = (kb1 - kb0 + 3) >> 2
        for wv in range(4):
            ks0 = min(kb1, kb0 + wv * per)
            ks1 = min(kb1, ks0 + per)
            ks = ks0
            while ks + 4 <= ks1:
                out.append((sb, wv, list(range(ks, ks + 4)), False))
                ks += 4
            if ks < ks1:
                out.append((sb, wv, list(range(ks, ks1)), True))
    return out


# ---- escape positions (lane, element) of a planted tile, by count -----------------------------------------------------
POSITIONS = {
    1: [(21, 4)],
    2: [(0, 0), (63, 7)],                                   # first dword low half, last dword high half
    3: [(5, 1), (5, 6), (40, 3)],                           # two escapes in one lane
    6: [(0, 7), (17, 2), (17, 3), (31, 0), (48, 5), (63, 0)],
}


class Plan:
    def __init__(self, cfg):
        self.cfg = cfg
        self.zero = {}                                      # tensor name -> flat indices
        self.cases = []                                     # (matrix kind, what, n-tile, {k-step: count})
        self.geometry = {}
        for kind in ("gate_up", "qkv", "down"):
            self._plan(kind)
        self.zero = {n: np.asarray(sorted(v), dtype=np.int64) for n, v in self.zero.items()}

    def transform(self, name, t):
        """for SpecDecModel.synthetic(transform=...): t is the float32 host tensor of `name`"""
        if name in self.zero:
            import torch
            t.view(-1)[torch.from_numpy(self.zero[name])] = 0
        return t

    def _plan(self, kind):
        cfg = self.cfg
        w = fused_bits(cfg, kind)
        N, K = w.shape
        KS, NT = K // 32, N // 16
        S, ksp = down_split(cfg) if kind == "down" else (1, KS)
        self.geometry[kind] = (N, K, S, ksp)
        natural = F.escape_counts(F.to_tiles(w)).reshape(NT, KS)
        src = _source(cfg, kind)
        bs = bursts(KS, S, ksp)
        groups = [b for b in bs if not b[3]]
        tails = [b for b in bs if b[3]]
        free = iter(range(NT))                              # every case takes an n-tile of its own

        def place(what, burst, counts, quiet=()):
            """plant counts[i] escapes in k-step burst[i] of an n-tile where the burst (and the bursts in `quiet`) have none"""
            steps = burst[2]
            for nt in free:
                if not natural[nt, steps].any() and not any(natural[nt, q[2]].any() for q in quiet):
                    break
            else:
                raise AssertionError(f"{kind}: no n-tile left for {what}")
            planted = {}
            for ks, c in zip(steps, counts):
                if not c:
                    continue
                planted[ks] = c
                for lane, el in POSITIONS[c]:
                    s = int(src[16 * nt + lane % 16, 32 * ks + 8 * (lane // 16) + el])
                    self.zero.setdefault(_names(kind)[s >> 32], []).append(s & 0xFFFFFFFF)
            self.cases.append((kind, what, nt, planted))

        def of_wave(lst, sb, wv):
            return [b for b in lst if b[0] == sb and b[1] == wv]

        # escapes in exactly one tile of a group: tile t in wave t, alternately the first and the last group of the wave's
        # range, with the wave's other bursts free of escapes (a group with escapes next to one without)
        sb = S - 1
        for t in range(4):
            mine = of_wave(groups, sb, t)
            g = mine[0] if t % 2 == 0 else mine[-1]
            others = [b for b in of_wave(bs, sb, t) if b is not g]
            place(f"tile {t} alone, wave {t}, {'first' if t % 2 == 0 else 'last'} group", g, [int(u == t) for u in range(4)], others)
        # all four tiles of a group, counts 1, 2, 3 and 6 (and in the other order in a last group)
        place("all four tiles: 1, 2, 3, 6", of_wave(groups, 0, 1)[0], [1, 2, 3, 6])
        place("all four tiles: 6, 3, 2, 1", of_wave(groups, 0, 2)[-1], [6, 3, 2, 1])
        # the tails of the finishing GEMM, every length that occurs: the last valid tile alone, every tile, and a tail with
        # none behind a group with some
        by_len = {}
        for tl in tails:
            by_len.setdefault(len(tl[2]), []).append(tl)
        for n, lst in sorted(by_len.items()):
            place(f"tail of {n}: last valid tile", lst[0], [0] * (n - 1) + [2], of_wave(groups, lst[0][0], lst[0][1]))
            place(f"tail of {n}: every tile", lst[-1], [6, 1, 3][:n])
            place(f"tail of {n} with none behind a group with some", of_wave(groups, lst[0][0], lst[0][1])[-1], [3, 0, 0, 1], [lst[0]])


@functools.lru_cache(maxsize=None)
def plan(intermediate):
    return Plan(config(intermediate))


def check(p):
    """The planted matrices on the host: every planted tile has exactly its count, no other tile changed its count, every
    matrix is packable and the records decode to the planted matrix."""
    seen = {}
    for kind in ("gate_up", "qkv", "down"):
        before = F.to_tiles(fused_bits(p.cfg, kind))
        tiles = F.to_tiles(fused_bits(p.cfg, kind, p.zero))
        N, K, S, ksp = p.geometry[kind]
        KS = K // 32
        want = F.escape_counts(before).reshape(N // 16, KS).copy()
        for k2, what, nt, planted in p.cases:
            if k2 != kind:
                continue
            for ks, c in planted.items():
                assert want[nt, ks] == 0, (kind, what)
                want[nt, ks] = c
        got = F.escape_counts(tiles).reshape(N // 16, KS)
        assert np.array_equal(got, want), kind
        codes, meta, ok = F.pack(tiles)
        assert ok and got.max() <= F.MAX_ESC, kind
        assert np.array_equal(F.unpack(codes, meta), tiles), kind
        assert np.array_equal((meta[:, 0] >> np.uint32(8)) & np.uint32(7), got.reshape(-1)), kind
        seen[kind] = sorted(what for k2, what, _, _ in p.cases if k2 == kind)
    return seen
