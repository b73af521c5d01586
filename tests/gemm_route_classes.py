"""The GEMM planner's decision space, enumerated through sd_gemm_route (no GPU): a universe of layer shapes, the class of
kernel instance / wave grid / raggedness every (shape, rows, need) point falls in, and one smallest witness per class.

tests/test_gemm_routes_cpu.py checks the planner's invariants over the whole universe; tests/test_gpu_gemm_routes.py runs
every witness as an integer-exact GEMM."""
import contextlib
import ctypes as C
import functools
import json
import os

from llmspeculativesampling_amd import _lib

GATHER, ROWMAJOR, FUSED, QKV, ONE_SLAB = (_lib.SD_GN_GATHER, _lib.SD_GN_ROWMAJOR, _lib.SD_GN_FUSED, _lib.SD_GN_QKV,
                                          _lib.SD_GN_ONE_SLAB)
KIND_NAMES = {_lib.SD_GEMM_NONE: "none", _lib.SD_GEMM_STREAM: "stream", _lib.SD_GEMM_STREAM_W16: "stream_w16",
              _lib.SD_GEMM_ROWS: "rows", _lib.SD_GEMM_MM: "mm"}
MAX_ROWS = 256
STREAM_MAX_ROWS = 64                                              # past it a GEMM needs X in the tile layout
GR_MAX_TILES = 7                                                  # rows_kernels.h
ROWS_LDS_CAP = 158 * 1024
QUERY_NEEDS = (0, ROWMAJOR, GATHER, FUSED, FUSED | QKV, ONE_SLAB)     # what the forward pass and the public entry ask for
RUN_NEEDS = (0, ROWMAJOR, FUSED, ONE_SLAB)                            # what sd_gemm_bf16_need runs
# tunables that reach instances the defaults do not (the NTW 8 instances are compiled and otherwise unreachable)
TUNABLES = ({"SD_GEMM_NTW": "8"}, {"SD_GEMM_NTW": "2"}, {"SD_GEMM_ROWS": "0"})

# ---- the shape universe -------------------------------------------------------------------------------------------------
# (arch, hidden, intermediate / ffn_dim, heads, KV heads, head_dim, vocab, OPT's word_embed_proj_dim): the public model cards
PUBLIC_MODELS = {
    "llama-2-7b": ("llama", 4096, 11008, 32, 32, 128, 32000, 0),
    "llama-2-13b": ("llama", 5120, 13824, 40, 40, 128, 32000, 0),
    "llama-2-70b": ("llama", 8192, 28672, 64, 8, 128, 32000, 0),
    "llama-3-8b": ("llama", 4096, 14336, 32, 8, 128, 128256, 0),
    "llama-3-70b": ("llama", 8192, 28672, 64, 8, 128, 128256, 0),
    "llama-3.2-1b": ("llama", 2048, 8192, 32, 8, 64, 128256, 0),
    "llama-3.2-3b": ("llama", 3072, 8192, 24, 8, 128, 128256, 0),
    "tinyllama-1.1b": ("llama", 2048, 5632, 32, 4, 64, 32000, 0),
    "codellama-34b": ("llama", 8192, 22016, 64, 8, 128, 32000, 0),
    "llama-68m": ("llama", 768, 3072, 12, 12, 64, 32000, 0),
    "opt-125m": ("opt", 768, 3072, 12, 12, 64, 50272, 768),
    "opt-350m": ("opt", 1024, 4096, 16, 16, 64, 50272, 512),
    "opt-1.3b": ("opt", 2048, 8192, 32, 32, 64, 50272, 2048),
    "opt-2.7b": ("opt", 2560, 10240, 32, 32, 80, 50272, 2560),
    "opt-6.7b": ("opt", 4096, 16384, 32, 32, 128, 50272, 4096),
    "opt-13b": ("opt", 5120, 20480, 40, 40, 128, 50272, 5120),
    "opt-30b": ("opt", 7168, 28672, 56, 56, 128, 50272, 7168),
    "opt-66b": ("opt", 9216, 36864, 72, 72, 128, 50272, 9216),
}
_CFG_DIR = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "configs")


def models():
    """name -> (arch, hidden, inter, heads, kv_heads, head_dim, vocab, proj_dim): every packaged config, then the cards."""
    out = {}
    for f in sorted(os.listdir(_CFG_DIR)):
        if not f.endswith(".json"):
            continue
        d = json.load(open(os.path.join(_CFG_DIR, f)))
        h, nh = d["hidden_size"], d["num_attention_heads"]
        if d["arch"] == "llama":
            out[f[:-5]] = ("llama", h, d["intermediate_size"], nh, d.get("num_key_value_heads") or nh, h // nh, d["vocab_size"], 0)
        else:
            out[f[:-5]] = ("opt", h, d["ffn_dim"], nh, nh, h // nh, d["vocab_size"], d.get("word_embed_proj_dim") or h)
    for name, m in PUBLIC_MODELS.items():
        if name in out:
            assert out[name] == m, (name, out[name], m)            # the card table and the packaged config agree
        out[name] = m
    return out


def shard(m, world):
    """The local geometry of one of `world` Megatron shards (tp.shard_config's rule, applied to either family), or None."""
    arch, h, inter, nh, nkv, hd, vocab, proj = m
    if world == 1:
        return m
    if nh % world or nkv % world or inter % (world * 32):
        return None
    return (arch, h, inter // world, nh // world, nkv // world, hd, vocab, proj)


def model_shapes(m):
    """{role: (N, K)} of the GEMMs one forward pass of the (possibly sharded) model runs."""
    arch, h, inter, nh, nkv, hd, vocab, proj = m
    ed = proj if arch == "opt" else h
    s = {"qkv": ((nh + 2 * nkv) * hd, h), "o": (h, nh * hd), "gate_up": ((2 if arch == "llama" else 1) * inter, h),
         "down": (h, inter), "lm_head": (vocab, ed)}
    if ed != h:
        s["project_in"], s["project_out"] = (h, ed), (ed, h)
    return s


# synthetic edges: N/16 odd; N/16 = 2 (mod 4); K/32 odd; K = 32; K/32 = 15, 16, 17 (gemm_bf16_mm needs >= 16 k-steps); N*K just
# under / over 16 Mi (where the k-slab GEMMs of >= 24 rows move to gemm_bf16_mm); N/16/8 = 63 and 64 (that route's limit)
SYNTHETIC = {
    "nt_odd": (16 * 321, 4096), "nt_2mod4": (16 * 322, 4096), "ks_odd": (4096, 32 * 129), "k_32": (4096, 32),
    "ks_15": (4096, 32 * 15), "ks_16": (4096, 32 * 16), "ks_17": (4096, 32 * 17),
    "nk_under_16mi": (4096 - 128, 4096), "nk_at_16mi": (4096, 4096), "nk_over_16mi": (4096 + 128, 4096),
    "nb_63": (16 * 8 * 63, 4096), "nb_64": (16 * 8 * 64, 4096),
}


def universe():
    """{(N, K): [label, ...]}: every GEMM of every model and of its TP 2/4/8 shards whose dimensions stay multiples of the
    tile (N % 16 == 0, K % 32 == 0), and the synthetic edges."""
    out = {}
    for name, m in models().items():
        for world in (1, 2, 4, 8):
            sm = shard(m, world)
            if sm is None:
                continue
            for role, (N, K) in model_shapes(sm).items():
                if N >= 16 and K >= 32 and N % 16 == 0 and K % 32 == 0:
                    out.setdefault((N, K), []).append(f"{name}{'' if world == 1 else f'/tp{world}'}:{role}")
    for name, nk in SYNTHETIC.items():
        out.setdefault(nk, []).append("edge:" + name)
    return out


# ---- the query ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def tunables(env):
    """The planner reads its tunables at every query / run: set them around the call only."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Route(_lib.SdGemmRouteInfo):
    def __repr__(self):
        return "Route(" + ", ".join(f"{f}={getattr(self, f)}" for f, _ in _lib.SdGemmRouteInfo._fields_) + ")"


def route(N, K, M, need):
    """sd_gemm_route's answer (under whatever tunables are set at the call)."""
    info = Route()
    if _lib.lib.sd_gemm_route(N, K, M, need, C.byref(info)) != _lib.SD_OK:
        _lib.check(_lib.SD_ERR_INVALID, "sd_gemm_route")
    return info


@functools.lru_cache(maxsize=None)
def rows_groups(NT, NG):
    """(fewest, most) n-tiles one n-group of gemm_bf16_rows owns: the kernel's own deal, t0 = g * NT / NG (rows_kernels.h)."""
    sizes = [(g + 1) * NT // NG - g * NT // NG for g in range(NG)]
    return min(sizes), max(sizes)


def class_key(N, K, M, need, r):
    """The class of one point, from the query's answer: a tuple of (field, value) pairs that starts with the kind."""
    NT, KS, Mpad = N // 16, K // 32, (M + 15) // 16 * 16
    kind = KIND_NAMES[r.kind]
    ragged_m, short_slab, slabs = M % 16 != 0, KS % r.ksp != 0 if r.ksp else False, r.S > 1
    if kind == "stream":
        x = "gather" if need & GATHER else ("rowmajor" if need & ROWMAJOR else "tiled")
        return (("kind", kind), ("MT", r.inst_mt), ("NTW", r.inst_ntw), ("UNROLL", r.inst_unroll), ("x", x),
                ("slabs", slabs), ("short_slab", short_slab), ("ragged_m", ragged_m))
    if kind == "rows":
        lo, hi = rows_groups(NT, r.NG)
        groups = "even" if lo == hi else ("empty" if lo == 0 else "short")     # short: a group with fewer tiles than nwn waves
        return (("kind", kind), ("MT", r.inst_mt), ("CH", r.inst_ch), ("WBM", r.inst_wbm), ("nwn", r.nwn),
                ("nwk", r.nwk), ("nld", r.nld), ("slabs", slabs), ("groups", groups),
                ("spare_mt", Mpad // 16 != r.inst_mt), ("short_slab", short_slab), ("ragged_m", ragged_m))
    if kind == "mm":
        BMT = 4 * r.mtw
        return (("kind", kind), ("mtw", r.mtw), ("slabs", slabs), ("row_blocks", (Mpad // 16 + BMT - 1) // BMT > 1),
                ("partial_block", (Mpad // 16) % BMT != 0), ("short_slab", short_slab), ("ragged_m", ragged_m))
    return (("kind", kind), ("ragged_m", ragged_m))


def sweep(needs, env=None, shapes=None, rows=range(1, MAX_ROWS + 1)):
    """Every (N, K, M, need, route) of shapes x rows x needs that has a question to ask (row-major and gathered operands exist
    up to 64 rows only), under the tunables `env`."""
    shapes = universe() if shapes is None else shapes
    with tunables(env or {}):
        for (N, K) in shapes:
            for need in needs:
                for M in rows:
                    if need & (GATHER | ROWMAJOR) and M > STREAM_MAX_ROWS:
                        continue
                    yield N, K, M, need, route(N, K, M, need)


def classes_of(points):
    """{class key: (N, K, M, need)}: per class the witness with the smallest N * K, and within that the smallest M."""
    best = {}
    for N, K, M, need, r in points:
        if r.kind == _lib.SD_GEMM_NONE:
            continue
        key, rank = class_key(N, K, M, need, r), (N * K, M, N, need)
        if key not in best or rank < best[key][0]:
            best[key] = (rank, (N, K, M, need))
    return {k: v[1] for k, v in best.items()}


_WITNESS_CACHE = {}


def witnesses(needs=RUN_NEEDS):
    """[(N, K, M, need, env, class key)]: one witness per class the planner selects over universe x 1..256 rows x needs, then
    one per class that only a tunable adds (env: the tunables to set around the call, {} for the defaults)."""
    needs = tuple(needs)
    if needs not in _WITNESS_CACHE:
        out, seen = [], set()
        for env in ({},) + TUNABLES:
            for key, (N, K, M, need) in sorted(classes_of(sweep(needs, env)).items(), key=lambda kv: (kv[1][0] * kv[1][1], kv[1], kv[0])):
                if key not in seen:
                    seen.add(key)
                    out.append((N, K, M, need, dict(env), key))
        _WITNESS_CACHE[needs] = out
    return _WITNESS_CACHE[needs]


# the (N, K) shapes and row counts of test_mfma_gemm_is_integer_exact_at_production_shapes (tests/test_gpu_production_parity.py)
OLD_EXACT_ROWS = (1, 5, 16, 17, 40, 60, 64, 72, 80, 96, 127, 128, 132, 144, 145, 150, 177, 200, 241, 256)


def old_exact_test_classes(shapes):
    """The classes that test reaches: x_tiled at every row count, plain rows up to 64."""
    return set(classes_of(sweep((0, ROWMAJOR), shapes={nk: [] for nk in shapes}, rows=OLD_EXACT_ROWS)))


def need_name(need):
    names = [n for b, n in ((GATHER, "gather"), (ROWMAJOR, "rowmajor"), (FUSED, "fused"), (QKV, "qkv"), (ONE_SLAB, "one_slab")) if need & b]
    return "|".join(names) or "tiled"


def format_witness_table(wit):
    lines = []
    for N, K, M, need, env, key in wit:
        tun = " ".join(f"{k}={v}" for k, v in env.items())
        lines.append(f"{N:>7} x {K:<6} M={M:<4} {need_name(need):<9} {tun:<15} " + " ".join(f"{f}={v}" for f, v in key))
    return "\n".join(lines)
