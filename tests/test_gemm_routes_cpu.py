"""The GEMM planner over every shape a user can bring (no GPU): sd_gemm_route - the launch helpers' own instance choice -
asked at every layer shape of the packaged configs, the public Llama / OPT cards, their TP 2/4/8 shards and a set of
synthetic edges (tests/gemm_route_classes.py), at every row count 1..256 and every `need` the forward pass and the public
GEMM entry use, under the default tunables and under SD_GEMM_NTW=8 / =2 and SD_GEMM_ROWS=0.

Counted by this test through the real query (`pytest -s` prints the tables; pinned in COUNTS below): over 208 distinct shapes
the planner selects 414 classes of (kernel instance, wave grid, raggedness) for x_tiled / row-major calls, of which
test_mfma_gemm_is_integer_exact_at_production_shapes reaches 97; 418 when the fused and one-slab plans are asked for as
well, 456 with the classes only SD_GEMM_NTW / SD_GEMM_ROWS reach.  tests/test_gpu_gemm_routes.py runs one witness of each
of the 456 as an integer-exact GEMM (55 shapes, the largest 361 M weights, 2.96 G weights in all)."""
import ctypes as C
import inspect
import os

import pytest

import gemm_route_classes as G
from llmspeculativesampling_amd import _lib

# What the sweep counts, pinned so that a planner change shows up here: the classes the planner selects over the universe
# for x_tiled / row-major operands (the public sd_gemm_bf16's reach), how many of those the older integer-exact test
# (test_mfma_gemm_is_integer_exact_at_production_shapes) reaches, the classes when the fused and one-slab plans are asked
# for too (what sd_gemm_bf16_need runs), and those plus the classes only a tunable adds (= the GPU file's witnesses).
COUNTS = {"plain": 414, "old_test": 97, "runnable": 418, "with_tunables": 456}
# The (N, K) the witnesses sit on, smallest first - tests/test_gpu_gemm_routes.py has one case per shape.  Pinned, so that
# collecting the GPU file costs no sweep; the sweep itself is compared with it here and there.
WITNESS_SHAPES = [
    (32, 32), (48, 32), (64, 32), (128, 32), (384, 1024), (384, 2048), (1024, 1024), (2048, 512), (768, 1536),
    (4096, 480), (4096, 544), (960, 2560), (1280, 2048), (2048, 1408), (768, 4096), (1280, 2560), (1280, 3072),
    (3072, 1536), (2560, 2048), (4096, 1376), (1536, 4096), (7168, 896), (2560, 2560), (8192, 1024), (5120, 1728),
    (3072, 3072), (1280, 8192), (9216, 1152), (2560, 5120), (5120, 3072), (4224, 4096), (5136, 4096), (5152, 4096),
    (9216, 2304), (11264, 2048), (3584, 7168), (10240, 2560), (3456, 9216), (16384, 2048), (9216, 4608),
    (12288, 4096), (14336, 4096), (13824, 5120), (22016, 4096), (50272, 2048), (20480, 5120), (28672, 4096),
    (50272, 2560), (27648, 5120), (18432, 9216), (50272, 4096), (50272, 5120), (36864, 9216), (50272, 7168),
    (44032, 8192),
]


@pytest.fixture(scope="module")
def default_points():
    return list(G.sweep(G.QUERY_NEEDS))


def _check_point(N, K, M, need, r, where):
    NT, KS, Mpad = N // 16, K // 32, (M + 15) // 16 * 16
    at = (where, N, K, M, G.need_name(need), r)
    kind = G.KIND_NAMES[r.kind]
    if M <= G.STREAM_MAX_ROWS:
        assert kind != "none", at                                  # up to 64 rows there is always a route
    if kind == "none":
        assert r.part_floats == 0, at
        return
    S, ksp = r.S, r.ksp
    if need & G.FUSED:
        assert S == 1, at
    assert S >= 1 and (S - 1) * ksp < KS <= S * ksp, at           # the slabs cover the k-range and none is empty
    assert r.part_floats == S * Mpad * N, at
    assert r.inst_mt > 0, at                                    # the launch helper has an instance for the route
    if kind == "stream":
        assert M <= G.STREAM_MAX_ROWS and r.inst_mt == Mpad // 16, at
        assert r.inst_ntw in (1, 2, 4, 8) and NT % r.inst_ntw == 0, at
        assert r.inst_unroll == (8 if r.inst_mt == 1 and 4 < (min(ksp, KS) + 3) // 4 <= 8 else
                                    1 if r.inst_ntw == 8 else 2 if r.inst_mt > 2 else 4), at
    elif kind == "stream_w16":
        assert need & G.QKV and M <= 16 and S == 1, at
    elif kind == "rows":
        assert not need & (G.GATHER | G.ROWMAJOR) and 16 < M <= 144, at
        assert 1 <= r.nwn <= G.GR_MAX_TILES and r.nwk >= 1 and r.nld >= 1, at
        assert r.nwn * r.nwk + r.nld <= 16, at
        assert r.NG * S == r.grid <= 256, at
        lo, hi = G.rows_groups(NT, r.NG)
        assert 1 <= lo and hi <= r.nwn, at                      # every n-group has a tile, no group more tiles than waves
        assert r.inst_mt >= Mpad // 16 and (r.inst_mt, r.inst_ch, r.inst_wbm) in {
            (2, 8, 1), (3, 8, 1), (3, 6, 1), (4, 8, 1), (4, 6, 1), (4, 4, 2), (5, 6, 1), (5, 4, 2), (8, 4, 2), (9, 4, 2)}, at
        assert r.lds_bytes == 1024 * r.inst_mt * max(2 * r.nwk * r.inst_ch, r.nwk * r.nwn), at
        assert r.lds_bytes <= G.ROWS_LDS_CAP, at
    else:
        assert kind == "mm" and not need & (G.GATHER | G.ROWMAJOR), at
        assert ksp % 2 == 0 and NT % 8 == 0 and r.mtw in (2, 4) and r.inst_mt == 4 * r.mtw, at
        assert r.inst_nt == (r.mtw == 4) and r.lds_bytes == 3 * (8 + 4 * r.mtw) * 2 * 1024 <= 144 * 1024, at


def test_every_route_keeps_the_planners_invariants(default_points):
    """Route exists up to 64 rows; the slab cut covers K with no empty slab (one slab when fused; gemm_bf16_mm: even slabs,
    128-column blocks); the rows plan's wave grid fits 16 waves, its grid the chip, its LDS the cap, and its instance is a
    compiled one (never launch_gemm_rows' error branch).  Default tunables, then SD_GEMM_NTW=8 / =2 and SD_GEMM_ROWS=0."""
    n = 0
    for N, K, M, need, r in default_points:
        _check_point(N, K, M, need, r, "default")
        n += 1
    for env in G.TUNABLES:
        for N, K, M, need, r in G.sweep(G.QUERY_NEEDS, env):
            _check_point(N, K, M, need, r, env)
            n += 1
    print(f"\n{len(G.universe())} shapes, {n} routes checked")
    assert n > 4 * 100 * 256


def test_tunables_are_read_at_the_call_and_move_the_instance():
    N, K = 4096, 2048                                              # 256 n-tiles: divisible by 8
    assert G.route(N, K, 40, G.ROWMAJOR).inst_ntw == 4
    with G.tunables({"SD_GEMM_NTW": "8"}):
        assert G.route(N, K, 40, G.ROWMAJOR).inst_ntw == 8 and G.route(N, K, 20, G.ROWMAJOR).inst_ntw == 4
    with G.tunables({"SD_GEMM_NTW": "2"}):
        assert G.route(N, K, 40, G.ROWMAJOR).inst_ntw == 2
    assert G.KIND_NAMES[G.route(N, K, 40, 0).kind] == "rows"
    with G.tunables({"SD_GEMM_ROWS": "0"}):
        assert G.KIND_NAMES[G.route(N, K, 40, 0).kind] == "stream"
    assert G.route(N, K, 40, G.ROWMAJOR).inst_ntw == 4 and "SD_GEMM_NTW" not in os.environ


def test_query_and_run_entry_reject_bad_arguments():
    info = _lib.SdGemmRouteInfo()
    lib = _lib.lib
    for N, K, M, need in ((4096, 4096, 0, 0), (4096, 4096, 257, 0), (4090, 4096, 1, 0), (4096, 4016, 1, 0), (4096, 4096, 1, 32),
                          (4096, 4096, 1, -1), (0, 4096, 1, 0)):
        assert lib.sd_gemm_route(N, K, M, need, C.byref(info)) == _lib.SD_ERR_INVALID, (N, K, M, need)
    assert lib.sd_gemm_route(4096, 4096, 1, 0, None) == _lib.SD_ERR_INVALID and b"sd_gemm_route" in lib.sd_last_error()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    # a gather needs a row table, the QKV route its epilogue: refused before anything is launched
    for need in (G.GATHER, G.QKV, G.FUSED | G.QKV, 32):
        assert lib.sd_gemm_bf16_need(p, p, 1, 16, 32, need, p, 64, p, None, None) == _lib.SD_ERR_INVALID, need
        assert b"sd_gemm_bf16_need" in lib.sd_last_error()
    assert lib.sd_gemm_bf16_need(None, p, 1, 16, 32, 0, p, 64, p, None, None) == _lib.SD_ERR_INVALID
    assert lib.sd_session_part_floats(None, 64) == 0


def _model_handle(m, layers=2):
    arch, h, inter, nh, nkv, hd, vocab, proj = m
    P = 0x1000                                                     # (sd_model_create and the planner never read the weights)
    arrays = [(C.c_void_p * layers)(*([P] * layers)) for _ in range(12)]
    w = _lib.SdModelWeights()
    w.embed = w.lm_head = w.final_norm_w = w.pos_embed = w.rope_cos = w.rope_sin = P
    (w.wqkv, w.bqkv, w.wo, w.bo, w.w_gate_up, w.b_fc1, w.w_down, w.b_fc2, w.norm1_w, w.norm1_b, w.norm2_w,
     w.norm2_b) = (C.cast(a, C.POINTER(C.c_void_p)) for a in arrays)
    c = _lib.SdModelConfig(arch=0 if arch == "llama" else 1, dtype=_lib.SD_BF16, vocab=vocab, hidden=h, inter=inter,
                           n_layers=layers, n_heads=nh, n_kv_heads=nkv, head_dim=hd, max_pos=2048, opt_pre_ln=1,
                           opt_proj_dim=proj or h, norm_eps=1e-5, logits_bf16_round=1, fused_layout=1)
    handle = C.c_void_p()
    if _lib.lib.sd_model_create(C.byref(c), C.byref(w), C.byref(handle)) != _lib.SD_OK:
        return None, arrays
    return handle, arrays


def test_no_route_leaves_more_slabs_than_the_session_reserves():
    """sd_session_part_floats (plan_scratch's reservation for the k-slabs) against the part floats of every route a pass of the
    model can take: every GEMM of the pass at need 0, the O / down projections of a shard as one slab, the lm_head and OPT's
    project_out gathered - at every row count up to the session's.  Every model (and shard) sd_model_create accepts."""
    checked = 0
    for name, m in G.models().items():
        for world in (1, 2, 4, 8):
            sm = G.shard(m, world)
            if sm is None:
                continue
            handle, keep = _model_handle(sm)
            if handle is None:                                     # (hidden > 8192, head_dim 80, widths off the 32-grid: not loadable)
                continue
            max_rows = _lib.lib.sd_model_max_rows(handle)
            shapes = G.model_shapes(sm)
            for rows in sorted({5, 16, 64, max_rows}):
                have = _lib.lib.sd_session_part_floats(handle, rows)
                assert have * 4 <= _lib.lib.sd_session_scratch_bytes(handle, rows)
                for role, (N, K) in shapes.items():
                    needs = [0] + ([G.ONE_SLAB] if role in ("o", "down") else []) + ([G.GATHER] if role in ("lm_head", "project_out") else [])
                    for need in needs:
                        for M in range(1, min(rows, 64 if need & G.GATHER else rows) + 1):
                            r = G.route(N, K, M, need)
                            assert r.kind != _lib.SD_GEMM_NONE or M > 64, (name, world, role, M)
                            assert r.part_floats <= have, (name, world, role, rows, M, need, r, have)
                            checked += 1
            _lib.lib.sd_model_destroy(handle)
            del keep
    print(f"\n{checked} (model, rows, GEMM, M, need) points within the reservation")
    assert checked > 100000


def test_class_counts_and_no_lost_coverage(default_points):
    """The class table.  Every class the older production-shape test reaches is a class of the sweep (its shapes are in the
    universe: nothing it covers is lost), and the counts are the ones this module and DESIGN.md quote."""
    from test_gpu_production_parity import GEMM_SHAPES, test_mfma_gemm_is_integer_exact_at_production_shapes as old
    assert str(G.OLD_EXACT_ROWS) in inspect.getsource(old)        # (the row list that test walks)
    uni = G.universe()
    assert all(nk in uni for nk in GEMM_SHAPES.values())
    plain = set(G.classes_of(p for p in default_points if p[3] in (0, G.ROWMAJOR)))
    queried = set(G.classes_of(default_points))
    old_classes = G.old_exact_test_classes(GEMM_SHAPES.values())
    wit = G.witnesses()
    runnable = [w for w in wit if not w[4]]
    assert old_classes <= plain <= queried
    assert {w[5] for w in runnable} == set(G.classes_of(p for p in default_points if p[3] in G.RUN_NEEDS))
    # the classes that only the query reaches are the gathered operand's and gemm_bf16_stream_w16's (no run entry)
    assert all(dict(k)["kind"] == "stream_w16" or dict(k).get("x") == "gather" for k in queried - {w[5] for w in runnable})
    for k in queried | {w[5] for w in wit}:
        assert dict(k).get("groups") != "empty", k                 # (NT >= NG in every rows plan: no n-group without a tile)
    print()
    for title, ks in (("x_tiled / row-major", plain), ("reached by the older exact test", old_classes),
                      ("runnable (+ fused, one-slab)", {w[5] for w in runnable}), ("witnessed (+ tunables)", {w[5] for w in wit}),
                      ("queried (+ gather, QKV)", queried)):
        per = {}
        for k in ks:
            per[dict(k)["kind"]] = per.get(dict(k)["kind"], 0) + 1
        print(f"{title:<34} {len(ks):>4}  " + "  ".join(f"{kd} {n}" for kd, n in sorted(per.items())))
    shapes = sorted({(w[0], w[1]) for w in wit}, key=lambda nk: (nk[0] * nk[1], nk))
    assert shapes == WITNESS_SHAPES
    print(f"{len(wit)} witnesses on {len(shapes)} shapes, largest {max(n * k for n, k in shapes) / 1e6:.0f} M weights, "
          f"{sum(n * k for n, k in shapes) / 1e9:.2f} G weights in all")
    print(G.format_witness_table(wit))
    got = {"plain": len(plain), "old_test": len(old_classes), "runnable": len(runnable), "with_tunables": len(wit)}
    assert got == COUNTS
