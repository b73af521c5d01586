"""Host-side checks of the key-blocked matrix-core prefill attention (attn_prefill_blocked_kernel, prefill_attn.h); no GPU:
the planner and the router the launch path uses (sd_prefill_attn_plan, sd_prefill_attn_route), the ABI of the new entry points, the block-edge layouts of
tests/prefill_block_layouts.py on the oracle alone (as test_prefill_probe_cpu.py checks prefill_probe_layouts'), and a numpy
restatement of the kernel's three sweeps for one row, which must reproduce the single-tile kernel's softmax bit for bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import attn_probe as P
import prefill_block_layouts as B
from prefill_probe_layouts import wide_models  # noqa: F401  (fixture)
from test_attn_probe_cpu import _check

NEW = ["sd_session_prefill_attn_blocked_launches", "sd_prefill_attn_plan", "sd_prefill_attn_route"]
LDS_MAX = 150 * 1024                                               # PA_LDS_MAX (engine.hip)


# ----------------------------------------------------------------------------- planner
def _plan(D, s_max, block=0):
    from llmspeculativesampling_amd import _lib
    k, b, lds = C.c_int(-1), C.c_int(-1), C.c_long(-1)
    assert _lib.lib.sd_prefill_attn_plan(D, s_max, block, C.byref(k), C.byref(b), C.byref(lds)) == _lib.SD_OK
    return k.value, b.value, lds.value


def _tile_lds(keys, D):
    """16 score rows of align64(keys) + 4 floats next to one 64-key V chunk at a row pitch of 2 D + 32 bytes."""
    return 16 * (((keys + 63) // 64) * 64 + 4) * 4 + 64 * (2 * D + 32)


def test_plan_switches_to_blocks_where_the_tile_stops_fitting():
    assert _plan(128, 2048)[0] == 1 and _plan(128, 2049)[0] == 2
    assert _plan(64, 2176)[0] == 1 and _plan(64, 2177)[0] == 2
    for D, edge in ((128, 2048), (64, 2176)):
        assert _tile_lds(edge, D) <= LDS_MAX < _tile_lds(edge + 1, D)          # the limits follow from the footprint
        assert _plan(D, edge) == (1, edge, _tile_lds(edge, D))
        k, b, lds = _plan(D, edge + 1)
        assert b > 0 and b % 64 == 0 and lds == _tile_lds(b, D)
        assert 2 * lds <= 160 * 1024                                           # at least two workgroups in a CU's LDS
        assert _plan(D, 1 << 20) == (k, b, lds)                                # no dependence on the context past the limit
    assert _plan(128, 37) == (1, 64, _tile_lds(37, 128))


def test_every_plan_fits_the_lds_budget():
    for D in (64, 128):
        for s_max in (1, 63, 64, 65, 293, 1040, 2048, 2049, 2176, 2177, 2304, 4096, 6144, 8192, 100000):
            for block in (0, 1, 64, 100, 128, 256, 512, 1024, 2048, 4096, 1 << 20):
                k, b, lds = _plan(D, s_max, block)
                assert k in (1, 2) and b % 64 == 0 and 0 < lds <= LDS_MAX, (D, s_max, block, k, b, lds)
                assert lds == _tile_lds(b, D)
                assert (k == 2) == (block > 0 or _tile_lds(s_max, D) > LDS_MAX)


def test_forced_block_is_rounded_up_to_a_multiple_of_64():
    assert _plan(128, 300, 100) == (2, 128, _tile_lds(128, 128))
    assert _plan(64, 5000, 100) == (2, 128, _tile_lds(128, 64))
    assert _plan(128, 300, 64)[1] == 64 and _plan(128, 300, 65)[1] == 128 and _plan(128, 37, 512)[:2] == (2, 512)


def test_no_plan_outside_head_dim_64_and_128():
    for D in (16, 32, 96, 256):
        assert _plan(D, 300) == (0, 0, 0) and _plan(D, 300, 128) == (0, 0, 0)


def test_plan_refuses_bad_arguments_and_takes_null_outputs():
    from llmspeculativesampling_amd import _lib
    assert _lib.lib.sd_prefill_attn_plan(128, 0, 0, None, None, None) == _lib.SD_ERR_INVALID
    assert _lib.lib.sd_prefill_attn_plan(128, 300, -1, None, None, None) == _lib.SD_ERR_INVALID
    assert _lib.lib.sd_prefill_attn_plan(128, 300, 0, None, None, None) == _lib.SD_OK


# ----------------------------------------------------------------------------- route
def _route(D, heads, rows, s_max, block=0, cus=256):
    from llmspeculativesampling_amd import _lib
    k = C.c_int(-1)
    assert _lib.lib.sd_prefill_attn_route(D, heads, rows, s_max, block, cus, C.byref(k)) == _lib.SD_OK
    return k.value


def test_route_below_the_tile_limit_does_not_look_at_the_launch_size():
    for heads in (1, 4, 12, 64):
        for rows in (32, 81, 256):
            assert _route(128, heads, rows, 2048) == 1 and _route(64, heads, rows, 2176) == 1 and _route(128, heads, rows, 37) == 1
    assert _route(32, 16, 256, 300) == 0 and _route(32, 16, 256, 300, 128) == 0


def test_route_past_the_tile_limit_takes_blocks_from_two_workgroups_per_cu():
    """The measured rule: heads x 16-row groups >= 2 x CUs -> the blocked kernel; fewer -> attn_kernel, the
    route of such passes before, while its key splits hold the pass."""
    for D, s_max in ((128, 2049), (128, 4096), (64, 2177), (64, 4096)):
        assert _route(D, 64, 256, s_max) == 2 and _route(D, 32, 256, s_max) == 2        # 1024 and 512 workgroups on 256 CUs
        assert _route(D, 31, 256, s_max) == 0 and _route(D, 12, 256, s_max) == 0 and _route(D, 8, 256, s_max) == 0
        assert _route(D, 40, 88, s_max) == 0 and _route(D, 40, 208, s_max) == 2          # 40 x 6 = 240, 40 x 13 = 520
        assert _route(D, 8, 256, s_max, cus=64) == 2 and _route(D, 8, 256, s_max, cus=65) == 0
        for block in (64, 100, 512):
            assert _route(D, 1, 32, s_max, block) == 2 and _route(D, 1, 32, 37, block) == 2      # a forced block: always


def test_route_takes_blocks_where_attn_kernel_cannot_hold_the_pass():
    """A 256-row pass is 32 row groups of attn_kernel, whose keys are cut over at most 64 / 32 = 2 workgroups: past 5760 keys at
    D = 128 and 5888 at D = 64 a chunk's score rows no longer fit the LDS (launch_attn's capacity error before); fewer row
    groups split further."""
    assert _route(128, 8, 256, 5760) == 0 and _route(128, 8, 256, 5761) == 2
    assert _route(64, 8, 256, 5888) == 0 and _route(64, 8, 256, 5889) == 2
    assert _route(128, 8, 128, 5761) == 0 and _route(128, 8, 128, 11520) == 0 and _route(128, 8, 128, 11521) == 2
    assert _route(128, 8, 256, 1 << 20) == 2


def test_route_refuses_bad_arguments():
    from llmspeculativesampling_amd import _lib
    k = C.c_int(0)
    for args in ((128, 0, 256, 300, 0, 256), (128, 8, 0, 300, 0, 256), (128, 8, 256, 0, 0, 256), (128, 8, 256, 300, -1, 256), (128, 8, 256, 300, 0, -1)):
        assert _lib.lib.sd_prefill_attn_route(*args, C.byref(k)) == _lib.SD_ERR_INVALID
    assert _lib.lib.sd_prefill_attn_route(128, 8, 256, 300, 0, 256, None) == _lib.SD_ERR_INVALID
    assert _route(128, 8, 256, 4096, cus=0) in (0, 2)                         # cus = 0: the device's count (256 without one)


# ----------------------------------------------------------------------------- ABI
def test_blocked_symbols_are_exported_declared_and_bound():
    """(Argument counts and classes against the header: test_abi_cpu.py.)"""
    from llmspeculativesampling_amd import _lib, engine
    bound = {n: res for n, res, _ in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and bound[name] is C.c_int, name
    assert _lib.lib.sd_session_prefill_attn_blocked_launches(None) == 0        # (a host integer: no session, no count)
    assert callable(engine.Session.prefill_attn_blocked_launches)
    assert _lib.lib.sd_version() == 7


# ----------------------------------------------------------------------------- layouts
@functools.lru_cache(maxsize=None)
def _oracle(name, dt, kvq=None):
    return P.ProbeOracle(name, P.DTYPES[dt], kvq)


def test_block_layout_table():
    lays = B.layouts()
    assert len(lays) == len(set(lays)) == 36
    assert all(0 <= l.marker <= l.S <= P.MAX_SEQ - 1 and l.n - B.TAIL <= l.probe < l.n for l in lays)
    assert {(l.n, l.S - l.n) for l in lays} == set(B.CALLS)
    by = lambda cls, S=None: {(l.S, l.marker, l.probe) for l in lays if l.cls == cls and S in (None, l.S)}
    # the first and the last key of every block, the first key of the last, partial block among them
    assert {m for _, m, _ in by("block_edge", 956)} == {k for b in range(128, 956, 128) for k in (b - 1, b)}
    assert {(293, 256, 255), (956, 896, 255), (200, 128, 199)} <= by("block_edge")
    # a row's own position at a block's last and first key, and the successor of each
    assert by("own") == {(293, 255, 218), (293, 256, 219), (956, 895, 195), (956, 896, 196), (256, 255, 255)}
    assert by("forbidden") == {(293, 255, 217), (293, 256, 218), (956, 895, 194), (956, 896, 195), (256, 255, 254),
                               (293, 293, 255), (956, 956, 255), (200, 200, 199), (256, 256, 255)}
    assert all(l.marker == l.S - l.n + l.probe + (l.cls == "forbidden") for l in lays if l.cls != "block_edge")


@pytest.mark.usefixtures("wide_models")
@pytest.mark.parametrize("name,dt,kvq", B.CASES, ids=B.CASE_IDS)
def test_block_layouts_discriminate_and_the_reference_alone_passes(name, dt, kvq):
    """Losing the marker - or leaking a forbidden one into the probed row - moves that row's fp32 logits by at least 20x the GPU
    test's tolerance, and the same-dtype oracle passes the GPU test's rule by itself (test_attn_probe_cpu._check)."""
    o32, o16 = _oracle(name, "fp32"), _oracle(name, dt, kvq)
    worst, e_max = float("inf"), 0.0
    for lay in B.layouts():
        r, e = _check(o32, o16, lay, P.discrimination, lambda o, l: o.logits(l))
        worst, e_max = min(worst, r), max(e_max, e)
    print(f"block edges {name} {dt} {kvq}: {len(B.layouts())} layouts, least discrimination {worst:.1f}x the tolerance, "
          f"reference error at most {e_max:.4f}")
    assert worst >= 20.0


# ----------------------------------------------------------------------------- the three sweeps, restated
def _exp32(x):
    """One deterministic fp32 function of each element (the kernel's is expf: any will do, the claim is about order)."""
    return np.array([math.exp(float(v)) for v in x], dtype=np.float32)


_DPP = [np.arange(32) ^ 1, np.arange(32) ^ 2, (np.arange(32) & ~7) | (7 - (np.arange(32) & 7)),
        (np.arange(32) & ~15) | (15 - (np.arange(32) & 15))]


def _half_reduce(v, op):
    """half_sums / half_maxes (common.h) on the 32 lanes of a half-wave: quad swaps, the two mirrors, then the second row
    takes the first row's lane 15; the result is read from lane 31."""
    v = v.astype(np.float32).copy()
    for perm in _DPP:
        v = op(v, v[perm])
    return op(v[31], v[15])


def _lane_sums(e, s0, s1):
    """A lane's partial sums over the keys hl + 64 k (s0) and hl + 32 + 64 k (s1) of `e` (a whole number of 64-key rounds,
    zero-padded keys excluded by `valid`), added in ascending key order onto the carried values."""
    vals, valid = e
    for k in range(0, len(vals), 64):
        for acc, off in ((s0, k), (s1, k + 32)):
            keep = valid[off:off + 32]
            acc[keep] = acc[keep] + vals[off:off + 32][keep]
    return s0, s1


def _pad64(x, fill):
    n = (len(x) + 63) // 64 * 64
    out = np.full(n, fill, dtype=np.float32)
    out[:len(x)] = x
    return out, np.arange(n) < len(x)


def _softmax_tile(row):
    """attn_prefill_kernel: the whole row at once."""
    vals, valid = _pad64(row, -np.inf)
    m = _half_reduce(vals.reshape(-1, 32).max(axis=0), np.maximum)
    e = _exp32(row - m)
    s0, s1 = _lane_sums(_pad64(e, 0.0), np.zeros(32, np.float32), np.zeros(32, np.float32))
    total = np.float32(_half_reduce(s0, np.add) + _half_reduce(s1, np.add))
    return m, total, (e / total).astype(np.float32)


def _softmax_blocked(row, kb):
    """attn_prefill_blocked_kernel: three sweeps over blocks of kb keys, the scores recomputed (here: re-read) per block."""
    blocks = [row[b:b + kb] for b in range(0, len(row), kb)]
    mx = np.full(32, -np.inf, dtype=np.float32)
    for blk in blocks:                                             # 1. running per-lane maxima
        vals, _ = _pad64(blk, -np.inf)
        mx = np.maximum(mx, vals.reshape(-1, 32).max(axis=0))
    m = _half_reduce(mx, np.maximum)
    s0, s1 = np.zeros(32, np.float32), np.zeros(32, np.float32)
    for blk in blocks:                                             # 2. per-lane partial sums carried across blocks
        s0, s1 = _lane_sums(_pad64(_exp32(blk - m), 0.0), s0, s1)
    total = np.float32(_half_reduce(s0, np.add) + _half_reduce(s1, np.add))
    p = np.concatenate([(_exp32(blk - m) / total).astype(np.float32) for blk in blocks])      # 3.
    return m, total, p


def test_three_sweeps_over_blocks_reproduce_the_tile_softmax_bit_for_bit():
    """1000 random fp32 rows of ragged length 1..700: maximum, denominator and probabilities of the blocked evaluation
    (blocks of 64 and of 128 keys) equal the single-tile evaluation's bit for bit - a block size that is a multiple of 64
    hands every lane's s0 and s1 the same additions in the same order.  A block size of 96 (not a multiple of 64) is shown to
    break it, so the check can fail."""
    rng = np.random.default_rng(2025)
    broke = 0
    for i in range(1000):
        n = int(rng.integers(1, 701))
        row = (rng.standard_normal(n) * rng.choice([0.5, 3.0, 8.0])).astype(np.float32)
        m, total, p = _softmax_tile(row)
        assert np.isfinite(total) and total >= 1.0
        for kb in (64, 128):
            mb, tb, pb = _softmax_blocked(row, kb)
            assert mb.tobytes() == m.tobytes() and tb.tobytes() == total.tobytes() and pb.tobytes() == p.tobytes(), (i, n, kb)
        if i < 200 and n > 96:
            broke += _softmax_blocked(row, 96)[1].tobytes() != total.tobytes()
    assert broke > 0
