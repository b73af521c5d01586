"""Every byte an e4m3 KV arena holds, at every store site and scale (`pytest -m gpu`).

The byte is a pure function of the K / V element rounded to the model's 16-bit type and of one fp32 scale,
e4m3(clamp(fl32(x * fl32(1 / scale)))) - fp8_store.e4m3_byte, in integers, checked against torch on all 2 x 65536 patterns by
test_fp8_store_cpu.py - so every comparison here is EXACT: no tolerance anywhere in this file.

  * planted values (OPT: k_proj = v_proj = 0, so the stored element is the bias bit for bit): 2 signs x 128 bf16 mantissas x
    4 exponents under 24 uniform power-of-two scales - every tie, every denormal, both flushes, both saturations - through
    store4_fp8 on gemm_small (<= 4 rows), the streaming kernel, the many-row kernels and a prefill call; the fp16 values at
    every e4m3 code boundary with both neighbours; the values on which x * (1 / s) and x / s differ at 0.3 and 1.7; +-Inf and
    NaN (NaN stays NaN);
  * natural values: twin sessions of one model on the same calls, one with a 16-bit arena, one with an e4m3 arena under one
    of four scale tables whose entries all differ (pow2, real = amax / 448, tight = real / 64, loose = real * 2^14): the
    expected byte is e4m3_byte(the twin's 16-bit element, that (layer, k|v, head)'s scale).  Every o_proj is zero, so every
    layer's K / V depend on tokens and positions alone.  Llama (to_fp8 on RoPE pairs) at H = 1024 / 256 and a GQA model
    (8 query heads on 2 KV heads, D = 32, 3 layers), OPT with its real weights; bf16 and fp16; 1 .. 130 rows; the small path
    on / off, norm on load 0 / 1 / 2, 12-bit records; positions 0, 1 and max - 5; sd_batch_forward and sd_batch_prefill over
    two streams with a table each; sd_session_forward_tree; a 2-rank loopback tensor-parallel target;
  * sd_session_compact_kv on arenas of random bytes (fp8 rows are D bytes).

An fp8 arena takes the fused attention + O launch off, so the twin is created under SD_FUSE_ATTN_O=0: the profile class
counts of the two sessions are asserted equal (and equal to seam_probe.expected_call for the probe models), which is what
makes the twin's 16-bit element the very number the fp8 session quantised.  Every other byte of the arena stays the
sentinel.  The stand-alone qkv_epilogue_kernel has no fp8 store: a 16-bit model is always in the fused layout."""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import fp8_store as F
import seam_probe as S
from test_gpu_attention_edges import _Env

pytestmark = pytest.mark.gpu

_MODELS = {}
_T0 = time.time()


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine)
    _MODELS.clear()
    print(f"test_gpu_fp8_store.py: {time.time() - _T0:.1f} s from import to the last test")


def _dev(toks):
    return torch.tensor(list(toks), dtype=torch.int32).cuda()


def _model(hip, name, dt, w12=False):
    key = (name, dt, w12)
    if key not in _MODELS:
        dtype = S.DTYPES[dt]
        _MODELS[key] = hip.engine.SpecDecModel.from_state_dict(F.config(name), S.cast_sd(F.state_dict(name), dtype), dtype=dtype,
                                                               w12=w12)
    return _MODELS[key]


def _set_scales(ses, table):
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32))
    assert t.shape == ses.kv_scale.shape, (t.shape, ses.kv_scale.shape)
    ses.kv_scale.copy_(t.to(ses.kv_scale.device))
    torch.cuda.synchronize()


def _sentinel(ses):
    ses.kv.view(torch.uint8).fill_(S.KV_SENTINEL)
    ses.cache_len = 0
    torch.cuda.synchronize()


def _run(ses, toks, pos0=0, profile=False):
    """One call (the logits of its last min(n, 64) rows are asked for, as seam_probe.expected_call assumes); with profile:
    the profile class counts + 12-bit-record launches."""
    w0 = ses.w12_launches()
    if profile:
        ses.profile(True)
    ses.forward(_dev(toks), min(len(toks), S.MAX_LOGIT_ROWS), pos0=pos0)
    torch.cuda.synchronize()
    if not profile:
        return None
    prof = ses.profile_read()
    ses.profile(False)
    got = {k: v[1] for k, v in prof.items()}
    got["w12"] = ses.w12_launches() - w0
    return {k: v for k, v in got.items() if v}


def _arena8(ses):
    return ses.kv.cpu().numpy()


def _bits16(ses, hi):
    """[L][2][Hkv][hi][D] patterns of a 16-bit arena's first `hi` slots."""
    return F.to_bits(ses.kv[:, :, :, :hi, :].cpu())


def _assert_bytes(got, want, what):
    """Exact; a NaN byte may carry either sign (S.1111.111)."""
    nan = (want & 0x7F) == F.NAN_BYTE
    bad = np.where(nan, (got & 0x7F) != F.NAN_BYTE, got != want)
    if bad.any():
        i = tuple(int(x[0]) for x in np.nonzero(bad))
        raise AssertionError((what, f"{int(bad.sum())} of {bad.size} bytes differ; first at {i}: got {int(got[i]):#04x} want {int(want[i]):#04x}"))


def _assert_arena(ses, want, lo, hi, what):
    """Slots [lo, hi) hold `want` [L][2][Hkv][hi - lo][D]; every other byte is the sentinel."""
    a = _arena8(ses)
    _assert_bytes(a[:, :, :, lo:hi, :], want, what)
    a[:, :, :, lo:hi, :] = S.KV_SENTINEL
    assert (a == S.KV_SENTINEL).all(), (what, "a byte outside the written slots changed")


# --------------------------------------------------------------------------- planted values
def _planted_model(hip, bits, dt, n_layers=F.PLANT_LAYERS):
    return hip.engine.SpecDecModel.from_state_dict(F.planted_config(n_layers), F.planted_state_dict(bits, dt, n_layers),
                                                   dtype=S.DTYPES[dt], w12=False)


def _uniform(bits, s):
    return np.full((bits.shape[0], 2, F.PLANT_HEADS), s, dtype=np.float32)


def _planted_rows(ses, bits, dt, scales, calls, label, routes=None):
    """Per scale: the arena refilled with the sentinel, then `calls` [(rows, pos0)]; every written row holds the planted
    bytes.  routes: {rows: env of the expected launch counts} asserted at the first scale."""
    for si, s in enumerate(scales):
        _set_scales(ses, _uniform(bits, s))
        _sentinel(ses)
        one = F.planted_expected(bits, dt, _uniform(bits, s))            # [L][2][H][D]
        hi = 0
        for n, pos0 in calls:
            got = _run(ses, F.tokens(n), pos0, profile=routes is not None and si == 0)
            if got is not None:
                want = S.expected_call(F.OPT, dt, n, routes, False, ses.max_rows)
                assert {k: v for k, v in want.items() if v} == got, (label, n, want, got)
            hi = max(hi, pos0 + n)
        want = np.broadcast_to(one[:, :, :, None, :], one.shape[:3] + (hi,) + one.shape[3:])
        _assert_arena(ses, want, 0, hi, (label, dt, "scale", s))


# (label, tunables, calls): 1 row + 5 rows is the issue's forward pair; the other calls put the same sweep on the kernels whose
# store code is another instance of the epilogue.  The OPT probe's GEMMs route 64 rows per pass, so 65 rows are 64 + 1 and
# 130 rows 64 + 64 + 2 (asserted through the launch counts): no gemm_bf16_mm pass exists at this size
PLANT_ROUTES = [
    ("small_path_1_4", {}, [(1, 0), (4, 1)]),
    ("streaming_1_5", {"SD_SMALL_PATH": 0}, [(1, 0), (5, 1)]),
    ("streaming_5_16", {}, [(5, 0), (16, 5)]),
    ("many_rows_17_65", {}, [(17, 0), (65, 17)]),
    ("prefill_130", {}, [(130, 0)]),
]


@pytest.mark.parametrize("label,env,calls", PLANT_ROUTES, ids=[r[0] for r in PLANT_ROUTES])
def test_every_bf16_mantissa_through_the_plain_store(hip, label, env, calls):
    """store4_fp8 behind EPI_QKV_PLAIN: 2 signs x 128 mantissas x 4 exponents, 24 uniform power-of-two scales from 'all flush'
    to 'all saturate' - every (sign, mantissa, e4m3 binade) class, every tie, every denormal."""
    bits = F.planted_bf16()
    with _Env(**env):
        ses = _planted_model(hip, bits, "bf16").new_session(S.MAX_POS, kv_dtype="fp8")
        assert ses.max_rows == 64
        _planted_rows(ses, bits, "bf16", F.sweep_scales(), calls, label, routes=env)


def test_fp16_values_at_every_code_boundary(hip):
    """The fp16 value at each e4m3 code boundary and its two fp16 neighbours, both signs, +-65504, the smallest denormal, random
    patterns elsewhere: scale 1 (the boundaries' own scale) and two other powers of two; 1, 5 and 17 rows."""
    bits = F.planted_fp16()
    ses = _planted_model(hip, bits, "fp16").new_session(S.MAX_POS, kv_dtype="fp8")
    _planted_rows(ses, bits, "fp16", [1.0, 2.0 ** -3, 2.0 ** 4], [(1, 0), (5, 1), (17, 6)], "fp16 boundaries", routes={})


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_contract_the_arena_holds_the_product_with_the_reciprocal(hip, dt):
    """The 16-bit values on which fl32(x * fl32(1 / s)) and fl32(x / s) round to different e4m3 codes at s = 0.3 and 1.7
    (fp8_store.contract_patterns), planted in every (layer, k|v, head): the arena holds the product's byte."""
    base = F.planted_bf16() if dt == "bf16" else F.planted_fp16()
    pats = {s: F.contract_patterns(dt, s) for s in F.CONTRACT_SCALES}
    assert all(pats.values()), pats
    bits, slots = base.copy(), []
    for h in range(F.PLANT_HEADS):
        for i, p in enumerate(p for s in F.CONTRACT_SCALES for p in pats[s]):
            bits[:, :, h * F.PLANT_D + 5 * i + h] = p
            slots.append(h * F.PLANT_D + 5 * i + h)
    for s in F.CONTRACT_SCALES:                                    # the case discriminates: the quotient gives other bytes
        a, b = F.e4m3_byte(bits, dt, s), F.e4m3_byte_div(bits, dt, s)
        assert (a != b)[:, :, slots].sum() >= 2 * bits.shape[0] * 2 * F.PLANT_HEADS
    ses = _planted_model(hip, bits, dt).new_session(S.MAX_POS, kv_dtype="fp8")
    _planted_rows(ses, bits, dt, list(F.CONTRACT_SCALES), [(1, 0), (5, 1)], "contract")


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_infinities_saturate_and_nan_stays_nan(hip, dt):
    """A one-layer model (NaN must not reach a later layer's rows): +-Inf bias gives 0x7e / 0xfe, NaN bias a NaN byte (S.1111.111
    with either sign), next to finite values in the same 4-byte store group; 1 row (bf16: gemm_small) and 5 rows."""
    bits = F.special_bits(dt)
    sp = F.SPECIALS[dt]
    assert F.e4m3_byte([sp["+inf"], sp["-inf"], sp["nan"], sp["-nan"], sp["nan_payload"]], dt, 0.3).tolist() == [0x7E, 0xFE, 0x7F, 0xFF, 0x7F]
    ses = _planted_model(hip, bits, dt, n_layers=1).new_session(S.MAX_POS, kv_dtype="fp8")
    _planted_rows(ses, bits, dt, [1.0, 0.3, 2.0 ** 12], [(1, 0), (5, 1)], "specials")


# --------------------------------------------------------------------------- natural values: twins
TWIN_ENV = {"SD_FUSE_ATTN_O": 0}                                   # what an fp8 arena does to the route, for the 16-bit twin
ROWS = (1, 4, 5, 8, 9, 17, 65, 130)
TWIN_CASES = [
    ("default", {}, False, "llama_h1024", "bf16", ROWS), ("default", {}, False, "llama_h1024", "fp16", ROWS),
    ("default", {}, False, "llama_h256", "bf16", ROWS), ("default", {}, False, "llama_h256", "fp16", ROWS),
    ("default", {}, False, F.OPT, "bf16", (1, 5, 17, 65)), ("default", {}, False, F.OPT, "fp16", (1, 5, 17, 65)),
    ("default", {}, False, F.GQA, "bf16", (1, 4, 5, 9, 17, 65)), ("default", {}, False, F.GQA, "fp16", (1, 5, 17, 65)),
    ("small_off", {"SD_SMALL_PATH": 0}, False, "llama_h1024", "bf16", (1, 4)),
    ("small_off", {"SD_SMALL_PATH": 0}, False, F.GQA, "bf16", (1, 4)),
    ("norm_on_load0", {"SD_NORM_ON_LOAD": 0}, False, "llama_h1024", "bf16", (1, 5, 8)),
    ("norm_on_load1", {"SD_NORM_ON_LOAD": 1}, False, "llama_h1024", "bf16", (5, 8)),
    ("norm_on_load2", {"SD_NORM_ON_LOAD": 2}, False, "llama_h1024", "fp16", (5, 8)),
    ("w12", {}, True, "llama_h1024", "bf16", (5, 8)),             # (1 .. 4 rows take the small path, which reads no records)
]


def _twins(hip, name, dt, env, w12=False):
    """(16-bit session, fp8 session) of one model.  The tunables are process-wide and sampled whenever a session is created,
    so both are created under the route's tunables plus SD_FUSE_ATTN_O=0 (which an fp8 arena implies anyway), and a test
    creates no other session while it runs them."""
    m = _model(hip, name, dt, w12)
    with _Env(**dict(env, **TWIN_ENV)):
        s16 = m.new_session(S.MAX_POS)
        s8 = m.new_session(S.MAX_POS, kv_dtype="fp8")
    return m, s16, s8


def _outside_attention(counts):
    return {k: v for k, v in counts.items() if k != "attention"}


@pytest.mark.parametrize("label,env,w12,name,dt,rows", TWIN_CASES, ids=[f"{c[0]}-{c[3]}-{c[4]}" for c in TWIN_CASES])
def test_every_stored_byte_is_the_twins_element_under_its_own_scale(hip, label, env, w12, name, dt, rows):
    """One call of n rows at position 0 into a 16-bit arena and, under each of the four tables, into an e4m3 arena: all
    layers, K and V, every head, exact.  The launch counts of the two sessions are equal class by class."""
    m, s16, s8 = _twins(hip, name, dt, env, w12)
    if name in S.CONTIG_MODELS:                                    # 130 rows are ONE contiguous pass on gemm_bf16_mm, whose
        assert s8.max_rows == s16.max_rows == 256                  # epilogue stores V through store4_fp8 and K through to_fp8
    tables = {k: F.scale_table(name, dt, k) for k in F.TABLES}
    for n in rows:
        toks = F.tokens(n)
        _sentinel(s16)
        c16 = _run(s16, toks, profile=True)
        bits = _bits16(s16, n)
        for ti, (kind, tab) in enumerate(tables.items()):
            _set_scales(s8, tab)
            _sentinel(s8)
            c8 = _run(s8, toks, profile=ti == 0)
            if ti == 0:
                assert _outside_attention(c8) == _outside_attention(c16) and c8["attention"] == c16["attention"], (label, n, c8, c16)
                if name != F.GQA:
                    want = S.expected_call(name, dt, n, dict(env, **TWIN_ENV), m.w12_packed if w12 else False, s8.max_rows)
                    assert {k: v for k, v in want.items() if v} == c8, (label, n, want, c8)
                    assert not w12 or c8.get("w12", 0) > 0, (label, n, c8)
            _assert_arena(s8, F.e4m3_byte_table(bits, dt, tab), 0, n, (label, name, dt, n, kind))


POS_CASES = [("llama_h256", "bf16"), ("llama_h1024", "fp16"), (F.OPT, "bf16"), (F.GQA, "bf16")]


@pytest.mark.parametrize("name,dt", POS_CASES, ids=[f"{n}-{d}" for n, d in POS_CASES])
def test_first_pass_at_positions_0_1_and_the_last(hip, name, dt):
    """5 rows at pos0 = 0, 1 and max_position - 5 behind a prefix (the last row of the RoPE / learned-position table, the last
    slots of the arena): every slot written so far - the prefix's too - against the twin, `real` and `pow2`."""
    _, s16, s8 = _twins(hip, name, dt, {})
    n = 5
    for pos0 in (0, 1, S.MAX_POS - n):
        for kind in ("real", "pow2"):
            tab = F.scale_table(name, dt, kind)
            _set_scales(s8, tab)
            for ses in (s16, s8):
                _sentinel(ses)
                if pos0:
                    ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
                _run(ses, F.tokens(n), pos0)
            _assert_arena(s8, F.e4m3_byte_table(_bits16(s16, pos0 + n), dt, tab), 0, pos0 + n, (name, dt, pos0, kind))


def _stream_pair(hip, name, dt):
    """Two streams with a table each (`real`, `tight`) and their twins: [(fp8 session, twin, table)]."""
    m = _model(hip, name, dt)
    out = []
    for kind in ("real", "tight"):
        with _Env(**TWIN_ENV):
            s16 = m.new_session(S.MAX_POS)
            s8 = m.new_session(S.MAX_POS, kv_dtype="fp8")
        tab = F.scale_table(name, dt, kind)
        _set_scales(s8, tab)
        out.append((s8, s16, tab))
    return out


@pytest.mark.parametrize("name,dt", [("llama_h256", "bf16"), (F.GQA, "fp16")])
def test_two_stream_batch_forward_each_arena_under_its_own_table(hip, name, dt):
    """One sd_batch_forward over two streams (cache lengths 0 and 2, 5 and 4 new rows), the sessions carrying different
    tables: each arena holds its own stream's bytes under its own scales."""
    pairs = _stream_pair(hip, name, dt)
    plan = [(0, F.tokens(5)), (2, tuple(S.ordinary(r + 7) for r in range(4)))]
    for which in (1, 0):                                           # the twins' batch, then the fp8 sessions'
        sess = [p[which] for p in pairs]
        seqs = []
        for ses, (pos0, toks) in zip(sess, plan):
            _sentinel(ses)
            if pos0:
                ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
            seqs.append(_dev(S.prefix_tokens(pos0) + list(toks)))
        n_new = [len(t) for _, t in plan]
        hip.engine.batch_forward(sess, seqs, n_new, n_new)
        torch.cuda.synchronize()
    for (s8, s16, tab), (pos0, toks) in zip(pairs, plan):
        hi = pos0 + len(toks)
        _assert_arena(s8, F.e4m3_byte_table(_bits16(s16, hi), dt, tab), 0, hi, ("batch_forward", name, dt, pos0))


@pytest.mark.parametrize("name,dt", [("llama_h256", "bf16"), (F.OPT, "fp16")])
def test_two_stream_batch_prefill_each_arena_under_its_own_table(hip, name, dt):
    """One sd_batch_prefill over two streams (33 rows from position 0, 20 rows behind 3 cached ones), a table each."""
    pairs = _stream_pair(hip, name, dt)
    plan = [(0, F.tokens(33)), (3, tuple(S.ordinary(r + 11) for r in range(20)))]
    for which in (1, 0):
        sess = [p[which] for p in pairs]
        seqs = []
        for ses, (pos0, toks) in zip(sess, plan):
            _sentinel(ses)
            if pos0:
                ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
            seqs.append(_dev(S.prefix_tokens(pos0) + list(toks)))
        hip.engine.batch_prefill(sess, seqs, [len(t) for _, t in plan])
        torch.cuda.synchronize()
    for (s8, s16, tab), (pos0, toks) in zip(pairs, plan):
        hi = pos0 + len(toks)
        _assert_arena(s8, F.e4m3_byte_table(_bits16(s16, hi), dt, tab), 0, hi, ("batch_prefill", name, dt, pos0))


@pytest.mark.parametrize("name,dt", [("llama_h256", "bf16"), (F.OPT, "bf16"), (F.GQA, "fp16")])
def test_tree_pass_slot_by_node_scale_by_head(hip, name, dt):
    """sd_session_forward_tree, seam_probe's 9 nodes behind 3 cached keys: the slot goes by node, the RoPE angle / learned
    position by depth, the scale by (layer, k|v, head) - slots [0, 12) against the twin's tree pass."""
    _, s16, s8 = _twins(hip, name, dt, {})
    base, N = S.TREE_BASE, S.TREE_NODES
    toks = F.tokens(N)
    pos, bits = S.tree_shape(N, base)
    tab = F.scale_table(name, dt, "real")
    _set_scales(s8, tab)
    logits = torch.empty((N, F.config(name).vocab_size), dtype=torch.float32, device="cuda")
    for ses in (s16, s8):
        _sentinel(ses)
        ses.forward(_dev(S.prefix_tokens(base)), 0, pos0=0)
        hip.engine.check(hip.lib.sd_session_forward_tree(
            ses.handle, _dev(toks).data_ptr(), (C.c_int32 * N)(*pos), (C.c_uint64 * N)(*bits), N, base, logits.data_ptr(),
            logits.stride(0), torch.cuda.current_stream().cuda_stream), "sd_session_forward_tree")
        torch.cuda.synchronize()
    assert pos[8] == base + 1                                      # slot base + 8 holds a depth-1 row: slot != position
    _assert_arena(s8, F.e4m3_byte_table(_bits16(s16, base + N), dt, tab), 0, base + N, ("tree", name, dt))


def test_two_rank_loopback_shards_hold_their_own_heads_under_their_own_tables(hip):
    """A 2-rank loopback tensor-parallel target of llama_h256 (one of the two KV heads per rank): rank r's e4m3 arena under
    rank r's own table (`real` of head r for rank 0, `tight` for rank 1) against rank r's own 16-bit twin, 5 and 17 rows."""
    from llmspeculativesampling_amd import tp
    from test_gpu_native_parity import _run_ranks
    name, dt, W = "llama_h256", "bf16", 2
    cfg, dtype = F.config(name), S.DTYPES[dt]
    sd16 = S.cast_sd(F.state_dict(name), dtype)
    groups = tp.TPGroup.loopback(W)
    shards = [tp.shard_model(cfg, sd16, r, W, group=groups[r], dtype=dtype, max_pos=S.MAX_POS) for r in range(W)]
    assert shards[0].cfg.num_key_value_heads == 1
    tabs = [F.scale_table(name, dt, kind)[:, :, r:r + 1] for r, kind in enumerate(("real", "tight"))]
    s16 = [m.new_session(S.MAX_POS) for m in shards]
    s8 = [m.new_session(S.MAX_POS, kv_dtype="fp8") for m in shards]
    for r in range(W):
        _set_scales(s8[r], tabs[r])
    hi = 0
    for sess in (s16, s8):
        for ses in sess:
            _sentinel(ses)
        hi = 0
        for n in (5, 17):
            _run_ranks([lambda r=r, n=n, hi=hi: sess[r].forward(_dev(F.tokens(n)), 1, pos0=hi) for r in range(W)])
            hi += n
    for r in range(W):
        _assert_arena(s8[r], F.e4m3_byte_table(_bits16(s16[r], hi), dt, tabs[r]), 0, hi, ("tp2", "rank", r))


def test_fp8_arena_is_refused_without_the_fused_layout(hip):
    """The fused QKV epilogue is the one fp8 store site: a 16-bit model registered WITHOUT the fused layout (the C API admits
    one; the Python engine never builds it) gets an error from sd_session_set_kv_fp8, not 16-bit rows in a 1-byte arena.
    No forward is run."""
    class Unfused(hip.engine.SpecDecModel):
        def _build(self, get):
            self.fused = False
            super()._build(get)

    sd = S.cast_sd(F.state_dict("llama_h256"), torch.bfloat16)
    m = Unfused(F.config("llama_h256"), lambda n: sd[n], dtype=torch.bfloat16, w12=False)
    assert m._c.fused_layout == 0
    with pytest.raises(ValueError, match="fused"):
        m.new_session(S.MAX_POS, kv_dtype="fp8")
    assert m.new_session(S.MAX_POS).kv.dtype == torch.bfloat16      # (a 16-bit arena is still fine)


# --------------------------------------------------------------------------- sd_session_compact_kv
@pytest.mark.parametrize("name,kv_dtype", [(F.GQA, "fp8"), (F.GQA, None), ("llama_h256", "fp8"), ("llama_h256", None)],
                         ids=["D32-fp8", "D32-bf16", "D128-fp8", "D128-bf16"])
def test_compact_kv_moves_whole_rows_of_the_arenas_own_width(hip, name, kv_dtype):
    """An arena of random bytes, an ascending index set of k = 1, 6 and 64 rows compacted to base = 0 and max_seq - 64: slot
    base + j of every (layer, k|v, head) plane holds what slot base + idx[j] held - a numpy gather of the arena before - and
    every byte outside rows [base, base + k) is unchanged.  fp8 rows are D bytes (32: two 16-byte pieces), bf16 rows 2 D."""
    ses = _model(hip, name, "bf16").new_session(S.MAX_POS, kv_dtype=kv_dtype)
    rng = np.random.default_rng(9)
    for base in (0, ses.max_seq - 64):
        for k in (1, 6, 64):
            idx = np.sort(rng.choice(64, size=k, replace=False)).astype(np.int32)
            raw = ses.kv.view(torch.uint8)
            raw.copy_(torch.from_numpy(rng.integers(0, 256, size=tuple(raw.shape), dtype=np.uint8)).cuda())
            torch.cuda.synchronize()
            before = raw.cpu().numpy().copy()
            idx_dev = torch.from_numpy(idx).cuda()
            hip.engine.check(hip.lib.sd_session_compact_kv(ses.handle, base, idx_dev.data_ptr(), k,
                                                           torch.cuda.current_stream().cuda_stream), "sd_session_compact_kv")
            torch.cuda.synchronize()
            want = before.copy()
            want[:, :, :, base:base + k, :] = before[:, :, :, base + idx, :]
            assert np.array_equal(raw.cpu().numpy(), want), (name, kv_dtype, base, k)
