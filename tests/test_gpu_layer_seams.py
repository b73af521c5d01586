"""Adversarial rows through every norm / fold / act route of the layer seams (`pytest -m gpu`).

The kernels between the GEMMs and attention - embed_kernel, embed_norm_kernel, norm_kernel, residual_norm_kernel,
qkv_epilogue_kernel, act_kernel, reduce_rows_kernel, reduce_addpos_kernel, logits_kernel, their fused twins in
gemm_epilogue_fold, the residual epilogue + norm-on-load pair, gemm_small's PRO_EMBED / PRO_RESID prologues and the
12-bit-record launches - through Session.forward, sd_batch_forward and sd_session_forward_tree on the probe models of
tests/seam_probe.py.  The rows are not i.i.d.: one hidden column at 16 .. 256 times the background (family A, one column
class per row: vector-group, 16-byte, 16-column-tile and register-group edges), all-zero / 2^-60 / alternating / large-mean
rows (family B); weights that are zero outside one k-slab of a split-K GEMM (family C: every loop of the consumers' folds);
one decisive intermediate column with gate pre-activations from -96 to 96, one decisive vocabulary column (family D); and
the K / V rows each pass writes, with every other arena byte held unchanged (E).  test_seam_probe_cpu.py shows on the
oracle alone that a norm which drops the planted column at ONE site - a fold that skips the slab, a gate of the wrong
sign, a position table read at the wrong offset - moves the observed rows by >= 20x the bar used here, and lists the
sites for which it cannot.

Bars, none taken from the code under test: fp32 - max-abs 1e-3 against the fp32 oracle; 16-bit -
_assert_within_reference_error of test_gpu_production_parity (HIP's error against the fp32 oracle at most 1.5x the
same-dtype oracle's own), per pass over all the logit rows the call returns.  Written K / V rows are held to the same rule
(fp32: the arena bar of test_gpu_parity), and every arena byte outside the slots a pass owns must be unchanged.

Every test asserts the route it claims from the session's profile class counts and w12_launches(), against
seam_probe.expected_launches - the launch sequence of forward_small / forward_impl restated per tunable."""
import ctypes as C
import os

import pytest
import torch

import seam_probe as S
from test_gpu_attention_edges import _Env, _Stats
from test_gpu_production_parity import _assert_within_reference_error

pytestmark = pytest.mark.gpu

_ORACLES, _MODELS = {}, {}


def _oracle(name, dt):
    if (name, dt) not in _ORACLES:
        _ORACLES[(name, dt)] = S.SeamOracle(name, S.DTYPES[dt])
    return _ORACLES[(name, dt)]


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine)
    _MODELS.clear()


def _model(hip, name, dt, w12=False):
    """One device model per (probe model, dtype, 12-bit records) for the whole file."""
    key = (name, dt, w12)
    if key not in _MODELS:
        dtype = S.DTYPES[dt]
        _MODELS[key] = hip.engine.SpecDecModel.from_state_dict(S.probe_config(name), S.cast_sd(S.probe_state_dict(name), dtype),
                                                               dtype=dtype, w12=w12)
    return _MODELS[key]


def _dev(toks):
    return torch.tensor(list(toks), dtype=torch.int32).cuda()


def _feed(ses, toks, pos0=0):
    """One pass: the logits of its last min(n, 64) rows (a session at cache_len 0 gets the prefix first)."""
    if pos0 and ses.cache_len != pos0:
        ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
    nl = min(len(toks), S.MAX_LOGIT_ROWS)
    return ses.forward(_dev(toks), nl, pos0=pos0).float().cpu().clone()


def _launches(ses, toks, pos0=0):
    """(logits, profile class counts + 12-bit-record launches) of one pass."""
    w0 = ses.w12_launches()
    ses.profile(True)
    out = _feed(ses, toks, pos0)
    prof = ses.profile_read()
    ses.profile(False)
    got = {k: v[1] for k, v in prof.items()}
    got["w12"] = ses.w12_launches() - w0
    return out, got


def _judge(st, got, name, dt, toks, pos0=0):
    nl = got.shape[0]
    truth = _oracle(name, "fp32").run(toks, pos0)[0][-nl:]
    ref16 = None if dt == "fp32" else _oracle(name, dt).run(toks, pos0)[0][-nl:]
    st.judge(got, truth, ref16, (len(toks), toks[:S.MAX_PLANTS], pos0))


def _run_route(hip, label, env, w12, name, dt, rows, contig=False):
    st = _Stats(f"{label} {name} {dt}")
    with _Env(**env):
        m = _model(hip, name, dt, w12)
        ses = m.new_session(S.MAX_POS)
        assert ses.max_rows == (256 if dt == "fp32" or name in S.CONTIG_MODELS else 64), ses.max_rows
        for n in rows:
            want = None
            for fam, toks in S.route_passes(name, dt, n):
                if contig and fam != "A":
                    continue
                _judge(st, _feed(ses, toks), name, dt, toks)
                if want is None:                                   # the route, once per row count
                    want = S.expected_call(name, dt, n, env, w12, ses.max_rows)
                    again, got = _launches(ses, toks)
                    _judge(st, again, name, dt, toks)
                    assert {k: v for k, v in want.items() if v} == {k: v for k, v in got.items() if v}, (st.label, n, want, got)
    st.report()


_ROUTE_CASES = [(lab, env, w12, name, dt, rows) for lab, env, w12, name, dts, rows in S.ROUTES for dt in dts]


@pytest.mark.parametrize("label,env,w12,name,dt,rows", _ROUTE_CASES, ids=[f"{c[0]}-{c[3]}-{c[4]}" for c in _ROUTE_CASES])
def test_planted_columns_and_degenerate_rows_through_every_route(hip, label, env, w12, name, dt, rows):
    """seam_probe.ROUTES: the fp32 per-op chain (embed_norm_kernel's vector and scalar load paths, embed_kernel + norm_kernel /
    to_operand_kernel, embed_kernel tiled + reduce_addpos_kernel, residual_norm_kernel in RES_PRE / RES_POST,
    qkv_epilogue_kernel, act_kernel, reduce_rows_kernel, logits_kernel with a partial last block at V = 500); the 16-bit
    default at 1 .. 65 rows (small path up to 4 bf16 rows, fused epilogues, fused attention + O up to 16 rows at D = 128,
    norm on load up to 8 rows at H = 1024); the small path off / with every seam a prologue / without the embedding
    prologue; norm on load 0 / 1 / 2; two-launch attention; 12-bit records.  Every family-A column class and family-B row
    rides every row count up to 16 (several passes where the plants outnumber the rows), one pass of each beyond."""
    _run_route(hip, label, env, w12, name, dt, rows)


@pytest.mark.parametrize("name,dt", S.PREFILL_MODELS, ids=[f"{n}-{d}" for n, d in S.PREFILL_MODELS])
def test_planted_columns_in_a_contiguous_prefill_pass(hip, name, dt):
    """One call of 130 rows at pos0 = 0, family A on rows 66 .. 73, logits of the last 64 rows.  H = 1024: ONE contiguous
    pass (> 80 rows: RowTab.contig, matrix-core prefill attention, the many-row GEMM kernels in front of every seam);
    H = 256: the model's GEMMs route 64 rows, so the call is cut into passes of 64 + 64 + 2 rows, the first without a
    head - the launch counts of all three are asserted."""
    _run_route(hip, "prefill", {}, False, name, dt, S.PREFILL_ROWS, contig=True)


def test_hidden_8192_fills_both_register_groups(hip):
    """H = 8192, the limit sd_model_create admits, ONE pass of 8 rows: residual_norm_kernel with 1024 threads and both
    register groups full (classes 4095 | 4096 | 8191), embed_norm_kernel's MAXV = 4 vectors per thread exactly full."""
    name, dt = "llama_h8192", "bf16"
    st = _Stats(f"h8192 {name} {dt}")
    m = _model(hip, name, dt)
    ses = m.new_session(16)
    toks = S.h8192_pass()
    assert [S.plant_column(name, t) for t in toks] == [4, 7, 8, 15, 16, 4095, 4096, 8191] and S.rn_threads(8192) == 1024
    out, got = _launches(ses, toks)
    _judge(st, out, name, dt, toks)
    want = S.expected_launches(name, dt, 8)
    assert {k: v for k, v in want.items() if v} == {k: v for k, v in got.items() if v}, (want, got)
    del _MODELS[(name, dt, False)]
    st.report()


# --------------------------------------------------------------------------- C. planted slabs
@pytest.mark.parametrize("case", S.C_CASES, ids=[c[0] for c in S.C_CASES])
def test_planted_slab_reaches_every_loop_of_the_fold(hip, case):
    """A weight that is zero outside ONE k-slab of its split-K GEMM (seam_probe.C_CASES; S and ksp from sd_gemm_route under
    the case's tunables): the first slab, the last slab and the first slab of each of the fold's loops (8-burst, 4-burst,
    scalar tail), one model each.  The logits are that slab's contribution alone, so a fold that skips it returns the
    logits of the all-zero weight - >= 20x the bar away (test_seam_probe_cpu.py)."""
    label, name, dt, env, n, weight, consumer = case
    Sn, ksp = S.c_slabs(case)
    toks, dtype = S.c_tokens(n), S.DTYPES[dt]
    st = _Stats(f"C {label} S={Sn} -> {consumer}")
    with _Env(**env):
        for s in S.slab_classes(Sn):
            sd = S.slab_state_dict(name, weight, ksp, s)
            m = hip.engine.SpecDecModel.from_state_dict(S.probe_config(name), S.cast_sd(sd, dtype), dtype=dtype,
                                                        w12=label in S.C_W12)
            ses = m.new_session(S.MAX_POS)
            out, got = _launches(ses, toks)
            nl = out.shape[0]
            truth = S.SeamOracle(name, sd=sd).forward(toks)[0][-nl:]
            ref16 = S.SeamOracle(name, dtype, sd=sd).forward(toks)[0][-nl:]
            st.judge(out, truth, ref16, (label, "slab", s))
            want = S.expected_call(name, dt, n, env, m.w12_packed if label in S.C_W12 else False, ses.max_rows)
            assert {k: v for k, v in want.items() if v} == {k: v for k, v in got.items() if v}, (st.label, want, got)
            if label in S.C_W12:                                   # the planted matrix itself streams as records
                kind = "down" if "down_proj" in weight else "gate_up"
                assert 0 in m.w12_packed.get(kind, []) and got["w12"] > 0, (st.label, m.w12_packed)
    st.report()


# --------------------------------------------------------------------------- D. activation columns
@pytest.mark.parametrize("label,name,dt,w12,env,rows", S.D_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in S.D_CASES])
def test_decisive_activation_column_at_every_layout_edge(hip, label, name, dt, w12, env, rows):
    """One intermediate column j - 0, 7 | 8 (the 8-gate / 8-up interleave of the fused layout), 15 | 16, 255 | 256
    (act_kernel's block edge), I - 1 - decides the logits of six tokens whose gate pre-activation sits at about -96 (expf
    overflows, SiLU = -0), -20, -+2^-10, 20 and 96: act_kernel (fp32), EPI_ACT_SILU in gemm_small (bf16, <= 4 rows; with
    SD_SMALL_PATH=2), in the streaming GEMM (small path off, norm on load 0), behind the norm-on-load operand load
    (H = 1024, 5 rows; norm on load 1 / 2), in the many-row kernels (17, 64, 65 rows), and in a model with 12-bit records."""
    st = _Stats(f"D {label} {name} {dt}")
    dtype = S.DTYPES[dt]
    with _Env(**env):
        for j in S.act_columns(name):
            sd = S.act_state_dict(name, j)
            m = hip.engine.SpecDecModel.from_state_dict(S.probe_config(name), S.cast_sd(sd, dtype), dtype=dtype, w12=w12)
            if w12:                                                # measured, not assumed: the planted matrix does not pack
                assert 0 not in m.w12_packed.get("gate_up", []) and 1 in m.w12_packed.get("gate_up", []), m.w12_packed
            o32 = S.SeamOracle(name, sd=sd)
            o16 = None if dt == "fp32" else S.SeamOracle(name, dtype, sd=sd)
            ses = m.new_session(S.MAX_POS)
            for n in rows:
                for i, toks in enumerate(S.act_passes(n)):
                    out, got = _launches(ses, toks)
                    nl = out.shape[0]
                    st.judge(out, o32.forward(toks)[0][-nl:], None if o16 is None else o16.forward(toks)[0][-nl:], (j, toks[:8]))
                    if i == 0:
                        want = S.expected_call(name, dt, n, env, m.w12_packed if w12 else False, ses.max_rows)
                        assert {k: v for k, v in want.items() if v} == {k: v for k, v in got.items() if v}, (st.label, j, n, want, got)
    st.report()


@pytest.mark.parametrize("label,name,dt,env,rows", S.RELU_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in S.RELU_CASES])
def test_opt_fc1_bias_cancels_to_a_decisive_remainder(hip, label, name, dt, env, rows):
    """OPT's fc1 + bias + ReLU at column j (0, 7 | 8, 15 | 16, 255 | 256, I - 1): the dot is 4 (1 + 2^-6 + 2^-14) for every
    row, the bias -4 (1 + 2^-6), and the 2^-12 that is left decides the logits through a scaled fc2 column - a kernel that
    rounds the dot to 16 bits before it adds the bias, or drops the bias path of its fold, returns 0 there.  act_kernel
    (fp32), EPI_ACT_RELU in gemm_small (bf16, 1 row; SD_SMALL_PATH=2) and in the streaming / many-row GEMMs."""
    st = _Stats(f"D relu {label} {name} {dt}")
    dtype = S.DTYPES[dt]
    with _Env(**env):
        for j in S.act_columns(name):
            sd = S.relu_state_dict(name, j, "cancel")
            m = hip.engine.SpecDecModel.from_state_dict(S.probe_config(name), S.cast_sd(sd, dtype), dtype=dtype, w12=False)
            ses = m.new_session(S.MAX_POS)
            for n in rows:
                toks = S.head_tokens(n)
                out, got = _launches(ses, toks)
                truth = S.SeamOracle(name, sd=sd).forward(toks)[0]
                st.judge(out, truth, None if dt == "fp32" else S.SeamOracle(name, dtype, sd=sd).forward(toks)[0], (j, n))
                want = S.expected_call(name, dt, n, env, False, ses.max_rows)
                assert {k: v for k, v in want.items() if v} == {k: v for k, v in got.items() if v}, (st.label, j, n, want, got)
    st.report()


@pytest.mark.parametrize("name,dt", S.HEAD_MODELS, ids=[f"{n}-{d}" for n, d in S.HEAD_MODELS])
def test_planted_head_column_is_every_rows_maximum(hip, name, dt):
    """lm_head row v - 0, 15 | 16, 255 | 256 (logits_kernel's block edge), V - 1 (V = 500: in the partial last block) - reads
    a channel every row carries, so column v is the maximum of every row (about 50 against < 10): 1 row (bf16: the small
    path's head), 5 and 17 rows, against the oracle, and the argmax itself."""
    st = _Stats(f"D head {name} {dt}")
    dtype = S.DTYPES[dt]
    for v in S.head_columns(name):
        sd = S.head_state_dict(name, v)
        m = hip.engine.SpecDecModel.from_state_dict(S.probe_config(name), S.cast_sd(sd, dtype), dtype=dtype, w12=False)
        ses = m.new_session(S.MAX_POS)
        for n in S.HEAD_ROWS:
            toks = S.head_tokens(n)
            out = _feed(ses, toks)
            truth = S.SeamOracle(name, sd=sd).forward(toks)[0]
            st.judge(out, truth, None if dt == "fp32" else S.SeamOracle(name, dtype, sd=sd).forward(toks)[0], (v, n))
            assert out.argmax(-1).tolist() == [v] * n, (st.label, v, n)
    st.report()


@pytest.mark.parametrize("name,dt,rows", [("llama_h96", "fp32", (1, 5)), ("llama_h256", "bf16", (1, 5, 17)),
                                          ("opt_proj_h128", "bf16", (5,))], ids=["fp32-V500", "bf16", "opt-proj"])
def test_logits_rows_with_a_leading_dimension_past_the_vocabulary(hip, name, dt, rows):
    """logits_out with a row stride of V + 24 floats (logits_kernel's ld; V = 500: its last block is partial): the same bits
    as the contiguous call, and not one float written between the rows or behind the last."""
    ses = _model(hip, name, dt).new_session(S.MAX_POS)
    V = S.probe_config(name).vocab_size
    for n in rows:
        toks = S.route_passes(name, dt, n)[-1][1]
        want = _feed(ses, toks)
        buf = torch.full((n + 1, V + 24), 7.5, dtype=torch.float32, device="cuda")
        got = ses.forward(_dev(toks), n, logits_out=buf[:, :V], pos0=0)
        assert got.stride(0) == V + 24 and torch.equal(got.cpu(), want), (name, n)
        assert bool((buf[:, V:] == 7.5).all()) and bool((buf[n] == 7.5).all()), (name, n)


# --------------------------------------------------------------------------- E. written K / V rows
def _sentinel(ses):
    ses.kv.view(torch.uint8).fill_(S.KV_SENTINEL)
    torch.cuda.synchronize()


def _check_kv(st, ses, before, slots, name, dt, past32, past16, what):
    """Arena slots `slots` (a range) against the oracle's K (after RoPE) / V rows of the same keys; every other byte of the
    arena as it was before the pass."""
    after = ses.kv.clone()
    lo, hi = slots.start, slots.stop
    a8, b8 = after.view(torch.uint8).clone(), before.view(torch.uint8).clone()
    a8[:, :, :, lo:hi, :] = 0
    b8[:, :, :, lo:hi, :] = 0
    assert torch.equal(a8, b8), (st.label, what, "a byte outside the pass's slots changed")
    if past32 is None:                                             # (fp8 arena: the sentinel half only)
        return
    for l in range(after.shape[0]):
        for j in range(2):
            got = after[l, j, :, lo:hi, :].float().cpu()
            truth = past32[l][j][0, :, lo:hi, :].float()
            assert bool(torch.isfinite(got).all()), (st.label, what, l, j)
            if dt == "fp32":
                e = float((got - truth).abs().max())
                assert e <= 1e-4 * max(1.0, float(truth.abs().max())), (st.label, what, l, j, e)
            else:
                ref16 = past16[l][j][0, :, lo:hi, :].float()
                _assert_within_reference_error(S.errors(got, ref16, truth), f"{st.label} {what} layer {l} {'kv'[j]}")


@pytest.mark.parametrize("name,dt,pos0s,n", S.KV_CASES, ids=[f"{c[0]}-{c[1]}" for c in S.KV_CASES])
def test_written_kv_rows_and_untouched_arena(hip, name, dt, pos0s, n):
    """The arena is filled with a sentinel byte, the prefix is fed, then ONE pass of 5 rows at pos0 in {0, 1, max_position - 5}
    (the last row of the RoPE / learned-position table): slots [pos0, pos0 + 5) of every layer, K / V plane and head hold
    the oracle's rows, every other byte is what it was - the prefix in front, the sentinel behind, all planes."""
    st = _Stats(f"kv {name} {dt}")
    m = _model(hip, name, dt)
    for pos0 in pos0s:
        fam, toks = S.kv_pass(name, dt, n)
        ses = m.new_session(S.MAX_POS)
        _sentinel(ses)
        if pos0:
            ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
        before = ses.kv.clone()
        assert bool((before.view(torch.uint8)[:, :, :, pos0:, :] == S.KV_SENTINEL).all())
        _judge(st, _feed(ses, toks, pos0), name, dt, toks, pos0)
        past16 = None if dt == "fp32" else _oracle(name, dt).run(toks, pos0)[1]
        _check_kv(st, ses, before, range(pos0, pos0 + n), name, dt, _oracle(name, "fp32").run(toks, pos0)[1], past16, pos0)
    st.report()


def test_fp8_arena_keeps_every_byte_outside_the_written_slots(hip):
    """The same pass into an e4m3 arena: only the sentinel half is asserted here; every stored byte is held to exact e4m3
    under its own scale by test_gpu_fp8_store.py."""
    name, dt, n = "llama_h256", "bf16", S.KV_ROWS
    st = _Stats(f"kv fp8 {name}")
    m = _model(hip, name, dt)
    for pos0 in (0, 1, S.MAX_POS - n):
        ses = m.new_session(S.MAX_POS, kv_dtype="fp8")
        _sentinel(ses)
        if pos0:
            ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
        before = ses.kv.clone()
        got = _feed(ses, S.kv_pass(name, dt, n)[1], pos0)
        assert bool(torch.isfinite(got).all())
        _check_kv(st, ses, before, range(pos0, pos0 + n), name, dt, None, None, pos0)
        assert bool((ses.kv[:, :, :, pos0:pos0 + n, :] != S.KV_SENTINEL).any())


@pytest.mark.parametrize("name,dt", S.TREE_CASES)
def test_tree_pass_writes_slots_by_node_and_positions_by_depth(hip, name, dt):
    """sd_session_forward_tree, 9 nodes behind 3 cached keys: node m's K / V row lands in slot 3 + m while its RoPE angle /
    learned position is its depth (3 + m // 8) - tab_slot against row_pos.  Logits and slots [3, 12) against the oracle's
    tree forward, every other byte unchanged."""
    st = _Stats(f"tree {name} {dt}")
    base, N = S.TREE_BASE, S.TREE_NODES
    cfg = S.probe_config(name)
    toks = S.tree_tokens(name)
    pos, bits = S.tree_shape(N, base)
    ses = _model(hip, name, dt).new_session(S.MAX_POS)
    _sentinel(ses)
    ses.forward(_dev(S.prefix_tokens(base)), 0, pos0=0)
    before = ses.kv.clone()
    logits = torch.empty((N, cfg.vocab_size), dtype=torch.float32, device="cuda")
    hip.engine.check(hip.lib.sd_session_forward_tree(
        ses.handle, _dev(toks).data_ptr(), (C.c_int32 * N)(*pos), (C.c_uint64 * N)(*bits), N, base, logits.data_ptr(),
        logits.stride(0), torch.cuda.current_stream().cuda_stream), "sd_session_forward_tree")
    truth, past32 = _oracle(name, "fp32").tree(toks, base, pos, bits)
    ref16, past16 = (None, None) if dt == "fp32" else _oracle(name, dt).tree(toks, base, pos, bits)
    st.judge(logits.cpu(), truth, ref16, "tree")
    _check_kv(st, ses, before, range(base, base + N), name, dt, past32, past16, "tree")
    assert pos[8] == base + 1 and pos[7] == base                   # slot 3 + 8 holds a depth-1 row: slot != position
    st.report()


@pytest.mark.parametrize("name,dt", S.BATCH_MODELS)
def test_two_stream_batch_writes_each_streams_own_arena(hip, name, dt):
    """One sd_batch_forward over two streams (cache lengths 0 and 2, 5 and 4 new rows): each stream's rows land in its own
    arena at its own positions, against its own oracle forward; every other byte of both arenas unchanged."""
    st = _Stats(f"batch {name} {dt}")
    m = _model(hip, name, dt)
    plan = [(pos0, toks) for _, pos0, toks in S.batch_plan(name, dt)]
    sess, seqs, befores = [], [], []
    for pos0, toks in plan:
        ses = m.new_session(S.MAX_POS)
        _sentinel(ses)
        if pos0:
            ses.forward(_dev(S.prefix_tokens(pos0)), 0, pos0=0)
        sess.append(ses)
        seqs.append(_dev(S.prefix_tokens(pos0) + list(toks)))
        befores.append(ses.kv.clone())
    n_new = [len(t) for _, t in plan]
    out = hip.engine.batch_forward(sess, seqs, n_new, n_new).float().cpu().clone()
    for ses, before, (pos0, toks), got in zip(sess, befores, plan, torch.split(out, n_new)):
        _judge(st, got, name, dt, toks, pos0)
        past16 = None if dt == "fp32" else _oracle(name, dt).run(toks, pos0)[1]
        _check_kv(st, ses, before, range(pos0, pos0 + len(toks)), name, dt, _oracle(name, "fp32").run(toks, pos0)[1], past16, pos0)
    st.report()
