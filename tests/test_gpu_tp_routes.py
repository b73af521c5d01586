"""The tensor-parallel forward through every reduce route, world size and entry (`pytest -m gpu`).

Shards of the probe models of tests/tp_probe.py run in one process through the loopback group: the GEMM kernels, tp_fold_kernel,
the in-place partial of a one-slab plan and tp_sum_kernel are the RCCL path's own; only the all-reduce itself is the
in-process rendezvous (RCCL's all-reduce at world > 1 needs more than one GPU and stays untested here).

Every test asserts the route it claims, at run time: the reduce-route classes from sd_gemm_route (tp_probe.reduce_routes), the
profile's class "other" - one scope per tp_fold_kernel launch and one per tp_sum_kernel launch - against the folds and
sums those routes imply, and Session.prefill_attn_launches() against sd_prefill_attn_route for the shard's head count.

Bars, none taken from the code under test: fp32 - max-abs 1e-3 against the fp32 oracle; bf16 -
_assert_within_reference_error of test_gpu_production_parity (HIP's error against the fp32 oracle at most 1.5x the
same-dtype oracle's own), per call over all returned logit rows.  Written K / V rows: the same rule (fp32: the arena bar of
test_gpu_parity) against KV heads [r Hkv / W, (r + 1) Hkv / W) of the unsharded oracle, and every arena byte outside the
slots a call owns unchanged.  All ranks' logits are torch.equal in every test.  test_tp_probe_cpu.py shows on the oracle
alone which plants move every observed row by >= 20x these bars under a dropped rank, a rank read twice or a skipped slab."""
import ctypes as C
import os

import pytest
import torch

import attn_probe as A
import tp_probe as P
from test_gpu_attention_edges import _Stats
from test_gpu_production_parity import _assert_within_reference_error

pytestmark = pytest.mark.gpu

_ORACLES, _MODELS = {}, {}
LIMIT_S = 90.0                     # one rank run: a few forward calls (the first one loads the code object)


def _oracle(name, dt, label="base", sd=None, world=0):
    """One oracle per (probe, dtype, plant) for the whole file; a plant's weights depend on the world size."""
    key = (name, dt, label, world if label != "base" else 0)
    if key not in _ORACLES:
        _ORACLES[key] = P.TpOracle(name, P.DTYPES[dt], sd=sd)
    return _ORACLES[key]


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine, tp, noise, sampling
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine, tp=tp, noise=noise, S=sampling)
    _MODELS.clear()
    _ORACLES.clear()


@pytest.fixture(autouse=True)
def _no_group_behind_a_failed_rank_run():
    """A rank parked in TpLoop::barrier holds its stream: after a rank run that failed, nothing more touches the GPU."""
    assert P.poisoned() is None, f"skipped without touching the GPU: {P.poisoned()}"
    yield


def _shards(hip, name, world, dt, label="base", sd=None):
    """The `world` shard models of a (probe, world, dtype, plant); the base weights' are kept for the whole file."""
    key = (name, world, dt, label)
    if key in _MODELS:
        return _MODELS[key]
    dtype = P.DTYPES[dt]
    full = P.cast_sd(sd if sd is not None else P.base_state_dict(name), dtype)
    ms = [hip.tp.shard_model(P.probe_config(name), full, r, world, dtype=dtype) for r in range(world)]
    if label == "base":
        _MODELS[key] = ms
    return ms


def _open(hip, shards, max_seq=P.MAX_POS, n=1):
    """A fresh loopback group bound to n new sessions per rank: [rank][i]."""
    groups = hip.tp.TPGroup.loopback(len(shards))
    out = []
    for m, g in zip(shards, groups):
        m.tp_group = g
        out.append([m.new_session(max_seq) for _ in range(n)])
    return out


def _dev(toks):
    return torch.tensor(list(toks), dtype=torch.int32).cuda()


def _sentinel(sessions):
    for ses in sessions:
        ses.kv.view(torch.uint8).fill_(P.KV_SENTINEL)
    torch.cuda.synchronize()


def _sentinel_from(sessions, pos0):
    """Every slot from pos0 on back to the sentinel: rows an earlier call wrote there cannot stand in for this call's."""
    for ses in sessions:
        ses.kv.view(torch.uint8)[:, :, :, pos0:, :] = P.KV_SENTINEL
    torch.cuda.synchronize()


def _same_on_every_rank(got, what):
    for r in range(1, len(got)):
        assert torch.equal(got[0], got[r]), (what, "rank", r, "differs from rank 0")
    return got[0].float().cpu()


def _check_kv(st, ses, before, slots, rank, world, dt, past32, past16, what):
    """Rank `rank`'s arena slots against its KV heads of the unsharded oracle; every other byte as it was."""
    after = ses.kv.clone()
    lo, hi = slots.start, slots.stop
    a8, b8 = after.view(torch.uint8).clone(), before.view(torch.uint8).clone()
    a8[:, :, :, lo:hi, :] = 0
    b8[:, :, :, lo:hi, :] = 0
    assert torch.equal(a8, b8), (st.label, what, rank, "a byte outside the call's slots changed")
    hk = after.shape[2]
    for l in range(after.shape[0]):
        for j in range(2):
            got = after[l, j, :, lo:hi, :].float().cpu()
            truth = past32[l][j][0, rank * hk:(rank + 1) * hk, lo:hi, :].float()
            assert bool(torch.isfinite(got).all()), (st.label, what, rank, l, j)
            if dt == "fp32":
                e = float((got - truth).abs().max())
                assert e <= 1e-4 * max(1.0, float(truth.abs().max())), (st.label, what, rank, l, j, e)
            else:
                ref16 = past16[l][j][0, rank * hk:(rank + 1) * hk, lo:hi, :].float()
                _assert_within_reference_error(P.errors(got, ref16, truth), f"{st.label} {what} rank {rank} layer {l} {'kv'[j]}")


def _prefill_kernel(hip, name, world, rows, s_max):
    cfg = P.probe_config(name)
    k = C.c_int(-1)
    hip.engine.check(hip.lib.sd_prefill_attn_route(cfg.head_dim, cfg.num_attention_heads // world, rows, s_max, 0, 0, C.byref(k)),
                     "sd_prefill_attn_route")
    return k.value


def _expected_prefill(hip, name, world, dt, n, pos0):
    """attn_prefill launches of a call: per pass of more than 80 rows (a contiguous one) of a 16-bit shard whose route is a
    matrix-core kernel, one per layer."""
    tot, pos = 0, pos0
    for m, _, _ in P.call_routes(name, world, dt, n):
        if dt != "fp32" and m > 80 and _prefill_kernel(hip, name, world, m, pos + m) != 0:
            tot += P.probe_config(name).num_hidden_layers
        pos += m
    return tot


def _profiled_forward(ses, toks, nl, pos0):
    ses.profile(True)
    return ses.forward(toks, nl, pos0=pos0).clone()


def _other(ses):
    prof = ses.profile_read()
    ses.profile(False)
    return prof.get("other", (0.0, 0))[1]


def _claim(hip, label, name, world, dt, n, pos0=0, passes=1):
    """(folds + sums, prefill-attention launches) that `passes` single-pass calls of n <= max_rows rows must show, with the
    line the file prints per asserted route."""
    routes = P.call_routes(name, world, dt, n)
    assert len(routes) == 1 and all(r[0] != "none" for r in routes[0][2].values()), (label, routes)
    folds, sums = P.expected_other(name, world, dt, n)
    r = routes[0][2]
    print(f"{label}: {name} world {world} {dt} rows {n}: o {r['o'][0]} [{r['o'][1]} slab(s)], down {r['down'][0]} [{r['down'][1]} slab(s)] -> "
          f"{passes} x ({folds} folds + {sums} sums)")
    return passes * (folds + sums)


# --------------------------------------------------------------------------- a. every reduce route
_A_CASES = [(name, world, dt, label) for name, world, dt in P.CASES for label, _ in P.plant_list(name, world, dt)]


@pytest.mark.parametrize("name,world,dt,label", _A_CASES, ids=[f"{c[0]}-w{c[1]}-{c[2]}-{c[3]}" for c in _A_CASES])
def test_every_reduce_route(hip, name, world, dt, label):
    """Session.forward on every rank at every tp_probe.probe_rows count behind 0 and 150 cached rows (a slab plant: at the row
    count whose route cuts its slab), the base weights and every rank / slab plant: stream S = 1 natural and forced (peers read
    the rank's GEMM output in place), stream S > 1, rows S = 1 / S > 1, mm S > 1 in front of tp_fold_kernel and
    tp_sum_kernel, worlds 2 / 4 / 8.  A call past a 64-row shard's limit is cut into passes; its arena rows must be
    contiguous.  Every call starts from sentinel bytes in every slot it may write, and holds every written K / V row and
    every other arena byte."""
    spec = dict(P.plant_list(name, world, dt))[label]
    sd = P.plant_state_dict(name, world, spec)
    o32 = _oracle(name, "fp32", label, sd, world)
    o16 = None if dt == "fp32" else _oracle(name, dt, label, sd, world)
    st = _Stats(f"tp {name} world {world} {dt} {label}")
    ses = [s[0] for s in _open(hip, _shards(hip, name, world, dt, label, sd))]
    mr = P.shard_max_rows(name, world, dt)
    assert [s.max_rows for s in ses] == [mr] * world, ([s.max_rows for s in ses], mr)
    _sentinel(ses)
    calls = P.plant_calls(name, world, dt, spec)
    for pos0 in (0, P.PREFIX):
        if pos0:
            pre = _dev(P.prefix_tokens(pos0))
            P.run_ranks([lambda s=s: s.forward(pre, 0, pos0=0) for s in ses], LIMIT_S)
        for n in [c[0] for c in calls if c[1] == pos0]:
            toks = P.tokens(n)
            dev, nl = _dev(toks), min(n, P.MAX_LOGIT_ROWS)
            routes = P.call_routes(name, world, dt, n)
            folds, sums = P.expected_other(name, world, dt, n)
            want_pa = _expected_prefill(hip, name, world, dt, n, pos0)
            _sentinel_from(ses, pos0)
            before = [s.kv.clone() for s in ses]
            pa0 = [s.prefill_attn_launches() for s in ses]
            got = P.run_ranks([lambda s=s: _profiled_forward(s, dev, nl, pos0) for s in ses], LIMIT_S)
            other = [_other(s) for s in ses]
            pa = [s.prefill_attn_launches() - a for s, a in zip(ses, pa0)]
            assert other == [folds + sums] * world, (st.label, n, pos0, other, folds, sums)
            assert pa == [want_pa] * world, (st.label, n, pos0, pa, want_pa)
            if spec is not None and spec[0] == "slab":            # the planted slab is a slab of the route that ran
                assert any(r[spec[1]][1:] == (spec[3], spec[4]) for _, _, r in routes), (st.label, routes)
            logits = _same_on_every_rank(got, (st.label, n, pos0))
            truth, past32 = o32.run(toks, pos0)
            ref16, past16 = (None, None) if o16 is None else o16.run(toks, pos0)
            st.judge(logits, truth[-nl:], None if ref16 is None else ref16[-nl:], (n, pos0))
            for r, s in enumerate(ses):
                _check_kv(st, s, before[r], range(pos0, pos0 + n), r, world, dt, past32, past16, (n, pos0))
            if pos0 == 0 and label in ("base", "rank0"):
                print(f"{name} world {world} {dt} rows {n}: " + "; ".join(
                    f"{m} rows o {r['o'][0]} [{r['o'][1]} slab(s)], down {r['down'][0]} [{r['down'][1]} slab(s)]" for m, _, r in routes)
                    + f" -> {folds} folds + {sums} sums, {want_pa} prefill-attention launches")
    st.report()


# --------------------------------------------------------------------------- d. prefill attention on a shard
@pytest.mark.parametrize("world", [2, 8])
def test_prefill_attention_on_a_shards_head_count(hip, world):
    """tp_h4096, bf16: prefill_attn_ok is not gated on the group.  World 2 (16 query heads per rank): a contiguous pass of 145
    rows takes the kernel sd_prefill_attn_route names for 16 heads, one launch per layer on every rank, and the logits and
    K / V rows meet the bars.  World 8 (4 heads per rank): the shard's row limit is 64 and Session.forward marks only passes of
    more than 80 rows contiguous, so a 145-row call (64 + 64 + 17) launches none here; the kernel on 4 heads per rank runs
    through sd_batch_prefill, in the next test."""
    name, dt, n = "tp_h4096", "bf16", 145
    st = _Stats(f"prefill attention {name} world {world}")
    ses = [s[0] for s in _open(hip, _shards(hip, name, world, dt))]
    _sentinel(ses)
    kernel = _prefill_kernel(hip, name, world, n, n)
    want = _expected_prefill(hip, name, world, dt, n, 0)
    if world == 2:
        assert ses[0].max_rows == 256 and kernel in (1, 2) and want == 1, (ses[0].max_rows, kernel, want)
    else:
        assert ses[0].max_rows == 64 and want == 0, (ses[0].max_rows, want)
    toks = P.tokens(n)
    dev = _dev(toks)
    before = [s.kv.clone() for s in ses]
    folds, sums = P.expected_other(name, world, dt, n)
    got = P.run_ranks([lambda s=s: _profiled_forward(s, dev, 64, 0) for s in ses], LIMIT_S)
    assert [_other(s) for s in ses] == [folds + sums] * world, (st.label, folds, sums)
    assert [s.prefill_attn_launches() for s in ses] == [want] * world
    assert [s.prefill_attn_blocked_launches() for s in ses] == [want if kernel == 2 else 0] * world
    truth, past32 = _oracle(name, "fp32").run(toks, 0)
    ref16, past16 = _oracle(name, dt).run(toks, 0)
    st.judge(_same_on_every_rank(got, st.label), truth[-64:], ref16[-64:], n)
    for r, s in enumerate(ses):
        _check_kv(st, s, before[r], range(0, n), r, world, dt, past32, past16, n)
    print(f"{name} world {world} rows {n}: " + "; ".join(
        f"{m} rows o {r['o'][0]} [{r['o'][1]} slab(s)], down {r['down'][0]} [{r['down'][1]} slab(s)]" for m, _, r in P.call_routes(name, world, dt, n))
        + f" -> {folds} folds + {sums} sums; {P.probe_config(name).num_attention_heads // world} heads per rank, "
        f"sd_prefill_attn_route kernel {kernel}, {want} launches per rank")
    st.report()


_BP_ROWS = (64, 40)                # two contiguous passes: 64 rows at cache 0, then 40 rows behind them (both >= 32 rows)


@pytest.mark.parametrize("world", [2, 8])
def test_batch_prefill_runs_prefill_attention_on_a_shards_head_count(hip, world):
    """sd_batch_prefill marks every pass contiguous, whatever its row count: engine.batch_prefill - what the batch and lookup
    loops prefill their target with - of 64 rows and then of 40 rows behind those 64 cached ones, on every rank of tp_h4096
    (world 2: 16 query heads per rank; world 8: 4 heads and ONE KV head per rank, on the 64-row shard).  Each pass of >= 32 rows
    takes the kernel sd_prefill_attn_route names for the shard's head count, one launch per layer; the K / V rows of both
    passes and the logits of a following 5-row pass meet the bars."""
    name, dt = "tp_h4096", "bf16"
    st = _Stats(f"batch prefill {name} world {world}")
    L, heads = P.probe_config(name).num_hidden_layers, P.probe_config(name).num_attention_heads // world
    ses = [s[0] for s in _open(hip, _shards(hip, name, world, dt))]
    assert all(n <= ses[0].max_rows for n in _BP_ROWS)
    _sentinel(ses)
    total = sum(_BP_ROWS)
    tail = P.tokens(5, salt=5)
    seq = _dev(P.prefix_tokens(total))
    tail_dev = _dev(tail)
    truth, past32 = _oracle(name, "fp32").run(tail, total)
    ref16, past16 = _oracle(name, dt).run(tail, total)
    pos = 0
    for n in _BP_ROWS:
        kernel = _prefill_kernel(hip, name, world, n, pos + n)
        assert kernel in (1, 2), (st.label, n, kernel)               # the matrix-core kernel is what this case is about
        want_other = _claim(hip, st.label, name, world, dt, n)
        before = [s.kv.clone() for s in ses]
        pa0 = [(s.prefill_attn_launches(), s.prefill_attn_blocked_launches()) for s in ses]

        def prefill(s):
            assert s.cache_len == pos
            s.profile(True)
            hip.engine.batch_prefill([s], [seq], [n])
        P.run_ranks([lambda s=s: prefill(s) for s in ses], LIMIT_S)
        assert [_other(s) for s in ses] == [want_other] * world, (st.label, n, want_other)
        assert [s.prefill_attn_launches() - a for s, (a, _) in zip(ses, pa0)] == [L] * world, (st.label, n)
        assert [s.prefill_attn_blocked_launches() - b for s, (_, b) in zip(ses, pa0)] == [L if kernel == 2 else 0] * world
        for r, s in enumerate(ses):
            _check_kv(st, s, before[r], range(pos, pos + n), r, world, dt, past32, past16, ("prefill", n))
        print(f"{st.label}: {n} rows behind {pos}: {heads} heads per rank, sd_prefill_attn_route kernel {kernel}, {L} launches per rank")
        pos += n
    want_other = _claim(hip, st.label + " following pass", name, world, dt, 5)
    got = P.run_ranks([lambda s=s: _profiled_forward(s, tail_dev, 5, total) for s in ses], LIMIT_S)
    assert [_other(s) for s in ses] == [want_other] * world
    st.judge(_same_on_every_rank(got, st.label), truth, ref16, "following pass")
    st.report()


# --------------------------------------------------------------------------- e. back-to-back passes
def _eight_passes(ses, devs, sync):
    out = []
    ses.profile(True)                                              # (events on the rank's own stream: no host wait)
    for i, d in enumerate(devs):
        out.append(ses.forward(d, 5, pos0=5 * i).clone())
        if sync:
            torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,world,dt", [("tp_h4096", 2, "bf16"), ("tp_h1024", 2, "bf16")], ids=["in-place-partial", "fold"])
def test_back_to_back_passes_equal_synchronised_ones(hip, name, world, dt):
    """Eight passes of 5 rows with different tokens, enqueued on each rank's stream with no host synchronisation between them,
    against the same eight passes with a device synchronisation after each: bit-identical logits.  tp_h4096 world 2: the
    forced one-slab plan, whose peers read the rank's GEMM output in place - the only thing between that read and the
    rank's next GEMM into the same buffer is the ev_out rendezvous; tp_h1024 world 2: the fold into tp_in.  Run once: a
    determinism check, and the logits are held to the bars as well."""
    routes = P.reduce_routes(name, world, 5)
    assert routes["o"][0] == ("stream S=1 forced" if name == "tp_h4096" else "stream S=1 natural"), routes
    assert (routes["down"][1] > 1) == (name == "tp_h1024"), routes
    st = _Stats(f"back to back {name} world {world}")
    shards = _shards(hip, name, world, dt)
    toks = [P.tokens(5, salt=7 * i + 1) for i in range(8)]
    devs = [_dev(t) for t in toks]
    runs = []
    for sync in (False, True):
        ses = [s[0] for s in _open(hip, shards)]
        want_other = _claim(hip, f"{st.label} sync={sync}", name, world, dt, 5, passes=8)
        got = P.run_ranks([lambda s=s: _eight_passes(s, devs, sync) for s in ses], LIMIT_S)
        assert [_other(s) for s in ses] == [want_other] * world, (st.label, sync, want_other)
        assert [s.prefill_attn_launches() for s in ses] == [0] * world
        runs.append([_same_on_every_rank([g[i] for g in got], (st.label, sync, i)) for i in range(8)])
    for i in range(8):
        assert torch.equal(runs[0][i], runs[1][i]), (st.label, "pass", i, "differs without the synchronisation")
    seq = [t for tk in toks for t in tk]
    truth, ref16 = _oracle(name, "fp32").run(seq, 0)[0], _oracle(name, dt).run(seq, 0)[0]
    st.judge(torch.cat(runs[0]), truth, ref16, "8 x 5 rows")
    st.report()


# --------------------------------------------------------------------------- b. sd_batch_forward under a group
_B_CACHE, _B_NEW = (0, 1, P.PREFIX), (1, 5, 9)


@pytest.mark.parametrize("name,world,dt", [("tp_h1024", 2, "fp32"), ("tp_h4096", 2, "bf16"), ("tp_h4096", 8, "bf16")],
                         ids=["h1024-w2-fp32", "h4096-w2-bf16", "h4096-w8-bf16"])
def test_batch_forward_under_a_group(hip, name, world, dt):
    """Three streams per rank, cache lengths (0, 1, 150), new rows (1, 5, 9): one pass of 15 rows whose reduce buffers are those
    of items[0]'s session.  Each stream's logits against the oracle's own forward of that stream, its K / V rows in its own
    arena, every rank equal - and bit-identical when the items are permuted (another session's buffers carry the reduce)."""
    st = _Stats(f"batch {name} world {world} {dt}")
    shards = _shards(hip, name, world, dt)
    plan = [(c, P.tokens(n, salt=3 * i)) for i, (c, n) in enumerate(zip(_B_CACHE, _B_NEW))]
    seqs = [_dev(P.prefix_tokens(c) + list(t)) for c, t in plan]
    pres = [_dev(P.prefix_tokens(c)) if c else None for c, _ in plan]
    total = sum(_B_NEW)
    folds, sums = P.expected_other(name, world, dt, total)
    per_order = []
    for order in ((0, 1, 2), (2, 0, 1)):
        sess = _open(hip, shards, n=3)
        _sentinel([s for rank in sess for s in rank])

        def prefixes(rank):
            for s, pre in zip(rank, pres):
                if pre is not None:
                    s.forward(pre, 0, pos0=0)
        P.run_ranks([lambda rank=rank: prefixes(rank) for rank in sess], LIMIT_S)
        befores = [[s.kv.clone() for s in rank] for rank in sess]

        def batch(rank):
            rank[order[0]].profile(True)
            n_new = [_B_NEW[i] for i in order]
            return hip.engine.batch_forward([rank[i] for i in order], [seqs[i] for i in order], n_new, n_new).clone()
        got = P.run_ranks([lambda rank=rank: batch(rank) for rank in sess], LIMIT_S)
        assert [_other(rank[order[0]]) for rank in sess] == [folds + sums] * world, (st.label, order, folds, sums)
        rows = _same_on_every_rank(got, (st.label, order))
        split = dict(zip(order, torch.split(rows, [_B_NEW[i] for i in order])))
        per_order.append(split)
        for i, (c, toks) in enumerate(plan):
            truth, past32 = _oracle(name, "fp32").run(toks, c)
            ref16, past16 = (None, None) if dt == "fp32" else _oracle(name, dt).run(toks, c)
            st.judge(split[i], truth, ref16, (order, i))
            for r, rank in enumerate(sess):
                _check_kv(st, rank[i], befores[r][i], range(c, c + len(toks)), r, world, dt, past32, past16, (order, i))
    for i in range(3):
        assert torch.equal(per_order[0][i], per_order[1][i]), (st.label, "stream", i, "changed with the order of the items")
    print(f"{st.label}: {total} rows, {P.reduce_routes(name, world, total) if dt != 'fp32' else 'fp32'} -> {folds} folds + {sums} sums")
    st.report()


# --------------------------------------------------------------------------- c. sd_session_forward_tree under a group
_TREES = sorted({(lay.base, lay.N) for lay in A.tree_layouts(bases=(1, P.PREFIX), sizes=(9, 40))})


@pytest.mark.parametrize("name,world,dt", P.CASES, ids=[f"{c[0]}-w{c[1]}-{c[2]}" for c in P.CASES])
def test_tree_forward_and_compaction_under_a_group(hip, name, world, dt):
    """attn_probe's trees of 9 and 40 nodes behind 1 and 150 cached keys through sd_session_forward_tree on every rank, against
    the oracle's tree forward on the full model; then sd_session_compact_kv of the last node's ancestor path on every rank
    and one more pass of 5 rows on the compacted arenas, against the oracle's causal forward of prefix + path + rows."""
    assert _TREES == [(1, 9), (1, 40), (P.PREFIX, 9), (P.PREFIX, 40)]
    st = _Stats(f"tree {name} world {world} {dt}")
    cfg = P.probe_config(name)
    V = cfg.vocab_size
    o32, o16 = _oracle(name, "fp32"), (None if dt == "fp32" else _oracle(name, dt))
    for base, N in _TREES:
        lay = next(l for l in A.tree_layouts(bases=(base,), sizes=(N,)))
        _, pos, bits = A.tree_inputs(lay)
        toks = P.tokens(N, salt=base)
        path = sorted(A.tree_ancestors(N - 1))
        tail = P.tokens(5, salt=11)
        dev, pre, idx, tail_dev = _dev(toks), _dev(P.prefix_tokens(base)), _dev(path), _dev(tail)
        pos_c, bits_c = (C.c_int32 * N)(*[int(p) for p in pos]), (C.c_uint64 * N)(*bits)
        ses = [s[0] for s in _open(hip, _shards(hip, name, world, dt))]
        _sentinel(ses)
        P.run_ranks([lambda s=s: s.forward(pre, 0, pos0=0) for s in ses], LIMIT_S)
        befores = [s.kv.clone() for s in ses]
        outs = [torch.empty((N, V), dtype=torch.float32, device="cuda") for _ in ses]

        def tree(s, out):
            hip.engine.check(hip.lib.sd_session_forward_tree(s.handle, dev.data_ptr(), pos_c, bits_c, N, base, out.data_ptr(),
                                                             out.stride(0), torch.cuda.current_stream().cuda_stream),
                             "sd_session_forward_tree")
            return out
        want_other = _claim(hip, f"{st.label} tree behind {base}", name, world, dt, N)
        pa0 = [s.prefill_attn_launches() for s in ses]             # (the 150-row prefix may have been a contiguous pass)
        for s in ses:
            s.profile(True)
        got = P.run_ranks([lambda s=s, o=o: tree(s, o) for s, o in zip(ses, outs)], LIMIT_S)
        assert [_other(s) for s in ses] == [want_other] * world, (st.label, base, N, want_other)
        truth, past32 = o32.tree(toks, base, [int(p) for p in pos], bits)
        ref16, past16 = (None, None) if o16 is None else o16.tree(toks, base, [int(p) for p in pos], bits)
        st.judge(_same_on_every_rank(got, (st.label, base, N)), truth, ref16, ("tree", base, N))
        for r, s in enumerate(ses):
            _check_kv(st, s, befores[r], range(base, base + N), r, world, dt, past32, past16, ("tree", base, N))

        def compact_and_go(s):
            hip.engine.check(hip.lib.sd_session_compact_kv(s.handle, base, idx.data_ptr(), len(path),
                                                           torch.cuda.current_stream().cuda_stream), "sd_session_compact_kv")
            s.cache_len = base + len(path)
            return s.forward(tail_dev, 5).clone()
        want_other = _claim(hip, f"{st.label} pass on the compacted arena", name, world, dt, 5)
        for s in ses:
            s.profile(True)
        got = P.run_ranks([lambda s=s: compact_and_go(s) for s in ses], LIMIT_S)
        assert [_other(s) for s in ses] == [want_other] * world, (st.label, base, N, "compacted", want_other)
        assert [s.prefill_attn_launches() for s in ses] == pa0     # (a tree pass, and 5 rows through Session.forward: not contiguous)
        assert [int(pos[i]) for i in path] == list(range(base, base + len(path)))      # the path's depths are consecutive positions
        seq = torch.tensor([P.prefix_tokens(base) + [toks[i] for i in path] + list(tail)])
        truth = o32.lm(seq).logits.float()[0, -5:]
        ref16 = None if o16 is None else o16.lm(seq).logits.float()[0, -5:]
        st.judge(_same_on_every_rank(got, (st.label, base, N, "compacted")), truth, ref16, ("compacted", base, N))
    st.report()


# --------------------------------------------------------------------------- f. the loops
def test_batch_and_queue_loops_with_a_tensor_parallel_target(hip):
    """speculative_sampling_batch (three prompts) and the prompt queue with a 2-rank fp32 tp_h1024 target, a replicated
    draft and the same device-RNG seeds on every rank: token-identical across the ranks and to the unsharded target's
    run, with at least one partial accept.  The loops own their sessions, so no profile is read here: the passes they make
    - sd_batch_prefill and stream-batched verify passes of an fp32 shard, one slab everywhere, no fold - are the routes that
    test_batch_forward_under_a_group and test_batch_prefill_runs_prefill_attention_on_a_shards_head_count assert."""
    from llmspeculativesampling_amd.synth import perturb_state_dict
    name, world = "tp_h1024", 2
    cfg = P.probe_config(name)
    tsd = P.base_state_dict(name)
    dsd = {k: v.to(torch.bfloat16).float() for k, v in perturb_state_dict(tsd, 71, 0.1).items()}
    mk = hip.engine.SpecDecModel.from_state_dict
    full = mk(cfg, tsd, dtype=torch.float32)
    drafts = [mk(cfg, dsd, dtype=torch.float32) for _ in range(world + 1)]
    shards = _shards(hip, name, world, "fp32")
    prompts = [torch.tensor([[P.ordinary(7 * i + j) for j in range(n)]]).cuda() for i, n in enumerate((6, 11, 17))]
    kw = dict(gamma=4, top_k=20, top_p=0.9, details=True, seeds=[31, 32, 33])
    for label, fn, extra in (("batch", hip.S.speculative_sampling_batch, {}), ("queue", hip.S.speculative_sampling_queue, {"slots": 2})):
        want, wd = fn(prompts, drafts[world], full, -1, None, 16, **kw, **extra)
        _open(hip, shards, n=0)                                     # a fresh group on the shard models
        res = P.run_ranks([lambda r=r: fn(prompts, drafts[r], shards[r], -1, None, 16, **kw, **extra) for r in range(world)], 2 * LIMIT_S)
        for outs, ds in res:
            for o, w, d, e in zip(outs, want, ds, wd):
                assert torch.equal(o, w) and d["acc_len"] == e["acc_len"], (label, o, w)
        acc = [a for d in wd for a in d["acc_len"]]
        assert any(0 < a < 4 for a in acc), (label, acc)
        print(f"{label} loop, 2-rank fp32 {name} target: accepted lengths {acc}")
