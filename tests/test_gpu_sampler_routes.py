"""Adversarial rows through every entry and give-up of norm_probs_kernel, against the CPU oracle.

Every case of tests/sampler_rows.py goes through the test hook sd_norm_probs_debug once per entry (workspace = route A, tile
maxima = route B, neither = route C / D; E where no fast entry applies or all give up) and the route word the kernel reports
is asserted, so a change to the launch conditions that quietly sends a case elsewhere fails here.  Expected values are
oracle.sampling_ref's with STABLE_TIES = True (lowest ids first inside a run of equal logits); none
comes from the kernels.  Bars: fp32 rows - identical support, atol 1e-6 + rtol 5e-6 to the oracle and 2.5e-7 to the fp64
softmax over the kept set (the bars of test_norm_probs_many_rows_vs_oracle); 16-bit dtype modes - bit-exact (a case whose
kept set moves when the reference's fp32 softmax denominator moves by one ulp may also match that other set; at most 5 %
of them, checked on the CPU); filter_only - kept set identical, kept values bit-equal to logit / T.  All entries must
agree with each other, and with the production entries sd_norm_probs / sd_norm_sample, bit for bit.

The debug hook launches its own instantiation of norm_probs_kernel (the one that records the route); the production
instantiations are compared with it bit for bit in test_production_entries_equal_the_debug_hook.

Against STABLE_TIES = False (the reference's unstable sort) the result must be equal up to tied logits
(assert_rows_equal_up_to_tied_logits): directly for 16-bit rows; for fp32 rows, where kernel and torch differ in the last
bits of every probability and the helper's exact multiset comparison cannot apply, through the oracle's own pair
(stable vs unstable) on the CPU - tests/test_sampler_rows_cpu.py - plus the bars above against the stable result."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle
import sampler_rows as R
from test_gpu_parity import assert_rows_equal_up_to_tied_logits

pytestmark = pytest.mark.gpu

CL_CAP = 128
CL_INTS = 1 + 2 * CL_CAP


@pytest.fixture(scope="module")
def hip():
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    import types
    return types.SimpleNamespace(lib=_lib.lib, L=_lib, S=S, engine=engine, noise=noise)


def _st():
    return torch.cuda.current_stream().cuda_stream


class Fixed:
    """oracle noise provider that hands out one recorded Exp(1) row"""
    def __init__(self, e):
        self.e = e

    def exponential(self, probs):
        return self.e.view_as(probs)


def launch(hip, x, T, k, p, dt, entry, filter_only=False, sample=None, ws=None):
    """x: (rows, V) fp32 CPU tensor.  Returns dict(out, err, route, n (list sizes), tok, serr)."""
    lib = hip.lib
    rows, V = x.shape
    xd = R.as_dtype(x, dt).float().cuda().contiguous()
    out = torch.zeros((rows, V), device="cuda") if entry == "tile" else torch.full((rows, V), 7.0, device="cuda")
    err = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
    route = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
    lists = torch.zeros((rows + 1, CL_INTS), dtype=torch.int32, device="cuda")     # (one spare list behind the rows')
    assert lib.sd_cand_list_bytes(rows) == rows * CL_INTS * 4
    if ws is None and entry == "ws":
        ws = torch.zeros(lib.sd_norm_workspace_bytes(rows), dtype=torch.uint8, device="cuda")
    tm = torch.cat([R.tile_maxima(xd[i:i + 1].cpu()) for i in range(rows)], 0).cuda() if entry == "tile" and V % 16 == 0 else None
    tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    serr = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    noise = seed = draw = None
    if sample is not None:
        noise, seed, draw = sample
    hip.L.check(lib.sd_norm_probs_debug(
        xd.data_ptr(), rows, V, V, float(T), int(k), float(p), R.DT_MODE[dt], out.data_ptr(), V, err.data_ptr(),
        ws.data_ptr() if entry == "ws" else None, None if filter_only else lists.data_ptr(), _st(),
        tm.data_ptr() if tm is not None else None, int(filter_only), int(sample is not None),
        noise.data_ptr() if noise is not None else None, seed or 0, draw or 0, tok.data_ptr() if sample is not None else None,
        serr.data_ptr() if sample is not None else None, route.data_ptr()), "sd_norm_probs_debug")
    torch.cuda.synchronize()
    lists = lists.cpu()
    assert not bool(lists[rows].any()), "a candidate list was written past its 128 entries"
    return dict(out=out.cpu(), err=err.cpu().tolist(), route=[r & 0xffffffff for r in route.cpu().tolist()],
                lists=lists, tok=int(tok), serr=int(serr))


def check_route(c, entry, word):
    must, mustnot = c["want"][entry]
    assert word & must == must and not word & mustnot, \
        f"{c['id']} [{entry}]: route {R.route_str(word)}; wanted {R.route_str(must)} and none of {R.route_str(mustnot)}"


def check_probs(c, got, x, filter_only=False):
    """one output row against the oracle under the bars of the module docstring"""
    T, k, p, dt = c["T"], c["k"], c["p"], c["dt"]
    exp = R.expected(x, T, k, p, dt, filter_only)
    assert exp is not None, c["id"]
    want, want_unstable = exp
    z = R.scaled(x, T, dt)[0]
    if filter_only:
        assert torch.equal(torch.isfinite(got), torch.isfinite(want[0])), c["id"]
        assert torch.equal(got, want[0]), c["id"]                      # kept values bit-equal to logit / T, -inf elsewhere
        return
    if dt:
        if not torch.equal(got, want[0]):
            alts = R.lowprec_alternative(x, T, k, p, dt)
            assert alts is not None and any(torch.equal(got, a[0]) for a in alts), \
                (c["id"], int((got != want[0]).sum()), "not denominator-sensitive" if alts is None else "matches neither set")
            return
        assert_rows_equal_up_to_tied_logits(got.numpy(), want_unstable[0].numpy(), z.numpy())
        return
    # identical support - except where the exact probability lies below 2^-148, two steps of the denormal grid: there expf's
    # documented 1 ulp (= 2^-149) decides between 0 and the smallest denormal, and torch's exp and the device's may differ
    z64 = torch.where(want[0] > 0, z.double(), torch.full_like(z, R.NEG, dtype=torch.float64))
    exact = torch.softmax(z64, 0)
    sure = (exact >= 2.0 ** -148) | (want[0] == 0)
    assert torch.equal((got > 0)[sure], (want[0] > 0)[sure]), (c["id"], int(((got > 0) != (want[0] > 0)).sum()))
    assert float(got[~sure].max() if (~sure).any() else 0.0) <= 2.0 ** -148, c["id"]
    np.testing.assert_allclose(got.numpy(), want[0].numpy(), atol=1e-6, rtol=5e-6, err_msg=c["id"])
    d = float((got.double() - exact).abs().max())
    assert d <= 2.5e-7, (c["id"], d)
    # against the reference's unstable sort: equal up to tied logits, in the tolerance form fp32 admits - the kept sets hold
    # the same multiset of logits (every token that differs has a twin with the same logit)
    tiny = ~sure                                                      # (entries below 2^-148 count as kept on both sides)
    zn, gk, uk = z.numpy(), ((got > 0) | tiny).numpy(), ((want_unstable[0] > 0) | tiny).numpy()
    np.testing.assert_array_equal(np.sort(zn[gk]), np.sort(zn[uk]), err_msg=c["id"])


def check_list(c, res, row=0):
    """the CandList of a row: written iff the kept set was decided on a list and holds <= 128 entries; equal to the row"""
    out, word = res["out"][row], res["route"][row]
    n = int(res["lists"][row, 0])
    nz = torch.nonzero(out > 0)[:, 0]
    if word & R.LIST:
        kept = word >> 16
        assert n == kept and n <= CL_CAP, (c["id"], n, kept)
        ids = res["lists"][row, 1:1 + n].long()
        pr = res["lists"][row, 1 + CL_CAP:1 + CL_CAP + n].view(torch.float32)
        assert torch.equal(out[ids], pr), c["id"]
        assert set(nz.tolist()) <= set(ids.tolist()) and len(set(ids.tolist())) == n, c["id"]
    else:
        assert n == -1, (c["id"], n)
        if word & (R.P_LIST | R.A | R.B | R.PRE) and not word & (R.BISECT | R.P_MASS) and not word & R.ERROR:
            assert (word >> 16) > CL_CAP, (c["id"], R.route_str(word))  # a list prefix decided it: only its size keeps the list out


@pytest.mark.parametrize("c", R.CASES, ids=[c["id"] for c in R.CASES])
def test_row_through_every_entry(hip, c):
    """One row through every entry its case lists: route word, oracle bars, candidate list, and bit equality of the entries.

    Found by this test and fixed in norm_probs_kernel: `bf16_valued_k64` (V = 32000, k = 64, p = 0).  Through the tile maxima
    the kept set stayed a sorted list whose softmax denominator is summed serially in rank order; through the workspace
    and without one, k = 64 overflows the candidate caps and the row ended in the general path, which without top-p summed
    the denominator through 1024 strided partials: 1 of 32000 probabilities differed by one ulp (2.98e-8).  The general
    path now finishes on a list whenever <= 1024 finite entries survive top-k, with or without top-p."""
    x = c["make"]()
    assert x.shape == (1, c["V"])
    results = {}
    for entry in c["want"]:
        res = launch(hip, x, c["T"], c["k"], c["p"], c["dt"], entry)
        print(c["id"], entry, R.route_str(res["route"][0]))
        results[entry] = res
    for entry, res in results.items():
        check_route(c, entry, res["route"][0])
        if c.get("error"):
            assert R.expected(x, c["T"], c["k"], c["p"], c["dt"]) is None      # the reference raises
            assert res["err"] == [1] and bool(torch.isnan(res["out"]).all()) and int(res["lists"][0, 0]) == -1, (c["id"], entry)
        else:
            assert res["err"] == [0], (c["id"], entry)
            check_probs(c, res["out"][0], x)
            check_list(c, res)
    first = next(iter(results.values()))
    for entry, res in results.items():                                        # A = B = C / D = E, bit for bit
        ga, gb = torch.nan_to_num(res["out"], nan=-5.0), torch.nan_to_num(first["out"], nan=-5.0)
        assert torch.equal(ga, gb), (c["id"], entry, "entries differ in", int((ga != gb).sum()), "elements, max abs",
                                     float((ga - gb).abs().max()), "max rel", float(((ga - gb).abs() / gb.clamp_min(1e-30)).max()))


@pytest.mark.parametrize("cid", R.FILTER_ONLY_IDS)
def test_filter_only(hip, cid):
    c = R.BY_ID[cid]
    x = c["make"]()
    res = launch(hip, x, c["T"], c["k"], c["p"], c["dt"], "plain", filter_only=True)   # (the filter takes no workspace / tiles)
    check_route(c, "plain", res["route"][0] & ~R.LIST)
    check_probs(c, res["out"][0], x, filter_only=True)
    # and the production entry
    xd = R.as_dtype(x, c["dt"]).float().cuda()
    out = torch.empty_like(xd)
    z = R.scaled(x, c["T"], c["dt"]).cuda()          # divided on the CPU: torch's GPU division by a scalar multiplies by 1 / T
    hip.L.check(hip.lib.sd_topk_topp_filter(z.data_ptr(), 1, c["V"], c["V"], c["k"], c["p"], R.DT_MODE[c["dt"]], out.data_ptr(),
                                            c["V"], _st()))
    assert torch.equal(out.cpu(), res["out"]), cid


@pytest.mark.parametrize("cid", R.SAMPLE_IDS)
def test_fused_sample(hip, cid):
    """token identical under supplied Exp(1) noise and under device Philox (variates read back through sd_philox_exp)"""
    c = R.BY_ID[cid]
    x = c["make"]()
    V = c["V"]
    want = R.expected(x, c["T"], c["k"], c["p"], c["dt"])[0]
    wd = want.to(R.DTYPES[c["dt"]])
    g = torch.Generator().manual_seed(V + len(cid))
    e_host = torch.empty(V).exponential_(generator=g)
    e_dev = torch.empty(V, device="cuda")
    seed, draw = 0x1234ABCD5678, 41 + len(cid)
    hip.L.check(hip.lib.sd_philox_exp(seed, draw, V, e_dev.data_ptr(), _st()))
    for entry in c["want"]:
        # 16-bit rows: the reference draws its variates in the row dtype (empty_like(probs).exponential_()), so the supplied
        # noise holds values of that dtype; device Philox variates are fp32 and have no 16-bit counterpart in the reference,
        # so that half runs on fp32 rows only
        e_sup = e_host.to(wd.dtype)
        runs = [(e_sup, (e_sup.float().cuda(), 0, 0))] + ([(e_dev.cpu(), (None, seed, draw))] if c["dt"] == 0 else [])
        for noise, sample in runs:
            res = launch(hip, x, c["T"], c["k"], c["p"], c["dt"], entry, sample=sample)
            check_route(c, entry, res["route"][0])
            tok = int(oracle.sample(wd, noise=Fixed(noise)))
            if c["dt"] and not torch.equal(res["out"][0], want[0]):
                check_probs(c, res["out"][0], x)                  # only a denominator-sensitive row may pass here
                continue
            assert res["serr"] == 0 and res["tok"] == tok, (cid, entry, res["tok"], tok)
            check_probs(c, res["out"][0], x)


def test_production_entries_equal_the_debug_hook(hip):
    """sd_norm_probs (with / without workspace) and sd_norm_sample launch the instantiations without the route word: same
    bits as the hook's, for a row of every family"""
    lib = hip.lib
    for cid in R.SAMPLE_IDS + ["error_nan_chunk15", "plateau_max_n1500_chunk_dt0", "masked_tail_dt2"]:
        c = R.BY_ID[cid]
        x = c["make"]()
        V = c["V"]
        xd = R.as_dtype(x, c["dt"]).float().cuda()
        for entry in ("plain", "ws"):
            if entry not in c["want"]:
                continue
            ref = launch(hip, x, c["T"], c["k"], c["p"], c["dt"], entry)
            out = torch.full((1, V), 3.0, device="cuda")
            err = torch.zeros(1, dtype=torch.int32, device="cuda")
            ws = torch.zeros(lib.sd_norm_workspace_bytes(1), dtype=torch.uint8, device="cuda")
            hip.L.check(lib.sd_norm_probs(xd.data_ptr(), 1, V, V, c["T"], c["k"], c["p"], R.DT_MODE[c["dt"]], out.data_ptr(), V,
                                          err.data_ptr(), ws.data_ptr() if entry == "ws" else None, _st()))
            assert torch.equal(torch.nan_to_num(out.cpu(), nan=-5.0), torch.nan_to_num(ref["out"], nan=-5.0)), (cid, entry)
            assert err.cpu().tolist() == ref["err"]
            if c.get("error"):
                continue
            tok = torch.zeros(1, dtype=torch.int32, device="cuda")
            serr = torch.zeros(1, dtype=torch.int32, device="cuda")
            refs = launch(hip, x, c["T"], c["k"], c["p"], c["dt"], entry, sample=(None, 99, 7))
            hip.L.check(lib.sd_norm_sample(xd.data_ptr(), V, c["T"], c["k"], c["p"], R.DT_MODE[c["dt"]], out.data_ptr(), err.data_ptr(),
                                           None, 99, 7, tok.data_ptr(), serr.data_ptr(), ws.data_ptr() if entry == "ws" else None, _st()))
            assert int(tok) == refs["tok"] and torch.equal(out.cpu(), refs["out"]), (cid, entry)


def _mixed_rows(V, n):
    fams = [lambda s: R.bf16_valued(s, V), lambda s: R.gauss(s, V), lambda s: R.plateau_max(s, V, 129), lambda s: R.masked(s, V, "tail"),
            lambda s: R.plateau_max(s, V, 1100), lambda s: R.plateau_kth(s, V, 64, 20), lambda s: R.masked(s, V, "filtered")]
    return torch.cat([fams[i % len(fams)](900 + i) for i in range(n)], 0)


@pytest.mark.parametrize("rows,entry", [(5, "ws"), (9, "ws"), (5, "tile"), (9, "plain")])
def test_several_rows_per_launch(hip, rows, entry):
    """rows of different families in one launch: each row takes its own route and equals its single-row launch"""
    V = 32000
    x = _mixed_rows(V, rows)
    T, k, p = R.HARNESS
    res = launch(hip, x, T, k, p, 0, entry)
    c = dict(id=f"rows{rows}_{entry}", T=T, k=k, p=p, dt=0)
    seen = set()
    for i in range(rows):
        one = launch(hip, x[i:i + 1], T, k, p, 0, entry)
        assert one["route"][0] == res["route"][i] and torch.equal(one["out"][0], res["out"][i]), (rows, entry, i)
        check_probs(c, res["out"][i], x[i:i + 1])
        check_list(c, res, i)
        seen.add(res["route"][i] & 0xffff)
    assert len(seen) >= 2                                                     # rows of one launch take different routes


@pytest.mark.parametrize("n_rows", [47, 48, 49, 97])
def test_norm_batch_chunking_and_misaligned_destinations(hip, n_rows):
    """sd_norm_batch cuts its rows into launches of 48; per-row destinations, row 5's 4 bytes off 16-byte alignment (its whole
    launch then runs without the workspace), with the fused sample under device Philox"""
    lib = hip.lib
    V = 8192
    T, k, p = R.HARNESS
    x = _mixed_rows(V, n_rows)
    xd = x.cuda().contiguous()
    arena = torch.full((n_rows, V + 8), 5.0, device="cuda")
    toks = torch.full((n_rows,), -1, dtype=torch.int32, device="cuda")
    errs = torch.full((n_rows, 2), -1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.sd_norm_workspace_bytes(n_rows), dtype=torch.uint8, device="cuda")
    tab = (hip.L.SdNormRow * n_rows)()
    for i in range(n_rows):
        off = 1 if i == 5 else (4 if i % 2 else 0)
        tab[i].probs_out = arena[i].data_ptr() + 4 * off
        tab[i].err = errs[i, 0:].data_ptr()
        tab[i].sample_err = errs[i, 1:].data_ptr()
        tab[i].exp_noise = None
        tab[i].philox_seed, tab[i].draw_index = 77, 1000 + i
        tab[i].tok_out = toks[i:].data_ptr()
    hip.L.check(lib.sd_norm_batch(xd.data_ptr(), n_rows, V, V, T, k, p, 0, tab, 1, ws.data_ptr(), _st()))
    torch.cuda.synchronize()
    a = arena.cpu()
    c = dict(id=f"batch{n_rows}", T=T, k=k, p=p, dt=0)
    e = torch.empty(V, device="cuda")
    for i in range(n_rows):
        off = 1 if i == 5 else (4 if i % 2 else 0)
        got = a[i, off:off + V]
        assert bool((a[i, :off] == 5.0).all()) and bool((a[i, off + V:] == 5.0).all()), i     # nothing written outside the row
        check_probs(c, got, x[i:i + 1])
        assert errs[i].tolist() == [0, 0], i
        hip.L.check(lib.sd_philox_exp(77, 1000 + i, V, e.data_ptr(), _st()))
        want = R.expected(x[i:i + 1], T, k, p, 0)[0]
        assert int(toks[i]) == int(oracle.sample(want, noise=Fixed(e.cpu()))), i


@pytest.mark.parametrize("V", [8192, 32000, 50272])
def test_misaligned_input_view_and_odd_row_stride(hip, V):
    """rows that start 4 bytes off 16-byte alignment with a stride that is not a multiple of 4: the scalar-load forms; a
    workspace is offered and must be declined"""
    lib = hip.lib
    T, k, p = R.HARNESS
    x = _mixed_rows(V, 3)
    ld = V + 1
    buf = torch.zeros(1 + 3 * ld + 8, device="cuda")
    view = buf[1:1 + 3 * ld].view(3, ld)[:, :V]
    view.copy_(x.cuda())
    out = torch.full((3, V), 7.0, device="cuda")
    err = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    route = torch.zeros(3, dtype=torch.int32, device="cuda")
    ws = torch.zeros(lib.sd_norm_workspace_bytes(3), dtype=torch.uint8, device="cuda")
    hip.L.check(lib.sd_norm_probs_debug(view.data_ptr(), 3, V, ld, T, k, p, 0, out.data_ptr(), V, err.data_ptr(), ws.data_ptr(), None,
                                        _st(), None, 0, 0, None, 0, 0, None, None, route.data_ptr()))
    c = dict(id=f"misaligned_V{V}", T=T, k=k, p=p, dt=0)
    for i in range(3):
        w = int(route[i])
        assert w & R.PRE and not w & (R.A | R.B), R.route_str(w)
        check_probs(c, out[i].cpu(), x[i:i + 1])
    assert err.tolist() == [0, 0, 0]


def test_workspace_is_clean_after_an_error_row(hip):
    """an error row, then a clean row through the SAME workspace and list buffers: the second launch is correct"""
    lib = hip.lib
    V = 32000
    ws = torch.zeros(lib.sd_norm_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    T, k, p = R.HARNESS
    for what, where in (("nan", "chunk15"), ("inf", "chunk0"), ("allneg", None)):
        bad = launch(hip, R.error_row(610, V, what, where), T, k, p, 0, "ws", ws=ws)
        assert bad["err"] == [1] and bad["route"][0] & R.ERROR and int(bad["lists"][0, 0]) == -1
        bads = launch(hip, R.error_row(610, V, what, where), T, k, p, 0, "ws", ws=ws, sample=(None, 5, 6))
        assert bads["err"] == [1] and bads["serr"] == 1 and bool(torch.isnan(bads["out"]).all())
        x = R.bf16_valued(611, V)
        good = launch(hip, x, T, k, p, 0, "ws", ws=ws)
        c = dict(id="after_" + what, T=T, k=k, p=p, dt=0)
        assert good["err"] == [0] and good["route"][0] & R.A and not good["route"][0] & R.ERROR
        check_probs(c, good["out"][0], x)
        check_list(c, good)


# --------------------------------------------------------------------------- candidate lists into the accept kernels
ACCEPT_KINDS = {
    # kind: (target-row maker(seed), (T, k, p)); V = 32000
    "support127": (lambda s: R.plateau_kth(s, 32000, 108, 20), (1.0, 20, 0.0)),      # 19 + 108 kept: a list
    "support128": (lambda s: R.plateau_kth(s, 32000, 109, 20), (1.0, 20, 0.0)),      # the largest list
    "support129": (lambda s: R.plateau_kth(s, 32000, 110, 20), (1.0, 20, 0.0)),      # n = -1: the dense passes
    "one_slot": (lambda s: R.same_slot(s, 32000), (1.0, 20, 0.9)),                   # every entry in one slot modulo 1024
    "zero_denormal": (lambda s: R.wide_range(s, 32000, clip=False), (1.0, 20, 0.0)),             # list entries of probability 0 / denormal
    "bf16_valued": (lambda s: R.bf16_valued(s, 32000), R.HARNESS),
}


def oracle_accept(P, Q, seq, L, gamma, uni, exp_row):
    """The accept block of oracle/specdec_ref.py (its lines 54-81: scan, residual sample with the max_fn(p) fallback, bonus
    sample) on given probability rows, drafted tokens and variates.  Returns (accepted, next token, fallback taken)."""
    n, accepted = L + gamma - 1, 0
    for i in range(gamma):
        j = int(seq[L + i])
        ratio = P[L + i - 1, j].item() / Q[L + i - 1, j].item()
        if bool(uni[i:i + 1] > ratio):
            n = L + i - 1
            break
        accepted += 1
    fallback = False
    noise = Fixed(exp_row)
    if n < L + gamma - 1:
        try:
            t = oracle.sample(oracle.max_fn(P[n:n + 1] - Q[n:n + 1]), noise)
        except RuntimeError:
            fallback = True
            t = oracle.sample(oracle.max_fn(P[n:n + 1]), noise)
    else:
        t = oracle.sample(P[n:n + 1], noise)
    return accepted, int(t), fallback


@pytest.mark.parametrize("mode", ["philox", "reject_equal_rows", "all_accept"])
@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", list(ACCEPT_KINDS))
def test_lists_into_accept_resample_vs_oracle(hip, kind, dt, mode):
    """sd_norm_probs_lists -> sd_accept_resample, and the same rows through sd_accept_resample_batch for 1 and 6 streams,
    against the oracle's accept block fed the device's own variates (sd_philox_uniform / sd_philox_exp), gamma in
    {1, 4, 8, 16}: accepted count, next token and flags identical.  The oracle reads the probability rows the device
    produced (they are held to the oracle by the tests above), so that this test judges the accept kernels alone.
    `reject_equal_rows`: q == p and r = 1.5 - the residual is zero on the whole list and sample(max_fn(p)) is taken;
    `all_accept`: r = 0 - the bonus sample from the last row."""
    lib = hip.lib
    V, L = 32000, 3
    make, (T, k, p) = ACCEPT_KINDS[kind]
    dtype = R.DTYPES[dt]
    res_sz = C.sizeof(hip.L.SdAcceptResult)
    for gamma in (1, 4, 8, 16):
        rows, S = gamma + 1, L + gamma + 1
        x = torch.cat([make(3000 + 17 * gamma + i) for i in range(rows)], 0)
        xd = R.as_dtype(x, dt).float().cuda().contiguous()
        p_hist = torch.zeros((S, V), device="cuda")
        lists = torch.zeros((rows, CL_INTS), dtype=torch.int32, device="cuda")
        ws = torch.zeros(lib.sd_norm_workspace_bytes(rows), dtype=torch.uint8, device="cuda")
        err = torch.zeros(rows, dtype=torch.int32, device="cuda")
        hip.L.check(lib.sd_norm_probs_lists(xd.data_ptr(), rows, V, V, T, k, p, R.DT_MODE[dt], p_hist[L - 1].data_ptr(), V,
                                            err.data_ptr(), ws.data_ptr(), lists.data_ptr(), _st()))
        assert err.tolist() == [0] * rows
        n_list = lists[:, 0].cpu().tolist()
        support = (p_hist[L - 1:L + gamma] > 0).sum(1).cpu().tolist()
        if kind in ("support127", "support128"):
            assert support == [int(kind[-3:])] * rows and n_list == support, (n_list, support)
        elif kind == "support129":
            assert support == [129] * rows and n_list == [-1] * rows, (n_list, support)
        else:
            assert all(0 < n <= CL_CAP for n in n_list), n_list
        if kind == "zero_denormal" and dt == 0:
            pr = lists[:, 1 + CL_CAP:].view(torch.float32).cpu()
            assert all(bool((pr[i, :n_list[i]] < 1e-38).any()) for i in range(rows))
        P = p_hist.cpu().to(dtype)
        if mode == "reject_equal_rows":
            Q = P.clone()
        else:                                                      # draft rows: the target's logits, perturbed, a wider top-k
            g = torch.Generator().manual_seed(gamma)
            xq = R.as_dtype(x + 0.5 * torch.randn(x.shape, generator=g), dt)
            with R.stable_ties(True):
                Q = torch.zeros((S, V), dtype=dtype)
                Q[L - 1:L + gamma] = oracle.norm_logits(xq, 1.0, 50, 0.0)
        q_hist = Q.float().cuda().contiguous()
        streams = []
        for s in range(6):                                         # same rows, own drafted tokens and Philox streams
            g = torch.Generator().manual_seed(100 * gamma + s)
            seq = torch.zeros(S + 8, dtype=torch.int32)
            seq[:L] = torch.randint(3, V, (L,), generator=g)
            for i in range(gamma):
                seq[L + i] = int(torch.multinomial(Q[L + i - 1].float(), 1, generator=g))
            seed, d_scan, d_res = 5000 + 13 * s + gamma, 7 + s, 40 + s
            if mode == "philox":
                u = torch.empty(gamma, device="cuda")
                hip.L.check(lib.sd_philox_uniform(seed, d_scan, gamma, u.data_ptr(), _st()))
                uni, r_dev = u.cpu(), None
            else:
                uni = torch.full((gamma,), 1.5 if mode == "reject_equal_rows" else 0.0)
                r_dev = uni.cuda()
            e = torch.empty(V, device="cuda")
            hip.L.check(lib.sd_philox_exp(seed, d_res, V, e.data_ptr(), _st()))
            want = oracle_accept(P, Q, seq, L, gamma, uni, e.cpu())
            if mode == "reject_equal_rows":
                assert want[0] == 0 and want[2]
            if mode == "all_accept":
                assert want[0] == gamma
            streams.append(dict(seq=seq, seed=seed, d_scan=d_scan, d_res=d_res, r=r_dev, want=want))

        def check(res_bytes, seq_dev, st, what):
            a = hip.L.SdAcceptResult.from_buffer_copy(res_bytes)
            acc, tok, fb = st["want"]
            assert (a.n_accepted, a.next_token, a.flags & 7) == (acc, tok, (1 if fb else 0) | (4 if acc == gamma else 0)), \
                (kind, dt, mode, gamma, what, a.n_accepted, a.next_token, a.flags, st["want"])
            assert a.n == L + acc - 1 and int(seq_dev[a.n + 1]) == tok

        st = streams[0]
        seq = st["seq"].cuda()
        res = torch.zeros(res_sz, dtype=torch.uint8, device="cuda")
        hip.L.check(lib.sd_accept_resample(p_hist.data_ptr(), q_hist.data_ptr(), V, V, seq.data_ptr(), L, gamma,
                                           st["r"].data_ptr() if st["r"] is not None else None, st["seed"], st["d_scan"],
                                           st["d_res"], res.data_ptr(), None, 0, R.DT_MODE[dt], lists.data_ptr(), _st()))
        check(res.cpu().numpy().tobytes(), seq.cpu(), st, "single")
        for n_streams in (1, 6):
            items = (hip.L.SdAcceptItem * n_streams)()
            lptr = (C.c_void_p * n_streams)()
            keep = []
            for s in range(n_streams):
                st = streams[s]
                ph, qh, sq, ls = p_hist.clone(), q_hist.clone(), st["seq"].cuda(), lists.clone()
                rs = torch.zeros(res_sz, dtype=torch.uint8, device="cuda")
                keep.append((ph, qh, sq, ls, rs))
                items[s].p_hist, items[s].q_hist, items[s].seq, items[s].L = ph.data_ptr(), qh.data_ptr(), sq.data_ptr(), L
                items[s].r = st["r"].data_ptr() if st["r"] is not None else None
                items[s].exp_noise = None
                items[s].philox_seed, items[s].draw_scan, items[s].draw_resample = st["seed"], st["d_scan"], st["d_res"]
                items[s].res, items[s].err_flags, items[s].n_err = rs.data_ptr(), None, 0
                lptr[s] = ls.data_ptr()
            hip.L.check(lib.sd_accept_resample_batch(items, n_streams, V, V, gamma, R.DT_MODE[dt], lptr, _st()))
            torch.cuda.synchronize()
            for s in range(n_streams):
                check(keep[s][4].cpu().numpy().tobytes(), keep[s][2].cpu(), streams[s], f"batch{n_streams}[{s}]")


# --------------------------------------------------------------------------- exact ties through a real head
def _plateau_head(sd, V, src):
    """lm_head (and OPT's tied embedding) with 150 copies of row `src` at scattered ids and its last 7 rows identical"""
    rng = np.random.default_rng(V + 5)
    ids = torch.from_numpy(rng.choice(V - 7, size=150, replace=False))
    sd = dict(sd)
    W = sd["lm_head.weight"].clone()
    W[ids] = W[src].clone()
    W[V - 7:] = W[V - 7].clone()
    sd["lm_head.weight"] = W
    if "model.decoder.embed_tokens.weight" in sd:
        sd["model.decoder.embed_tokens.weight"] = W
    return sd, set(ids.tolist()) | {src}


@pytest.mark.parametrize("kp", [(20, 0.9), (20, 0.0)], ids=["k20_p0.9", "k20_p0"])
@pytest.mark.parametrize("arch", ["llama", "opt"])
def test_exact_ties_through_a_real_head(hip, arch, kp, capsys, monkeypatch):
    """bf16 pairs whose lm_head holds 150 copies of one row and 7 identical last rows, so that exact ties reach the sampler
    through the head's own tile maxima.  The duplicated row is that of the first token the unmodified pair generates, so
    the plateau is sampled from (asserted).  Single stream: the native loop is bit-equal to the Python-orchestrated loop;
    6 streams: the fused tail is bit-equal to SD_BATCH_FUSED_TAIL=0; and the p_hist rows of the first verify equal the
    oracle's norm_logits (stable ties) of the logits the same forward returned, under the bars of this file."""
    from test_gpu_native_parity import BF16_CFG, OPT_BF16_CFG
    from llmspeculativesampling_amd.config import ModelConfig
    from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict
    import llmspeculativesampling_amd.sampling.kvcache_model as KM
    cfg = ModelConfig(**(OPT_BF16_CFG if arch == "opt" else BF16_CFG))
    V, gamma = cfg.vocab_size, 4
    k, p = kp
    kw = dict(gamma=gamma, top_k=k, top_p=p)
    dsd0 = make_state_dict(cfg, 5, dtype=torch.bfloat16)
    prompt = torch.from_numpy(np.random.default_rng(3).integers(3, V, size=(1, 24))).cuda()
    dm0 = hip.engine.SpecDecModel.from_state_dict(cfg, dsd0, dtype=torch.bfloat16)
    first = hip.S.speculative_sampling(prompt, dm0, dm0, -1, None, 4, rng=hip.noise.DeviceNoise(123), **kw)
    src = int(first[0, 24])
    del dm0
    dsd, plateau = _plateau_head(dsd0, V, src)
    tsd = {n: v.to(torch.bfloat16) for n, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    tsd, _ = _plateau_head(tsd, V, src)                              # (the perturbation must not break the ties)
    dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.bfloat16)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.bfloat16)

    # ---- single stream: native loop == Python-orchestrated loop; the latter's first verify is captured
    cap = {}
    orig = KM.KVCacheModel.forward_rows

    def spy(self, seq32, upto, n_rows_out):
        if self._model is tm and "logits" not in cap:
            ses, fwd = self._session, self._session.forward

            def fwd_spy(*a, **k2):
                out = fwd(*a, **k2)
                cap["logits"] = out[:n_rows_out].float().clone()
                return out
            ses.forward = fwd_spy
            try:
                orig(self, seq32, upto, n_rows_out)
            finally:
                del ses.forward
            cap["probs"] = self._probs[upto - n_rows_out:upto].clone()
            return
        orig(self, seq32, upto, n_rows_out)

    a, da = hip.S.speculative_sampling(prompt, dm, tm, -1, None, 40, details=True, rng=hip.noise.DeviceNoise(123), **kw)
    monkeypatch.setattr(KM.KVCacheModel, "forward_rows", spy)
    b, db = hip.S.speculative_sampling(prompt, dm, tm, -1, None, 40, details=True, rng=hip.noise.DeviceNoise(123), verbose=True, **kw)
    monkeypatch.setattr(KM.KVCacheModel, "forward_rows", orig)
    capsys.readouterr()
    assert torch.equal(a, b)
    assert da["acc_len"] == db["acc_len"] and float(da["acc_rate"]) == float(db["acc_rate"])
    assert plateau & set(a[0, 24:].tolist()), "no plateau token was generated: the case tests nothing"
    assert cap["logits"].shape == (gamma + 1, V)
    dt = 1 if tm.norm_mode & 0x30 else 0
    c = dict(id=f"head_{arch}", T=1.0, k=k, p=p, dt=dt)
    n_tied = 0
    for i in range(gamma + 1):
        x = cap["logits"][i:i + 1].cpu().to(torch.bfloat16).float()  # the logits as the bf16 head leaves them
        check_probs(c, cap["probs"][i].cpu(), x)
        n_tied += int((x[0, sorted(plateau)] == x[0, src]).all()) and int((x[0, V - 7:] == x[0, V - 1]).all())
    assert n_tied == gamma + 1                                       # the ties are exact in every verify row

    # ---- 6 streams: fused tail == dense tail
    rng = np.random.default_rng(17)
    prompts = [torch.from_numpy(rng.integers(3, V, size=(1, 5 + 7 * (i % 5)))).cuda() for i in range(6)]
    prompts[0] = prompt
    seeds = [4100 + i for i in range(6)]
    runs = {}
    try:
        for mode in ("0", "1"):
            os.environ["SD_BATCH_FUSED_TAIL"] = mode
            runs[mode] = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 24, details=True, seeds=seeds, **kw)
    finally:
        os.environ.pop("SD_BATCH_FUSED_TAIL", None)
    (o0, d0), (o1, d1) = runs["0"], runs["1"]
    hit = 0
    for x0, x1, e0, e1, pr in zip(o0, o1, d0, d1, prompts):
        assert torch.equal(x0, x1), (x0, x1)
        assert e0["acc_len"] == e1["acc_len"] and float(e0["acc_rate"]) == float(e1["acc_rate"])
        hit += bool(plateau & set(x1[0, pr.shape[1]:].tolist()))
    assert hit >= 1
