"""Token scoring on the device (`pytest -m gpu`): sd_score_rows against the numpy truth of adversarial rows (tests/score_rows.py)
and bit for bit against sd_token_logprobs; sd_score_sequence / quality.score_tokens against the float64 log-softmax, the order
and the ranks of the CPU oracle's own logits over the sequence."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import oracle
import score_rows as SR
from test_gpu_logprobs import FP32_BAR, _bf16_pair
from llmspeculativesampling_amd.config import load_config
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF     # a NaN bit pattern no computation produces
SENT_I = -77777           # no id, no rank


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def hip():
    import types
    from llmspeculativesampling_amd import _lib, engine, quality
    return types.SimpleNamespace(lib=_lib.lib, L=_lib, engine=engine, quality=quality)


# ----------------------------------------------------------------------------- K: the kernel
class Out:
    """The four outputs of one launch over n rows, prefilled with sentinels."""

    def __init__(self, n, top_n):
        self.n, self.top_n = n, top_n
        self.lp = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.rank = torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")
        self.ids = torch.full((n, max(top_n, 1)), SENT_I, dtype=torch.int32, device="cuda")
        self.tlp = torch.full((n, max(top_n, 1)), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)

    def untouched(self):
        return (bool((self.lp.view(torch.int32) == SENTINEL).all()) and bool((self.rank == SENT_I).all())
                and bool((self.ids == SENT_I).all()) and bool((self.tlp.view(torch.int32) == SENTINEL).all()))

    def all_written(self):
        top = self.top_n > 0
        return (not bool((self.lp.view(torch.int32) == SENTINEL).any()) and not bool((self.rank == SENT_I).any())
                and not (top and bool((self.ids == SENT_I).any())) and not (top and bool((self.tlp.view(torch.int32) == SENTINEL).any())))

    def host(self):
        return self.lp.cpu(), self.rank.cpu(), self.ids.cpu(), self.tlp.cpu()


def _launch(hip, logits, ld, V, mode, top_n, groups, toks, rank=True, tops=True, expect=0):
    """One sd_score_rows call: item i = rows groups[i] = (first row of `logits` viewed as rows of stride ld, row count), scored
    at toks (one per row, in launch order); -> Out."""
    n = sum(r for _, r in groups)
    tok = torch.tensor(toks, dtype=torch.int32, device="cuda")
    out = Out(n, top_n)
    items = (hip.L.SdScoreItem * len(groups))()
    o = 0
    for it, (r0, rows) in zip(items, groups):
        it.logits, it.ld, it.rows = logits.data_ptr() + 4 * r0 * ld, ld, rows
        it.tokens, it.logprob = tok.data_ptr() + 4 * o, out.lp.data_ptr() + 4 * o
        it.rank = out.rank.data_ptr() + 4 * o if rank else None
        it.top_ids = out.ids.data_ptr() + 4 * o * top_n if tops else None
        it.top_logprobs = out.tlp.data_ptr() + 4 * o * top_n if tops else None
        o += rows
    assert hip.lib.sd_score_rows(items, len(groups), V, top_n, mode, _st()) == expect, hip.lib.sd_last_error()
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _cases(V, dt, top_n):
    """80 (kind, row, Truth, token): every kind of score_rows.pool at its first tokens - the two at the cut come first."""
    per_kind = [(kind, x, tr, SR.tokens(kind, x, tr, top_n)) for kind, x, tr in SR.pool(V, dt)]
    out = [(kind, x, tr, toks[j]) for j in range(12) for kind, x, tr, toks in per_kind if j < len(toks)]
    assert len(out) >= 40
    return (out + out)[:80]                                       # (a sorted row has few distinct tokens: cases may repeat)


def _check_row(what, tr, t, top_n, lp, rank, ids, tlp):
    assert rank == tr.rank[t], (what, "rank", rank, tr.rank[t])
    assert SR.within_bar(lp, float(tr.logp[t])), (what, "logprob", lp, float(tr.logp[t]))
    want_ids, want_lp = tr.top(top_n)
    assert ids == want_ids, (what, "top_ids", ids, want_ids)
    for j, (g, w) in enumerate(zip(tlp, want_lp)):
        assert (math.isnan(g) and math.isnan(w)) or SR.within_bar(g, w), (what, "top_logprobs", j, g, w)


@pytest.mark.parametrize("top_n", [1, 5, 20])
@pytest.mark.parametrize("pad", [0, 3], ids=["ld_V", "ld_V_plus_3"])
@pytest.mark.parametrize("V", [257, 8192, 50272])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["fp32", "bf16_round", "f16_round"])
def test_k1_kernel_against_the_truth(hip, dt, V, pad, top_n):
    """1 item x 80 rows, 16 items x 5 rows and 1 item x 1 row over a slab of row stride V or V + 3 (every row after the first
    starts off a 16-byte boundary): every output entry is overwritten, top_ids and rank equal the truth exactly, logprob and
    top_logprobs lie within 2^-17 * max(1, |want|) of the float64 log-softmax of the rounded row, -inf exactly."""
    cases = _cases(V, dt, top_n)
    ld, n = V + pad, 80
    slab = torch.zeros(n * ld + 4, dtype=torch.float32)
    for r in range(n):
        slab[r * ld:r * ld + V] = cases[r][1]
    dev = slab.cuda()
    for groups in ([(0, 80)], [(5 * i, 5) for i in range(16)], [(7, 1)]):
        rows = [r for r0, k in groups for r in range(r0, r0 + k)]
        out = _launch(hip, dev, ld, V, dt, top_n, groups, [cases[r][3] for r in rows])
        assert out.all_written()
        lp, rank, ids, tlp = out.host()
        for i, r in enumerate(rows):
            kind, _, tr, t = cases[r]
            _check_row((kind, t, dt, V, ld, top_n, len(groups)), tr, t, top_n, float(lp[i]), int(rank[i]), ids[i].tolist(), tlp[i].tolist())


@pytest.mark.parametrize("V", [257, 8192])
def test_k2_bits_of_the_existing_kernel(hip, V):
    """On one slab (row stride V + 3), in all three modes: logprob is sd_token_logprobs' float bit for bit, and where the token
    is in the row's top list the two floats of the new kernel are bit-equal."""
    top_n, ld = 20, V + 3
    listed = 0
    for dt in (0, 1, 2):
        cases = _cases(V, dt, top_n)
        slab = torch.zeros(80 * ld + 4, dtype=torch.float32)
        for r in range(80):
            slab[r * ld:r * ld + V] = cases[r][1]
        dev = slab.cuda()
        toks = [c[3] for c in cases]
        out = _launch(hip, dev, ld, V, dt, top_n, [(0, 80)], toks)
        tok = torch.tensor(toks, dtype=torch.int32, device="cuda")
        old = torch.full((80,), SENTINEL, dtype=torch.int32, device="cuda")
        items = (hip.L.SdLogprobItem * 5)()
        for i, it in enumerate(items):
            it.logits, it.ld, it.rows = dev.data_ptr() + 4 * 16 * i * ld, ld, 16
            it.tokens, it.res, it.out = tok.data_ptr() + 4 * 16 * i, None, old.data_ptr() + 4 * 16 * i
        assert hip.lib.sd_token_logprobs(items, 5, V, dt, _st()) == 0, hip.lib.sd_last_error()
        torch.cuda.synchronize()
        assert torch.equal(out.lp.view(torch.int32), old), dt
        lp, _, ids, tlp = (x.view(torch.int32) if x.dtype == torch.float32 else x for x in out.host())
        for r in range(80):
            for j in range(top_n):
                if int(ids[r, j]) == toks[r]:
                    listed += 1
                    assert int(tlp[r, j]) == int(lp[r]), (dt, r, j)
    assert listed >= 3 * 12                                       # (every kind's first case is scored at the cut)


def test_k3_edges(hip):
    """The edges of sd_score_rows: V below top_n, V = 1, void rows, tokens out of range, NULL outputs, refused calls."""
    # V = 7 with top_n = 20: the tail entries are -1 / NaN; V = 1
    x7 = SR.row("gauss", 9, 7)
    tr = SR.Truth(x7, 0)
    out = _launch(hip, x7.cuda(), 7, 7, 0, 20, [(0, 1)], [3])
    assert out.all_written()
    lp, rank, ids, tlp = out.host()
    _check_row("V 7", tr, 3, 20, float(lp[0]), int(rank[0]), ids[0].tolist(), tlp[0].tolist())
    assert ids[0, 7:].tolist() == [-1] * 13 and bool(torch.isnan(tlp[0, 7:]).all())
    out = _launch(hip, torch.tensor([0.3]).cuda(), 1, 1, 0, 5, [(0, 1)], [0])
    lp, rank, ids, tlp = out.host()
    assert float(lp[0]) == 0.0 and int(rank[0]) == 1 and ids[0].tolist() == [0, -1, -1, -1, -1] and float(tlp[0, 0]) == 0.0
    assert bool(torch.isnan(tlp[0, 1:]).all())
    # void rows between live ones; a token at -1 and at V (the column past the row holds a finite value: it must not be read)
    V, ld, top_n = 257, 260, 5
    rows = [SR.row("gauss", 5, V)] + [SR.void_row(k, 3, V) for k in SR.VOID_KINDS] + [SR.row("gauss", 6, V)] * 3
    slab = torch.full((len(rows), ld), 1000.0)
    for r, x in enumerate(rows):
        slab[r, :V] = x
    toks = [3, 4, 5, 6, -1, V, 8]
    dev = slab.cuda()
    out = _launch(hip, dev, ld, V, 0, top_n, [(0, 7)], toks)
    assert out.all_written()
    lp, rank, ids, tlp = out.host()
    for r in (1, 2, 3):
        assert math.isnan(float(lp[r])) and int(rank[r]) == 0 and ids[r].tolist() == [-1] * top_n and bool(torch.isnan(tlp[r]).all()), r
    t0, t6 = SR.Truth(rows[0], 0), SR.Truth(rows[4], 0)
    _check_row("live 0", t0, 3, top_n, float(lp[0]), int(rank[0]), ids[0].tolist(), tlp[0].tolist())
    _check_row("live 6", t6, 8, top_n, float(lp[6]), int(rank[6]), ids[6].tolist(), tlp[6].tolist())
    for r in (4, 5):
        assert math.isnan(float(lp[r])) and int(rank[r]) == 0, r
        assert ids[r].tolist() == t6.top(top_n)[0] and torch.equal(tlp[r], tlp[6]), r
    # rank = NULL; top_n = 0 with NULL top arrays: the other outputs are the same bits
    a = _launch(hip, dev, ld, V, 0, top_n, [(0, 7)], toks, rank=False)
    assert bool((a.rank == SENT_I).all()) and torch.equal(a.ids, out.ids)
    assert torch.equal(a.lp.view(torch.int32), out.lp.view(torch.int32)) and torch.equal(a.tlp.view(torch.int32), out.tlp.view(torch.int32))
    b = _launch(hip, dev, ld, V, 0, 0, [(0, 7)], toks, tops=False)
    assert torch.equal(b.lp.view(torch.int32), out.lp.view(torch.int32)) and torch.equal(b.rank, out.rank)
    assert bool((b.ids == SENT_I).all()) and bool((b.tlp.view(torch.int32) == SENTINEL).all())
    c = _launch(hip, dev, ld, V, 0, 0, [(0, 7)], toks, rank=False, tops=False)
    assert torch.equal(c.lp.view(torch.int32), out.lp.view(torch.int32)) and bool((c.rank == SENT_I).all())
    # after a refused call the sentinels stand
    for kw in (dict(top_n=21), dict(top_n=top_n, tops=False), dict(top_n=top_n, mode=3), dict(top_n=top_n, groups=[(0, 81)]),
               dict(top_n=top_n, V=ld + 1)):
        kw = dict(dict(V=V, mode=0, groups=[(0, 7)]), **kw)
        n = sum(k for _, k in kw["groups"])
        r = _launch(hip, dev, ld, kw["V"], kw["mode"], kw["top_n"], kw["groups"], [0] * n, tops=kw.get("tops", True),
                    expect=hip.L.SD_ERR_INVALID)
        assert r.untouched(), kw


@pytest.mark.parametrize("V,lanes,top_n", [(8192, 19, 20), (50272, 19, 20), (172035, 19, 20), (50272, 3, 5)])
def test_k4_crowded_stripes(hip, V, lanes, top_n):
    """Rows whose largest entries crowd the stripes of `lanes` < top_n lanes: the first threshold keeps lanes * V / 256 ids -
    several thinning rounds (608 and 3 700 ids), and past the list's 12288 ids (V = 172035: 12 768) the exact cut by bisection."""
    x = SR.stripes(3, V, lanes)
    assert int((x >= 10.0).sum()) >= lanes * (V // 1024) * 4
    # which path a row takes follows from the kernel's lane mapping (16-byte group g of an aligned row -> lane g % 256) and its
    # list of 12288 ids (SCORE_CAND, csrc/score_kernels.h): a change of either has to move these shapes with it
    assert (int((x >= 10.0).sum()) > 12288) == (V == 172035) and int((x >= 10.0).sum()) > 64
    tr = SR.Truth(x, 0)
    toks = tr.cut_tokens(top_n) + [0, V - 1]
    dev = x.cuda()
    assert dev.data_ptr() % 16 == 0
    for t in toks:
        out = _launch(hip, dev, V, V, 0, top_n, [(0, 1)], [t])
        lp, rank, ids, tlp = out.host()
        _check_row((V, lanes, t), tr, t, top_n, float(lp[0]), int(rank[0]), ids[0].tolist(), tlp[0].tolist())


# ----------------------------------------------------------------------------- E: sequences
LOGIT_BAR = FP32_BAR      # a pair of fp32 logits moves by at most 2 x the 1e-3 logit bar against each other


@functools.lru_cache(maxsize=None)
def _model(name):
    """(config, state dict, oracle model, its float64 logits over SEQ(name))"""
    if name == "llama":
        cfg = load_config("tiny-llama-target")
        sd = perturb_state_dict(make_state_dict(cfg, 21), 22, 0.12)
    else:
        cfg = load_config("tiny-opt-post")
        sd = make_state_dict(cfg, 22)
    return cfg, sd, oracle.RefCausalLM(cfg, sd)


@functools.lru_cache(maxsize=None)
def _seq(name, seed=900, n=200):
    cfg, _, om = _model(name)
    ids = torch.from_numpy(np.random.default_rng(seed).integers(3, cfg.vocab_size, size=(1, n)))
    with torch.no_grad():
        return ids, om(ids, use_cache=False).logits[0].double()


@functools.lru_cache(maxsize=None)
def _engine(name):
    from llmspeculativesampling_amd import engine
    cfg, sd, _ = _model(name)
    return engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)


def _shares(x, toks, top_n):
    """From the oracle alone: per row whether the top_n cut is separated by more than the bar, and the rank window."""
    srt = x.sort(dim=-1, descending=True).values
    cut = (srt[:, top_n - 1] - srt[:, top_n]) > LOGIT_BAR
    xt = x.gather(-1, toks[:, None])
    lo = 1 + (x > xt + LOGIT_BAR).sum(-1)
    hi = (x >= xt - LOGIT_BAR).sum(-1)                            # 1 + #{v != t : x_v >= x_t - bar}: t itself is the 1
    return srt, cut, lo, hi


def _check_sequence(what, x, ids, first, n, top_n, lp, rank, top_ids, top_lp, bar=LOGIT_BAR, exact=True):
    """Scores of tokens first .. n - 1 of ids against the oracle logits x (row p predicts token p + 1)."""
    rows = x[first - 1:n - 1]
    toks = ids[0, first:n]
    k = n - first
    assert tuple(lp.shape) == tuple(rank.shape) == (k,) and tuple(top_ids.shape) == tuple(top_lp.shape) == (k, top_n), what
    lsm = torch.log_softmax(rows, dim=-1)
    err = float((lp.double() - lsm.gather(-1, toks[:, None])[:, 0]).abs().max())
    print(f"{what}: {k} tokens, worst |logprob - truth| {err:.3g} (bar {bar:.3g})")
    assert err <= bar, (what, err)
    srt, cut, lo, hi = _shares(rows, toks, top_n)
    if exact:
        assert float(cut.double().mean()) >= 0.9 and float((lo == hi).double().mean()) >= 0.75, what
    r64 = rank.to(torch.int64)
    assert bool(((lo <= r64) & (r64 <= hi)).all()), (what, "rank outside its window")
    listed = torch.zeros_like(rows, dtype=torch.bool).scatter_(-1, top_ids.to(torch.int64), True)
    assert bool((listed.sum(-1) == top_n).all()), (what, "an id is listed twice")
    must = rows > (srt[:, top_n, None] + bar)
    assert bool((listed | ~must).all()), (what, "an id above the cut by more than the bar is missing")
    assert bool((rows.gather(-1, top_ids.to(torch.int64)) >= srt[:, top_n - 1, None] - bar).all()), (what, "a listed id lies below the cut")
    assert float((top_lp.double() - lsm.gather(-1, top_ids.to(torch.int64))).abs().max()) <= bar, what
    assert bool((top_lp[:, :-1] >= top_lp[:, 1:]).all()), (what, "the list is not descending")
    hit = top_ids.to(torch.int64) == toks[:, None]                # the token's own float, where it is listed
    assert torch.equal(top_lp.view(torch.int32)[hit], lp.view(torch.int32)[:, None].expand(-1, top_n)[hit]), what
    assert bool((hit.any(-1) == (r64 <= top_n)).all()), (what, "rank and list disagree")


@pytest.mark.parametrize("top_n", [5, 20])
@pytest.mark.parametrize("input_len", [1, 40])
@pytest.mark.parametrize("name", ["llama", "opt"])
def test_e1_score_tokens_against_the_oracle(hip, name, input_len, top_n):
    """200 ids through the fp32 tiny models: logprobs within 2e-3 of the float64 log-softmax of the oracle's logits; ids and ranks
    held by margin (two logits move by at most 2e-3 against each other), after the oracle alone has shown that at least 0.9 of
    the rows have a separated cut and 0.75 a rank window of width 0 - there the checks are exact."""
    ids, x = _seq(name)
    s = hip.quality.score_tokens(ids.cuda(), _engine(name), input_len, top_n)
    assert isinstance(s, hip.quality.TokenScores) and all(t.is_cuda for t in s)
    assert s.logprobs.dtype == s.top_logprobs.dtype == torch.float32 and s.ranks.dtype == s.top_ids.dtype == torch.int32
    assert tuple(s.logprobs.shape) == tuple(s.ranks.shape) == (1, 200 - input_len)
    _check_sequence(f"{name} input_len {input_len} top_n {top_n}", x, ids, input_len, 200, top_n, s.logprobs[0].cpu(), s.ranks[0].cpu(),
                    s.top_ids.cpu(), s.top_logprobs.cpu())
    srt, cut, lo, hi = _shares(x[input_len - 1:-1], ids[0, input_len:], top_n)
    same = s.top_ids.cpu().to(torch.int64).sort(-1).values == x[input_len - 1:-1].topk(top_n, dim=-1).indices.sort(-1).values
    assert bool(same.all(-1)[cut].all())                          # separated cut: the id set is the oracle's
    assert bool((s.ranks[0].cpu().to(torch.int64) == lo)[lo == hi].all())
    zero = hip.quality.score_tokens(ids.cuda(), _engine(name), input_len, 0)
    assert torch.equal(zero.logprobs, s.logprobs) and torch.equal(zero.ranks, s.ranks) and tuple(zero.top_ids.shape) == (200 - input_len, 0)


def _score_sequence(hip, ses, ids, n, first, top_n, slab_rows, ld_slab=None, expect=0):
    V = ses.model.cfg.vocab_size
    ld = ld_slab or V + 3
    dev_ids = ids[0, :n].to(device="cuda", dtype=torch.int32).contiguous()
    slab = torch.empty(max(slab_rows, 1) * ld + 4, dtype=torch.float32, device="cuda")
    out = Out(n - first, top_n)
    so = hip.L.SdScoreOut(out.lp.data_ptr(), out.rank.data_ptr(), out.ids.data_ptr(), out.tlp.data_ptr())
    rc = hip.lib.sd_score_sequence(ses.handle, dev_ids.data_ptr(), n, first, top_n, slab.data_ptr(), ld, slab_rows, C.byref(so), _st())
    torch.cuda.synchronize()
    assert rc == expect, hip.lib.sd_last_error()
    return out


@pytest.mark.parametrize("name", ["llama", "opt"])
def test_e2_pass_edges(hip, name):
    """sd_score_sequence through ctypes on a session of 16 rows per pass: slab_rows 1 / 3 / 64, a prompt of several passes
    (first - 1 = 40 > 16), no prompt at all (first = 1), a last pass of one row - every variant within E1's bars; then another
    sequence on the same session gets its own results (the cache is rewritten from position 0)."""
    ids, x = _seq(name)
    m = _engine(name)
    ses = m.new_session(200, max_rows=16)
    assert ses.max_rows == 16 and ses.max_pass_rows == 16
    top_n = 5
    for slab_rows, first, n in ((1, 41, 60), (3, 1, 17), (3, 41, 60), (64, 41, 106), (64, 1, 200)):
        assert slab_rows == 1 or n == 200 or (n - first) % min(slab_rows, 16) == 1      # (the last pass holds one row)
        out = _score_sequence(hip, ses, ids, n, first, top_n, slab_rows)
        assert out.all_written()
        lp, rank, tid, tlp = out.host()
        _check_sequence(f"{name} slab_rows {slab_rows} first {first} n {n}", x, ids, first, n, top_n, lp, rank, tid, tlp, exact=n == 200)
    big = m.new_session(200)                                      # ... and passes of 64 rows with a last pass of one
    assert big.max_pass_rows >= 64
    out = _score_sequence(hip, big, ids, 41 + 65, 41, top_n, 64)
    _check_sequence(f"{name} 64-row passes", x, ids, 41, 106, top_n, *out.host(), exact=False)
    ids2, x2 = _seq(name, seed=901, n=90)
    out = _score_sequence(hip, ses, ids2, 90, 30, top_n, 64)
    _check_sequence(f"{name} second sequence", x2, ids2, 30, 90, top_n, *out.host(), exact=False)
    # the refusals that read the session: nothing is launched
    V = m.cfg.vocab_size
    small = m.new_session(50, max_rows=16)
    for kw in (dict(n=60, ld_slab=V - 1), dict(n=52), dict(n=60, first=60)):
        r = _score_sequence(hip, small, ids, kw["n"], kw.get("first", 5), top_n, 4, ld_slab=kw.get("ld_slab"), expect=hip.L.SD_ERR_INVALID)
        assert r.untouched(), kw
    tps = (C.c_void_p * 2)()                                      # a session bound to a tensor-parallel group of two (never run)
    assert hip.lib.sd_tp_create_loopback(2, tps) == 0 and hip.lib.sd_session_set_tp(small.handle, tps[0]) == 0
    try:
        assert _score_sequence(hip, small, ids, 40, 5, top_n, 4, expect=hip.L.SD_ERR_INVALID).untouched()
        assert "tensor-parallel" in hip.lib.sd_last_error().decode()
    finally:
        assert hip.lib.sd_session_set_tp(small.handle, None) == 0
        for t in tps:
            hip.lib.sd_tp_destroy(t)
    assert _score_sequence(hip, small, ids, 51, 5, top_n, 4).all_written()   # (n - 1 == max_seq fits)


def test_e3_agreement_with_get_score(hip):
    """get_score_native against quality.get_score on an E1 output: each within 2e-3 of the oracle's mean; and a bf16 model
    within test L5's bar, 2 x 0.04 x the largest |logit| of the fp32 truth."""
    ids, x = _seq("llama")
    want = float(torch.log_softmax(x[:-1], dim=-1).gather(-1, ids[0, 1:, None])[39:].mean())
    a = float(hip.quality.get_score_native(ids.cuda(), _engine("llama"), 40))
    b = float(hip.quality.get_score(ids.cuda(), _engine("llama"), 40))
    print("native", a, "get_score", b, "oracle", want)
    assert abs(a - want) <= FP32_BAR and abs(b - want) <= FP32_BAR
    cfg, _, tm, ot = _bf16_pair()
    ids = torch.from_numpy(np.random.default_rng(902).integers(3, cfg.vocab_size, size=(1, 120)))
    with torch.no_grad():
        logits = ot(ids, use_cache=False).logits[0].double()
    bar = 2 * 0.04 * float(logits.abs().max())
    s = hip.quality.score_tokens(ids.cuda(), tm, 20, 5)
    truth = torch.log_softmax(logits[19:-1], dim=-1)
    err = float((s.logprobs[0].cpu().double() - truth.gather(-1, ids[0, 20:, None])[:, 0]).abs().max())
    print(f"bf16: worst |logprob - truth| {err:.3g} (bar {bar:.3g})")
    assert err <= bar
    assert float((s.top_logprobs.cpu().double() - truth.gather(-1, s.top_ids.cpu().to(torch.int64))).abs().max()) <= bar
    assert abs(float(hip.quality.get_score_native(ids.cuda(), tm, 20)) - float(hip.quality.get_score(ids.cuda(), tm, 20))) <= bar
