"""Per-request repetition / frequency / presence penalties (`pytest -m gpu`): sd_penalize_rows bit for bit against
sampling.utils.apply_penalties on the CPU, and the four native loops against the CPU oracle run on models whose logits carry
the same penalties (tests/penalised_model.py), each prompt under its own Philox variates."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import oracle
from penalised_model import PenalisedModel
from philox_replay import PhiloxOracleNoise
from test_gpu_logprobs import _bf16_pair, _check, _corr_oracles
from test_gpu_native_parity import _st
from test_gpu_spec_queue import _models, _prompts
from llmspeculativesampling_amd.sampling.utils import apply_penalties

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF     # a NaN bit pattern no computation produces
ROUND_BF16, DT_BF16, DT_F16 = 1, 16, 32
MODES = {"fp32": 0, "round_bf16": ROUND_BF16, "dt_bf16": DT_BF16, "dt_f16": DT_F16, "round_bf16_dt_bf16": ROUND_BF16 | DT_BF16}
# every (theta, f, pi) of {1, 0.5, 1.8} x {0, 1.5, -0.7}^2: 27 triples over the 32 items of two launches
TRIPLES = list(itertools.product((1.0, 0.5, 1.8), (0.0, 1.5, -0.7), (0.0, 1.5, -0.7)))
ROWS, ITEMS = 17, 16


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


# ----------------------------------------------------------------------------- K: the kernel
def _histories(V, rng):
    """(tokens, hist0, prompt_len) per item, 32 of them; row r of an item sees tokens[:hist0 + r], so every history has 16
    entries behind hist0, each of which is new to the row that first sees it."""
    fresh = lambda n: rng.choice(V, size=n, replace=False)
    tail = lambda: fresh(ROWS - 1)
    kinds = [
        lambda: (np.concatenate([fresh(40), tail()]), 40, 40 + ROWS),                            # prompt only: f / pi do nothing
        lambda: (np.concatenate([fresh(5), np.full(300, 7 % V), tail()]), 305, 3),               # one token 300 times
        lambda: (fresh(min(V, 600)), min(V, 600) - ROWS + 1, 100),                                # all distinct
        lambda: (np.concatenate([[0, V - 1, 0, V - 1, V - 1], tail()]), 5, 2),                   # the two ends of the row
        lambda: (np.concatenate([[-1, V, V + 5, 2 ** 30, -2 ** 31, 3], fresh(20), tail()]), 26, 1),   # ids outside [0, V)
        lambda: (np.concatenate([rng.integers(0, V, size=20000), tail()]), 20000, 9000),         # past any table or window limit
        lambda: (np.concatenate([rng.integers(0, min(V, 50), size=200), tail()]), 200, 0),       # no prompt at all, many repeats
        lambda: (np.concatenate([rng.integers(0, V, size=1), tail()]), 1, 1),                    # hist0 = 1
    ]
    return [kinds[i % len(kinds)]() for i in range(2 * ITEMS)]


def _logits(V, n, rng, hist):
    """n rows of N(0, 8^2) with 0, -0, +-inf and a NaN planted at ids in the first item's history and at ids outside it."""
    x = torch.from_numpy(rng.standard_normal((n, V)).astype(np.float32)) * 8
    special = [0.0, -0.0, float("inf"), float("-inf"), float("nan")]
    cols = [int(t) for t in hist if 0 <= t < V][:5] + [int(c) for c in rng.choice(V, size=5, replace=False)]
    for r in range(n):
        for j, c in enumerate(cols):
            x[r, (c + 3 * r) % V] = special[j % 5]
    return x


def _as_read(x, mode):
    """The row as the sampler reads it (pending rounding applied), in the dtype apply_penalties is to work in."""
    if mode & 3:
        x = x.to(torch.bfloat16).float()
    dt = {DT_BF16: torch.bfloat16, DT_F16: torch.float16}.get(mode & 48)
    return x.to(dt) if dt else x


def _same_bits(got, want):
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan])


@functools.lru_cache(maxsize=None)
def _kernel_case(V):
    rng = np.random.default_rng(V)
    hists = _histories(V, rng)
    n = 2 * ITEMS * ROWS
    x = _logits(V, n, rng, hists[0][0])
    return hists, x


@pytest.mark.parametrize("V", [512, 8192, 32000, 50272])
@pytest.mark.parametrize("mode", list(MODES))
def test_k1_kernel_bit_for_bit_against_apply_penalties(hip, mode, V):
    """Two launches of 16 items x 17 rows over slabs of row stride V + 3 whose first row starts 4 bytes past a 16-byte boundary:
    in the first the output rows share the input rows' misalignment (the 16-byte body), in the second they do not (scalar
    throughout).  Every row equals apply_penalties of the row as the sampler reads it under the history seq[:hist0 + r]; the
    input slab and the output slab's padding columns keep their bytes; a second run gives the same bytes."""
    m = MODES[mode]
    hists, x = _kernel_case(V)
    if m & 48 and not m & 3:                                      # rows that live in a 16-bit type hold values of that type
        x = _as_read(x, m).float()
    ld, n = V + 3, 2 * ITEMS * ROWS
    assert any(len(set(h[:h0].tolist())) > 8192 for h, h0, _ in hists) or V < 50272
    slab = torch.zeros(n * ld + 8, dtype=torch.float32)
    slab[1:1 + n * ld].view(n, ld)[:, :V] = x
    dev_in = slab.cuda()
    keep = dev_in.clone()
    seqs = [torch.tensor(h, dtype=torch.int64).to(torch.int32).cuda() for h, _, _ in hists]
    for launch, out_off in ((0, 1), (1, 2)):
        out = torch.full((ITEMS * ROWS * ld + 8,), SENTINEL, dtype=torch.int32, device="cuda")
        items = (hip.L.SdPenaltyItem * ITEMS)()
        for i, it in enumerate(items):
            k = launch * ITEMS + i
            _, hist0, P = hists[k]
            setattr(it, "in", dev_in.data_ptr() + 4 * (1 + k * ROWS * ld))
            it.out, it.ld_in, it.ld_out, it.rows = out.data_ptr() + 4 * (out_off + i * ROWS * ld), ld, ld, ROWS
            it.seq, it.hist0, it.prompt_len, it.pen = seqs[k].data_ptr(), hist0, P, hip.L.SdPenalty(*TRIPLES[k % len(TRIPLES)])
        runs = []
        for _ in range(2):
            assert hip.lib.sd_penalize_rows(items, ITEMS, V, m, _st()) == 0, hip.lib.sd_last_error()
            torch.cuda.synchronize()
            runs.append(out.cpu())
        assert torch.equal(runs[0], runs[1])
        assert torch.equal(dev_in.view(torch.int32), keep.view(torch.int32))
        got = runs[0][out_off:out_off + ITEMS * ROWS * ld].view(ITEMS * ROWS, ld)
        assert got[:-1, V:].eq(SENTINEL).all() and runs[0][:out_off].eq(SENTINEL).all()
        for i in range(ITEMS):
            k = launch * ITEMS + i
            h, hist0, P = hists[k]
            pen = TRIPLES[k % len(TRIPLES)]
            for r in range(ROWS):
                row = _as_read(x[k * ROWS + r], m)
                want = apply_penalties(row, h[:hist0 + r], P, *pen).float()
                g = got[i * ROWS + r, :V].view(torch.float32)
                assert _same_bits(g, want), (mode, V, "item", k, "row", r, pen)
                if pen == (1.0, 0.0, 0.0):
                    assert _same_bits(g, row.float())             # a neutral item: rounded and copied
                if P >= hist0 + r and pen[0] == 1.0:
                    assert _same_bits(g, row.float())             # a prompt-only history: f and pi do nothing


def test_k2_one_item_one_row_and_the_refusals(hip):
    V, ld = 700, 701
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((3, ld)).astype(np.float32)).cuda()
    seq = torch.tensor([5, 6, 5, 699, 0, 5], dtype=torch.int32, device="cuda")
    out = torch.full((3, ld), SENTINEL, dtype=torch.int32, device="cuda")
    items = (hip.L.SdPenaltyItem * 2)()
    for i, it in enumerate(items):
        setattr(it, "in", x[i].data_ptr())
        it.out, it.ld_in, it.ld_out, it.rows = out[i].data_ptr(), ld, ld, 1
        it.seq, it.hist0, it.prompt_len, it.pen = seq.data_ptr(), 5 + i, 2, hip.L.SdPenalty(1.8, 1.5, -0.7)
    assert hip.lib.sd_penalize_rows(items, 2, V, 0, _st()) == 0, hip.lib.sd_last_error()
    torch.cuda.synchronize()
    for i in range(2):
        want = apply_penalties(x[i, :V].cpu(), seq[:5 + i].cpu(), 2, 1.8, 1.5, -0.7)
        assert _same_bits(out[i, :V].cpu().view(torch.float32), want)
    assert out[2].eq(SENTINEL).all() and out[:2, V:].eq(SENTINEL).all()
    out.fill_(SENTINEL)
    bad = [dict(rows=0), dict(rows=18), dict(ld_in=V - 1), dict(ld_out=V - 1), dict(hist0=0), dict(prompt_len=-1), dict(seq=None),
           dict(out=None), dict(pen=hip.L.SdPenalty(0.0, 0, 0)), dict(pen=hip.L.SdPenalty(1.0, float("nan"), 0)),
           dict(pen=hip.L.SdPenalty(1.0, 0, float("inf")))]
    for over in bad:
        saved = {k: getattr(items[1], k) for k in over}
        if "pen" in saved:                                        # (a copy: the attribute is a view of the item)
            saved["pen"] = hip.L.SdPenalty(saved["pen"].repetition, saved["pen"].frequency, saved["pen"].presence)
        for k, v in over.items():
            setattr(items[1], k, v)
        assert hip.lib.sd_penalize_rows(items, 2, V, 0, _st()) == hip.L.SD_ERR_INVALID, over
        assert b"item 1" in hip.lib.sd_last_error(), (over, hip.lib.sd_last_error())
        for k, v in saved.items():
            setattr(items[1], k, v)
    for args in ((None, 1, V, 0), (items, 0, V, 0), (items, 17, V, 0), (items, 2, 0, 0), (items, 2, 65537, 0), (items, 2, V, 3)):
        assert hip.lib.sd_penalize_rows(*args, _st()) == hip.L.SD_ERR_INVALID, args
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all()                                 # nothing was launched


# ----------------------------------------------------------------------------- L: the loops
LENS, BUDGETS = [7, 9, 20, 12, 8], [16, 12, 20, 14, 16]
SEEDS = [6100 + i for i in range(5)]
PARAMS = [(1.0, 20, 0.9), (0.7, 0, 0.95), (1.3, 5, 0.0), (1.0, 40, 0.9), (0.9, 20, 0.0)]
PENS = [(1.8, 0.0, 0.0), (1.0, 0.0, 0.0), (0.6, 1.5, -0.7), (1.0, 0.0, 0.0), (1.0, 1.5, 1.5)]
SHARED = 4


def _cols(params, pens):
    return dict(temperature=[t[0] for t in params], top_k=[t[1] for t in params], top_p=[t[2] for t in params],
                repetition_penalty=[p[0] for p in pens], frequency_penalty=[p[1] for p in pens], presence_penalty=[p[2] for p in pens])


@functools.lru_cache(maxsize=None)
def _loop_prompts():
    V = _models("corr")[0].vocab_size
    prompts = _prompts(V, LENS, 2100)
    for p in prompts[1:]:
        p[0, :SHARED] = prompts[0][0, :SHARED]
    return prompts


@functools.lru_cache(maxsize=None)
def _oracle_runs(gamma, pens):
    """Every prompt's oracle run on the wrapped fp32 pair under its own Philox variates, its own (T, k, p) and ITS penalties."""
    from llmspeculativesampling_amd import _lib
    od, ot = _corr_oracles()
    runs = []
    for pf, s, m, (T, k, p), pen in zip(_loop_prompts(), SEEDS, BUDGETS, PARAMS, pens):
        L = pf.shape[1]
        runs.append(oracle.speculative_sampling(pf, PenalisedModel(od, L, *pen), PenalisedModel(ot, L, *pen), -1, None, m, details=True,
                                                gamma=gamma, temperature=T, top_k=k, top_p=p,
                                                noise=PhiloxOracleNoise(_lib.lib, s, gamma, _st)))
    return runs


def _assert_runs(wants, outs, ds, what):
    for i, ((want, wd), got, gd) in enumerate(zip(wants, outs, ds)):
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"{what}: prompt {i}")
        assert gd["acc_len"] == wd["acc_len"], (what, i)


def _condition(gamma):
    """On the CPU: every penalised prompt's oracle output differs from its unpenalised one (else the test shows nothing)."""
    pen, plain = _oracle_runs(gamma, tuple(PENS)), _oracle_runs(gamma, tuple([(1.0, 0.0, 0.0)] * len(PENS)))
    for i, p in enumerate(PENS):
        same = torch.equal(pen[i][0], plain[i][0])
        assert same == (p == (1.0, 0.0, 0.0)), (gamma, i, p)
    return pen


@pytest.mark.parametrize("gamma", [1, 4])
def test_l1_queue_batch_and_single_stream_equal_the_oracle(hip, gamma):
    """Five prompts with a shared prefix of 4 tokens through 2 slots, three of them penalised, every one with its own (T, k, p):
    tokens and accepted lengths of every prompt equal the oracle's on the wrapped pair, the batch loop's (the first four as
    streams) and the single-stream loop's."""
    wants = _condition(gamma)
    dm, tm = _models("corr")[4:]
    prompts = [p.cuda() for p in _loop_prompts()]
    t = {}
    outs, ds = hip.S.speculative_sampling_queue_requests(prompts, dm, tm, -1, None, BUDGETS, gamma=gamma, details=True, seeds=SEEDS,
                                                         slots=2, prefill_chunk=8, _timing=t, shared_prefix=SHARED, **_cols(PARAMS, PENS))
    assert t["copied_rows"] > 0 and any(a > 0 for a in t["admit_iter"])
    _assert_runs(wants, outs, ds, "queue")
    bouts, bds = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, -1, None, 12, gamma=gamma, details=True, seeds=SEEDS[:4],
                                                  **_cols(PARAMS[:4], PENS[:4]))
    for i, (o, d) in enumerate(zip(bouts, bds)):                   # (one budget for all streams: the common prefix of the runs)
        n = min(o.shape[1], wants[i][0].shape[1])
        assert n >= LENS[i] + 12 and torch.equal(o[:, :n].cpu(), wants[i][0][:, :n]), i
    singles = [hip.S.speculative_sampling(pf, dm, tm, -1, None, m, gamma=gamma, details=True, rng=hip.noise.DeviceNoise(s),
                                          temperature=T, top_k=k, top_p=p, repetition_penalty=pen[0], frequency_penalty=pen[1],
                                          presence_penalty=pen[2])
               for pf, m, s, (T, k, p), pen in zip(prompts, BUDGETS, SEEDS, PARAMS, PENS)]
    _assert_runs(singles, outs, ds, "single stream")


def test_l2_autoregressive_loops_equal_the_oracle(hip):
    """Three streams of the `corr` target, two of them penalised, and the same three one at a time, against the oracle's
    autoregressive reference on the wrapped model."""
    tm = _models("corr")[5]
    ot = _corr_oracles()[1]
    prompts, pens, seeds, N = _loop_prompts()[:3], PENS[:3], SEEDS[:3], 16
    wants, plain = [[oracle.autoregressive_sampling(pf, PenalisedModel(ot, pf.shape[1], *pen), N, -1, 1.0, 20, 0.9,
                                                    noise=PhiloxOracleNoise(hip.lib, s, 1, _st))
                     for pf, s, pen in zip(prompts, seeds, table)] for table in (pens, [(1.0, 0.0, 0.0)] * 3)]
    for w, p, pen in zip(wants, plain, pens):
        assert torch.equal(w, p) == (pen == (1.0, 0.0, 0.0))
    cols = {k: v for k, v in _cols(PARAMS[:3], pens).items() if k.endswith("penalty")}
    outs = hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts], tm, N, -1, top_k=20, top_p=0.9, seeds=seeds, **cols)
    for i, (o, w) in enumerate(zip(outs, wants)):
        np.testing.assert_array_equal(o.cpu().numpy(), w.numpy(), err_msg=f"stream {i}")
    for i, (pf, s, pen) in enumerate(zip(prompts, seeds, pens)):
        o = hip.S.autoregressive_sampling(pf.cuda(), tm, N, -1, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(s),
                                          repetition_penalty=pen[0], frequency_penalty=pen[1], presence_penalty=pen[2])
        np.testing.assert_array_equal(o.cpu().numpy(), wants[i].numpy(), err_msg=f"single stream {i}")


def test_l3_bf16_fused_tail_equals_the_dense_tail_and_scores_stay_raw(hip):
    """The bf16 pair (V = 8192, where the draft head can leave tile maxima), four streams, two of them penalised, scores on: the
    fused tail - penalised passes without tile maxima, the others on them - against SD_BATCH_FUSED_TAIL=0, bit for bit; and the
    scores are those of the raw rows: each within test_gpu_logprobs' bf16 bar of the fp32 truth of the unpenalised model."""
    cfg, dm, tm, ot = _bf16_pair()
    lens = [12, 5, 20, 9]
    prompts = [p.cuda() for p in _prompts(cfg.vocab_size, lens, 1500)]
    # (8192 ids and a dozen tokens: a run seldom repeats a token by itself, so the two penalised streams REWARD their histories -
    # repetition < 1, negative frequency / presence - which moves the output for certain)
    pens = dict(repetition_penalty=[0.3, 1.0, 1.0, 1.0], frequency_penalty=[0.0, 0.0, 0.0, -4.0], presence_penalty=[-6.0, 0.0, 0.0, -4.0])
    runs = {}
    old = os.environ.get("SD_BATCH_FUSED_TAIL")
    try:
        for tail in ("1", "0"):
            os.environ["SD_BATCH_FUSED_TAIL"] = tail
            runs[tail] = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 12, gamma=4, top_k=20, top_p=0.9, details=True,
                                                          seeds=[61, 62, 63, 64], logprobs=True, **pens)
    finally:
        os.environ.pop("SD_BATCH_FUSED_TAIL", None)
        if old is not None:
            os.environ["SD_BATCH_FUSED_TAIL"] = old
    (o1, d1, l1), (o0, d0, l0) = runs["1"], runs["0"]
    for a, b, da, db, la, lb in zip(o1, o0, d1, d0, l1, l0):
        assert torch.equal(a, b) and torch.equal(la, lb) and da["acc_len"] == db["acc_len"]
    plain = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 12, gamma=4, top_k=20, top_p=0.9, seeds=[61, 62, 63, 64])
    assert not torch.equal(plain[0], o1[0]) and not torch.equal(plain[3], o1[3])
    assert torch.equal(plain[1], o1[1]) and torch.equal(plain[2], o1[2])     # the neutral neighbours are left alone
    for i, (o, lp, L) in enumerate(zip(o1, l1, lens)):
        _check(ot, o, lp, L, bar=2 * 0.04, rel=True, what=f"bf16 stream {i}")


def test_l4_presence_forbids_repeats_and_neutral_lists_change_nothing(hip):
    dc, _, _, _, dm, tm = _models("corr")
    prompts = [p.cuda() for p in _loop_prompts()]
    kw = dict(gamma=4, top_k=20, top_p=0.9)
    outs = hip.S.speculative_sampling_queue_requests(prompts, dm, tm, -1, None, 20, seeds=SEEDS, slots=2, presence_penalty=1e4, **kw)
    for o, L in zip(outs, LENS):
        new = o[0, L:].tolist()
        assert len(new) >= 20 and len(set(new)) == len(new), new
    o = hip.S.autoregressive_sampling(prompts[0], tm, 20, -1, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(5), presence_penalty=1e4)
    assert len(set(o[0, LENS[0]:].tolist())) == 20
    # all-neutral lists: the block goes through the _penalties entries and is dropped there
    N = len(prompts)
    neutral = dict(repetition_penalty=[1.0] * N, frequency_penalty=[0.0] * N, presence_penalty=[0.0] * N)
    t0, t1 = {}, {}
    a, da = hip.S.speculative_sampling_queue_shared(prompts, dm, tm, 2, None, BUDGETS, details=True, seeds=SEEDS, slots=2, _timing=t0, **kw)
    b, db = hip.S.speculative_sampling_queue_requests(prompts, dm, tm, 2, None, BUDGETS, details=True, seeds=SEEDS, slots=2, _timing=t1,
                                                      **kw, **neutral)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and [d["acc_len"] for d in da] == [d["acc_len"] for d in db]
    assert all(t0[k] == t1[k] for k in ("iterations", "target_passes", "draft_passes", "admit_iter", "finish_iter"))
    n4 = {k: v[:4] for k, v in neutral.items()}
    a = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, 2, None, 12, seeds=SEEDS[:4], **kw)
    b = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, 2, None, 12, seeds=SEEDS[:4], **kw, **n4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    na, nb = hip.noise.DeviceNoise(9), hip.noise.DeviceNoise(9)
    a = hip.S.speculative_sampling(prompts[2], dm, tm, 2, None, 12, rng=na, **kw)
    b = hip.S.speculative_sampling(prompts[2], dm, tm, 2, None, 12, rng=nb, frequency_penalty=-0.0, **kw)
    assert torch.equal(a, b) and (na.seed, na.draw) == (nb.seed, nb.draw)
    a = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 10, 2, top_k=20, top_p=0.9, seeds=SEEDS[:3])
    b = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 10, 2, top_k=20, top_p=0.9, seeds=SEEDS[:3], **{k: v[:3] for k, v in neutral.items()})
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_l5_logprobs_with_penalties_are_the_raw_scores(hip):
    """logprobs=True with penalties, fp32 `corr` pair, queue and single stream: tokens are the penalised run's, every score is
    within test_gpu_logprobs' bar of the float64 log-softmax of the UNPENALISED oracle target's logits at those tokens."""
    dm, tm = _models("corr")[4:]
    ot = _corr_oracles()[1]
    prompts = [p.cuda() for p in _loop_prompts()]
    cols = _cols(PARAMS, PENS)
    base = hip.S.speculative_sampling_queue_requests(prompts, dm, tm, -1, None, BUDGETS, gamma=4, seeds=SEEDS, slots=2, **cols)
    outs, lps = hip.S.speculative_sampling_queue_requests(prompts, dm, tm, -1, None, BUDGETS, gamma=4, seeds=SEEDS, slots=2, logprobs=True,
                                                          **cols)
    assert all(torch.equal(a, b) for a, b in zip(base, outs))
    for i, (o, lp, L) in enumerate(zip(outs, lps, LENS)):
        _check(ot, o, lp, L, what=f"queue prompt {i}")
    T, k, p = PARAMS[2]
    o, lp = hip.S.speculative_sampling(prompts[2], dm, tm, -1, None, BUDGETS[2], gamma=4, rng=hip.noise.DeviceNoise(SEEDS[2]), logprobs=True,
                                       temperature=T, top_k=k, top_p=p, repetition_penalty=PENS[2][0], frequency_penalty=PENS[2][1],
                                       presence_penalty=PENS[2][2])
    assert torch.equal(o, outs[2]) and torch.equal(lp, lps[2])
    o, lp = hip.S.autoregressive_sampling(prompts[4], tm, 12, -1, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(3), logprobs=True,
                                          presence_penalty=1.5, frequency_penalty=1.5)
    _check(ot, o, lp, LENS[4], what="autoregressive")
