"""Per-request logit_bias / allowed_token_ids / banned_token_ids / min_tokens (`pytest -m gpu`): sd_edit_rows bit for bit
against apply_logit_edits o apply_penalties on the CPU, and the native loops against the CPU oracle run on models whose logits
carry the same penalties and edits (tests/edited_model.py), each prompt under its own Philox variates."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
from edited_model import EditedModel
from philox_replay import PhiloxOracleNoise
from test_gpu_logprobs import _bf16_pair, _check, _corr_oracles
from test_gpu_native_parity import _st
from test_gpu_penalties import (BUDGETS, ITEMS, LENS, MODES, PARAMS, ROWS, SEEDS, SENTINEL, SHARED, _as_read, _histories, _loop_prompts,
                                _same_bits)
from test_gpu_spec_queue import _models, _prompts
from llmspeculativesampling_amd.sampling._loop_common import allowed_mask_words
from llmspeculativesampling_amd.sampling.utils import apply_logit_edits, apply_penalties

pytestmark = pytest.mark.gpu

NEUTRAL_PEN = (1.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


# ----------------------------------------------------------------------------- K: the kernel
N_ROWS = [17, 1, 16, 2, 9, 17, 3, 17, 8, 17, 4, 17, 17, 6, 17, 12]          # rows per item
SPECIAL_IDS = [10, 11, 12, 13, 14]                                            # 0, -0, +inf, -inf, NaN in every row
PENS = [(1.8, 1.5, -0.7), (0.5, 0.0, 0.0), (1.0, -0.7, 1.5)]


def _planted(V):
    """Bias ids at the row's two ends, around the unaligned head (ids 0..3), on both sides of the first window edge whatever
    the head (4095 .. 4099), on the specials, and one id >= V, which is ignored."""
    return sorted({0, 1, 2, 3, 4095, 4096, 4097, 4098, 4099, V - 1, *SPECIAL_IDS} & set(range(V))) + [V + 7]


def _item_spec(i, V, hist, hist0, P, rng):
    """Item i of the launch: kind i % 6 = neutral throughout, bias only, mask only, min_tokens only, penalties only, everything."""
    kind, rows = i % 6, N_ROWS[i]
    spec = dict(pen=NEUTRAL_PEN, bias={}, mask=None, m=0, eos=int(rng.integers(0, V)))
    in_hist = sorted({int(t) for t in hist[:hist0 + rows] if 0 <= t < V})
    if kind in (1, 5):
        n = {1: 1, 7: 1024, 13: 300, 5: 40, 11: 1024}[i]                   # n_bias 1, 1024 and sizes between
        ids = [4096 if V > 4096 else 3] if n == 1 else _planted(V) + in_hist[:8]
        if n > 1:
            rest = rng.choice(V, size=min(V, 2 * n), replace=False).tolist()
            ids = (ids + [t for t in rest if t not in set(ids)])[:n]
        vals = (rng.standard_normal(len(ids)) * 5).astype(np.float32).tolist()
        vals[0], vals[-1] = 1e4, -1e4
        if len(vals) > 4:
            vals[1], vals[2], vals[3] = 0.0, -0.0, 1e-3                        # +0 on a logit of -0 gives +0; 1e-3 drowns in a 16-bit sum
        spec["bias"] = dict(zip(ids, vals))
    if kind in (2, 5):
        if i == 2:
            allowed, banned = [V - 1], []                                      # a single allowed id, the row's last
        elif i == 8:
            allowed, banned = None, [4096 % V]                                 # every id but one
        elif i == 14:
            allowed, banned = list(range(0, V - 19)), [12]                     # the last word partly set; a banned +inf
        else:
            allowed, banned = rng.choice(V, size=V // 2, replace=False).tolist(), in_hist[:3] + [14]
        spec["mask"] = allowed_mask_words(V, allowed, banned)
    if kind in (3, 5):
        # j = hist0 + r - P crosses m inside the item's rows: the first rows lose EOS, the later ones keep it
        spec["m"] = max(1, hist0 - P + (rows + 1) // 2) if hist0 + rows // 2 > P else 5
        if i == 9:
            spec["eos"] = -1                                                   # no EOS id: min_tokens does nothing
        elif i == 3:
            spec["eos"] = 13
        if i == 15:
            spec["m"] = 10 ** 6                                                # every row below it
    if kind in (4, 5):
        spec["pen"] = PENS[i % 3]
    return spec


@functools.lru_cache(maxsize=None)
def _kernel_case(V):
    rng = np.random.default_rng(V + 1)
    hists = _histories(V, rng)[:ITEMS]
    x = torch.from_numpy(rng.standard_normal((ITEMS * ROWS, V)).astype(np.float32)) * 8
    x[:, SPECIAL_IDS] = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")])
    x[:, V - 1] = float("nan")
    x[::2, 0] = -0.0
    specs = [_item_spec(i, V, h, h0, P, rng) for i, (h, h0, P) in enumerate(hists)]
    return hists, x, specs


@pytest.mark.parametrize("V", [512, 8192, 32000, 50272])
@pytest.mark.parametrize("mode", list(MODES))
def test_k1_kernel_bit_for_bit_against_the_definitions(hip, mode, V):
    """One launch of 16 items x 1..17 rows over slabs of row stride V + 3.  Item i's input rows start i % 4 elements past a
    16-byte boundary (and the odd stride moves every later row on); the output rows of items 0..11 share that offset (the
    16-byte body), those of items 12..15 do not (scalar throughout).  Every row equals apply_logit_edits(apply_penalties(row as
    the sampler reads it)); rows past an item's count, the padding columns and the raw input slab keep their bytes; a second run
    gives the same bytes."""
    m = MODES[mode]
    hists, x, specs = _kernel_case(V)
    if m & 48 and not m & 3:                                      # rows that live in a 16-bit type hold values of that type
        x = _as_read(x, m).float()
    ld = V + 3
    span = (ROWS * ld + 4 + 3) // 4 * 4                           # an item's rows and room for its offset, 16 bytes apart
    in_off = [i % 4 for i in range(ITEMS)]
    out_off = [o if i < 12 else (o + 1 + i % 3) % 4 for i, o in enumerate(in_off)]
    slab = torch.zeros(ITEMS * span + 4, dtype=torch.float32)
    for i in range(ITEMS):
        slab[i * span + in_off[i]:][:ROWS * ld].view(ROWS, ld)[:, :V] = x[i * ROWS:(i + 1) * ROWS]
    dev_in = slab.cuda()
    assert dev_in.data_ptr() % 16 == 0 and span % 4 == 0
    keep = dev_in.clone()
    out = torch.full((ITEMS * span + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    seqs = [torch.tensor(h, dtype=torch.int64).to(torch.int32).cuda() for h, _, _ in hists]
    ids = [torch.tensor(sorted(s["bias"]), dtype=torch.int32).cuda() for s in specs]
    vals = [torch.tensor([s["bias"][t] for t in sorted(s["bias"])], dtype=torch.float32).cuda() for s in specs]
    masks = [torch.from_numpy(s["mask"].view(np.int32)).cuda() if s["mask"] is not None else None for s in specs]
    items = (hip.L.SdLogitEditItem * ITEMS)()
    for i, (it, s) in enumerate(zip(items, specs)):
        _, hist0, P = hists[i]
        setattr(it, "in", dev_in.data_ptr() + 4 * (i * span + in_off[i]))
        it.out, it.ld_in, it.ld_out, it.rows = out.data_ptr() + 4 * (i * span + out_off[i]), ld, ld, N_ROWS[i]
        it.seq, it.hist0, it.prompt_len, it.pen = seqs[i].data_ptr(), hist0, P, hip.L.SdPenalty(*s["pen"])
        nb = len(s["bias"])
        it.edit = hip.L.SdLogitEdit(ids[i].data_ptr() if nb else None, vals[i].data_ptr() if nb else None, nb,
                                    masks[i].data_ptr() if masks[i] is not None else None, s["m"])
        it.eos_token_id = s["eos"]
    assert {len(s["bias"]) for s in specs} >= ({0, 1, 1024} if V > 1024 else {0, 1})
    runs = []
    for _ in range(2):
        assert hip.lib.sd_edit_rows(items, ITEMS, V, m, _st()) == 0, hip.lib.sd_last_error()
        torch.cuda.synchronize()
        runs.append(out.cpu())
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(dev_in.view(torch.int32), keep.view(torch.int32))          # the raw rows are not written
    crossed = 0
    for i, s in enumerate(specs):
        h, hist0, P = hists[i]
        blk = runs[0][i * span:(i + 1) * span]
        got = blk[out_off[i]:][:ROWS * ld].view(ROWS, ld)
        assert blk[:out_off[i]].eq(SENTINEL).all() and got[:-1, V:].eq(SENTINEL).all() and got[N_ROWS[i]:, :V].eq(SENTINEL).all(), i
        floors = set()
        for r in range(N_ROWS[i]):
            row = _as_read(x[i * ROWS + r], m)
            y = apply_penalties(row, h[:hist0 + r], P, *s["pen"])
            want = apply_logit_edits(y, hist0 + r - P, s["eos"], s["bias"], s["mask"], s["m"]).float()
            g = got[r, :V].view(torch.float32)
            assert _same_bits(g, want), (mode, V, "item", i, "row", r, {k: v for k, v in s.items() if k not in ("bias", "mask")})
            if i % 6 == 0:
                assert _same_bits(g, row.float())                 # neutral throughout: rounded and copied
            if s["eos"] >= 0 and s["m"] > 0:
                floors.add(hist0 + r - P < s["m"])
                assert (float(g[s["eos"]]) == float("-inf")) or hist0 + r - P >= s["m"]
        crossed += floors == {True, False}
    assert crossed >= 2                                           # items whose rows lie on both sides of their min_tokens


def test_k2_one_item_one_row_and_the_refusals(hip):
    V, ld = 700, 701                                              # 700 = 21 * 32 + 28: the mask's last word is partial
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((3, ld)).astype(np.float32)).cuda()
    seq = torch.tensor([5, 6, 5, 699, 0, 5], dtype=torch.int32, device="cuda")
    out = torch.full((3, ld), SENTINEL, dtype=torch.int32, device="cuda")
    bias = {0: 2.5, 5: -3.0, 699: 1.25, 704: 9.0}
    mask = allowed_mask_words(V, None, [6, 698])
    ids = torch.tensor(sorted(bias), dtype=torch.int32, device="cuda")
    vals = torch.tensor([bias[t] for t in sorted(bias)], dtype=torch.float32, device="cuda")
    words = torch.from_numpy(mask.view(np.int32)).cuda()
    edit = lambda: hip.L.SdLogitEdit(ids.data_ptr(), vals.data_ptr(), len(bias), words.data_ptr(), 4)
    items = (hip.L.SdLogitEditItem * 2)()
    for i, it in enumerate(items):
        setattr(it, "in", x[i].data_ptr())
        it.out, it.ld_in, it.ld_out, it.rows = out[i].data_ptr(), ld, ld, 1
        it.seq, it.hist0, it.prompt_len, it.pen = seq.data_ptr(), 5 + i, 2, hip.L.SdPenalty(1.8, 1.5, -0.7)
        it.edit, it.eos_token_id = edit(), 699
    assert hip.lib.sd_edit_rows(items, 2, V, 0, _st()) == 0, hip.lib.sd_last_error()
    torch.cuda.synchronize()
    for i in range(2):                                            # j = 3 (below min_tokens 4: no EOS), then j = 4
        y = apply_penalties(x[i, :V].cpu(), seq[:5 + i].cpu(), 2, 1.8, 1.5, -0.7)
        want = apply_logit_edits(y, 3 + i, 699, bias, mask, 4)
        assert _same_bits(out[i, :V].cpu().view(torch.float32), want)
        assert (float(want[699]) == float("-inf")) == (i == 0) and float(want[6]) == float("-inf")
    assert out[2].eq(SENTINEL).all() and out[:2, V:].eq(SENTINEL).all()
    out.fill_(SENTINEL)
    E = hip.L.SdLogitEdit
    bad = [dict(rows=0), dict(rows=18), dict(ld_in=V - 1), dict(ld_out=V - 1), dict(hist0=0), dict(prompt_len=-1), dict(seq=None),
           dict(out=None), dict(pen=hip.L.SdPenalty(0.0, 0, 0)), dict(pen=hip.L.SdPenalty(1.0, float("nan"), 0)),
           dict(edit=E(ids.data_ptr(), vals.data_ptr(), -1, None, 0)), dict(edit=E(ids.data_ptr(), vals.data_ptr(), 1025, None, 0)),
           dict(edit=E(None, vals.data_ptr(), 2, None, 0)), dict(edit=E(ids.data_ptr(), None, 2, None, 0)),
           dict(edit=E(None, None, 0, words.data_ptr(), -1))]
    for over in bad:
        for k, v in over.items():
            setattr(items[1], k, v)
        assert hip.lib.sd_edit_rows(items, 2, V, 0, _st()) == hip.L.SD_ERR_INVALID, over
        assert b"item 1" in hip.lib.sd_last_error(), (over, hip.lib.sd_last_error())
        items[1].out, items[1].ld_in, items[1].ld_out, items[1].rows = out[1].data_ptr(), ld, ld, 1          # put back
        items[1].seq, items[1].hist0, items[1].prompt_len, items[1].pen = seq.data_ptr(), 6, 2, hip.L.SdPenalty(1.8, 1.5, -0.7)
        items[1].edit = edit()
    for args in ((None, 1, V, 0), (items, 0, V, 0), (items, 17, V, 0), (items, 2, 0, 0), (items, 2, 65537, 0), (items, 2, V, 3)):
        assert hip.lib.sd_edit_rows(*args, _st()) == hip.L.SD_ERR_INVALID, args
    torch.cuda.synchronize()
    assert out.eq(SENTINEL).all()                                 # nothing was launched


# ----------------------------------------------------------------------------- L: the loops
EOS = 2                                                           # (the prompts hold ids >= 3)


@functools.lru_cache(maxsize=None)
def _plain_runs(gamma):
    """The five prompts' oracle runs without penalties or edits (what a banned id is chosen from)."""
    od, ot = _corr_oracles()
    return [oracle.speculative_sampling(pf, od, ot, EOS, None, m, details=True, gamma=gamma, temperature=T, top_k=k, top_p=p,
                                        noise=PhiloxOracleNoise(_lib().lib, s, gamma, _st))
            for pf, s, m, (T, k, p) in zip(_loop_prompts(), SEEDS, BUDGETS, PARAMS)]


def _lib():
    from llmspeculativesampling_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _requests(gamma):
    """Per prompt: penalties AND edits (a bias that pulls EOS in, held off by min_tokens); fully neutral; an allowed set of 12
    ids under top_k = 5; three banned ids the plain run emits; penalties only."""
    V = _models("corr")[0].vocab_size
    plain = _plain_runs(gamma)
    new3 = list(dict.fromkeys(plain[3][0][0, LENS[3]:].tolist()))[:3]
    rng = np.random.default_rng(77)
    return [dict(pen=(1.8, 0.0, 0.0), bias={EOS: 9.0, 17: -2.0, V - 1: 1.5}, allowed=None, banned=[], m=6),
            dict(pen=NEUTRAL_PEN, bias=None, allowed=None, banned=[], m=0),
            dict(pen=NEUTRAL_PEN, bias=None, allowed=sorted(rng.choice(np.arange(3, V), size=11, replace=False).tolist() + [EOS]), banned=[], m=3),
            dict(pen=NEUTRAL_PEN, bias=None, allowed=None, banned=new3, m=0),
            dict(pen=(1.0, 1.5, 1.5), bias=None, allowed=None, banned=[], m=0)]


def _cols(reqs, params=None):
    kw = dict(repetition_penalty=[r["pen"][0] for r in reqs], frequency_penalty=[r["pen"][1] for r in reqs],
              presence_penalty=[r["pen"][2] for r in reqs], logit_bias=[r["bias"] for r in reqs],
              allowed_token_ids=[r["allowed"] for r in reqs], banned_token_ids=[r["banned"] or None for r in reqs],
              min_tokens=[r["m"] for r in reqs])
    if params is not None:
        kw.update(temperature=[t[0] for t in params], top_k=[t[1] for t in params], top_p=[t[2] for t in params])
    return kw


def _one(r):
    return dict(repetition_penalty=r["pen"][0], frequency_penalty=r["pen"][1], presence_penalty=r["pen"][2], logit_bias=r["bias"],
                allowed_token_ids=r["allowed"], banned_token_ids=r["banned"] or None, min_tokens=r["m"])


def _wrap(om, L, r):
    return EditedModel(om, L, EOS, r["pen"], r["bias"], r["allowed"], r["banned"], r["m"])


@functools.lru_cache(maxsize=None)
def _oracle_runs(gamma):
    """Every prompt's oracle run on the wrapped fp32 pair under its own Philox variates, its own (T, k, p) and ITS request."""
    od, ot = _corr_oracles()
    runs = []
    for pf, s, m, (T, k, p), r in zip(_loop_prompts(), SEEDS, BUDGETS, PARAMS, _requests(gamma)):
        L = pf.shape[1]
        runs.append(oracle.speculative_sampling(pf, _wrap(od, L, r), _wrap(ot, L, r), EOS, None, m, details=True, gamma=gamma,
                                                temperature=T, top_k=k, top_p=p, noise=PhiloxOracleNoise(_lib().lib, s, gamma, _st)))
    return runs


def _assert_runs(wants, outs, ds, what):
    for i, ((want, wd), got, gd) in enumerate(zip(wants, outs, ds)):
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"{what}: prompt {i}")
        assert gd["acc_len"] == wd["acc_len"], (what, i)


def _condition(gamma):
    """On the CPU: every edited or penalised prompt's oracle output differs from its plain one, the neutral one's does not
    (else the test shows nothing); and the edits are visible in the oracle's own output."""
    wants, plain, reqs = _oracle_runs(gamma), _plain_runs(gamma), _requests(gamma)
    for i in range(len(reqs)):
        assert torch.equal(wants[i][0], plain[i][0]) == (i == 1), (gamma, i)
    new = [w[0][0, L:].tolist() for w, L in zip(wants, LENS)]
    assert EOS not in new[0][:6] and set(new[2]) <= set(reqs[2]["allowed"]) and EOS not in new[2][:3]
    assert not set(new[3]) & set(reqs[3]["banned"])
    return wants


@pytest.mark.parametrize("gamma", [1, 4])
def test_l1_queue_batch_and_single_stream_equal_the_oracle(hip, gamma):
    """Five prompts with a shared prefix of 4 tokens through 2 slots, each with its own (T, k, p) and its own request - one with
    penalties and edits, one neutral, so a slot changes hands between an edited and a neutral request: tokens and accepted
    lengths of every prompt equal the oracle's on the wrapped pair, the batch loop's (the first four as streams) and the
    single-stream loop's."""
    wants = _condition(gamma)
    reqs = _requests(gamma)
    dm, tm = _models("corr")[4:]
    prompts = [p.cuda() for p in _loop_prompts()]
    t = {}
    outs, ds = hip.S.speculative_sampling_queue_edits(prompts, dm, tm, EOS, None, BUDGETS, gamma=gamma, details=True, seeds=SEEDS,
                                                         slots=2, prefill_chunk=8, _timing=t, shared_prefix=SHARED, **_cols(reqs, PARAMS))
    assert t["copied_rows"] > 0 and any(a > 0 for a in t["admit_iter"])
    _assert_runs(wants, outs, ds, "queue")
    bouts, bds = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, EOS, None, 12, gamma=gamma, details=True, seeds=SEEDS[:4],
                                                  **_cols(reqs[:4], PARAMS[:4]))
    for i, o in enumerate(bouts):                                  # (one budget for all streams: the common prefix of the runs)
        n = min(o.shape[1], wants[i][0].shape[1])
        ended = EOS in wants[i][0][0, LENS[i]:n].tolist()
        assert (n >= LENS[i] + 12 or ended) and torch.equal(o[:, :n].cpu(), wants[i][0][:, :n]), i
    singles = [hip.S.speculative_sampling(pf, dm, tm, EOS, None, m, gamma=gamma, details=True, rng=hip.noise.DeviceNoise(s),
                                          temperature=T, top_k=k, top_p=p, **_one(r))
               for pf, m, s, (T, k, p), r in zip(prompts, BUDGETS, SEEDS, PARAMS, reqs)]
    _assert_runs(singles, outs, ds, "single stream")


def test_l2_autoregressive_loops_equal_the_oracle(hip):
    """Three streams of the `corr` target - penalties and edits, neutral, an allowed set - and the same three one at a time,
    against the oracle's autoregressive reference on the wrapped model."""
    tm = _models("corr")[5]
    ot = _corr_oracles()[1]
    prompts, reqs, seeds, N = _loop_prompts()[:3], _requests(4)[:3], SEEDS[:3], 16
    neutral = dict(pen=NEUTRAL_PEN, bias=None, allowed=None, banned=[], m=0)
    wants, plain = [[oracle.autoregressive_sampling(pf, _wrap(ot, pf.shape[1], r), N, EOS, 1.0, 20, 0.9,
                                                    noise=PhiloxOracleNoise(hip.lib, s, 1, _st))
                     for pf, s, r in zip(prompts, seeds, table)] for table in (reqs, [neutral] * 3)]
    for i, (w, p) in enumerate(zip(wants, plain)):
        assert torch.equal(w, p) == (i == 1)
    outs = hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts], tm, N, EOS, top_k=20, top_p=0.9, seeds=seeds, **_cols(reqs))
    for i, (o, w) in enumerate(zip(outs, wants)):
        np.testing.assert_array_equal(o.cpu().numpy(), w.numpy(), err_msg=f"stream {i}")
    for i, (pf, s, r) in enumerate(zip(prompts, seeds, reqs)):
        o = hip.S.autoregressive_sampling(pf.cuda(), tm, N, EOS, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(s), **_one(r))
        np.testing.assert_array_equal(o.cpu().numpy(), wants[i].numpy(), err_msg=f"single stream {i}")


def _loops(hip, prompts, N, eos, gamma=4, **kw):
    """The five loops on the same prompts and seeds -> {loop: [new tokens per prompt]}.  kw: scalars / one value for all."""
    dm, tm = _models("corr")[4:]
    n = len(prompts)
    seeds = SEEDS[:n]
    new = lambda outs: [o[0, pf.shape[1]:].tolist() for o, pf in zip(outs, prompts)]
    runs = {
        "queue": new(hip.S.speculative_sampling_queue_edits(prompts, dm, tm, eos, None, N, gamma=gamma, seeds=seeds, slots=2, **kw)),
        "batch": new(hip.S.speculative_sampling_batch(prompts, dm, tm, eos, None, N, gamma=gamma, seeds=seeds, **kw)),
        "single": new([hip.S.speculative_sampling(pf, dm, tm, eos, None, N, gamma=gamma, rng=hip.noise.DeviceNoise(s), **kw)
                       for pf, s in zip(prompts, seeds)]),
        "ar_batch": new(hip.S.autoregressive_sampling_batch(prompts, tm, N, eos, seeds=seeds, **{k: v for k, v in kw.items()})),
        "ar": new([hip.S.autoregressive_sampling(pf, tm, N, eos, rng=hip.noise.DeviceNoise(s), **kw) for pf, s in zip(prompts, seeds)]),
    }
    return runs


def test_l3a_an_allowed_set_smaller_than_top_k_holds_every_token(hip):
    prompts = [p.cuda() for p in _loop_prompts()[:3]]
    allowed = [5, 77, 130, 131, 300]
    for filt in (dict(top_k=20, top_p=0.9), dict(top_k=0, top_p=0.9)):
        for loop, news in _loops(hip, prompts, 10, -1, allowed_token_ids=allowed, **filt).items():
            for toks in news:
                assert len(toks) >= 10 and set(toks) <= set(allowed), (filt, loop, toks)


def test_l3b_a_banned_id_never_appears(hip):
    prompts = [p.cuda() for p in _loop_prompts()[:3]]
    kw = dict(top_k=20, top_p=0.9)
    base = _loops(hip, prompts, 10, -1, **kw)
    for loop in base:
        assert base[loop] == base["queue"] or loop.startswith("ar")
    # ids the unedited runs of these seeds emit, in the speculative and in the autoregressive loops
    banned = sorted({toks[len(toks) // 2] for loop in ("queue", "ar") for toks in base[loop]} | {base["queue"][0][0], base["ar"][0][0]})
    edited = _loops(hip, prompts, 10, -1, banned_token_ids=banned, **kw)
    for loop, news in edited.items():
        assert any(set(toks) & set(banned) for toks in base[loop]), loop
        for toks in news:
            assert len(toks) >= 10 and not set(toks) & set(banned), (loop, toks, banned)


@pytest.mark.parametrize("gamma", [4, 8])
def test_l3c_min_tokens_holds_eos_off_exactly_that_long(hip, gamma):
    """A bias of +1e4 on EOS: with min_tokens = 6 the output is exactly six other tokens and then EOS, with 0 EOS alone.  At
    gamma 8 the first verify pass holds output tokens 0..8 and so straddles the sixth; at gamma 4 the second pass does."""
    prompts = [p.cuda() for p in _loop_prompts()[:3]]
    kw = dict(top_k=20, top_p=0.9, logit_bias={EOS: 1e4})
    for loop, news in _loops(hip, prompts, 12, EOS, gamma=gamma, min_tokens=6, **kw).items():
        for toks in news:
            assert len(toks) == 7 and toks[6] == EOS and EOS not in toks[:6], (loop, toks)
    for loop, news in _loops(hip, prompts, 12, EOS, gamma=gamma, min_tokens=0, **kw).items():
        assert all(toks == [EOS] for toks in news), (loop, news)


def test_l4_neutral_lists_change_nothing_and_scores_stay_raw(hip):
    dm, tm = _models("corr")[4:]
    ot = _corr_oracles()[1]
    prompts = [p.cuda() for p in _loop_prompts()]
    kw = dict(gamma=4, top_k=20, top_p=0.9)
    N = len(prompts)
    neutral = dict(logit_bias=[None, {}, None, {}, None], allowed_token_ids=[None] * N, banned_token_ids=[[], None, [], None, []],
                   min_tokens=[0] * N)
    t0, t1 = {}, {}
    a, da = hip.S.speculative_sampling_queue_shared(prompts, dm, tm, 2, None, BUDGETS, details=True, seeds=SEEDS, slots=2, _timing=t0, **kw)
    b, db = hip.S.speculative_sampling_queue_edits(prompts, dm, tm, 2, None, BUDGETS, details=True, seeds=SEEDS, slots=2, _timing=t1,
                                                      **kw, **neutral)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and [d["acc_len"] for d in da] == [d["acc_len"] for d in db]
    assert all(t0[k] == t1[k] for k in ("iterations", "target_passes", "draft_passes", "admit_iter", "finish_iter"))
    n4 = {k: v[:4] for k, v in neutral.items()}
    a = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, 2, None, 12, seeds=SEEDS[:4], **kw)
    b = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, 2, None, 12, seeds=SEEDS[:4], **kw, **n4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    na, nb = hip.noise.DeviceNoise(9), hip.noise.DeviceNoise(9)
    a = hip.S.speculative_sampling(prompts[2], dm, tm, 2, None, 12, rng=na, **kw)
    b = hip.S.speculative_sampling(prompts[2], dm, tm, 2, None, 12, rng=nb, logit_bias={}, banned_token_ids=[], min_tokens=0, **kw)
    assert torch.equal(a, b) and (na.seed, na.draw) == (nb.seed, nb.draw)
    a = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 10, 2, top_k=20, top_p=0.9, seeds=SEEDS[:3])
    b = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 10, 2, top_k=20, top_p=0.9, seeds=SEEDS[:3], **{k: v[:3] for k, v in neutral.items()})
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # logprobs=True under edits: the edited run's tokens, the RAW rows' scores - each within test_gpu_logprobs' bar of the
    # float64 log-softmax of the unwrapped oracle target's logits at those tokens
    reqs = _requests(4)
    cols = _cols(reqs, PARAMS)
    base = hip.S.speculative_sampling_queue_edits(prompts, dm, tm, EOS, None, BUDGETS, gamma=4, seeds=SEEDS, slots=2, **cols)
    outs, lps = hip.S.speculative_sampling_queue_edits(prompts, dm, tm, EOS, None, BUDGETS, gamma=4, seeds=SEEDS, slots=2, logprobs=True,
                                                          **cols)
    assert all(torch.equal(x, y) for x, y in zip(base, outs))
    for i, (o, lp, L) in enumerate(zip(outs, lps, LENS)):
        _check(ot, o, lp, L, what=f"queue prompt {i}")
    T, k, p = PARAMS[0]
    o, lp = hip.S.speculative_sampling(prompts[0], dm, tm, EOS, None, BUDGETS[0], gamma=4, rng=hip.noise.DeviceNoise(SEEDS[0]), logprobs=True,
                                       temperature=T, top_k=k, top_p=p, **_one(reqs[0]))
    assert torch.equal(o, outs[0]) and torch.equal(lp, lps[0])
    o, lp = hip.S.autoregressive_sampling(prompts[2], tm, 12, EOS, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(3), logprobs=True,
                                          **_one(reqs[2]))
    assert set(o[0, LENS[2]:].tolist()) <= set(reqs[2]["allowed"])
    _check(ot, o, lp, LENS[2], what="autoregressive")


def test_l5_bf16_fused_tail_equals_the_dense_tail_and_scores_stay_raw(hip):
    """The bf16 pair (V = 8192, where the draft head can leave tile maxima), four streams, two of them edited (one with
    penalties as well), scores on: the fused tail - edited passes without tile maxima, the others on them - against
    SD_BATCH_FUSED_TAIL=0, bit for bit; the neutral neighbours equal the call without keywords; the edited streams keep to their
    allowed set and off their banned ids; and the scores are those of the raw rows: each within test_gpu_logprobs' bf16 bar of
    the fp32 truth of the unedited model."""
    cfg, dm, tm, ot = _bf16_pair()
    lens = [12, 5, 20, 9]
    prompts = [p.cuda() for p in _prompts(cfg.vocab_size, lens, 1500)]
    kw = dict(gamma=4, top_k=20, top_p=0.9, seeds=[61, 62, 63, 64])
    plain = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 12, **kw)
    allowed = sorted(np.random.default_rng(5).choice(cfg.vocab_size, size=64, replace=False).tolist())
    banned = sorted(set(plain[3][0, lens[3]:].tolist()))[:4]
    edits = dict(allowed_token_ids=[allowed, None, None, None], banned_token_ids=[None, None, None, banned],
                 logit_bias=[{allowed[0]: 2.0}, None, None, {7: -1.0}], min_tokens=[0, 0, 0, 3],
                 repetition_penalty=[1.0, 1.0, 1.0, 0.3], presence_penalty=[0.0, 0.0, 0.0, -6.0])
    runs = {}
    old = os.environ.get("SD_BATCH_FUSED_TAIL")
    try:
        for tail in ("1", "0"):
            os.environ["SD_BATCH_FUSED_TAIL"] = tail
            runs[tail] = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 12, details=True, logprobs=True, **kw, **edits)
    finally:
        os.environ.pop("SD_BATCH_FUSED_TAIL", None)
        if old is not None:
            os.environ["SD_BATCH_FUSED_TAIL"] = old
    (o1, d1, l1), (o0, d0, l0) = runs["1"], runs["0"]
    for a, b, da, db, la, lb in zip(o1, o0, d1, d0, l1, l0):
        assert torch.equal(a, b) and torch.equal(la, lb) and da["acc_len"] == db["acc_len"]
    assert set(o1[0][0, lens[0]:].tolist()) <= set(allowed) and not set(o1[3][0, lens[3]:].tolist()) & set(banned)
    assert torch.equal(plain[1], o1[1]) and torch.equal(plain[2], o1[2])     # the neutral neighbours are left alone
    for i, (o, lp, L) in enumerate(zip(o1, l1, lens)):
        _check(ot, o, lp, L, bar=2 * 0.04, rel=True, what=f"bf16 stream {i}")


class _RecordingLib:
    """The module's `lib` with every loop entry's name and the set of non-NULL members of its last argument, the sd_loop_opts
    (an empty set: opts was NULL), written down before the call goes through."""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if "_generate" not in name:
            return fn

        def entry(*args):
            opts = args[-1]
            assert opts is None or isinstance(opts, _lib().SdLoopOpts), opts
            self._calls.append((name, {f for f, _ in _lib().SdLoopOpts._fields_ if opts is not None and getattr(opts, f)}))
            return fn(*args)
        return entry


def test_l6_which_entry_a_call_takes(hip, monkeypatch):
    """Every wrapper's call, read off a recording `lib` in its module: neutral keywords (absent, or spelt out as neutral values)
    produce the call that was made before the keywords existed - a NULL sd_loop_opts where nothing else asks for a member -
    penalties alone set member penalties, edits member edits, with or without penalties and scores beside them.  The whole set
    of non-NULL members is compared."""
    import importlib
    calls = []
    for mod in ("speculative_sampling", "batch", "autoregressive_sampling"):
        m = importlib.import_module("llmspeculativesampling_amd.sampling." + mod)
        monkeypatch.setattr(m, "lib", _RecordingLib(m.lib, calls))
    dm, tm = _models("corr")[4:]
    prompts = [p.cuda() for p in _loop_prompts()[:3]]
    kw = dict(top_k=20, top_p=0.9)
    neutral1 = dict(logit_bias={}, allowed_token_ids=None, banned_token_ids=[], min_tokens=0)
    neutral3 = dict(logit_bias=[None, {}, None], allowed_token_ids=[None] * 3, banned_token_ids=[[], None, []], min_tokens=[0, 0, 0])
    edits1 = dict(logit_bias={17: 1.0}, banned_token_ids=[5], min_tokens=2)
    edits3 = dict(logit_bias=[None, {17: 1.0}, None], min_tokens=[0, 0, 3])
    pen = dict(presence_penalty=0.5)

    def took(fn, *args, **more):
        del calls[:]
        fn(*args, **more)
        assert len(calls) == 1, calls
        return calls[0]
    LP, PEN, ED = "logprobs", "penalties", "edits"
    single = lambda **more: took(hip.S.speculative_sampling, prompts[0], dm, tm, EOS, None, 6, rng=hip.noise.DeviceNoise(3), **kw, **more)
    assert single() == single(**neutral1) == ("sd_spec_generate", set())
    assert single(logprobs=True) == single(logprobs=True, **neutral1) == ("sd_spec_generate", {LP})
    assert single(**pen) == single(**pen, **neutral1) == ("sd_spec_generate", {PEN})
    assert single(**edits1) == single(min_tokens=1) == ("sd_spec_generate", {ED})
    assert single(**edits1, **pen, logprobs=True) == ("sd_spec_generate", {LP, PEN, ED})
    batch = lambda **more: took(hip.S.speculative_sampling_batch, prompts, dm, tm, EOS, None, 6, seeds=SEEDS[:3], **kw, **more)
    assert batch() == batch(**neutral3) == batch(**neutral1) == ("sd_spec_batch_generate", set())
    assert batch(logprobs=True, **neutral3) == ("sd_spec_batch_generate", {LP})
    assert batch(**pen, **neutral3) == ("sd_spec_batch_generate", {PEN})
    assert batch(**edits3) == ("sd_spec_batch_generate", {ED})
    assert batch(**edits1, **pen, logprobs=True) == ("sd_spec_batch_generate", {LP, PEN, ED})
    assert batch(temperature=[1.0, 0.7, 1.0], **neutral3) == ("sd_spec_batch_generate", {"row_params"})
    queue = lambda **more: took(hip.S.speculative_sampling_queue_edits, prompts, dm, tm, EOS, None, 6, seeds=SEEDS[:3], slots=2, **kw, **more)
    plain = took(hip.S.speculative_sampling_queue_requests, prompts, dm, tm, EOS, None, 6, seeds=SEEDS[:3], slots=2, **kw)
    assert plain == ("sd_spec_queue_generate", set()) and queue() == queue(**neutral3) == queue(**neutral1) == plain
    assert queue(logprobs=True, **neutral3) == ("sd_spec_queue_generate", {LP})
    assert queue(**pen, **neutral3) == ("sd_spec_queue_generate", {PEN})
    assert queue(**edits3) == ("sd_spec_queue_generate", {ED})
    assert queue(**edits1, **pen, logprobs=True) == ("sd_spec_queue_generate", {LP, PEN, ED})
    ar = lambda **more: took(hip.S.autoregressive_sampling, prompts[0], tm, 6, EOS, rng=hip.noise.DeviceNoise(3), **kw, **more)
    assert ar() == ar(**neutral1) == ("sd_ar_batch_generate", set())
    assert ar(**pen, **neutral1) == ("sd_ar_batch_generate", {PEN})
    assert ar(**edits1) == ("sd_ar_batch_generate", {ED}) and ar(**edits1, **pen) == ("sd_ar_batch_generate", {PEN, ED})
    arb = lambda **more: took(hip.S.autoregressive_sampling_batch, prompts, tm, 6, EOS, seeds=SEEDS[:3], **kw, **more)
    assert arb() == arb(**neutral3) == ("sd_ar_batch_generate", set())
    assert arb(logprobs=True, **neutral3) == ("sd_ar_batch_generate", {LP})
    assert arb(**pen, **neutral3) == ("sd_ar_batch_generate", {PEN}) and arb(**edits3) == ("sd_ar_batch_generate", {ED})
