"""Per-token target log-probabilities (`pytest -m gpu`): sd_token_logprobs against the float64 truth of adversarial rows
(tests/logprob_rows.py), and the four native loops' `logprobs=True` against the float64 log-softmax of the CPU oracle's own
target logits over the finished output - with tokens, details, Philox positions and cache lengths held to the runs without."""
import contextlib
import ctypes as C
import functools
import math
import os
import sys

import pytest
import torch

import oracle
import logprob_rows as LR
from test_gpu_native_parity import BF16_CFG, _st
from test_gpu_spec_queue import BUDGETS, KW, LENS, SEEDS, _corr_case, _ends, _models, _oracle, _prompts
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

pytestmark = pytest.mark.gpu

FP32_BAR = 2e-3           # 2 x the fp32 logit bar of 1e-3 (test_gpu_parity.py, north_star): a log-softmax moves by at most twice
                          # the largest logit error (once through the picked logit, once through the log-sum-exp)
SENTINEL = 0x7FC0BEEF     # a NaN bit pattern no computation produces


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise, quality
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise, quality=quality)


# ----------------------------------------------------------------------------- K: the kernel
def _launch(hip, logits, ld, V, mode, groups, toks):
    """One sd_token_logprobs call: item i = rows groups[i] = (first row of `logits` viewed as rows of stride ld, row count),
    scored at toks[first row ..]; -> the (total rows,) output tensor (prefilled with the sentinel)."""
    n = sum(r for _, r in groups)
    tok = torch.tensor(toks, dtype=torch.int32, device="cuda")
    out = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    items = (hip.L.SdLogprobItem * len(groups))()
    o = 0
    for it, (r0, rows) in zip(items, groups):
        it.logits, it.ld, it.rows = logits.data_ptr() + 4 * r0 * ld, ld, rows
        it.tokens, it.out = tok.data_ptr() + 4 * o, out.data_ptr() + 4 * o
        it.res = None
        o += rows
    assert hip.lib.sd_token_logprobs(items, len(groups), V, mode, _st()) == 0, hip.lib.sd_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("pad", [0, 3], ids=["ld_V", "ld_V_plus_3"])
@pytest.mark.parametrize("V", [257, 8192, 50272])
@pytest.mark.parametrize("dt", [0, 1, 2], ids=["fp32", "bf16_round", "f16_round"])
def test_k1_kernel_against_the_float64_truth(hip, dt, V, pad):
    """16 items x 17 rows (272 workgroups), then 1 item x 5 rows and 1 item x 1 row, over a slab of row stride V or V + 3 (every
    row after the first starts off a 16-byte boundary): each (row kind, token) of logprob_rows.pool within
    2^-17 * max(1, |want|) of the float64 log-softmax of the rounded row; a token at a -inf entry scores -inf."""
    cases = LR.pool(V, dt)
    ld, n = V + pad, 16 * 17
    slab = torch.zeros(n * ld + 4, dtype=torch.float32)
    for r in range(n):
        slab[r * ld:r * ld + V] = cases[r % len(cases)][1]
    assert n >= len(cases)
    dev = slab.cuda()
    toks = [cases[r % len(cases)][2] for r in range(n)]
    want = [cases[r % len(cases)][3] for r in range(n)]
    for groups in ([(17 * i, 17) for i in range(16)], [(34, 5)], [(7, 1)]):
        got = _launch(hip, dev, ld, V, dt, groups, [t for r0, rows in groups for t in toks[r0:r0 + rows]]).cpu().tolist()
        rows = [r for r0, k in groups for r in range(r0, r0 + k)]
        worst = max((abs(g - want[r]) / max(1.0, abs(want[r])) for g, r in zip(got, rows) if not math.isinf(want[r])), default=0.0)
        print(f"dt {dt} V {V} ld {ld} items {len(groups)}: worst {worst / LR.BAR:.3f} of the bar")
        for g, r in zip(got, rows):
            assert LR.within_bar(g, want[r]), (cases[r % len(cases)][0], toks[r], g, want[r])
    if dt == 0:
        eq = [g for g, r in zip(_launch(hip, dev, ld, V, 0, [(0, 17)], toks[:17]).cpu().tolist(), range(17)) if cases[r][0] == "equal"]
        assert eq and all(abs(g + math.log(V)) <= LR.BAR * math.log(V) for g in eq)


def _res_blocks(hip, n_accepted):
    blocks = (hip.L.SdAcceptResult * len(n_accepted))()
    for b, n in zip(blocks, n_accepted):
        b.n_accepted = n
    dev = torch.frombuffer(bytearray(bytes(blocks)), dtype=torch.uint8).cuda()
    return dev, [dev.data_ptr() + i * C.sizeof(hip.L.SdAcceptResult) for i in range(len(n_accepted))]


def test_k2_hard_cases(hip):
    V, ld = 257, 260
    rows = torch.stack([LR.row("gauss", 70 + r, V) for r in range(5)])
    slab = torch.zeros(5, ld)
    slab[:, :V] = rows
    toks = [3, 100, 256, 0, 17]
    clean = _launch(hip, slab.cuda(), ld, V, 0, [(0, 5)], toks).cpu()
    assert all(LR.within_bar(float(g), LR.truth(rows[r], toks[r], 0)) for r, g in enumerate(clean))
    # a NaN in row 2 (not at the scored token): NaN there, the neighbours bit-equal to the clean launch
    bad = slab.clone()
    bad[2, 77] = float("nan")
    got = _launch(hip, bad.cuda(), ld, V, 0, [(0, 5)], toks).cpu()
    assert math.isnan(float(got[2])) and torch.equal(got[[0, 1, 3, 4]], clean[[0, 1, 3, 4]])
    # a row of nothing but -inf; a token of -1 and of V (the column past the row holds a finite value: it must not be read as x[t])
    bad = slab.clone()
    bad[1, :V] = float("-inf")
    bad[:, V:] = 1000.0
    got = _launch(hip, bad.cuda(), ld, V, 0, [(0, 5)], [3, 100, 256, -1, V]).cpu()
    assert math.isnan(float(got[1])) and math.isnan(float(got[3])) and math.isnan(float(got[4]))
    assert torch.equal(got[[0, 2]], clean[[0, 2]])
    # with a result block only rows r <= n_accepted are scored; the other floats keep their bits
    g = 4
    keep, ptrs = _res_blocks(hip, [0, 2, g])
    assert torch.equal(_launch(hip, slab.cuda(), ld, V, 0, [(0, g + 1)] * 3, toks * 3).cpu(), clean.repeat(3))   # (no block: every row)
    items = (hip.L.SdLogprobItem * 3)()
    dev, tok = slab.cuda(), torch.tensor(toks, dtype=torch.int32, device="cuda")
    out = torch.full((3, g + 1), SENTINEL, dtype=torch.int32, device="cuda")
    for i, it in enumerate(items):
        it.logits, it.ld, it.rows, it.tokens, it.res, it.out = dev.data_ptr(), ld, g + 1, tok.data_ptr(), ptrs[i], out[i].data_ptr()
    assert hip.lib.sd_token_logprobs(items, 3, V, 0, _st()) == 0
    torch.cuda.synchronize()
    for i, n_acc in enumerate([0, 2, g]):
        assert torch.equal(out[i, :n_acc + 1].view(torch.float32).cpu(), clean[:n_acc + 1]), n_acc
        assert out[i, n_acc + 1:].cpu().tolist() == [SENTINEL] * (g - n_acc), n_acc
    del keep
    # the refusals
    for bad_items, n, v in ((None, 1, V), (items, 0, V), (items, 17, V), (items, 3, ld + 1)):
        assert hip.lib.sd_token_logprobs(bad_items, n, v, 0, _st()) == hip.L.SD_ERR_INVALID
    for rows_bad in (0, 18):
        items[1].rows = rows_bad
        assert hip.lib.sd_token_logprobs(items, 3, V, 0, _st()) == hip.L.SD_ERR_INVALID
    torch.cuda.synchronize()
    assert out[0, 1:].cpu().tolist() == [SENTINEL] * g              # nothing was launched


# ----------------------------------------------------------------------------- L: the loops
def _truth(om, out, L):
    """float64 log-softmax of the oracle model's own logits over the finished output, at every new token; and the largest |logit|."""
    ids = out.cpu().to(torch.int64)
    logits = om(ids, use_cache=False).logits[0].double()
    lsm = torch.log_softmax(logits, dim=-1)
    return lsm[L - 1:-1].gather(-1, ids[0, L:, None])[:, 0], float(logits.abs().max())


def _check(om, out, lp, L, bar=FP32_BAR, rel=False, what=""):
    assert lp.dtype == torch.float32 and lp.device == out.device and tuple(lp.shape) == (1, out.shape[1] - L), (what, lp.shape, out.shape, L)
    want, scale = _truth(om, out, L)
    tol = bar * scale if rel else bar
    err = float((lp[0].cpu().double() - want).abs().max()) if want.numel() else 0.0
    print(f"{what}: {want.numel()} tokens, worst |logprob - truth| {err:.3g} (bar {tol:.3g})")
    assert err <= tol, (what, err, tol)


@functools.lru_cache(maxsize=None)
def _corr_oracles():
    dc, dsd, tc, tsd = _models("corr")[:4]
    return oracle.RefCausalLM(dc, dsd), oracle.RefCausalLM(tc, tsd)


@functools.lru_cache(maxsize=None)
def _two_ends():
    """Of _corr_case's prompts (gamma 4): one whose oracle run ends at the EOS and one whose run ends at its length."""
    prompts, eos, wants = _corr_case()
    by_eos, by_len = _ends(wants, eos)
    return by_eos.index(True), by_len.index(True)


@pytest.mark.parametrize("gamma", [1, 4, 16])
def test_l1_single_stream_against_the_oracle(hip, gamma):
    """fp32 `corr` pair; two prompts of the queue test's case, with its EOS: at gamma 4 one run ends by that EOS and one by
    max_len.  Tokens equal the oracle's on the same Philox stream; one score per new token; every score within 2e-3 of the
    float64 log-softmax of the oracle target's own logits."""
    prompts, eos, wants = _corr_case()
    dm, tm = _models("corr")[4:]
    ot = _corr_oracles()[1]
    kw = dict(KW, gamma=gamma)
    ends = []
    for i in _two_ends():
        want = wants[i] if gamma == 4 else _oracle(hip.lib, "corr", [prompts[i]], [SEEDS[i]], [BUDGETS[i]], eos, kw)[0]
        out, det, lp = hip.S.speculative_sampling(prompts[i].cuda(), dm, tm, eos, None, BUDGETS[i], details=True,
                                                  rng=hip.noise.DeviceNoise(SEEDS[i]), logprobs=True, **kw)
        assert torch.equal(out.cpu(), want[0]) and det["acc_len"] == want[1]["acc_len"]
        _check(ot, out, lp, LENS[i], what=f"gamma {gamma} prompt {i}")
        ends.append(int(out[0, -1]) == eos and out.shape[1] < LENS[i] + BUDGETS[i])
        out2, lp2 = hip.S.speculative_sampling(prompts[i].cuda(), dm, tm, eos, None, BUDGETS[i], rng=hip.noise.DeviceNoise(SEEDS[i]),
                                               logprobs=True, **kw)
        assert torch.equal(out2, out) and torch.equal(lp2, lp)    # (without details: tokens and scores alone)
    if gamma == 4:
        assert ends == [True, False]


def _check_all(om, outs, lps, lens, what, **kw):
    assert len(outs) == len(lps) == len(lens)
    for i, (o, lp, L) in enumerate(zip(outs, lps, lens)):
        _check(om, o, lp, L, what=f"{what} {i}", **kw)


def test_l2_batch_loop(hip):
    prompts, eos, _ = _corr_case()
    dm, tm = _models("corr")[4:]
    ps, seeds = prompts[2:6], SEEDS[2:6]
    wants = _oracle(hip.lib, "corr", ps, seeds, [12] * 4, eos, KW)
    outs, ds, lps = hip.S.speculative_sampling_batch([p.cuda() for p in ps], dm, tm, eos, None, 12, details=True, seeds=seeds,
                                                     logprobs=True, **KW)
    for (w, wd), o, d in zip(wants, outs, ds):
        assert torch.equal(o.cpu(), w) and d["acc_len"] == wd["acc_len"]
    _check_all(_corr_oracles()[1], outs, lps, LENS[2:6], "batch stream")


QUEUE_VARIANTS = {
    "plain": dict(),
    "per_prompt_params": dict(temperature=[1.0, 0.7, 1.3, 1.0, 0.9, 1.1, 1.0], top_k=[20, 0, 5, 40, 20, 1, 8],
                              top_p=[0.9, 0.8, 0.0, 0.95, 0.9, 0.5, 0.0]),
}


@pytest.mark.parametrize("variant", list(QUEUE_VARIANTS))
def test_l2_queue(hip, variant):
    """test_queue_equals_oracle_per_prompt's case - 7 prompts through 3 slots, prefill_chunk 8: slots change hands, streams end
    by EOS and by length - with scores: every prompt's scores land with that prompt (they fit ITS tokens' truth)."""
    prompts, eos, wants = _corr_case()
    dm, tm = _models("corr")[4:]
    kw = dict(KW, **QUEUE_VARIANTS[variant])
    args = ([p.cuda() for p in prompts], dm, tm, eos, None, BUDGETS)
    outs, ds, lps = hip.S.speculative_sampling_queue_logprobs(*args, details=True, seeds=SEEDS, slots=3, prefill_chunk=8, **kw)
    if variant == "plain":
        for (w, wd), o, d in zip(wants, outs, ds):
            assert torch.equal(o.cpu(), w) and d["acc_len"] == wd["acc_len"]
    base, bd = hip.S.speculative_sampling_queue(*args, details=True, seeds=SEEDS, slots=3, prefill_chunk=8, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, base)) and ds == bd
    _check_all(_corr_oracles()[1], outs, lps, LENS, f"queue[{variant}] prompt")
    outs2, lps2 = hip.S.speculative_sampling_queue_logprobs(*args, seeds=SEEDS, slots=3, prefill_chunk=8, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs2, outs)) and all(torch.equal(a, b) for a, b in zip(lps2, lps))


def test_l2_queue_shared_prefix(hip):
    dc, _, _, _, dm, tm = _models("corr")
    lens, budgets, seeds = [7, 9, 20, 12, 8], [10, 6, 12, 8, 10], [3100 + i for i in range(5)]
    prompts = _prompts(dc.vocab_size, lens, 1200)
    for p in prompts[1:]:
        p[0, :6] = prompts[0][0, :6]
    args = ([p.cuda() for p in prompts], dm, tm, -1, None, budgets)
    kw = dict(KW, seeds=seeds, slots=2, prefill_chunk=8, shared_prefix=6)
    t = {}
    outs, lps = hip.S.speculative_sampling_queue_logprobs(*args, _timing=t, **kw)
    assert t["copied_rows"] > 0
    base = hip.S.speculative_sampling_queue_shared(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(outs, base))
    _check_all(_corr_oracles()[1], outs, lps, lens, "shared-prefix prompt")


def test_l3_several_verify_passes_per_iteration(hip):
    """16 streams at gamma 16: 16 * 17 verify rows are more than one pass holds, every pass writes the same logit slab - the
    loop has to score a pass's streams before the next pass overwrites their rows."""
    dc, _, _, _, dm, tm = _models("corr")
    assert 16 * 17 > tm.new_session(8).max_pass_rows
    kw = dict(gamma=16, top_k=20, top_p=0.9)
    lens, seeds = [3 + (5 * i) % 11 for i in range(16)], [4200 + i for i in range(16)]
    prompts = [p.cuda() for p in _prompts(dc.vocab_size, lens, 1300)]
    outs, lps = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 20, seeds=seeds, logprobs=True, **kw)
    for p, s, o in zip(prompts, seeds, outs):
        assert torch.equal(o, hip.S.speculative_sampling(p, dm, tm, -1, None, 20, rng=hip.noise.DeviceNoise(s), **kw))
    _check_all(_corr_oracles()[1], outs, lps, lens, "16 x gamma 16 stream")


@contextlib.contextmanager
def _spy():
    """Records the KVCacheModels and DeviceNoise objects the wrappers open, so that a test can read the cache lengths and Philox
    positions a call leaves behind."""
    mods = [sys.modules["llmspeculativesampling_amd.sampling." + m] for m in ("speculative_sampling", "batch", "autoregressive_sampling")]
    seen = dict(kv=[], noise=[])
    saved = []

    def wrap(fn):
        def inner(*a, **k):
            r = fn(*a, **k)
            seen["kv"] += [x for x in r if hasattr(x, "_session")]
            return r
        return inner

    def noise_of(cls):
        def inner(*a, **k):
            n = cls(*a, **k)
            seen["noise"].append(n)
            return n
        return inner

    for m in mods:
        for name in ("open_stream", "open_spec_slot", "DeviceNoise"):
            if hasattr(m, name):
                saved.append((m, name, getattr(m, name)))
                setattr(m, name, (noise_of if name == "DeviceNoise" else wrap)(getattr(m, name)))
    try:
        yield seen
    finally:
        for m, name, fn in saved:
            setattr(m, name, fn)


def _state(seen, extra_noise=()):
    return ([kv._session.cache_len for kv in seen["kv"]], [(n.seed, n.draw) for n in list(seen["noise"]) + list(extra_noise)])


TIMES = ("approx_time", "target_time", "other_time", "target_model_time", "target_pre_cache_time", "target_post_prob_time")


def _untimed(d):
    return {k: v for k, v in d.items() if k not in TIMES} if isinstance(d, dict) else [_untimed(x) for x in d]


@pytest.mark.parametrize("family", ["single", "batch", "queue", "ar", "ar_batch"])
def test_l4_nothing_else_moves(hip, family):
    """logprobs=True against False with the same seeds: tokens, details (the measured times aside), Philox positions and cache
    lengths agree bit for bit."""
    dc, _, _, _, dm, tm = _models("corr")
    prompts = [p.cuda() for p in _prompts(dc.vocab_size, [9, 4, 17, 6, 11], 1400)]
    seeds = [5100 + i for i in range(5)]
    runs = []
    for on in (False, True):
        with _spy() as seen:
            mine = [hip.noise.DeviceNoise(seeds[0])]
            if family == "single":
                r = hip.S.speculative_sampling(prompts[0], dm, tm, 2, None, 14, details=True, rng=mine[0], logprobs=on, **KW)
            elif family == "batch":
                r = hip.S.speculative_sampling_batch(prompts[:4], dm, tm, 2, None, 14, details=True, seeds=seeds[:4], logprobs=on, **KW)
            elif family == "queue":
                f = hip.S.speculative_sampling_queue_logprobs if on else hip.S.speculative_sampling_queue_shared
                r = f(prompts, dm, tm, 2, None, [14, 6, 9, 12, 7], details=True, seeds=seeds, slots=2, prefill_chunk=8, **KW)
            elif family == "ar":
                r = hip.S.autoregressive_sampling(prompts[0], tm, 14, 2, top_k=20, top_p=0.9, rng=mine[0], logprobs=on)
                r = (r, {}) if not on else (r[0], {}, r[1])
            else:
                r = hip.S.autoregressive_sampling_batch(prompts[:3], tm, 14, 2, top_k=20, top_p=0.9, seeds=seeds[:3], logprobs=on)
                r = (r, {}) if not on else (r[0], {}, r[1])
            runs.append((r, _state(seen, mine)))
    (off, off_state), (on, on_state) = runs
    assert len(on) == len(off) + 1
    toks = lambda x: [x] if isinstance(x, torch.Tensor) else list(x)
    assert all(torch.equal(a, b) for a, b in zip(toks(off[0]), toks(on[0]))) and len(toks(off[0])) == len(toks(on[0]))
    assert _untimed(off[1]) == _untimed(on[1])
    assert off_state == on_state and off_state[0] and off_state[1]
    assert all(lp.shape[1] == o.shape[1] - p.shape[1] for lp, o, p in zip(toks(on[2]), toks(on[0]), prompts))


@functools.lru_cache(maxsize=None)
def _bf16_pair():
    from llmspeculativesampling_amd import engine
    cfg = ModelConfig(**BF16_CFG)
    dsd = make_state_dict(cfg, 5, dtype=torch.bfloat16)
    tsd = {k: v.to(torch.bfloat16) for k, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    return (cfg, engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.bfloat16),
            engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.bfloat16),
            oracle.RefCausalLM(cfg, {k: v.float() for k, v in tsd.items()}))


def test_l4_dense_tail_and_fused_tail_score_the_same_slab(hip):
    """SD_BATCH_FUSED_TAIL=0 against the default on a bf16 pair, scores on: both tails read the same logit slab, so tokens and
    scores are bit-equal."""
    cfg, dm, tm, _ = _bf16_pair()
    prompts = [p.cuda() for p in _prompts(cfg.vocab_size, [12, 5, 20, 9], 1500)]
    runs = []
    old = os.environ.get("SD_BATCH_FUSED_TAIL")
    try:
        for tail in (None, "0"):
            os.environ.pop("SD_BATCH_FUSED_TAIL", None)
            if tail is not None:
                os.environ["SD_BATCH_FUSED_TAIL"] = tail
            runs.append(hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 12, seeds=[61, 62, 63, 64], logprobs=True, **KW))
    finally:
        os.environ.pop("SD_BATCH_FUSED_TAIL", None)
        if old is not None:
            os.environ["SD_BATCH_FUSED_TAIL"] = old
    (o1, l1), (o2, l2) = runs
    assert all(torch.equal(a, b) for a, b in zip(o1, o2)) and all(torch.equal(a, b) for a, b in zip(l1, l2))
    assert all(lp.shape[1] >= 12 for lp in l1)


def test_l5_bf16_pair_against_an_fp32_truth(hip):
    """The bf16 pair, one stream and four; the truth is the fp32 oracle forward of the same (bf16-valued) target weights.  Bar:
    2 x the bf16 logit bar of test_gpu_parity.py (0.04 x the largest |logit| of the truth), for the reason FP32_BAR gives."""
    cfg, dm, tm, ot = _bf16_pair()
    lens = [12, 5, 20, 9]
    prompts = [p.cuda() for p in _prompts(cfg.vocab_size, lens, 1500)]
    out, lp = hip.S.speculative_sampling(prompts[0], dm, tm, -1, None, 12, rng=hip.noise.DeviceNoise(61), logprobs=True, **KW)
    _check(ot, out, lp, lens[0], bar=2 * 0.04, rel=True, what="bf16 single stream")
    outs, lps = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 12, seeds=[61, 62, 63, 64], logprobs=True, **KW)
    _check_all(ot, outs, lps, lens, "bf16 batch stream", bar=2 * 0.04, rel=True)


def test_l6_autoregressive(hip):
    """One stream fed a prompt longer than one chunk of the model's rows (an fp32 model that holds 512 positions), and three
    streams of the `corr` target; fp32; the one model is the target."""
    cfg = ModelConfig(**BF16_CFG)
    sd = make_state_dict(cfg, 9)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    long_L = 300
    assert m.new_session(8).max_rows < long_L
    p = _prompts(cfg.vocab_size, [long_L], 1600)[0].cuda()
    out, lp = hip.S.autoregressive_sampling(p, m, 8, -1, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(71), logprobs=True)
    assert out.shape[1] == long_L + 8
    _check(oracle.RefCausalLM(cfg, sd), out, lp, long_L, what="autoregressive, long prompt")
    dc, _, tc, _, dm, tm = _models("corr")
    ot = _corr_oracles()[1]
    lens = [5, 13, 2]
    ps = [q.cuda() for q in _prompts(tc.vocab_size, lens, 1700)]
    eos = int(hip.S.autoregressive_sampling(ps[0], tm, 10, -1, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(81))[0, lens[0] + 4])
    outs, lps = hip.S.autoregressive_sampling_batch(ps, tm, 10, eos, top_k=20, top_p=0.9, seeds=[81, 82, 83], logprobs=True)
    assert outs[0].shape[1] <= lens[0] + 5                        # stream 0 ends at its EOS, the others go on
    _check_all(ot, outs, lps, lens, "autoregressive stream")


def test_l7_the_score(hip):
    """score_from_logprobs of an L1 run against quality.get_score of its output: each side is within 2e-3 of the truth."""
    prompts, eos, _ = _corr_case()
    dm, tm = _models("corr")[4:]
    i = _two_ends()[1]
    out, lp = hip.S.speculative_sampling(prompts[i].cuda(), dm, tm, eos, None, BUDGETS[i], rng=hip.noise.DeviceNoise(SEEDS[i]),
                                         logprobs=True, **KW)
    a, b = float(hip.quality.score_from_logprobs(lp)), float(hip.quality.get_score(out, tm, LENS[i]))
    print("score from the loop", a, "get_score", b)
    assert abs(a - b) <= 4e-3
