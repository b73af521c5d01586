"""Continuous batching (`pytest -m gpu`): speculative_sampling_queue / sd_spec_queue_generate - a prompt queue behind the
slots of the lock-step speculative loop - held per prompt to the CPU oracle fed the device's Philox variates
(tests/philox_replay.py), to the single-stream loop and to speculative_sampling_batch; and the mixed pass it rests on (verify
rows of several streams plus prompt rows without logits in one sd_batch_forward) held to per-stream forwards."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from philox_replay import PhiloxOracleNoise
from test_gpu_native_parity import BF16_CFG, DETAILS_KEYS, _pair, _st
from test_gpu_parity import MID_CFGS
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

pytestmark = pytest.mark.gpu

KW = dict(gamma=4, top_k=20, top_p=0.9)


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


def _prompts(V, lens, seed):
    return [torch.from_numpy(np.random.default_rng(seed + i).integers(3, V, size=(1, L))) for i, L in enumerate(lens)]


@functools.lru_cache(maxsize=None)
def _models(kind):
    from llmspeculativesampling_amd import engine
    dc, dsd, tc, tsd = _pair(kind, seed=21)
    return (dc, dsd, tc, tsd, engine.SpecDecModel.from_state_dict(dc, dsd, dtype=torch.float32),
            engine.SpecDecModel.from_state_dict(tc, tsd, dtype=torch.float32))


def _oracle(lib, kind, prompts, seeds, budgets, eos, kw):
    dc, dsd, tc, tsd = _models(kind)[:4]
    od, ot = oracle.RefCausalLM(dc, dsd), oracle.RefCausalLM(tc, tsd)
    return [oracle.speculative_sampling(p, od, ot, eos, None, m, details=True, noise=PhiloxOracleNoise(lib, s, kw["gamma"], _st), **kw)
            for p, s, m in zip(prompts, seeds, budgets)]


def _assert_equals_oracle(wants, outs, ds):
    for i, ((want, wd), got, gd) in enumerate(zip(wants, outs, ds)):
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy(), err_msg=f"prompt {i}")
        assert gd["acc_len"] == wd["acc_len"], i
        assert gd["target_call_times"] == wd["target_call_times"] and gd["approx_call_times"] == wd["approx_call_times"], i
        assert set(gd) == DETAILS_KEYS


# ----------------------------------------------------------------------------- 1 / 2: token-exact against the oracle
LENS, BUDGETS = [1, 2, 9, 40, 13, 5, 23], [24, 6, 12, 6, 24, 6, 12]
SEEDS = [7100 + i for i in range(7)]


@functools.lru_cache(maxsize=None)
def _corr_case():
    """The seven prompts of test 1, the EOS id and the oracle's runs with it.  The EOS is a token the oracle generates: the
    first id, scanning the EOS-free runs of the prompts whose slots are reused (the first four of seven in three slots) in
    order, that ends at least one of those four early and leaves at least one of them to run to its length."""
    from llmspeculativesampling_amd import _lib
    V = _models("corr")[0].vocab_size
    prompts = _prompts(V, LENS, 300)
    free = _oracle(_lib.lib, "corr", prompts, SEEDS, BUDGETS, -1, KW)
    gen = [w[0][0, L:].tolist() for w, L in zip(free, LENS)]
    for cand in [t for g in gen[:4] for t in g[:-1]]:
        early = [cand in g[:m - 1] for g, m in zip(gen[:4], BUDGETS)]      # (before the budget's last token: a real early stop)
        if any(early) and not all(cand in g for g in gen[:4]) and not any(cand in p[0].tolist() for p in prompts):
            return prompts, cand, _oracle(_lib.lib, "corr", prompts, SEEDS, BUDGETS, cand, KW)
    raise AssertionError("no token of the first four runs serves as EOS")


def _ends(wants, eos):
    by_eos = [int(w[0][0, -1]) == eos and w[0].shape[1] < L + m for w, L, m in zip(wants, LENS, BUDGETS)]
    by_len = [w[0].shape[1] >= L + m for w, L, m in zip(wants, LENS, BUDGETS)]
    return by_eos, by_len


@pytest.mark.parametrize("slots", [3, 1])
def test_queue_equals_oracle_per_prompt(hip, slots):
    """7 prompts of lengths 1 .. 40 through 3 slots (and through 1), prefill_chunk 8: the 40-token prompt joins over several
    iterations, a 1-token prompt joins at once, streams end at EOS and at their length and later prompts take both kinds of
    slot.  Tokens, acc_len and call counts of every prompt equal the oracle's on that prompt's own Philox stream."""
    prompts, eos, wants = _corr_case()
    by_eos, by_len = _ends(wants, eos)
    assert any(by_eos[:4]) and any(by_len[:4]), (by_eos, by_len)  # both kinds of end free a slot that a later prompt takes
    dm, tm = _models("corr")[4:]
    t = {}
    outs, ds = hip.S.speculative_sampling_queue([p.cuda() for p in prompts], dm, tm, eos, None, BUDGETS, details=True, seeds=SEEDS,
                                                slots=slots, prefill_chunk=8, _timing=t, **KW)
    _assert_equals_oracle(wants, outs, ds)
    calls = [wd["target_call_times"] for _, wd in wants]
    assert t["iterations"] == len(t["verify"]) and max(calls) <= t["iterations"] <= sum(calls)
    assert (t["iterations"] == sum(calls)) == (slots == 1)        # one slot: one stream at a time; three: they overlap
    assert all(a <= f for a, f in zip(t["admit_iter"], t["finish_iter"]))
    assert t["admit_iter"][0] == 0 and t["admit_iter"] == sorted(t["admit_iter"])                    # FIFO
    if slots == 3:
        # the 1-token prompt decodes at once, so the other two join beside it, 8 prompt rows a pass between them: prompt 1's one
        # row rides iteration 0 with 7 of prompt 2's eight, whose last rides iteration 1
        start = [0, 1, 2]
        assert t["admit_iter"][:3] == start
        ends = [s0 + c for s0, c in zip(start, calls)]            # the boundary at which each of the three frees its slot
        print("calls", calls, "admit", t["admit_iter"], "finish", t["finish_iter"], "ends", (by_eos, by_len))
        if max(ends) >= min(ends) + 5:
            # the 40-token prompt takes the first slot that comes free; its 39 target rows ride 5 verify passes at 8 a pass next
            # to a stream that is still running (the oracle's call counts say one is), then it decodes
            assert t["admit_iter"][3] == min(ends) + 5


def test_queue_equals_oracle_opt_pair(hip):
    dc = _models("opt")[0]
    lens, budgets, seeds = [6, 1, 19, 11], [10, 8, 6, 12], [51, 52, 53, 54]
    prompts = _prompts(dc.vocab_size, lens, 500)
    wants = _oracle(hip.lib, "opt", prompts, seeds, budgets, 2, KW)
    dm, tm = _models("opt")[4:]
    outs, ds = hip.S.speculative_sampling_queue([p.cuda() for p in prompts], dm, tm, 2, None, budgets, details=True, seeds=seeds,
                                                slots=2, prefill_chunk=8, **KW)
    _assert_equals_oracle(wants, outs, ds)


def test_queue_equals_oracle_with_random_seed(hip):
    """The reseed quirk (every uniform of the call is torch.Generator(42).rand(1), the stream restarts at (42, 0) before the
    residual sample), as in the batch loop."""
    kw = dict(KW, random_seed=42)
    dc = _models("corr")[0]
    lens, budgets, seeds = [3, 17, 8, 1, 12], [12, 6, 10, 8, 6], [61, 62, 63, 64, 65]
    prompts = _prompts(dc.vocab_size, lens, 600)
    wants = _oracle(hip.lib, "corr", prompts, seeds, budgets, 2, kw)
    dm, tm = _models("corr")[4:]
    outs, ds = hip.S.speculative_sampling_queue([p.cuda() for p in prompts], dm, tm, 2, None, budgets, details=True, seeds=seeds,
                                                slots=2, prefill_chunk=8, **kw)
    _assert_equals_oracle(wants, outs, ds)


# ----------------------------------------------------------------------------- 3: nothing to queue
def test_queue_with_a_slot_per_prompt_equals_the_batch_loop(hip):
    dc, _, _, _, dm, tm = _models("corr")
    prompts = [p.cuda() for p in _prompts(dc.vocab_size, [9, 30, 2, 17], 700)]
    seeds = [900 + i for i in range(4)]
    want, wd = hip.S.speculative_sampling_batch(prompts, dm, tm, 2, None, 16, details=True, seeds=seeds, **KW)
    for slots in (4, 16):
        got, gd = hip.S.speculative_sampling_queue(prompts, dm, tm, 2, None, 16, details=True, seeds=seeds, slots=slots, **KW)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert gd == wd
    assert [o.shape for o in hip.S.speculative_sampling_queue(prompts, dm, tm, 2, None, 16, seeds=seeds, slots=4, **KW)] == \
        [o.shape for o in want]                                   # (without details: the list alone)


# ----------------------------------------------------------------------------- 4: passes without room
def _singles(hip, prompts, dm, tm, eos, budgets, seeds, kw):
    return [hip.S.speculative_sampling(p, dm, tm, eos, None, m, details=True, rng=hip.noise.DeviceNoise(s), **kw)
            for p, m, s in zip(prompts, budgets, seeds)]


@pytest.mark.parametrize("slots,n", [(8, 10), (9, 11)], ids=["slots8", "slots9_verify_pass_is_full"])
def test_queue_without_room_in_the_verify_pass(hip, slots, n):
    """gamma 8.  slots 8, N 10: 8 x 9 = 72 verify rows are more than the 64 logit rows a mixed pass may hold; at least one pass
    carries prompt rows only, and every prompt equals its single-stream run.  (With 8 slots a joiner sits next to at most 7
    streams = 63 logit rows, so its rows do ride; the prompt-only passes are the call's first prefill.)  slots 9, N 11: a
    joiner sits next to 8 streams = 72 logit rows, its verify pass takes no prompt row, and the progress guarantee's extra
    pass inside the loop carries them."""
    dc, _, _, _, dm, tm = _models("corr")
    kw = dict(gamma=8, top_k=20, top_p=0.9)
    lens = [4 + 3 * (i % 5) for i in range(n)]
    # prompt 0 is done after at most 2 iterations, the others need at least 4 (an iteration gives 1 .. 9 tokens): whoever takes
    # its slot joins next to `slots - 1` running streams
    budgets = [2 if i == 0 else 28 + i % 3 for i in range(n)]
    seeds = [1300 + i for i in range(n)]
    prompts = [p.cuda() for p in _prompts(dc.vocab_size, lens, 800)]
    t = {}
    outs, ds = hip.S.speculative_sampling_queue(prompts, dm, tm, -1, None, budgets, details=True, seeds=seeds, slots=slots, _timing=t,
                                                **kw)
    print("passes", {k: t[k] for k in ("iterations", "target_passes", "draft_passes", "extra_passes", "prefill_passes")})
    assert t["extra_passes"] >= 1
    if slots == 9:
        assert t["extra_passes"] - t["prefill_passes"] >= 1
    for (so, sdet), o, d in zip(_singles(hip, prompts, dm, tm, -1, budgets, seeds, kw), outs, ds):
        assert torch.equal(so, o)
        assert sdet["acc_len"] == d["acc_len"] and sdet["target_call_times"] == d["target_call_times"]


# ----------------------------------------------------------------------------- 5: slots are refilled
def test_queue_refills_slots(hip):
    """12 prompts, 4 slots, every fourth prompt long (40 tokens), the others short (4): as three calls of four streams the
    work costs c_0 + c_4 + c_8 iterations (each call waits for its long stream); the queue starts prompt 4 while prompt 0
    still runs and needs fewer - and no fewer than the streams' calls spread evenly over 4 slots."""
    dc, _, _, _, dm, tm = _models("corr")
    lens = list(range(5, 17))
    budgets = [40 if i % 4 == 0 else 4 for i in range(12)]
    seeds = [2100 + i for i in range(12)]
    prompts = _prompts(dc.vocab_size, lens, 900)
    wants = _oracle(hip.lib, "corr", prompts, seeds, budgets, -1, KW)
    c = [wd["target_call_times"] for _, wd in wants]
    assert all(ci >= 8 for ci in c[::4]) and all(ci <= 4 for i, ci in enumerate(c) if i % 4)      # 1 .. 5 tokens per iteration
    t = {}
    outs, ds = hip.S.speculative_sampling_queue([p.cuda() for p in prompts], dm, tm, -1, None, budgets, details=True, seeds=seeds,
                                                slots=4, _timing=t, **KW)
    _assert_equals_oracle(wants, outs, ds)
    print("iterations", t["iterations"], "calls", c, "admit", t["admit_iter"], "finish", t["finish_iter"])
    assert t["admit_iter"][4] < t["finish_iter"][0]
    assert math.ceil(sum(c) / 4) <= t["iterations"] < c[0] + c[4] + c[8]


# ----------------------------------------------------------------------------- 6: the mixed pass itself
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_forward_verify_rows_plus_prompt_rows_without_logits(hip, dtype):
    """One sd_batch_forward as the queue issues it: 3 streams x 5 verify rows (all logit rows) and, behind them, one item of
    13 prompt rows with n_logits = 0.  Logits and the joiner's K / V rows against each stream's own sd_session_forward, by the
    method and bar of test_gpu_parity.test_batch_forward_equals_per_stream_forward (fp32: bit-equal; bf16: 0.03 of the
    largest logit, K / V within 0.05)."""
    cfg = ModelConfig(**MID_CFGS["llama_d64_gqa"]) if dtype == torch.bfloat16 else load_config("tiny-llama-target")
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, 31, dtype=dtype), dtype=dtype)
    rng = np.random.default_rng(9)
    lens, new, nlog = [17, 40, 9, 4], [5, 5, 5, 13], [5, 5, 5, 0]       # (the joiner: a second chunk, 4 of its rows are cached)
    seqs = [torch.from_numpy(rng.integers(3, cfg.vocab_size, size=(L + n,)).astype(np.int32)).cuda() for L, n in zip(lens, new)]
    solo = [m.new_session(96) for _ in lens]
    both = [m.new_session(96) for _ in lens]
    want = []
    for ses, ses2, sq, L, n, nl in zip(solo, both, seqs, lens, new, nlog):
        ses.forward(sq[:L], 0)
        ses2.forward(sq[:L], 0)
        want.append(ses.forward(sq[L:L + n], nl).clone())
    got = hip.engine.batch_forward(both, seqs, new, nlog).clone()
    want = torch.cat(want, 0)
    assert got.shape == want.shape == (15, cfg.vocab_size)
    if dtype == torch.float32:
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 0.03 * float(want.abs().max())
    for a, b, L, n in zip(solo, both, lens, new):
        assert a.cache_len == b.cache_len == L + n
        for (ka, va), (kb, vb) in zip(a.past_key_values(), b.past_key_values()):
            for x, y in ((ka, kb), (va, vb)):
                assert torch.equal(x, y) if dtype == torch.float32 else float((x.float() - y.float()).abs().max()) < 0.05


# ----------------------------------------------------------------------------- 7: a 16-bit pair
def test_queue_bf16_pair_shapes_and_ranges(hip):
    """bf16 claims no token-exactness against another pass composition: the prompt is preserved, every
    output has between max_len and max_len + gamma new tokens or is cut after its first new EOS, acc_len lies in 0..gamma."""
    cfg = ModelConfig(**BF16_CFG)
    dsd = make_state_dict(cfg, 5, dtype=torch.bfloat16)
    tsd = {k: v.to(torch.bfloat16) for k, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.bfloat16)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.bfloat16)
    gamma, lens, budgets = 4, [12, 1, 33, 7, 20], [16, 8, 8, 24, 8]
    prompts = [p.cuda() for p in _prompts(cfg.vocab_size, lens, 1000)]
    probe = hip.S.speculative_sampling_queue(prompts[:1], dm, tm, -1, None, 16, seeds=[77], slots=1, **KW)
    eos = int(probe[0][0, lens[0] + 5])                           # a token prompt 0 is likely to produce again
    t = {}
    outs, ds = hip.S.speculative_sampling_queue(prompts, dm, tm, eos, None, budgets, details=True, seeds=[77, 78, 79, 80, 81], slots=2,
                                                prefill_chunk=8, _timing=t, **KW)
    for p, o, d, L, m in zip(prompts, outs, ds, lens, budgets):
        assert torch.equal(o[:, :L], p)
        n_eos = int((o[0] == eos).sum()) - int((p[0] == eos).sum())
        if n_eos:
            assert n_eos == 1 and int(o[0, -1]) == eos and o.shape[1] <= L + m + gamma
        else:
            assert L + m <= o.shape[1] <= L + m + gamma
        assert d["acc_len"] and all(0 <= a <= gamma for a in d["acc_len"]) and d["target_call_times"] == len(d["acc_len"])
    assert t["iterations"] >= max(len(d["acc_len"]) for d in ds)
