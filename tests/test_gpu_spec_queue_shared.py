"""The prompt queue with a shared prompt prefix (`pytest -m gpu`): speculative_sampling_queue_shared(shared_prefix=P) /
sd_spec_queue_generate with donor sessions - the prefix goes through each model once, into a donor pair of sessions, and every admitted
prompt starts on a copy of its K / V rows.  Held per prompt to the CPU oracle on that prompt's own Philox stream and to the
same call without sharing; the row and pass counts are derived from the prompt lengths, not measured."""
import functools

import pytest
import torch

from test_gpu_native_parity import BF16_CFG
from test_gpu_spec_queue import KW, _assert_equals_oracle, _models, _oracle, _prompts
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

pytestmark = pytest.mark.gpu

# P = 9 is no multiple of the 8-row attention group: the rest of a prompt starts inside a group.  Two prompts have L == P (only
# P - 1 rows are copied: the last token is a decode row), one has budget 0 (L >= T: finished at admission, it takes no slot).
P, LENS, BUDGETS = 9, [9, 10, 16, 29, 9, 41], [12, 6, 24, 6, 0, 12]
SEEDS = [8100 + i for i in range(6)]
EOS = 2
COUNTS = ("iterations", "target_passes", "draft_passes", "extra_passes", "prefill_passes", "prompt_rows", "copied_rows",
          "admit_iter", "finish_iter")


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine)


def _shared_prompts(V, lens, seed, p=P):
    ps = _prompts(V, lens, seed)
    for q in ps[1:]:
        q[0, :p] = ps[0][0, :p]
    return ps


@functools.lru_cache(maxsize=None)
def _case(kind):
    """The six prompts and the oracle's run of each (computed once; the slot counts share it)."""
    from llmspeculativesampling_amd import _lib
    prompts = _shared_prompts(_models(kind)[0].vocab_size, LENS, 1100)
    return prompts, _oracle(_lib.lib, kind, prompts, SEEDS, BUDGETS, EOS, KW)


@pytest.mark.parametrize("slots", [2, 1])
@pytest.mark.parametrize("kind", ["corr", "opt"])
def test_shared_prefix_equals_oracle_and_the_unshared_call(hip, kind, slots):
    prompts, wants = _case(kind)
    dm, tm = _models(kind)[4:]
    run = lambda t, **kw: hip.S.speculative_sampling_queue_shared([p.cuda() for p in prompts], dm, tm, EOS, None, BUDGETS, details=True,   # noqa: E731
                                                           seeds=SEEDS, slots=slots, prefill_chunk=8, _timing=t, **kw, **KW)
    ts, t0 = {}, {}
    outs, ds = run(ts, shared_prefix=P)
    plain, pd = run(t0, shared_prefix=0)
    print("shared", {k: ts[k] for k in COUNTS}, "\nplain ", {k: t0[k] for k in COUNTS})
    _assert_equals_oracle(wants, outs, ds)
    for a, b, da, db in zip(outs, plain, ds, pd):
        assert torch.equal(a, b)
        assert da["acc_len"] == db["acc_len"] and da["target_call_times"] == db["target_call_times"]
    # the counts follow from the lengths: a prompt that takes a slot copies c = min(P, L - 1) rows per model and forwards the
    # other L - 1 - c; the donors forward P' = min(P, max L - 1) rows once
    admitted = [L for L, m in zip(LENS, BUDGETS) if m > 0]
    p_rows = min(P, max(LENS) - 1)
    assert p_rows == P and len(admitted) == 5
    assert ts["copied_rows"] == sum(min(P, L - 1) for L in admitted) == 44
    assert ts["prompt_rows"] == p_rows + sum(L - 1 - min(P, L - 1) for L in admitted) == 65
    assert t0["copied_rows"] == 0 and t0["prompt_rows"] == sum(L - 1 for L in admitted) == 100
    assert ts["target_passes"] <= t0["target_passes"]
    assert ts["admit_iter"][:2] == ([0, 0] if slots == 2 else [0, ds[0]["target_call_times"]])   # c == L - 1: active at its boundary
    assert ts["admit_iter"][4] == ts["finish_iter"][4] and outs[4].shape[1] == LENS[4]       # the budget-0 prompt never decodes


def test_shared_prefix_zero_is_the_plain_queue(hip):
    """speculative_sampling_queue, speculative_sampling_queue_shared without the argument and with shared_prefix=0: the same
    tokens and the same counts."""
    prompts, _ = _case("corr")
    dm, tm = _models("corr")[4:]
    calls = [(hip.S.speculative_sampling_queue, {}), (hip.S.speculative_sampling_queue_shared, {}),
             (hip.S.speculative_sampling_queue_shared, dict(shared_prefix=0))]
    ts = [{} for _ in calls]
    outs = [fn([p.cuda() for p in prompts], dm, tm, EOS, None, BUDGETS, seeds=SEEDS, slots=2, prefill_chunk=8, _timing=t, **kw, **KW)
            for t, (fn, kw) in zip(ts, calls)]
    for other, t in zip(outs[1:], ts[1:]):
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
        assert {k: ts[0][k] for k in COUNTS} == {k: t[k] for k in COUNTS}


def test_shared_prefix_longer_than_every_cacheable_row(hip):
    """Every prompt IS the prefix (L == P for all): the donors hold P' = P - 1 rows, each prompt copies them and decodes at its
    boundary - no prompt row is forwarded outside the donors."""
    dc, _, _, _, dm, tm = _models("corr")
    prompts = _shared_prompts(dc.vocab_size, [P, P, P], 1200)
    seeds, budgets = [31, 32, 33], [6, 10, 6]
    wants = _oracle(hip.lib, "corr", prompts, seeds, budgets, EOS, KW)
    t = {}
    outs, ds = hip.S.speculative_sampling_queue_shared([p.cuda() for p in prompts], dm, tm, EOS, None, budgets, details=True, seeds=seeds,
                                                slots=2, _timing=t, shared_prefix=P, **KW)
    _assert_equals_oracle(wants, outs, ds)
    assert (t["prompt_rows"], t["copied_rows"], t["prefill_passes"], t["extra_passes"]) == (P - 1, 3 * (P - 1), 1, 1)


def test_shared_prefix_bf16_pair_shapes_and_ranges(hip):
    """As test_queue_bf16_pair_shapes_and_ranges: bf16 claims no token-exactness against another pass composition - the prompt is
    preserved, every output has between max_len and max_len + gamma new tokens or is cut after its first new EOS, the token ids
    are in range, acc_len lies in 0..gamma."""
    cfg = ModelConfig(**BF16_CFG)
    dsd = make_state_dict(cfg, 5, dtype=torch.bfloat16)
    tsd = {k: v.to(torch.bfloat16) for k, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.bfloat16)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.bfloat16)
    gamma, lens, budgets = 4, [12, 9, 33, 10, 20], [16, 8, 8, 24, 8]
    prompts = [p.cuda() for p in _shared_prompts(cfg.vocab_size, lens, 1300)]
    probe = hip.S.speculative_sampling_queue_shared(prompts[:1], dm, tm, -1, None, 16, seeds=[77], slots=1, **KW)
    eos = int(probe[0][0, lens[0] + 5])                           # a token prompt 0 is likely to produce again
    t = {}
    outs, ds = hip.S.speculative_sampling_queue_shared(prompts, dm, tm, eos, None, budgets, details=True, seeds=[77, 78, 79, 80, 81], slots=2,
                                                prefill_chunk=8, _timing=t, shared_prefix=P, **KW)
    for p, o, d, L, m in zip(prompts, outs, ds, lens, budgets):
        assert torch.equal(o[:, :L], p)
        assert int(o.min()) >= 0 and int(o.max()) < cfg.vocab_size
        n_eos = int((o[0] == eos).sum()) - int((p[0] == eos).sum())
        if n_eos:
            assert n_eos == 1 and int(o[0, -1]) == eos and o.shape[1] <= L + m + gamma
        else:
            assert L + m <= o.shape[1] <= L + m + gamma
        assert d["acc_len"] and all(0 <= a <= gamma for a in d["acc_len"]) and d["target_call_times"] == len(d["acc_len"])
    assert t["copied_rows"] == sum(min(P, L - 1) for L in lens) and t["prompt_rows"] == P + sum(L - 1 - min(P, L - 1) for L in lens)
