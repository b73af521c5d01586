"""Per-request temperature / top_k / top_p (`pytest -m gpu`): sd_norm_batch_rows and the lock-step loops behind
speculative_sampling_batch / speculative_sampling_queue / speculative_sampling_queue_shared.

K1 / K2 hold a row of a mixed launch to the SCALAR launch of that row alone with its own triple, bit for bit - the scalar
entries are pinned to the oracle by test_gpu_sampler_routes.py and test_norm_probs_many_rows_vs_oracle - and fp32 rows to the
oracle directly under those bars (check_probs of test_gpu_sampler_routes, imported, not restated).  L1 - L4 hold every prompt
of a mixed call to the CPU oracle fed that prompt's own Philox variates (tests/philox_replay.py) and to the single-stream
loop, token for token.

The fp32 pairs of L1 / L2 reach entry A in the loop (V = 8192, a workspace) but never entry B: the head leaves tile maxima
for 16-bit models only.  Entry B under per-request parameters is covered by K2 at kernel level and by L5 in the loop: a bf16
pair whose fused tail (tile maxima in the passes that allow them) must equal SD_BATCH_FUSED_TAIL=0 bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import oracle
import sampler_rows as R
from golden_io import logits_row
from philox_replay import PhiloxOracleNoise
from test_gpu_native_parity import BF16_CFG, DETAILS_KEYS, _st
from test_gpu_sampler_routes import CL_INTS, check_probs, launch
from test_gpu_spec_queue import _models, _prompts
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

pytestmark = pytest.mark.gpu

# (temperature, top_k, top_p), cycled over rows / prompts
P = [(1.0, 20, 0.9), (0.7, 0, 0.95), (1.0, 0, 0.0), (1.3, 1, 0.0), (0.5, 64, 0.5), (1.0, 65, 0.9), (2.0, 200, 0.0),
     (-1.0, 20, 0.9)]                                             # the last: entry A eligible, entry B not
# every row can take entry B (and A): different T > 0, k in 1..64, p
P_ELIGIBLE = [(1.0, 20, 0.9), (0.7, 1, 0.0), (1.3, 64, 0.5), (0.5, 5, 0.95), (2.0, 33, 0.0)]


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


def _eligible_a(k):
    return 1 <= k <= 64


# ----------------------------------------------------------------------------- K1: rows
N_MAX = 49                                                        # one row past the 48-row launch boundary


@functools.lru_cache(maxsize=None)
def _rows_input(V, dt):
    """49 logit rows as the dtype mode sees them (values of the dtype, carried as fp32): (CPU fp32, device)."""
    x = torch.cat([logits_row(7000 + i, V, 3.0) for i in range(N_MAX)], 0)
    x = R.as_dtype(x, dt).float().contiguous()
    return x, x.cuda()


def _buffers(n, V, fill=7.0):
    return dict(out=torch.full((n, V), fill, device="cuda"), err=torch.full((n,), -1, dtype=torch.int32, device="cuda"),
                tok=torch.full((n,), -1, dtype=torch.int32, device="cuda"), serr=torch.full((n,), -1, dtype=torch.int32, device="cuda"))


def _norm_rows(hip, b, r0, n):
    """the SdNormRow array of rows [r0, r0 + n) writing into rows [0, n) of the buffers `b`; row r draws (seed 500 + r, draw r)"""
    rows = (hip.L.SdNormRow * n)()
    for i, it in enumerate(rows):
        it.probs_out = b["out"][i].data_ptr()
        it.err = b["err"][i:].data_ptr()
        it.tok_out = b["tok"][i:].data_ptr()
        it.sample_err = b["serr"][i:].data_ptr()
        it.philox_seed, it.draw_index = 500 + r0 + i, r0 + i
    return rows


def _params(hip, table, n):
    return (hip.L.SdRowSampling * n)(*[hip.L.SdRowSampling(*table[i % len(table)]) for i in range(n)])


@functools.lru_cache(maxsize=None)
def _scalar_rows(V, dt, use_ws, sample):
    """The reference, once per setting: row r through the existing scalar sd_norm_batch ALONE with P[r % 8]."""
    from llmspeculativesampling_amd import _lib
    import types
    hip = types.SimpleNamespace(L=_lib, lib=_lib.lib)
    _, xd = _rows_input(V, dt)
    b = _buffers(N_MAX, V)
    ws = torch.zeros(_lib.lib.sd_norm_workspace_bytes(1), dtype=torch.uint8, device="cuda") if use_ws else None
    for r in range(N_MAX):
        T, k, p = P[r % len(P)]
        one = {name: t[r:r + 1] for name, t in b.items()}
        _lib.check(_lib.lib.sd_norm_batch(xd[r].data_ptr(), 1, V, V, T, k, p, R.DT_MODE[dt], _norm_rows(hip, one, r, 1), sample,
                                          ws.data_ptr() if use_ws else None, _st()), "sd_norm_batch")
    torch.cuda.synchronize()
    return {name: t.cpu() for name, t in b.items()}


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", [8192, 512], ids=["V8192_fast_entries", "V512_none"])
def test_rows_equal_their_scalar_launches(hip, V, dt):
    """K1.  Row r of ONE sd_norm_batch_rows call == sd_norm_batch of row r alone with P[r]: probability row, error word, token,
    sample error word, bit for bit - 1, 5, 48 and 49 rows, with and without a workspace, with and without the fused sample."""
    _, xd = _rows_input(V, dt)
    for n in (1, 5, 48, N_MAX):
        for use_ws in (True, False):
            for sample in (0, 1):
                want = _scalar_rows(V, dt, use_ws, sample)
                b = _buffers(n, V)
                ws = torch.zeros(hip.lib.sd_norm_workspace_bytes(n), dtype=torch.uint8, device="cuda") if use_ws else None
                hip.L.check(hip.lib.sd_norm_batch_rows(xd.data_ptr(), n, V, V, _params(hip, P, n), R.DT_MODE[dt],
                                                       _norm_rows(hip, b, 0, n), sample, ws.data_ptr() if use_ws else None, _st()),
                            "sd_norm_batch_rows")
                torch.cuda.synchronize()
                for name, t in b.items():
                    got = t.cpu()
                    for r in range(n):
                        assert torch.equal(got[r], want[name][r]), (name, "row", r, P[r % len(P)], dict(n=n, ws=use_ws, sample=sample))
                assert b["err"].cpu().tolist() == [0] * n
                assert b["serr"].cpu().tolist() == [0 if sample else -1] * n
                assert all((0 <= t < V) if sample else t == -1 for t in b["tok"].cpu().tolist())


@pytest.mark.parametrize("V", [8192, 512])
def test_rows_against_the_oracle(hip, V):
    """K1, oracle part: the fp32 rows of one 49-row call against oracle.norm_logits with each row's own triple, under the
    bars of test_norm_probs_many_rows_vs_oracle as check_probs applies them."""
    x, xd = _rows_input(V, 0)
    b = _buffers(N_MAX, V)
    ws = torch.zeros(hip.lib.sd_norm_workspace_bytes(N_MAX), dtype=torch.uint8, device="cuda")
    hip.L.check(hip.lib.sd_norm_batch_rows(xd.data_ptr(), N_MAX, V, V, _params(hip, P, N_MAX), 0, _norm_rows(hip, b, 0, N_MAX), 0,
                                           ws.data_ptr(), _st()), "sd_norm_batch_rows")
    got = b["out"].cpu()
    for r in range(N_MAX):
        T, k, p = P[r % len(P)]
        check_probs(dict(id=f"row{r}", T=T, k=k, p=p, dt=0), got[r], x[r:r + 1])


# ----------------------------------------------------------------------------- K2: routes
def _rows_debug(hip, x, table, entry, with_ws):
    """sd_norm_batch_rows_debug on the rows of x (CPU fp32), outputs pre-zeroed and tile maxima built as
    test_gpu_sampler_routes.launch does.  Returns (out, route words, list sizes)."""
    n, V = x.shape
    xd = x.cuda().contiguous()
    b = _buffers(n, V, fill=0.0 if entry == "tile" else 7.0)
    route = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    lists = torch.zeros((n + 1, CL_INTS), dtype=torch.int32, device="cuda")
    ws = torch.zeros(hip.lib.sd_norm_workspace_bytes(n), dtype=torch.uint8, device="cuda") if with_ws else None
    tm = torch.cat([R.tile_maxima(x[i:i + 1]) for i in range(n)], 0).cuda() if entry == "tile" else None
    hip.L.check(hip.lib.sd_norm_batch_rows_debug(xd.data_ptr(), n, V, V, _params(hip, table, n), 0, _norm_rows(hip, b, 0, n), 0,
                                                 ws.data_ptr() if with_ws else None, _st(), tm.data_ptr() if tm is not None else None,
                                                 lists.data_ptr(), route.data_ptr()), "sd_norm_batch_rows_debug")
    torch.cuda.synchronize()
    lists = lists.cpu()
    assert not bool(lists[n].any())
    assert b["err"].cpu().tolist() == [0] * n
    return b["out"].cpu(), [w & 0xffffffff for w in route.cpu().tolist()], lists[:n, 0].tolist()


def test_routes_with_a_workspace(hip):
    """K2.  Entry A is per row: with a workspace each row's route word is the word sd_norm_probs_debug reports for that row
    alone with a workspace - A for exactly the rows with 1 <= k <= 64, beside rows with k == 0 and k > 64."""
    x = _rows_input(8192, 0)[0][:len(P)]
    out, words, sizes = _rows_debug(hip, x, P, "ws", True)
    for r, (T, k, p) in enumerate(P):
        one = launch(hip, x[r:r + 1], T, k, p, 0, "ws")
        assert words[r] == one["route"][0], (r, R.route_str(words[r]), R.route_str(one["route"][0]))
        assert bool(words[r] & R.A) == _eligible_a(k), (r, R.route_str(words[r]))
        assert not words[r] & R.B
        assert torch.equal(out[r], one["out"][0]) and sizes[r] == int(one["lists"][0, 0]), r


def test_routes_with_tile_maxima_all_rows_eligible(hip):
    """K2.  Entry B is per launch: with tile maxima and a table of eligible rows only (different T > 0, k, p) every row
    reports B and equals its scalar tile launch bit for bit."""
    n = 7
    x = _rows_input(8192, 0)[0][:n]
    out, words, sizes = _rows_debug(hip, x, P_ELIGIBLE, "tile", False)
    for r in range(n):
        T, k, p = P_ELIGIBLE[r % len(P_ELIGIBLE)]
        one = launch(hip, x[r:r + 1], T, k, p, 0, "tile")
        assert words[r] & R.B and one["route"][0] & R.B and not words[r] & R.A, (r, R.route_str(words[r]))
        assert words[r] == one["route"][0], (r, R.route_str(words[r]), R.route_str(one["route"][0]))
        assert torch.equal(out[r], one["out"][0]) and sizes[r] == int(one["lists"][0, 0]), r


@pytest.mark.parametrize("with_ws", [True, False], ids=["ws", "no_ws"])
def test_routes_with_tile_maxima_and_ineligible_rows(hip, with_ws):
    """K2.  The full table holds rows entry B cannot serve (k == 0, k > 64, T < 0): the launch drops the tile maxima, no row
    reports B, the rows with 1 <= k <= 64 report A when a workspace is given - and every row still equals its scalar launch."""
    x = _rows_input(8192, 0)[0][:len(P)]
    out, words, _ = _rows_debug(hip, x, P, "tile", with_ws)
    for r, (T, k, p) in enumerate(P):
        assert not words[r] & R.B, (r, R.route_str(words[r]))
        assert bool(words[r] & R.A) == (with_ws and _eligible_a(k)), (r, R.route_str(words[r]))
        one = launch(hip, x[r:r + 1], T, k, p, 0, "ws" if with_ws else "plain")
        assert words[r] == one["route"][0] and torch.equal(out[r], one["out"][0]), (r, R.route_str(words[r]))


# ----------------------------------------------------------------------------- L: the loops
V8K_CFG = dict(arch="llama", vocab_size=8192, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
               num_key_value_heads=2, max_position_embeddings=256, rms_norm_eps=1e-5)


@functools.lru_cache(maxsize=None)
def _pair_models(kind):
    """(cfg_d, sd_d, cfg_t, sd_t, draft, target), fp32: test_gpu_spec_queue's tiny pairs, or "v8k" - a Llama pair with V = 8192
    (the norm's workspace entry applies), built like _pair("corr")."""
    if kind != "v8k":
        return _models(kind)
    from llmspeculativesampling_amd import engine
    cfg = ModelConfig(**V8K_CFG)
    dsd = make_state_dict(cfg, 21)
    tsd = perturb_state_dict(dsd, 22, 0.12)
    return (cfg, dsd, cfg, tsd, engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.float32),
            engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.float32))


def _oracle_runs(lib, kind, prompts, seeds, budgets, eos, gamma, triples, **more):
    dc, dsd, tc, tsd = _pair_models(kind)[:4]
    od, ot = oracle.RefCausalLM(dc, dsd), oracle.RefCausalLM(tc, tsd)
    return [oracle.speculative_sampling(pf, od, ot, eos, None, m, details=True, gamma=gamma, temperature=T, top_k=k, top_p=p,
                                        noise=PhiloxOracleNoise(lib, s, gamma, _st), **more)
            for pf, s, m, (T, k, p) in zip(prompts, seeds, budgets, triples)]


def _assert_equal_runs(wants, outs, ds, what):
    for i, ((want, wd), got, gd) in enumerate(zip(wants, outs, ds)):
        np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy(), err_msg=f"{what}: prompt {i}")
        assert gd["acc_len"] == wd["acc_len"], (what, i)
        assert gd["target_call_times"] == wd["target_call_times"] and gd["approx_call_times"] == wd["approx_call_times"], (what, i)
        assert set(gd) == DETAILS_KEYS


def _columns(triples):
    return dict(temperature=[t[0] for t in triples], top_k=[t[1] for t in triples], top_p=[t[2] for t in triples])


Q_LENS, Q_BUDGETS = [1, 2, 9, 40, 13, 5], [24, 6, 12, 6, 24, 6]
Q_SEEDS = [8100 + i for i in range(6)]


@pytest.mark.parametrize("kind", ["corr", "opt", "v8k"])
def test_queue_with_per_prompt_parameters_equals_oracle_and_single_stream(hip, kind):
    """L1.  Six prompts with the first six rows of P - all different - through 3 slots: every slot that changes hands changes
    parameters.  Tokens, acc_len and call counts of every prompt equal the oracle's run and the single-stream loop's run with
    that prompt's own triple on its own Philox stream."""
    dc, _, _, _, dm, tm = _pair_models(kind)
    triples, gamma = P[:6], 4
    prompts = _prompts(dc.vocab_size, Q_LENS, 300)
    wants = _oracle_runs(hip.lib, kind, prompts, Q_SEEDS, Q_BUDGETS, -1, gamma, triples)
    t = {}
    outs, ds = hip.S.speculative_sampling_queue([pf.cuda() for pf in prompts], dm, tm, -1, None, Q_BUDGETS, gamma=gamma, details=True,
                                                seeds=Q_SEEDS, slots=3, prefill_chunk=8, _timing=t, **_columns(triples))
    print("admit", t["admit_iter"], "finish", t["finish_iter"])
    assert any(a > 0 for a in t["admit_iter"][3:]), t["admit_iter"]   # a slot changed hands mid-call, hence parameters
    _assert_equal_runs(wants, outs, ds, "oracle")
    singles = [hip.S.speculative_sampling(pf.cuda(), dm, tm, -1, None, m, gamma=gamma, details=True, rng=hip.noise.DeviceNoise(s),
                                          temperature=T, top_k=k, top_p=p)
               for pf, m, s, (T, k, p) in zip(prompts, Q_BUDGETS, Q_SEEDS, triples)]
    _assert_equal_runs(singles, outs, ds, "single stream")


B_LENS = [9, 11, 13, 15]
B_SEEDS = [930 + i for i in range(4)]


@pytest.mark.parametrize("gamma", [2, 8])
@pytest.mark.parametrize("table", ["eligible", "mixed"])
def test_batch_loop_with_per_stream_parameters_equals_oracle(hip, table, gamma):
    """L2.  Four streams on the V = 8192 pair, once with four eligible, different triples and once with rows 0 to 3 of P
    (two of them k == 0): every stream equals the oracle's run with its triple."""
    dc, _, _, _, dm, tm = _pair_models("v8k")
    triples = P_ELIGIBLE[:4] if table == "eligible" else P[:4]
    prompts = _prompts(dc.vocab_size, B_LENS, 40)
    wants = _oracle_runs(hip.lib, "v8k", prompts, B_SEEDS, [16] * 4, -1, gamma, triples)
    outs, ds = hip.S.speculative_sampling_batch([pf.cuda() for pf in prompts], dm, tm, -1, None, 16, gamma=gamma, details=True,
                                                seeds=B_SEEDS, **_columns(triples))
    _assert_equal_runs(wants, outs, ds, "oracle")


def test_batch_loop_with_per_stream_parameters_and_random_seed(hip):
    """L2, the reseed quirk: random_seed=42 with rows 0 to 3 of P."""
    dc, _, _, _, dm, tm = _pair_models("v8k")
    triples, gamma = P[:4], 4
    prompts = _prompts(dc.vocab_size, B_LENS, 40)
    wants = _oracle_runs(hip.lib, "v8k", prompts, B_SEEDS, [16] * 4, -1, gamma, triples, random_seed=42)
    outs, ds = hip.S.speculative_sampling_batch([pf.cuda() for pf in prompts], dm, tm, -1, None, 16, gamma=gamma, details=True,
                                                seeds=B_SEEDS, random_seed=42, **_columns(triples))
    _assert_equal_runs(wants, outs, ds, "oracle")


def test_the_loops_without_per_row_parameters_refuse_row_params(hip, monkeypatch):
    """sd_spec_generate and sd_ar_batch_generate sample with sampling's own triple: a non-NULL row_params in their sd_loop_opts
    is SD_ERR_INVALID behind the entry's own refusals (which read the sessions, hence a GPU test) and ahead of the other
    members - the logprob block beside it is wrong too - and nothing runs: the same wrapper call without it gives the
    tokens of an untouched Philox stream."""
    import ctypes as C
    import importlib
    from llmspeculativesampling_amd import _lib
    from llmspeculativesampling_amd.sampling import _loop_common as LC
    dc, _, _, _, dm, tm = _pair_models("corr")
    prompt = _prompts(dc.vocab_size, [9], 40)[0].cuda()
    calls = {"sd_spec_generate": lambda rng: hip.S.speculative_sampling(prompt, dm, tm, -1, None, 6, gamma=4, rng=rng),
             "sd_ar_batch_generate": lambda rng: hip.S.autoregressive_sampling(prompt, tm, 6, -1, rng=rng)}
    keep = (_lib.SdRowSampling * 1)(_lib.SdRowSampling(1.0, 20, 0.9))
    bad = lambda *a: _lib.SdLoopOpts(row_params=keep, logprobs=C.pointer(_lib.SdLogprobBlock()))
    for mod, entry in (("speculative_sampling", "sd_spec_generate"), ("autoregressive_sampling", "sd_ar_batch_generate")):
        m = importlib.import_module("llmspeculativesampling_amd.sampling." + mod)
        want = calls[entry](hip.noise.DeviceNoise(77))
        rng = hip.noise.DeviceNoise(77)
        monkeypatch.setattr(m, "loop_opts", bad)
        with pytest.raises((ValueError, RuntimeError)) as e:
            calls[entry](rng)
        err = e.value if isinstance(e.value, ValueError) else e.value.__cause__   # (speculative_sampling re-raises as the reference does)
        assert isinstance(err, ValueError) and entry + ": row_params: " in str(err), err
        monkeypatch.setattr(m, "loop_opts", LC.loop_opts)
        assert torch.equal(calls[entry](rng), want)               # (the refused call drew nothing)


COUNTS = ("iterations", "target_passes", "draft_passes", "extra_passes", "prefill_passes", "prompt_rows", "admit_iter", "finish_iter")


def test_uniform_sequences_equal_scalars_in_the_queue(hip):
    """L3.  temperature=[1]*N, top_k=[20]*N, top_p=[0.9]*N against the scalar call: identical outputs, details and pass
    counts (fp32 "corr")."""
    dc, _, _, _, dm, tm = _pair_models("corr")
    N = len(Q_LENS)
    prompts = [pf.cuda() for pf in _prompts(dc.vocab_size, Q_LENS, 300)]
    runs = []
    for kw in (dict(temperature=1, top_k=20, top_p=0.9), dict(temperature=[1] * N, top_k=[20] * N, top_p=[0.9] * N)):
        t = {}
        outs, ds = hip.S.speculative_sampling_queue(prompts, dm, tm, 2, None, Q_BUDGETS, gamma=4, details=True, seeds=Q_SEEDS, slots=3,
                                                    prefill_chunk=8, _timing=t, **kw)
        runs.append((outs, ds, t))
    (o0, d0, t0), (o1, d1, t1) = runs
    assert all(torch.equal(a, b) for a, b in zip(o0, o1)) and d0 == d1
    assert {k: t0[k] for k in COUNTS} == {k: t1[k] for k in COUNTS}


@functools.lru_cache(maxsize=None)
def _bf16_pair():
    from llmspeculativesampling_amd import engine
    cfg = ModelConfig(**BF16_CFG)
    dsd = make_state_dict(cfg, 5, dtype=torch.bfloat16)
    tsd = {k: v.to(torch.bfloat16) for k, v in perturb_state_dict({a: b.float() for a, b in dsd.items()}, 6, 0.05).items()}
    return (cfg, engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.bfloat16),
            engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.bfloat16))


def test_uniform_sequences_equal_scalars_in_the_bf16_batch_loop(hip):
    """L3, the 16-bit loop: the passes are the same, so the bits are the same (the head's tile maxima serve every draft pass
    of both calls)."""
    cfg, dm, tm = _bf16_pair()
    prompts = [pf.cuda() for pf in _prompts(cfg.vocab_size, [12, 1, 33, 7], 1000)]
    seeds = [77, 78, 79, 80]
    runs = []
    for kw in (dict(temperature=1, top_k=20, top_p=0.9), dict(temperature=[1] * 4, top_k=[20] * 4, top_p=[0.9] * 4)):
        t = {}
        outs, ds = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 16, gamma=4, details=True, seeds=seeds, _timing=t, **kw)
        runs.append((outs, ds, [(n, ctx) for _, _, n, ctx in t["verify"]]))
    (o0, d0, v0), (o1, d1, v1) = runs
    assert all(torch.equal(a, b) for a, b in zip(o0, o1)) and d0 == d1 and v0 == v1


def test_shared_prefix_queue_with_per_prompt_parameters_equals_oracle(hip):
    """L4.  speculative_sampling_queue_shared(shared_prefix=5) with per-prompt parameters equals the oracle per prompt."""
    dc, _, _, _, dm, tm = _pair_models("corr")
    lens, budgets, seeds = [6, 14, 9, 22, 7], [10, 8, 12, 6, 10], [8300 + i for i in range(5)]
    head = _prompts(dc.vocab_size, [5], 77)[0]
    prompts = [torch.cat([head, pf[:, 5:]], 1) if L > 5 else head[:, :L] for pf, L in zip(_prompts(dc.vocab_size, lens, 1100), lens)]
    triples = P[:5]
    wants = _oracle_runs(hip.lib, "corr", prompts, seeds, budgets, -1, 4, triples)
    t = {}
    outs, ds = hip.S.speculative_sampling_queue_shared([pf.cuda() for pf in prompts], dm, tm, -1, None, budgets, gamma=4, details=True,
                                                       seeds=seeds, slots=2, prefill_chunk=8, _timing=t, shared_prefix=5,
                                                       **_columns(triples))
    assert t["copied_rows"] > 0
    _assert_equal_runs(wants, outs, ds, "oracle")


@pytest.mark.parametrize("entry", ["batch_eligible", "batch_mixed", "queue_mixed"])
def test_bf16_fused_tail_equals_the_dense_tail_under_per_request_parameters(hip, entry):
    """L5.  A bf16 pair, where the draft head can leave tile maxima: with all-eligible triples every draft pass takes entry B,
    with rows of P only the passes whose active streams are all eligible do (in the queue that changes as slots change hands).
    Under the same seeds the fused tail must equal SD_BATCH_FUSED_TAIL=0 - no tile maxima, the dense accept - bit for bit."""
    cfg, dm, tm = _bf16_pair()
    runs = {}
    try:
        for mode in ("0", "1"):
            os.environ["SD_BATCH_FUSED_TAIL"] = mode
            if entry == "queue_mixed":
                prompts = [pf.cuda() for pf in _prompts(cfg.vocab_size, Q_LENS, 1000)]
                # (eligible rows first: the first passes run on tile maxima, later ones lose them to a k == 0 neighbour)
                triples = [P[0], P[3], P[4], P[1], P[2], P[5]]
                runs[mode] = hip.S.speculative_sampling_queue(prompts, dm, tm, -1, None, Q_BUDGETS, gamma=4, details=True, seeds=Q_SEEDS,
                                                              slots=3, prefill_chunk=8, **_columns(triples))
            else:
                prompts = [pf.cuda() for pf in _prompts(cfg.vocab_size, [12, 1, 33, 7], 1000)]
                triples = P_ELIGIBLE[:4] if entry == "batch_eligible" else P[:4]
                runs[mode] = hip.S.speculative_sampling_batch(prompts, dm, tm, -1, None, 16, gamma=4, details=True,
                                                              seeds=[77, 78, 79, 80], **_columns(triples))
    finally:
        os.environ.pop("SD_BATCH_FUSED_TAIL", None)
    (o0, d0), (o1, d1) = runs["0"], runs["1"]
    for a, b, da, db in zip(o0, o1, d0, d1):
        assert torch.equal(a, b), (a, b)
        assert da["acc_len"] == db["acc_len"] and float(da["acc_rate"]) == float(db["acc_rate"])
