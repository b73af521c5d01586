"""The prompt-lookup loops token for token (`pytest -m gpu`): sd_lookup_generate and sd_lookup_batch_generate on the fp32 tiny
target against tests/lookup_reference.run fed the device's own Philox variates (tests/philox_replay.py) - tokens, acc_len and
match_len per iteration, the final Philox position - and one bf16 run of the native loop against the Python-level composition
of the same C entries.  The prompts and seeds are lookup_reference's constants; test_lookup_cpu.py shows on the reference alone
that they give every kind of iteration, and the runs here are held to the same condition."""
import ctypes as C

import numpy as np
import pytest
import torch

import lookup_reference as R
from philox_replay import PhiloxOracleNoise
from llmspeculativesampling_amd.config import ModelConfig
from llmspeculativesampling_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu

G, NMAX, NMIN, MAX_LEN = R.PARITY_GAMMA, R.PARITY_NGRAM_MAX, R.PARITY_NGRAM_MIN, R.PARITY_MAX_LEN
assert MAX_LEN <= 48


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


@pytest.fixture(scope="module")
def tiny(hip):
    cfg, sd, om = R.parity_model()
    return cfg, om, hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)


def _st():
    return torch.cuda.current_stream().cuda_stream


_REFS = {}                                                        # one reference run per (prompt, seed, top_k, eos), shared by the tests


def _reference(hip, om, prompt, seed, top_k, eos=-1):
    key = (tuple(prompt[0].tolist()), seed, top_k, eos)
    if key not in _REFS:
        _REFS[key] = R.run(om, prompt, eos, MAX_LEN, G, 1, top_k, 0, NMAX, NMIN, PhiloxOracleNoise(hip.lib, seed, G, _st))
    return _REFS[key]


@pytest.mark.parametrize("case", list(R.PARITY_CASES))
def test_single_stream_loop_equals_the_reference(hip, tiny, case):
    cfg, om, tm = tiny
    ps, seed, top_k = R.PARITY_CASES[case]
    prompt = R.parity_prompt(cfg, ps)
    want, wd = _reference(hip, om, prompt, seed, top_k)
    nz = hip.noise.DeviceNoise(seed)
    got, gd = hip.S.prompt_lookup_sampling(prompt.cuda(), tm, -1, None, MAX_LEN, G, 1, top_k, 0, NMAX, NMIN, details=True, rng=nz)
    print(case, "acc_len", gd["acc_len"], "match_len", gd["match_len"])
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    assert gd["acc_len"] == wd["acc_len"] and gd["match_len"] == wd["match_len"]
    assert gd["target_call_times"] == gd["approx_call_times"] == len(wd["acc_len"])
    assert (nz.seed, nz.draw) == (seed, wd["draws"]) and wd["draws"] == (2 * G + 2) * len(wd["acc_len"])
    assert R.admissible(wd, G, NMAX) == []
    assert gd["approx_time"] > 0 and gd["target_time"] > 0
    # the same call without details (no timing events, no match_len array read): the same tokens
    plain = hip.S.prompt_lookup_sampling(prompt.cuda(), tm, -1, None, MAX_LEN, G, 1, top_k, 0, NMAX, NMIN,
                                         rng=hip.noise.DeviceNoise(seed))
    assert isinstance(plain, torch.Tensor) and torch.equal(plain, got)


def test_single_stream_loop_stops_at_a_new_eos_like_the_reference(hip, tiny):
    cfg, om, tm = tiny
    ps, seed, top_k = R.PARITY_CASES["b_top4"]
    prompt = R.parity_prompt(cfg, ps)
    full, _ = _reference(hip, om, prompt, seed, top_k)
    eos = int(full[0, prompt.shape[1] + 9])                       # a token the run really generates
    want, wd = _reference(hip, om, prompt, seed, top_k, eos)
    got, gd = hip.S.prompt_lookup_sampling(prompt.cuda(), tm, eos, None, MAX_LEN, G, 1, top_k, 0, NMAX, NMIN, details=True,
                                           rng=hip.noise.DeviceNoise(seed))
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    assert gd["acc_len"] == wd["acc_len"] and int(got[0, -1]) == eos and got.shape[1] < prompt.shape[1] + MAX_LEN


def test_lock_step_loop_equals_three_single_reference_runs(hip, tiny):
    cfg, om, tm = tiny
    prompts = [R.parity_prompt(cfg, ps, n) for ps, n, _ in R.PARITY_BATCH]
    seeds = [s for _, _, s in R.PARITY_BATCH]
    full, _ = _reference(hip, om, prompts[2], seeds[2], 4)
    eos = int(full[0, prompts[2].shape[1] + 14])                  # stream 2 stops early, the others go on
    wants = [_reference(hip, om, p, s, 4, eos) for p, s in zip(prompts, seeds)]
    outs, ds = hip.S.prompt_lookup_sampling_batch([p.cuda() for p in prompts], tm, eos, None, MAX_LEN, G, 1, 4, 0, NMAX, NMIN,
                                                  details=True, seeds=seeds)
    lens = []
    for (want, wd), got, gd in zip(wants, outs, ds):
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
        assert gd["acc_len"] == wd["acc_len"] and gd["match_len"] == wd["match_len"]
        assert gd["target_call_times"] == len(wd["acc_len"])
        lens.append(len(wd["acc_len"]))
    assert len(set(lens)) > 1                                     # a done stream dropped out while the others ran on
    # ... and each stream equals its single-stream run
    for p, s, got in zip(prompts, seeds, outs):
        one = hip.S.prompt_lookup_sampling(p.cuda(), tm, eos, None, MAX_LEN, G, 1, 4, 0, NMAX, NMIN, rng=hip.noise.DeviceNoise(s))
        assert torch.equal(one, got)


def test_lock_step_loop_with_one_stream_per_verify_pass(hip, tiny, monkeypatch):
    """A target pass of gamma + 1 rows holds one stream: while several streams are active the verify takes one pass per stream,
    with no candidate lists and the dense accept launch; the lists come back once a single stream is left.  The reference does
    not depend on how the passes are cut, so the runs are those of the one-pass case above."""
    cfg, om, tm = tiny
    from llmspeculativesampling_amd.sampling import lookup
    real = lookup.spec_scratch
    monkeypatch.setattr(lookup, "spec_scratch", lambda draft_ses, target_ses, norm_ws, per_pass: real(draft_ses, target_ses, norm_ws, G + 1))
    noises = []                                                   # the streams' Philox positions, as the wrapper leaves them
    monkeypatch.setattr(lookup, "DeviceNoise", lambda seed: noises.append(hip.noise.DeviceNoise(seed)) or noises[-1])
    prompts = [R.parity_prompt(cfg, ps, n) for ps, n, _ in R.PARITY_BATCH]
    seeds = [s for _, _, s in R.PARITY_BATCH]
    full, _ = _reference(hip, om, prompts[2], seeds[2], 4)
    eos = int(full[0, prompts[2].shape[1] + 14])                  # stream 2 stops early, the others go on
    wants = [_reference(hip, om, p, s, 4, eos) for p, s in zip(prompts, seeds)]
    outs, ds = hip.S.prompt_lookup_sampling_batch([p.cuda() for p in prompts], tm, eos, None, MAX_LEN, G, 1, 4, 0, NMAX, NMIN,
                                                  details=True, seeds=seeds)
    lens = []
    for (want, wd), got, gd in zip(wants, outs, ds):
        print("acc_len", gd["acc_len"], "match_len", gd["match_len"])
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
        assert gd["acc_len"] == wd["acc_len"] and gd["match_len"] == wd["match_len"]
        assert gd["target_call_times"] == len(wd["acc_len"])
        lens.append(len(wd["acc_len"]))
    assert [(nz.seed, nz.draw) for nz in noises] == [(s, wd["draws"]) for s, (_, wd) in zip(seeds, wants)]
    # every stream runs iterations 0 .. len - 1: some iteration had several active streams (one pass each), a later one had one
    lens.sort()
    assert lens[-2] >= 1 and lens[-1] > lens[-2], lens


BF16_CFG = dict(arch="llama", vocab_size=8192, hidden_size=256, intermediate_size=704, num_hidden_layers=2,
                num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-6)


def _python_loop(hip, tm, prompt, max_len, gamma, temperature, top_k, top_p, nmax, nmin, seed):
    """The iteration composed in Python from the same C entries: sd_lookup_propose, the target forward + sd_norm_probs
    (KVCacheModel.forward_rows), sd_accept_scan, sd_resample - one synchronisation per iteration."""
    from llmspeculativesampling_amd.sampling._loop_common import open_stream
    lib, Lb = hip.lib, hip.L
    host = [int(t) for t in prompt[0].tolist()]
    T = len(host) + max_len
    cap = T + gamma + 2
    target, seq32 = open_stream(tm, prompt[0], cap, cap + 1, temperature, top_k, top_p)
    p_hist = target._probs
    ld, V = p_hist.stride(0), tm.cfg.vocab_size
    q_hist = torch.empty((cap, ld), dtype=torch.float32, device="cuda")
    info = torch.zeros(2, dtype=torch.int32, device="cuda")
    res_dev = torch.zeros(C.sizeof(Lb.SdAcceptResult), dtype=torch.uint8, device="cuda")
    draw, acc_len, match_len = 0, [], []
    while len(host) < T:
        L, d = len(host), draw
        draw += 2 * gamma + 2
        item = Lb.SdLookupItem(seq32.data_ptr(), L, q_hist.data_ptr(), info.data_ptr())
        Lb.check(lib.sd_lookup_propose(item, 1, V, ld, gamma, nmax, nmin, _st()), "sd_lookup_propose")
        target.forward_rows(seq32, L + gamma, min(L + gamma - target.cache_len, gamma + 1))
        Lb.check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), ld, seq32.data_ptr(), L, gamma, None, seed, d + gamma + 1,
                                    res_dev.data_ptr(), _st()), "sd_accept_scan")
        Lb.check(lib.sd_resample(p_hist.data_ptr(), q_hist.data_ptr(), ld, V, seq32.data_ptr(), L, gamma, None, seed,
                                 d + 2 * gamma + 1, res_dev.data_ptr(), None, tm.norm_mode, _st()), "sd_resample")
        torch.cuda.synchronize()
        res = Lb.SdAcceptResult.from_buffer_copy(res_dev.cpu().numpy().tobytes())
        assert not res.flags & 2
        target.check_errors(L - 1, L + gamma)
        acc_len.append(res.n_accepted)
        match_len.append(int(info[0]))
        host = host + seq32[L:L + res.n_accepted].tolist() + [res.next_token]
        target.rollback(res.n + 1)
    return host, acc_len, match_len, draw


def test_native_bf16_loop_bit_equals_the_python_composition(hip):
    """bf16 weights, a vocabulary wide enough for the head's tile maxima and the candidate lists (top_k 20), a prompt that
    repeats so that drafts are accepted: tokens, acc_len, match_len and the Philox position bit-equal."""
    cfg = ModelConfig(**BF16_CFG)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, 5, dtype=torch.bfloat16), dtype=torch.bfloat16)
    base = np.random.default_rng(3).integers(3, cfg.vocab_size, size=8)
    prompt = torch.from_numpy(np.concatenate([base, base, base])[None]).cuda()
    kw = (40, 4, 1, 20, 0.9, 3, 1)
    nz = hip.noise.DeviceNoise(123)
    a, da = hip.S.prompt_lookup_sampling(prompt, tm, -1, None, *kw, details=True, rng=nz)
    host, acc_len, match_len, draw = _python_loop(hip, tm, prompt, *kw, 123)
    assert a[0].tolist() == host
    assert da["acc_len"] == acc_len and da["match_len"] == match_len and nz.draw == draw
    assert max(match_len) == 3
