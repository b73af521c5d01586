"""Parity of the HIP path (through the C ABI) against the reference's golden vectors and the oracle.

Run with ``pytest -m gpu`` on an MI355X.  Bars: token ids bit-exact; probabilities within 1e-6
absolute with an identical support set; fp32 logits within 1e-3 (north_star); bf16 logits within
0.25 of the reference's bf16 forward (same bar the oracle is held to).
"""
import os
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from golden_io import DT, dense_from_sparse, events, load, logits_row, model_pair
from llmspeculativesampling_amd.config import load_config
from llmspeculativesampling_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    import types
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


def _st():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------- G1 norm_probs
G1_META, G1 = load("g1_norm_logits")


def assert_rows_equal_up_to_tied_logits(got, want, z):
    """got / want: probability rows (numpy); z: the scaled logits they were made from.  16-bit rows must match bit for
    bit, except that where the top-p cut falls inside a run of EQUAL logits the reference keeps whichever members its
    unstable sort happened to put first (oracle.sampling_ref.STABLE_TIES) and the kernels keep the lowest ids: the
    probability multiset is then still identical and every token that differs has a twin with the same logit."""
    if np.array_equal(got, want):
        return
    np.testing.assert_array_equal(np.sort(got), np.sort(want))
    diff = np.nonzero((got > 0) != (want > 0))[0]
    assert len(diff) and len(diff) % 2 == 0
    vals = {float(z[i]) for i in diff}
    for v in vals:
        ids = [i for i in diff if float(z[i]) == v]
        assert sum(got[i] > 0 for i in ids) == sum(want[i] > 0 for i in ids), (v, ids)


@pytest.mark.parametrize("case", G1_META, ids=[c["id"] for c in G1_META])
def test_norm_probs_golden(hip, case):
    if case.get("dtype", "float32") != "float32":
        # bf16 / fp16 rows: the reference rounds every intermediate tensor to the row dtype (SD_NORM_DT_*): bit-exact
        dt = DT[case["dtype"]]
        x = logits_row(case["seed"], case["V"], case["scale"], dtype=dt)
        want = dense_from_sparse(case["V"], G1[case["id"] + "_idx"], G1[case["id"] + "_val"])
        got = hip.S.norm_logits(x.cuda(), case["T"], case["k"], case["p"])
        assert got.dtype == dt
        assert_rows_equal_up_to_tied_logits(got.float().cpu().numpy()[0], want, (x.float() / case["T"]).to(dt).float().numpy()[0])
        return
    if case["kind"] == "error":
        row = torch.tensor([[float(v) for v in case["row"]]], device="cuda")
        with pytest.raises(RuntimeError, match="norm logits error"):
            hip.S.norm_logits(row, case["T"], case["k"], case["p"])
        return
    if case["kind"] == "inline":
        x = torch.tensor([[float(v) for v in case["row"]]], dtype=torch.float32)
        want = np.array(case["expect"], dtype=np.float32)
    else:
        x = logits_row(case["seed"], case["V"], case["scale"])
        want = G1[case["id"] + "_dense"] if case["dense"] else dense_from_sparse(
            case["V"], G1[case["id"] + "_idx"], G1[case["id"] + "_val"])
    got = hip.S.norm_logits(x.cuda(), case["T"], case["k"], case["p"]).cpu().numpy()[0]
    np.testing.assert_array_equal(got > 0, want > 0)            # identical support set
    np.testing.assert_allclose(got, want, atol=1e-6, rtol=5e-6)


def test_norm_probs_many_rows_vs_oracle(hip):
    """Random rows, several (T,k,p) incl. the general top-p path (no top-k) at V = 32000 / 50272.

    Tolerance: 1e-6 absolute + 5e-6 relative.  The relative part is the reference's own rounding: torch's
    fp32 row sum over V = 32000 is off by up to 2.5e-6 relative (its probabilities differ from the fp64
    softmax by 1.3e-6 on these rows, measured); the HIP kernel is held to 2.5e-7 of the fp64 result below."""
    for V in (1000, 32000, 50272):
        for (T, k, p) in [(1.0, 20, 0.9), (0.8, 0, 0.9), (1.0, 0, 0.0), (1.0, 2000, 0.99), (1.0, 50, 0.0)]:
            rows = torch.cat([logits_row(4242 + i, V, 3.0) for i in range(3)], 0)
            got = hip.S.norm_logits(rows.cuda(), T, k, p).cpu()
            for i in range(rows.shape[0]):
                want = oracle.norm_logits(rows[i:i + 1], T, k, p)[0]
                assert torch.equal(got[i] > 0, want > 0), (V, T, k, p, i)
                np.testing.assert_allclose(got[i].numpy(), want.numpy(), atol=1e-6, rtol=5e-6)
                z = torch.where(want > 0, (rows[i] / T).double(), torch.full((V,), float("-inf"), dtype=torch.float64))
                exact = torch.softmax(z, 0)
                assert float((got[i].double() - exact).abs().max()) <= 2.5e-7, (V, T, k, p, i)


# --------------------------------------------------------------------------- G2 sample / G3 max_fn
G2_META, G2 = load("g2_sample")


@pytest.mark.parametrize("case", G2_META["sample"], ids=[c["id"] for c in G2_META["sample"]])
def test_sample_golden(hip, case):
    if case["id"] == "allzero_raises":
        st = torch.get_rng_state()
        with pytest.raises(RuntimeError, match="prob error"):
            hip.S.sample(torch.zeros(1, case["V"], device="cuda"))
        assert torch.equal(st, torch.get_rng_state())          # invalid rows raise before any draw
        return
    if "inline_probs" in case:
        probs = torch.tensor([case["inline_probs"]], dtype=torch.float32)
        noise = torch.tensor(case["inline_noise"], dtype=torch.float32)
    else:
        probs = oracle.norm_logits(logits_row(case["seed"], case["V"]), case["T"], case["k"], case["p"])
        noise = torch.from_numpy(G2[case["id"] + "_noise"].copy())
    rp = hip.noise.ReplayNoise([("exp", noise)], "cuda")
    tok = hip.S.sample(probs.cuda(), noise=rp)
    assert int(tok) == case["token"]


def test_sample_live_generator_matches_reference_cpu(hip):
    """Default noise = torch's global CPU generator: same token as torch.multinomial on CPU."""
    for s in range(6):
        p = oracle.norm_logits(logits_row(900 + s, 32000), 1.0, 20, 0.9)
        torch.manual_seed(s)
        want = torch.multinomial(p, 1)
        torch.manual_seed(s)
        got = hip.S.sample(p.cuda())
        assert int(got) == int(want)


@pytest.mark.parametrize("case", [c for c in G2_META["max_fn"] if c["id"] != "p_equals_q"],
                         ids=lambda c: c["id"])
def test_max_fn_golden(hip, case):
    i = int(case["id"][1:])
    V = case["V"]
    pr = oracle.norm_logits(logits_row(case["seed_p"], V), case["T"], case["k"], case["p"])
    qr = oracle.norm_logits(logits_row(case["seed_p"], V) + case["mix"] * logits_row(case["seed_q"], V, 1.0),
                            case["T"], case["k"], case["p"])
    got = hip.S.max_fn((pr - qr).cuda()).cpu().numpy()[0]
    want = dense_from_sparse(V, G2[f"m{i}_idx"], G2[f"m{i}_val"])
    np.testing.assert_array_equal(got > 0, want > 0)
    np.testing.assert_allclose(got, want, atol=1e-6, rtol=1e-6)


def test_device_philox_sampling_statistics(hip):
    """Throughput-mode RNG: chi-square of token marginals against the distribution (not bit parity)."""
    V = 64
    p = torch.softmax(torch.linspace(0, 3, V), 0)[None]
    pc = p.cuda()
    nz = hip.noise.DeviceNoise(seed=1234)
    n = 4000
    counts = np.zeros(V)
    for _ in range(n):
        counts[int(hip.S.sample(pc, noise=nz))] += 1
    exp = p.numpy()[0] * n
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    assert chi2 < 130.0, chi2          # dof 63: mean 63, p(chi2 > 130) ~ 1e-6


# --------------------------------------------------------------------------- G4 accept / resample kernels
class TableModel:
    def __init__(self, table):
        from types import SimpleNamespace
        self.table = table
        self.config = SimpleNamespace(is_encoder_decoder=False)
        self.device = torch.device("cpu")

    def __call__(self, ids, past_key_values=None, use_cache=True):
        from types import SimpleNamespace
        past = past_key_values[0][0].shape[2] if past_key_values else 0
        q = ids.shape[1]
        kv = torch.zeros(1, 1, past + q, 1)
        return SimpleNamespace(logits=self.table[past:past + q][None].clone(), past_key_values=[(kv, kv)])


G4_META, G4 = load("g4_accept")


@pytest.mark.parametrize("case", G4_META, ids=[c["id"] for c in G4_META])
def test_accept_resample_kernels_golden(hip, case):
    """The reference's own traces over position-table models: the probability rows are a pure function of
    the position, so they are normalised once by the HIP norm kernel and the accept-scan / resample
    kernels then have to reproduce every (accepted count, next token) of the recorded trace."""
    rng = np.random.default_rng(case["table_seed"])
    V, S, L0, gamma = case["V"], case["S"], case["L"], case["gamma"]
    z = rng.standard_normal((S, V), dtype=np.float32) * 2.0
    eps = rng.standard_normal((S, V), dtype=np.float32) * 2.0
    prompt = rng.integers(3, V, size=(1, L0))
    q_hist = hip.S.norm_logits(torch.from_numpy(z).cuda(), 1.0, case["top_k"], case["top_p"])
    p_hist = hip.S.norm_logits(torch.from_numpy(z + np.float32(case["sigma"]) * eps).cuda(), 1.0,
                               case["top_k"], case["top_p"])
    nz = hip.noise.ReplayNoise(events(G4, case["id"]), "cuda")
    want = G4[case["id"] + "_out"]
    seq = torch.zeros(S + 8, dtype=torch.int32, device="cuda")
    seq[:L0] = torch.from_numpy(prompt[0].astype(np.int32)).cuda()
    host = list(prompt[0])
    T = L0 + case["max_len"]
    res = torch.zeros(C.sizeof(hip.L.SdAcceptResult), dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    acc_len = []
    lib = hip.lib
    while len(host) < T:
        L = len(host)
        for i in range(gamma):
            e = nz.exponential(V)
            hip.L.check(lib.sd_sample(q_hist[L + i - 1].data_ptr(), V, e.data_ptr(), 0, 0, seq[L + i].data_ptr(),
                                      err.data_ptr(), 0, _st()))
        nz.skip_exponential(V)                                    # discarded target sample
        r, token = nz.uniforms(gamma, case["random_seed"])
        hip.L.check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), V, seq.data_ptr(), L, gamma,
                                       r.data_ptr(), 0, 0, res.data_ptr(), _st()))
        out = hip.L.SdAcceptResult.from_buffer_copy(res.cpu().numpy().tobytes())
        nz.realign(token, min(out.n_accepted + 1, gamma))
        e = nz.exponential(V)
        hip.L.check(lib.sd_resample(p_hist.data_ptr(), q_hist.data_ptr(), V, V, seq.data_ptr(), L, gamma,
                                    e.data_ptr(), 0, 0, res.data_ptr(), None, 0, _st()))
        out = hip.L.SdAcceptResult.from_buffer_copy(res.cpu().numpy().tobytes())
        assert not (out.flags & 2)
        acc_len.append(out.n_accepted)
        host = host + seq[L:L + out.n_accepted].cpu().tolist() + [out.next_token]
        assert out.n == L + out.n_accepted - 1
        if 2 in host[L0:]:                                         # EOS rule (eos = 2, none in the prompt)
            host = host[:L0 + host[L0:].index(2) + 1]
            break
    assert acc_len == case["acc_len"]
    np.testing.assert_array_equal(np.array(host, dtype=np.int32), want)
    assert nz.exhausted()


@pytest.mark.parametrize("mode", ["philox", "always_reject_equal_rows", "all_accept"])
def test_fused_accept_resample_on_candidate_lists_equals_the_two_dense_kernels(hip, mode):
    """sd_accept_resample (one launch, the sample working on the target rows' candidate lists from sd_norm_probs_lists)
    against sd_accept_scan + sd_resample (two launches, two passes over V) on the same rows, drafted tokens and Philox
    draws: the whole result block and the appended token must be identical.  The strong tokens' ids agree modulo 1024, so
    several candidates share one per-thread partial of the dense normaliser sum (the fused kernel has to add them in
    index order); `always_reject_equal_rows` (p == q, r = 1.5) forces the zero-residual fallback sample(max_fn(p_n));
    `all_accept` the bonus sample."""
    lib = hip.lib
    V, gamma, L = 32000, 4, 7
    S = L + gamma + 1
    rng = np.random.default_rng(77)
    res_sz = C.sizeof(hip.L.SdAcceptResult)
    for trial in range(12):
        z = (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
        base = int(rng.integers(0, 1024))
        strong = [base + 1024 * int(k) for k in rng.choice(31, size=7, replace=False)]
        z[:, strong] += 8.0 + rng.standard_normal((S, len(strong))).astype(np.float32)
        sigma = 0.0 if mode != "philox" else [0.3, 1.0, 3.0][trial % 3]
        zp = z + np.float32(sigma) * (rng.standard_normal((S, V)) * 2.0).astype(np.float32)
        q_hist = hip.S.norm_logits(torch.from_numpy(z).cuda(), 1.0, 20, 0.9).contiguous()
        p_hist = torch.zeros((S, V), dtype=torch.float32, device="cuda")
        rows = gamma + 1
        ws = torch.empty(lib.sd_norm_workspace_bytes(rows), dtype=torch.uint8, device="cuda")
        lists = torch.empty(lib.sd_cand_list_bytes(rows), dtype=torch.uint8, device="cuda")
        zt = torch.from_numpy(zp).cuda()
        err = torch.zeros(rows, dtype=torch.int32, device="cuda")
        hip.L.check(lib.sd_norm_probs_lists(zt[L - 1].data_ptr(), rows, V, V, 1.0, 20, 0.9, 0, p_hist[L - 1].data_ptr(), V,
                                            err.data_ptr(), ws.data_ptr(), lists.data_ptr(), _st()))
        assert torch.equal(p_hist[L - 1:L + gamma], hip.S.norm_logits(zt[L - 1:L + gamma], 1.0, 20, 0.9))
        n_list = np.frombuffer(lists.cpu().numpy().tobytes(), dtype=np.int32).reshape(rows, -1)[:, 0]
        assert (n_list > 0).all() and (n_list <= 20).all()         # every row got its list
        seq0 = torch.zeros(S + 8, dtype=torch.int32, device="cuda")
        seq0[:L] = torch.from_numpy(rng.integers(3, V, size=L).astype(np.int32)).cuda()
        serr = torch.zeros(1, dtype=torch.int32, device="cuda")
        for i in range(gamma):                                     # the drafted tokens: samples of the q rows
            hip.L.check(lib.sd_sample(q_hist[L + i - 1].data_ptr(), V, None, 11 + trial, i, seq0[L + i].data_ptr(),
                                      serr.data_ptr(), 0, _st()))
        r = None
        if mode == "always_reject_equal_rows":
            r = torch.full((gamma,), 1.5, dtype=torch.float32, device="cuda")
        seed, d_scan, d_res = 1000 + trial, 5, 9
        out = {}
        for which in ("dense", "fused"):
            seq = seq0.clone()
            res = torch.zeros(res_sz, dtype=torch.uint8, device="cuda")
            if which == "dense":
                hip.L.check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), V, seq.data_ptr(), L, gamma,
                                               r.data_ptr() if r is not None else None, seed, d_scan, res.data_ptr(), _st()))
                hip.L.check(lib.sd_resample(p_hist.data_ptr(), q_hist.data_ptr(), V, V, seq.data_ptr(), L, gamma, None, seed,
                                            d_res, res.data_ptr(), None, 0, _st()))
            else:
                hip.L.check(lib.sd_accept_resample(p_hist.data_ptr(), q_hist.data_ptr(), V, V, seq.data_ptr(), L, gamma,
                                                   r.data_ptr() if r is not None else None, seed, d_scan, d_res,
                                                   res.data_ptr(), None, 0, 0, lists.data_ptr(), _st()))
            out[which] = (res.cpu().numpy().tobytes(), seq.cpu().numpy().copy())
        a = hip.L.SdAcceptResult.from_buffer_copy(out["dense"][0])
        assert out["fused"][0] == out["dense"][0], (trial, a.n_accepted, a.next_token)
        np.testing.assert_array_equal(out["fused"][1], out["dense"][1])
        assert a.next_token >= 0
        if mode == "always_reject_equal_rows":
            assert a.n_accepted == 0 and (a.flags & 1)             # the residual was empty: fallback taken
        if mode == "all_accept":
            assert a.n_accepted == gamma


def test_resample_fallback_when_residual_is_zero(hip):
    """p == q at the rejected position: max_fn(p-q) is all zero, the reference's sample raises and it
    falls back to sample(max_fn(p)) (speculative_sampling.py:2007-2010)."""
    V, L, gamma = 128, 3, 2
    p = oracle.norm_logits(logits_row(77, V), 1.0, 10, 0.0)
    hist = p.repeat(8, 1).cuda()
    seq = torch.zeros(16, dtype=torch.int32, device="cuda")
    nzidx = int(torch.nonzero(p[0])[0])
    seq[L] = nzidx
    seq[L + 1] = nzidx
    r = torch.tensor([2.0, 2.0], device="cuda")                  # force a reject at i = 0
    res = torch.zeros(C.sizeof(hip.L.SdAcceptResult), dtype=torch.uint8, device="cuda")
    noise = torch.empty(V).exponential_(1)
    hip.L.check(hip.lib.sd_accept_scan(hist.data_ptr(), hist.data_ptr(), V, seq.data_ptr(), L, gamma, r.data_ptr(),
                                       0, 0, res.data_ptr(), _st()))
    hip.L.check(hip.lib.sd_resample(hist.data_ptr(), hist.data_ptr(), V, V, seq.data_ptr(), L, gamma,
                                    noise.cuda().data_ptr(), 0, 0, res.data_ptr(), None, 0, _st()))
    out = hip.L.SdAcceptResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert out.n_accepted == 0 and out.n == L - 1 and (out.flags & 1)
    want = oracle.sample(oracle.max_fn(p), oracle.RecordedNoise([("exp", noise[None])]))
    assert out.next_token == int(want)


# --------------------------------------------------------------------------- G6 logits
G6_META, G6 = load("g6_logits")


def _engine_model(hip, cfg_name, seed, dtype, sd=None):
    cfg = load_config(cfg_name)
    sd = sd if sd is not None else make_state_dict(cfg, seed, dtype=dtype)
    return cfg, hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=dtype)


@pytest.mark.parametrize("case", G6_META, ids=[c["id"] for c in G6_META])
def test_forward_logits_golden(hip, case):
    """Prefill + incremental forwards (q = 12, 1, 2, 5 new rows) against the reference model classes."""
    dtype = DT[case["dtype"]]
    cfg, m = _engine_model(hip, case["cfg"], case["seed"], dtype)
    ses = m.new_session(64)
    ids = torch.from_numpy(G6[case["id"] + "_ids"]).cuda()
    pos = 0
    tol = 1e-3 if dtype == torch.float32 else 0.25
    for si, q in enumerate(case["splits"]):
        out = torch.empty((q, cfg.vocab_size), dtype=torch.float32, device="cuda")
        ses.forward(ids[pos:pos + q], q, logits_out=out)
        want = G6[f"{case['id']}_s{si}"]
        np.testing.assert_allclose(out.cpu().numpy(), want, atol=tol, rtol=0)
        pos += q
    assert ses.cache_len == 20
    k0 = ses.past_key_values()[0][0]
    assert list(k0.shape) == case["kv_shape"]                     # the reference's (1, H_kv, S, D) view


def test_forward_rollback_is_pure(hip):
    """Rolling the arena back and re-feeding gives bit-identical logits (rollback = length counter)."""
    cfg, m = _engine_model(hip, "tiny-llama-target", 12, torch.float32)
    ses = m.new_session(64)
    ids = torch.from_numpy(G6["tiny-llama-target_float32_ids"]).cuda()
    a = ses.forward(ids[:12], 1).clone()
    b = ses.forward(ids[12:17], 5).clone()
    ses.rollback(12)
    b2 = ses.forward(ids[12:17], 5).clone()
    assert torch.equal(b, b2)
    ses.rollback(0)
    a2 = ses.forward(ids[:12], 1).clone()
    assert torch.equal(a, a2)


# --------------------------------------------------------------------------- G5 end-to-end traces
G5_META, G5 = load("g5_traces")


@pytest.mark.parametrize("case", G5_META["spec"], ids=[c["id"] for c in G5_META["spec"]])
def test_speculative_trace_golden(hip, case):
    """speculative_sampling through the HIP engine, fed the noise the reference consumed: the token ids,
    accepted lengths and call counts of the reference's own run must come out."""
    dcfg, dsd, tcfg, tsd = model_pair(case)
    dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.float32)
    tm = dm if case["target_spec"][0] == "same" else hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.float32)
    prompt = torch.from_numpy(G5[case["id"] + "_prompt"].astype(np.int64))[None].cuda()
    nz = hip.noise.ReplayNoise(events(G5, case["id"]), "cuda")
    out, d = hip.S.speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"], details=True, rng=nz,
                                        **case["kwargs"])
    np.testing.assert_array_equal(out.cpu().numpy()[0], G5[case["id"] + "_out"])
    assert d["acc_len"] == case["acc_len"]
    assert d["target_call_times"] == case["target_call_times"]
    assert d["approx_call_times"] == case["approx_call_times"]
    assert abs(float(d["acc_rate"]) - case["acc_rate"]) < 1e-4
    assert nz.exhausted()
    assert out.dtype == torch.int64 and out.shape[0] == 1


def test_speculative_live_host_rng_matches_reference_seed(hip):
    """rng="host": with the same outer torch.manual_seed the reference used, the tokens of its run come out
    (this is the drop-in's default mode)."""
    for cid in ("llama_corr", "llama_seeded", "opt_post_pair"):
        case = [c for c in G5_META["spec"] if c["id"] == cid][0]
        dcfg, dsd, tcfg, tsd = model_pair(case)
        dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.float32)
        tm = hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.float32)
        prompt = torch.from_numpy(G5[cid + "_prompt"].astype(np.int64))[None].cuda()
        torch.manual_seed(case["outer_seed"])
        out = hip.S.speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"], **case["kwargs"])
        np.testing.assert_array_equal(out.cpu().numpy()[0], G5[cid + "_out"])


G7_META, G7 = load("g7_multi")


@pytest.mark.parametrize("case", G7_META, ids=[c["id"] for c in G7_META])
def test_multi_speculative_trace_golden(hip, case):
    """multi_speculative_sampling(strategy="iid") through the HIP engine, fed the noise the
    reference consumed ((width, V) draws for the batched samples): its tokens, acc_len list, acc_rate and call counts."""
    from golden_io import events_ragged
    dcfg, dsd, tcfg, tsd = model_pair(case)
    dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.float32)
    tm = dm if case["target_spec"][0] == "same" else hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.float32)
    prompt = torch.from_numpy(G7[case["id"] + "_prompt"].astype(np.int64))[None].cuda()
    nz = hip.noise.ReplayNoise(events_ragged(G7, case["id"]), "cuda")
    out, d = hip.S.multi_speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"], width=case["width"],
                                              strategy="iid", details=True, rng=nz, **case["kwargs"])
    np.testing.assert_array_equal(out.cpu().numpy()[0], G7[case["id"] + "_out"])
    assert d["acc_len"] == case["acc_len"]
    assert d["target_call_times"] == case["target_call_times"]
    assert d["approx_call_times"] == case["approx_call_times"]
    assert abs(float(d["acc_rate"]) - case["acc_rate"]) < 1e-4
    assert nz.exhausted()
    assert out.dtype == torch.int64 and out.shape[0] == 1 and out.is_cuda


def test_multi_speculative_live_host_rng_and_device_rng(hip):
    """Default rng="host" under the reference's outer seed reproduces its run; rng="device" (Philox) is deterministic
    per seed, respects max_len and equals the oracle fed the same models in distribution only (not checked here)."""
    for cid in ("m_llama_corr", "m_llama_seeded", "m_opt_post_pair"):
        case = [c for c in G7_META if c["id"] == cid][0]
        dcfg, dsd, tcfg, tsd = model_pair(case)
        dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.float32)
        tm = hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.float32)
        prompt = torch.from_numpy(G7[cid + "_prompt"].astype(np.int64))[None].cuda()
        torch.manual_seed(case["outer_seed"])
        out = hip.S.multi_speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"], width=case["width"],
                                               strategy="iid", **case["kwargs"])
        np.testing.assert_array_equal(out.cpu().numpy()[0], G7[cid + "_out"])
        runs = [hip.S.multi_speculative_sampling(prompt, dm, tm, case["eos"], None, case["max_len"],
                                                 width=case["width"], strategy="iid",
                                                 rng=hip.noise.DeviceNoise(5), details=True, **case["kwargs"])
                for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1]["acc_len"] == runs[1][1]["acc_len"]
        g = case["kwargs"].get("gamma", 4)
        assert case["L"] + case["max_len"] <= runs[0][0].shape[1] <= case["L"] + case["max_len"] + g
        assert torch.equal(runs[0][0][:, :case["L"]], prompt)
    with pytest.raises(NotImplementedError):
        hip.S.multi_speculative_sampling(prompt, dm, tm, 2, None, 4)                    # default strategy "beam"
    with pytest.raises(RuntimeError):
        hip.S.multi_speculative_sampling(prompt, dm, tm, 2, None, 4, strategy="bogus")


def test_accept_multi_kernel_vs_reference_rule(hip):
    """sd_accept_multi on synthetic rows against a literal restatement of the reference's replica scan
    (speculative_sampling.py:1611-1638): choice, run length, early stop on the first all-accepting replica, uniforms
    consumed, NaN / zero-q ratios."""
    import ctypes as C
    L_ = hip.L
    rng = np.random.default_rng(3)
    V, S, Lp = 64, 24, 5
    for trial in range(40):
        W, gamma = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        P = rng.random((W, S, V)).astype(np.float32)
        Q = rng.random((W, S, V)).astype(np.float32)
        if trial % 3 == 0:
            Q = P.copy()                                   # ratio exactly 1 -> always accepted
        if trial % 5 == 1:
            Q[:, Lp:, :] *= 4.0                            # low ratios -> early rejects
        seq = rng.integers(0, V, size=(W, S)).astype(np.int32)
        if trial % 7 == 2:
            P[0, Lp - 1, seq[0, Lp]] = 0.0
            Q[0, Lp - 1, seq[0, Lp]] = 0.0                 # 0/0 = NaN -> reject
        r = rng.random(W * gamma).astype(np.float32)
        # reference rule
        k = 0
        max_l, choice, allacc = 0, 0, False
        for w in range(W):
            cur_l, cur_all = 0, True
            for i in range(gamma):
                ri = torch.tensor([r[k]])
                k += 1
                j = int(seq[w, Lp + i])
                ratio = torch.tensor(P[w, Lp + i - 1, j]) / torch.tensor(Q[w, Lp + i - 1, j])
                if ri < torch.min(torch.tensor([1]), ratio):
                    cur_l += 1
                else:
                    cur_all = False
                    break
            if cur_l > max_l:
                max_l, choice = cur_l, w
                if cur_all:
                    allacc = True
                    break
        Pd, Qd = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
        sd_, rd = torch.from_numpy(seq).cuda(), torch.from_numpy(r).cuda()
        items = (L_.SdMultiItem * W)()
        for w in range(W):
            items[w].p_hist, items[w].q_hist, items[w].seq = Pd[w].data_ptr(), Qd[w].data_ptr(), sd_[w].data_ptr()
        res = torch.zeros(C.sizeof(L_.SdMultiResult), dtype=torch.uint8, device="cuda")
        L_.check(L_.lib.sd_accept_multi(items, W, V, Lp, gamma, rd.data_ptr(), 0, 0, res.data_ptr(), _st()),
                 "sd_accept_multi")
        out = L_.SdMultiResult.from_buffer_copy(res.cpu().numpy().tobytes())
        assert (out.choice, out.chosen.n_accepted, out.n_uniform, bool(out.chosen.flags & 4)) == \
            (choice, max_l, k, allacc), trial
        assert out.chosen.n == Lp + max_l - 1
        assert [out.chosen.drafted[i] for i in range(gamma)] == [int(x) for x in seq[choice, Lp:Lp + gamma]]


@pytest.mark.parametrize("case", G5_META["ar"], ids=[c["id"] for c in G5_META["ar"]])
def test_autoregressive_trace_golden(hip, case):
    cfg = load_config(case["cfg"])
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, case["seed"]), dtype=torch.float32)
    prompt = torch.from_numpy(G5[case["id"] + "_prompt"].astype(np.int64))[None].cuda()
    nz = hip.noise.ReplayNoise(events(G5, case["id"]), "cuda")
    out = hip.S.autoregressive_sampling(prompt, m, case["N"], case["eos"], rng=nz, **case["kwargs"])
    np.testing.assert_array_equal(out.cpu().numpy()[0], G5[case["id"] + "_out"])


def test_kvcache_model_api_matches_oracle(hip):
    """KVCacheModel drop-in: generate / rollback / _prob_history / _past_key_values against the oracle wrapper."""
    cfg = load_config("tiny-llama-target")
    sd = make_state_dict(cfg, 12)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    prompt = torch.from_numpy(np.random.default_rng(5).integers(3, cfg.vocab_size, size=(1, 9)))
    rec = oracle.RecordingNoise()
    torch.manual_seed(3)
    okv = oracle.RefKVCacheModel(oracle.RefCausalLM(cfg, sd), 1.0, 20, 0.9, noise=rec)
    ox = okv.generate(prompt, 4)
    kv = hip.S.KVCacheModel(m, 1.0, 20, 0.9, noise=hip.noise.ReplayNoise(rec.events, "cuda"))
    x = kv.generate(prompt.cuda(), 4)
    assert torch.equal(x.cpu(), ox)
    assert kv._prob_history.shape == okv._prob_history.shape
    assert float((kv._prob_history.cpu() - okv._prob_history).abs().max()) < 1e-5
    k, v = kv._past_key_values[0]
    ok, ov = okv._past_key_values[0]
    assert k.shape == ok.shape and float((k.cpu() - ok).abs().max()) < 1e-4
    kv.rollback(10)
    okv.rollback(10)
    assert kv._prob_history.shape == okv._prob_history.shape == (1, 10, cfg.vocab_size)
    assert kv._past_key_values[0][0].shape == okv._past_key_values[0][0].shape
    with pytest.raises(NotImplementedError):                      # its own arguments are transformers 4.35 objects
        kv.beam_sample()
    with pytest.raises(RuntimeError, match="before beam_sample_with_kv_cache"):
        kv.beam_rollback(0, 0)                                    # (the beam draft side itself: test_beam_speculative_sampling_v2_vs_oracle)


def test_batch_size_assert(hip):
    cfg = load_config("tiny-llama-draft")
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, 21), dtype=torch.float32)
    with pytest.raises(AssertionError, match="input batch size must be 1"):
        hip.S.speculative_sampling(torch.ones(2, 4, dtype=torch.int64).cuda(), m, m, 2, None, 4)


# --------------------------------------------------------------------------- kernel-level checks
@pytest.mark.parametrize("N,K", [(2304, 768), (5120, 13824), (32000, 768), (1024, 5120)])
def test_gemm_bf16_stream_vs_fp32_reference(hip, N, K):
    """The MFMA weight-streaming GEMM (tile-packed bf16 weights, split-K partials) against a plain PyTorch fp32
    matmul of the same bf16-rounded operands; fp32 accumulation both sides, so only the summation order differs."""
    g = torch.Generator(device="cuda").manual_seed(N + K)
    W = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    Wp = torch.empty_like(W)
    hip.L.check(hip.lib.sd_pack_weight_bf16(W.data_ptr(), Wp.data_ptr(), N, K, _st()))
    # the packed layout is a pure permutation of 16x32 tiles
    ref_pack = W.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(N, K)
    assert torch.equal(Wp, ref_pack)
    part = torch.empty(64 * 64 * N, dtype=torch.float32, device="cuda")
    for M in (1, 5, 16, 17, 33, 40, 64, 100, 128, 200, 256):          # 65+: the balanced kernel or gemm_bf16_mm
        x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        S = C.c_int(0)
        ref = x.float() @ W.float().t()
        if M <= 64:
            hip.L.check(hip.lib.sd_gemm_bf16(Wp.data_ptr(), x.data_ptr(), 0, M, N, K, part.data_ptr(), part.numel(),
                                             out.data_ptr(), C.byref(S), _st()))
            err = float((out - ref).abs().max())
            assert err <= 2e-4 * float(ref.abs().max()) + 1e-5, (M, N, K, S.value, err)
        # the same product with the activations in the operand layout the forward keeps them in (16-row tiles)
        Mp = (M + 15) // 16 * 16
        xt = torch.zeros(Mp * K, dtype=torch.bfloat16, device="cuda")
        hip.L.check(hip.lib.sd_pack_activation_bf16(x.data_ptr(), xt.data_ptr(), M, K, _st()))
        xpad = torch.zeros(Mp, K, dtype=torch.bfloat16, device="cuda")
        xpad[:M] = x
        assert torch.equal(xt, xpad.view(Mp // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1))
        if M > 64 and (N // 16) % 8 != 0:
            continue                                                   # more than 64 rows only through gemm_bf16_mm
        out2 = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        hip.L.check(hip.lib.sd_gemm_bf16(Wp.data_ptr(), xt.data_ptr(), 1, M, N, K, part.data_ptr(), part.numel(),
                                         out2.data_ptr(), C.byref(S), _st()))
        err2 = float((out2 - ref).abs().max())
        assert err2 <= 2e-4 * float(ref.abs().max()) + 1e-5, (M, N, K, S.value, err2)
        if M <= 16:
            assert torch.equal(out2, out), (M, N, K)                   # same kernel, same summation order
        # (17..64 rows in the tile layout take the balanced one-workgroup-per-CU kernel, rows_kernels.h: another k-split)


def test_norm_sample_fused_matches_two_step(hip):
    """sd_norm_sample == norm_logits followed by sample on the same noise, for the fast (k <= 64) and general paths."""
    for V, (T, k, p) in [(32000, (1.0, 20, 0.9)), (32000, (0.7, 50, 0.95)), (50272, (1.0, 20, 0.9)),
                         (4096, (1.0, 0, 0.9)), (4096, (1.0, 200, 0.0)), (512, (1.0, 0, 0.0)), (32000, (1.0, 1, 0.0))]:
        for i in range(4):
            x = logits_row(8800 + i, V, 3.0).cuda()
            noise = torch.empty(V).exponential_(1).cuda()
            probs = hip.S.norm_logits(x, T, k, p)
            want = hip.S.sample(probs, noise=hip.noise.ReplayNoise([("exp", noise.cpu())], "cuda"))
            out = torch.empty(V, dtype=torch.float32, device="cuda")
            tok = torch.zeros(1, dtype=torch.int32, device="cuda")
            err = torch.zeros(2, dtype=torch.int32, device="cuda")
            for ws in (None, torch.empty(hip.lib.sd_norm_workspace_bytes(1), dtype=torch.uint8, device="cuda")):
                out.fill_(-1.0)
                hip.L.check(hip.lib.sd_norm_sample(x.data_ptr(), V, T, k, p, 0, out.data_ptr(), err[0].data_ptr(),
                                                   noise.data_ptr(), 0, 0, tok.data_ptr(), err[1].data_ptr(),
                                                   ws.data_ptr() if ws is not None else None, _st()))
                assert torch.equal(out, probs[0])          # one-workgroup and 16-workgroup paths agree bit for bit
                assert int(tok) == int(want) and not bool(err.any())
            ref = oracle.sample(oracle.norm_logits(x.cpu(), T, k, p), oracle.RecordedNoise([("exp", noise.cpu()[None])]))
            assert int(tok) == int(ref)


# --------------------------------------------------------------------------- production head sizes / long prompts
MID_CFGS = {
    "llama_d128": dict(arch="llama", vocab_size=1024, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                       num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-5),
    "llama_d64_gqa": dict(arch="llama", vocab_size=1024, hidden_size=256, intermediate_size=704, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-6),
    "opt_d32_post": dict(arch="opt", vocab_size=1024, hidden_size=128, ffn_dim=256, num_hidden_layers=2,
                         num_attention_heads=4, max_position_embeddings=512, do_layer_norm_before=False,
                         word_embed_proj_dim=64),
    "opt_d64_pre": dict(arch="opt", vocab_size=1024, hidden_size=128, ffn_dim=512, num_hidden_layers=2,
                        num_attention_heads=2, max_position_embeddings=512, do_layer_norm_before=True,
                        word_embed_proj_dim=128),
}


@pytest.mark.parametrize("name", list(MID_CFGS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_production_head_dims_vs_oracle(hip, name, dtype):
    """Head dims 32 / 64 / 128 (the MFMA QK^T path), GQA, a 150-token prompt fed as 64-row chunks, then
    incremental steps of 1, 2, 5 and 9 rows (more rows than one attention row-group), against the oracle forward
    in the same dtype.  fp32: 1e-3 (north_star); bf16: the two bf16 pipelines round at the same points, so they
    agree to a few bf16 ulps of the logit scale."""
    from llmspeculativesampling_amd.config import ModelConfig
    cfg = ModelConfig(**MID_CFGS[name])
    sd = make_state_dict(cfg, 77, dtype=dtype)
    om = oracle.RefCausalLM(cfg, sd)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=dtype)
    ses = m.new_session(256)
    ids = torch.from_numpy(np.random.default_rng(9).integers(3, cfg.vocab_size, size=(1, 167)))
    past, pos = None, 0
    for q in (150, 1, 2, 5, 9):
        chunk = ids[:, pos:pos + q]
        o = om(chunk, past_key_values=past)
        past = o.past_key_values
        nl = min(q, 9)
        got = ses.forward(chunk[0].to(torch.int32).cuda(), nl).cpu()
        want = o.logits.float()[0, -nl:]
        scale = float(want.abs().max())
        tol = 1e-3 if dtype == torch.float32 else 0.04 * scale
        assert float((got - want).abs().max()) <= tol, (name, q, float((got - want).abs().max()), scale)
        pos += q
    k, v = ses.past_key_values()[1]
    ok, ov = past[1]
    ktol = 1e-4 if dtype == torch.float32 else 0.05
    assert float((k.float().cpu() - ok.float()).abs().max()) <= ktol * max(1.0, float(ok.float().abs().max()))
    assert float((v.float().cpu() - ov.float()).abs().max()) <= ktol * max(1.0, float(ov.float().abs().max()))


@pytest.mark.parametrize("name", ["llama_d128", "llama_d64_gqa", "opt_d32_post"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_forward_long_context_split_keys_vs_oracle(hip, name, dtype):
    """Contexts past 384 keys take the split-key attention path (each row group's keys cut over up to 8 workgroups,
    merged by attn_combine_kernel): a 900-token prompt in 64-row chunks, then steps of 1, 5 and 9 rows, against the
    oracle forward.  fp32 1e-3 (north_star).  bf16: on this path the softmax weights are not rounded to bf16 before
    P.V (the reference rounds them), so the bound is the same few-ulps-of-logit-scale one as the short-context test."""
    from llmspeculativesampling_amd.config import ModelConfig
    cfg = ModelConfig(**dict(MID_CFGS[name], max_position_embeddings=1024))
    sd = make_state_dict(cfg, 78, dtype=dtype)
    om = oracle.RefCausalLM(cfg, sd)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=dtype)
    ses = m.new_session(960)
    ids = torch.from_numpy(np.random.default_rng(10).integers(3, cfg.vocab_size, size=(1, 915)))
    past, pos = None, 0
    for q in (900, 1, 5, 9):
        chunk = ids[:, pos:pos + q]
        o = om(chunk, past_key_values=past)
        past = o.past_key_values
        nl = min(q, 9)
        got = ses.forward(chunk[0].to(torch.int32).cuda(), nl).cpu()
        want = o.logits.float()[0, -nl:]
        scale = float(want.abs().max())
        tol = 1e-3 if dtype == torch.float32 else 0.04 * scale
        assert float((got - want).abs().max()) <= tol, (name, q, float((got - want).abs().max()), scale)
        pos += q


@pytest.mark.parametrize("arch", ["llama", "opt"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_prefill_chunks_over_64_rows_vs_oracle(hip, dtype, arch):
    """Single-sequence calls carry up to 256 rows (positions implicit in the row table; bf16: the many-row
    GEMMs with their fused QKV / activation epilogues): a 230-token prompt in one call, 300 more
    in two, then decode steps, against the oracle forward; and the KV rows equal those of 64-row chunks closely."""
    from llmspeculativesampling_amd.config import ModelConfig
    if arch == "llama":
        cfg = ModelConfig(arch="llama", vocab_size=1024, hidden_size=512, intermediate_size=1024, num_hidden_layers=2,
                          num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=1024, rms_norm_eps=1e-5)
    else:
        cfg = ModelConfig(arch="opt", vocab_size=1024, hidden_size=512, ffn_dim=1024, num_hidden_layers=2,
                          num_attention_heads=8, max_position_embeddings=1024, do_layer_norm_before=True,
                          word_embed_proj_dim=512)
    sd = make_state_dict(cfg, 79, dtype=dtype)
    om = oracle.RefCausalLM(cfg, sd)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=dtype)
    assert hip.lib.sd_model_max_rows(m.handle) == 256
    ses, ses64 = m.new_session(600), m.new_session(600, max_rows=64)
    assert ses.max_rows == 256 and ses64.max_rows == 64
    ids = torch.from_numpy(np.random.default_rng(12).integers(3, cfg.vocab_size, size=(1, 545)))
    past, pos = None, 0
    for q in (230, 300, 1, 5, 9):
        chunk = ids[:, pos:pos + q]
        o = om(chunk, past_key_values=past)
        past = o.past_key_values
        nl = min(q, 9)
        got = ses.forward(chunk[0].to(torch.int32).cuda(), nl).cpu()
        ses64.forward(chunk[0].to(torch.int32).cuda(), nl)
        want = o.logits.float()[0, -nl:]
        scale = float(want.abs().max())
        tol = 1e-3 if dtype == torch.float32 else 0.04 * scale
        assert float((got - want).abs().max()) <= tol, (q, float((got - want).abs().max()), scale)
        pos += q
    ktol = 1e-4 if dtype == torch.float32 else 0.05
    ref = ses64.kv[:, :, :, :pos].float()
    assert float((ses.kv[:, :, :, :pos].float() - ref).abs().max()) <= ktol * max(1.0, float(ref.abs().max()))


def test_speculative_bf16_statistics_vs_oracle(hip):
    """bf16 end to end (fused epilogues, MFMA attention): same recorded noise into the oracle's bf16 CPU run and the
    HIP run.  bf16 rounding-order differences may flip an occasional token, so the bar is statistical: accept-length
    histograms within a few counts and most iterations token-identical until the first divergence."""
    from llmspeculativesampling_amd.config import ModelConfig
    from llmspeculativesampling_amd.synth import perturb_state_dict
    cfg = ModelConfig(**MID_CFGS["llama_d64_gqa"])
    dsd = make_state_dict(cfg, 5, dtype=torch.bfloat16)
    tsd = {k2: v2.to(torch.bfloat16) for k2, v2 in perturb_state_dict({k3: v3.float() for k3, v3 in dsd.items()}, 6, 0.08).items()}
    prompt = torch.from_numpy(np.random.default_rng(3).integers(3, cfg.vocab_size, size=(1, 24)))
    rec = oracle.RecordingNoise()
    torch.manual_seed(11)
    want, wd = oracle.speculative_sampling(prompt, oracle.RefCausalLM(cfg, dsd), oracle.RefCausalLM(cfg, tsd), 2, None,
                                           40, gamma=4, top_k=20, top_p=0.9, details=True, noise=rec)
    dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.bfloat16)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.bfloat16)
    torch.manual_seed(11)
    got, gd = hip.S.speculative_sampling(prompt.cuda(), dm, tm, 2, None, 40, gamma=4, top_k=20, top_p=0.9, details=True)
    w, g = want[0].tolist(), got[0].cpu().tolist()
    common = 0
    for a, b in zip(w, g):
        if a != b:
            break
        common += 1
    assert common >= 24 + 8, (common, w, g)                 # identical well past the prompt
    assert abs(float(np.mean(gd["acc_len"])) - float(np.mean(wd["acc_len"]))) <= 1.0
    assert abs(float(gd["acc_rate"]) - float(wd["acc_rate"])) <= 0.15


def test_native_iteration_matches_python_loop(hip, capsys):
    """sd_spec_generate (the native loop, one stream wait per iteration, device Philox) == the Python-orchestrated loop with the
    same Philox seed (verbose=True keeps the Python path), incl. the random_seed quirk and an all-accept pair."""
    from llmspeculativesampling_amd.synth import perturb_state_dict
    cfg = load_config("tiny-llama-target")
    dsd = make_state_dict(cfg, 11)
    prompt = torch.from_numpy(np.random.default_rng(2).integers(3, cfg.vocab_size, size=(1, 70))).cuda()   # > 64: chunked prefill
    for tsd, kw in ((perturb_state_dict(dsd, 12, 0.12), dict(top_k=20, top_p=0.9)),
                    (perturb_state_dict(dsd, 12, 0.12), dict(top_k=20, top_p=0.9, random_seed=42)),
                    (dsd, dict(top_k=10, top_p=0.0, gamma=3))):
        dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.float32)
        tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.float32)
        a, da = hip.S.speculative_sampling(prompt, dm, tm, 2, None, 30, details=True, rng=hip.noise.DeviceNoise(77), **kw)
        b, db = hip.S.speculative_sampling(prompt, dm, tm, 2, None, 30, details=True, rng=hip.noise.DeviceNoise(77),
                                           verbose=True, **kw)
        capsys.readouterr()
        assert torch.equal(a, b)
        assert da["acc_len"] == db["acc_len"] and da["target_call_times"] == db["target_call_times"]
        assert abs(float(da["acc_rate"]) - float(db["acc_rate"])) < 1e-9


def test_get_score_matches_oracle(hip):
    """evaluation.py:109-132 get_score (the harness's untimed quality proxy) through the engine vs torch-CPU."""
    from llmspeculativesampling_amd.quality import get_score
    cfg = load_config("tiny-llama-target")
    sd = make_state_dict(cfg, 12)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    out = torch.from_numpy(np.random.default_rng(4).integers(3, cfg.vocab_size, size=(1, 90)))     # > 64 rows: chunked
    got = float(get_score(out.cuda(), m, 20))
    lg = oracle.RefCausalLM(cfg, sd)(out).logits[:, :-1, :]
    lp = torch.gather(torch.log_softmax(lg, -1), -1, out[:, 1:, None])
    want = float(lp[:, 19:, :].mean())
    assert abs(got - want) < 1e-4


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_batch_forward_equals_per_stream_forward(hip, dtype):
    """sd_batch_forward: three sequences of different lengths share one pass over the weights; every stream's logits and
    KV rows equal what its own sd_session_forward produces (fp32: bit-exact, the rows are independent)."""
    from llmspeculativesampling_amd.config import ModelConfig
    cfg = ModelConfig(**MID_CFGS["llama_d64_gqa"]) if dtype == torch.bfloat16 else load_config("tiny-llama-target")
    sd = make_state_dict(cfg, 31, dtype=dtype)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=dtype)
    rng = np.random.default_rng(8)
    lens, new, nlog = [17, 40, 9], [1, 2, 5], [1, 1, 5]
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
    if dtype == torch.float32:
        assert torch.equal(got, want)
    else:
        assert float((got - want).abs().max()) <= 0.03 * float(want.abs().max())
    for a, b, L, n in zip(solo, both, lens, new):
        assert a.cache_len == b.cache_len == L + n
        ka, kb = a.past_key_values()[-1][0], b.past_key_values()[-1][0]
        assert torch.equal(ka, kb) if dtype == torch.float32 else float((ka.float() - kb.float()).abs().max()) < 0.05


@pytest.mark.parametrize("kw", [dict(top_k=20, top_p=0.9), dict(top_k=20, top_p=0.9, random_seed=42), dict(top_k=5, top_p=0.0, gamma=2)],
                         ids=["plain", "seeded", "gamma2"])
def test_stream_batched_decode_equals_per_stream(hip, kw):
    """speculative_sampling_batch: 5 streams of different prompt lengths decode in lockstep through shared weight passes;
    every stream's tokens / accepted lengths equal its own single-stream speculative_sampling run with the same Philox
    seed (fp32: the rows of a pass are computed independently, so this is bit-exact), incl. a stream that stops early
    at EOS while the others go on."""
    from llmspeculativesampling_amd.synth import perturb_state_dict
    cfg = load_config("tiny-llama-target")
    dsd = make_state_dict(cfg, 11)
    tsd = perturb_state_dict(dsd, 12, 0.12)
    dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.float32)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.float32)
    rng = np.random.default_rng(21)
    prompts = [torch.from_numpy(rng.integers(3, cfg.vocab_size, size=(1, L))).cuda() for L in (9, 30, 70, 2, 17)]
    seeds = [900 + i for i in range(len(prompts))]
    # choose an EOS id that stream 1 is known to generate early (from its own single-stream run)
    probe = hip.S.speculative_sampling(prompts[1], dm, tm, -1, None, 24, rng=hip.noise.DeviceNoise(seeds[1]), **kw)
    eos = int(probe[0, prompts[1].shape[1] + 3])
    singles = [hip.S.speculative_sampling(p, dm, tm, eos, None, 24, details=True, rng=hip.noise.DeviceNoise(sd), **kw)
               for p, sd in zip(prompts, seeds)]
    outs, ds = hip.S.speculative_sampling_batch(prompts, dm, tm, eos, None, 24, details=True, seeds=seeds, **kw)
    lens = set()
    for (so, sdet), bo, bd in zip(singles, outs, ds):
        assert torch.equal(so, bo), (so, bo)
        assert sdet["acc_len"] == bd["acc_len"]
        assert abs(float(sdet["acc_rate"]) - float(bd["acc_rate"])) < 1e-9
        lens.add(bo.shape[1])
    assert singles[1][0].shape[1] < prompts[1].shape[1] + 24          # the EOS stream really stopped early


def test_config1_full_size_opt_pair_fp32_vs_oracle(hip):
    """BASELINE configs[0] at full size: opt-125m draft -> opt-350m target (post-LN, 512<->1024 projections, V=50272),
    fp32, gamma=4, top_k 20, top_p 0.9, a 128-token prompt (SURVEY.md 8(d) C1 inputs; max_len shortened to bound the
    CPU time of the oracle).  Same random-init weights, the oracle's recorded noise replayed into the HIP path: identical
    token ids and accepted lengths, fp32 logits of the prefill within 1e-3."""
    dcfg, tcfg = load_config("opt-125m"), load_config("opt-350m")
    dsd, tsd = make_state_dict(dcfg, 0), make_state_dict(tcfg, 1)
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(4, tcfg.vocab_size, (1, 128), generator=g)
    od, ot = oracle.RefCausalLM(dcfg, dsd), oracle.RefCausalLM(tcfg, tsd)
    rec = oracle.RecordingNoise()
    torch.manual_seed(123)
    want, wd = oracle.speculative_sampling(prompt, od, ot, 2, None, 12, gamma=4, top_k=20, top_p=0.9, details=True, noise=rec)
    dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.float32)
    tm = hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.float32)
    # logits of the target prefill against the oracle forward
    ses = tm.new_session(160)
    got_logits = ses.forward(prompt[0].to(torch.int32).cuda(), 4).cpu()
    ref_logits = ot(prompt).logits[0, -4:].float()
    assert float((got_logits - ref_logits).abs().max()) <= 1e-3
    got, gd = hip.S.speculative_sampling(prompt.cuda(), dm, tm, 2, None, 12, gamma=4, top_k=20, top_p=0.9, details=True,
                                         rng=hip.noise.ReplayNoise(rec.events, "cuda"))
    assert torch.equal(got.cpu(), want)
    assert gd["acc_len"] == wd["acc_len"]


def test_error_paths_match_reference_exceptions(hip, capsys):
    """NaN logits -> RuntimeError('norm logits error') from norm_logits and wrapped as RuntimeError('s') by
    speculative_sampling (reference utils.py:203-207, speculative_sampling.py:2044-2046), on both loop implementations."""
    cfg = load_config("tiny-llama-draft")
    sd = make_state_dict(cfg, 21)
    bad = {k: v.clone() for k, v in sd.items()}
    bad["lm_head.weight"][7, :] = float("nan")                   # every logit row gets a NaN at token 7
    good = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    broken = hip.engine.SpecDecModel.from_state_dict(cfg, bad, dtype=torch.float32)
    prompt = torch.arange(3, 12, dtype=torch.int64)[None].cuda()
    with pytest.raises(RuntimeError, match="norm logits error"):
        hip.S.KVCacheModel(broken, 1.0, 20, 0.9)._forward_with_kvcache(prompt)
    for rng in ("host", "device"):
        with pytest.raises(RuntimeError, match="^s$"):
            hip.S.speculative_sampling(prompt, good, broken, 2, None, 8, top_k=20, top_p=0.9, rng=rng)
        with pytest.raises(RuntimeError, match="^s$"):
            hip.S.speculative_sampling(prompt, broken, good, 2, None, 8, top_k=20, top_p=0.9, rng=rng)
    capsys.readouterr()
    # the engine refuses what it cannot hold instead of writing out of bounds
    ses = good.new_session(16)
    with pytest.raises(hip.L.SpecDecError, match="capacity"):
        ses.forward(torch.zeros(17, dtype=torch.int32, device="cuda"), 1)


def test_kvcache_full_history_long_prefill(hip):
    """Standalone KVCacheModel (full_history, the reference's behaviour): a 150-token prompt is normalised for every
    position, in chunks, and matches the oracle wrapper's (1, S, V) history."""
    cfg = load_config("tiny-llama-target")
    sd = make_state_dict(cfg, 12)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    prompt = torch.from_numpy(np.random.default_rng(6).integers(3, cfg.vocab_size, size=(1, 150)))
    okv = oracle.RefKVCacheModel(oracle.RefCausalLM(cfg, sd), 0.9, 30, 0.95)
    last = okv._forward_with_kvcache(prompt)
    kv = hip.S.KVCacheModel(m, 0.9, 30, 0.95)
    got = kv._forward_with_kvcache(prompt.cuda())
    assert kv._prob_history.shape == okv._prob_history.shape == (1, 150, cfg.vocab_size)
    assert float((kv._prob_history.cpu() - okv._prob_history).abs().max()) < 2e-5
    assert torch.equal(kv._prob_history.cpu() > 0, okv._prob_history > 0)
    assert float((got.cpu() - last).abs().max()) < 2e-5


def test_host_rng_autoregressive_matches_reference_seed(hip):
    """autoregressive_sampling with the default host RNG reproduces the reference's run under its outer seed."""
    case = G5_META["ar"][0]
    cfg = load_config(case["cfg"])
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, case["seed"]), dtype=torch.float32)
    prompt = torch.from_numpy(G5[case["id"] + "_prompt"].astype(np.int64))[None].cuda()
    torch.manual_seed(77)
    out = hip.S.autoregressive_sampling(prompt, m, case["N"], case["eos"], **case["kwargs"])
    np.testing.assert_array_equal(out.cpu().numpy()[0], G5[case["id"] + "_out"])


def test_evaluation_driver_runs_offline(tmp_path):
    """tools/evaluate_offline.py (the reference driver's three loops) end to end on tiny models and
    synthetic prompts: every loop prints its result lines in the reference's wording."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = tmp_path / "log.txt"
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "evaluate_offline.py"), "--approx_model_name",
                        "tiny-llama-draft", "--target_model_name", "tiny-llama-target", "--n-prompts", "40",
                        "--max_tokens", "8", "--repeats", "1", "--dtype", "float32", "--seed", "7", "--log_file",
                        str(log)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = log.read_text()
    assert "large model total time" in text and "google speculative decoding (with KVCache) total time" in text
    assert "iid multi-draft speculative decoding (gamma 4, width 2) total time" in text
    assert text.count("average accepted len") == 2 and text.count("power/token:") == 3


@pytest.mark.parametrize("L,gamma,max_len,width", [(1, 4, 6, 1), (9, 1, 7, 1), (9, 16, 20, 1), (12, 4, 0, 1), (7, 5, 3, 1),
                                                   (1, 3, 5, 3), (9, 4, 0, 2), (6, 2, 9, 8)],
                         ids=["prompt1", "gamma1", "gamma16", "maxlen0", "T_mid_iteration", "multi_prompt1", "multi_maxlen0",
                              "multi_width8"])
def test_edge_shapes_vs_oracle(hip, L, gamma, max_len, width):
    """Edge shapes of the loops (one-token prompt, gamma 1 and 16, max_len 0, a target length reached in the middle of an
    iteration, width 8): the oracle (pinned to the reference by G4/G5/G7) runs with live noise that is recorded, the HIP
    path replays that noise and must produce the same tokens and statistics."""
    from llmspeculativesampling_amd.synth import perturb_state_dict
    cfg = load_config("tiny-llama-target")
    dsd = make_state_dict(cfg, 11)
    tsd = perturb_state_dict(dsd, 12, 0.15)
    prompt = torch.from_numpy(np.random.default_rng([L, gamma]).integers(3, cfg.vocab_size, size=(1, L)))
    rec = oracle.RecordingNoise()
    torch.manual_seed(1000 + L + gamma)
    od, ot = oracle.RefCausalLM(cfg, dsd), oracle.RefCausalLM(cfg, tsd)
    kw = dict(gamma=gamma, top_k=20, top_p=0.9, details=True)
    if width == 1:
        want, dw = oracle.speculative_sampling(prompt, od, ot, 2, None, max_len, noise=rec, **kw)
    else:
        want, dw = oracle.multi_speculative_sampling(prompt, od, ot, 2, None, max_len, width=width, strategy="iid",
                                                     noise=rec, **kw)
    dm = hip.engine.SpecDecModel.from_state_dict(cfg, dsd, dtype=torch.float32)
    tm = hip.engine.SpecDecModel.from_state_dict(cfg, tsd, dtype=torch.float32)
    nz = hip.noise.ReplayNoise(rec.events, "cuda")
    if width == 1:
        got, dg = hip.S.speculative_sampling(prompt.cuda(), dm, tm, 2, None, max_len, rng=nz, **kw)
    else:
        got, dg = hip.S.multi_speculative_sampling(prompt.cuda(), dm, tm, 2, None, max_len, width=width, strategy="iid",
                                                   rng=nz, **kw)
    assert torch.equal(got.cpu(), want)
    assert dg["acc_len"] == dw["acc_len"] and dg["target_call_times"] == dw["target_call_times"]
    assert nz.exhausted()
    if max_len == 0:
        assert torch.equal(got.cpu(), prompt) and dg["target_call_times"] == 0


def test_autoregressive_edge_shapes_vs_oracle(hip):
    """autoregressive_sampling: N = 0 returns the prompt, a one-token prompt, N = 1."""
    cfg = load_config("tiny-opt-post")
    sd = make_state_dict(cfg, 43)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    for L, N in ((5, 0), (1, 4), (3, 1)):
        prompt = torch.from_numpy(np.random.default_rng([L, N]).integers(3, cfg.vocab_size, size=(1, L)))
        rec = oracle.RecordingNoise()
        torch.manual_seed(50 + L)
        want = oracle.autoregressive_sampling(prompt, oracle.RefCausalLM(cfg, sd), N, 2, top_k=10, top_p=0.9, noise=rec)
        got = hip.S.autoregressive_sampling(prompt.cuda(), m, N, 2, top_k=10, top_p=0.9,
                                            rng=hip.noise.ReplayNoise(rec.events, "cuda"))
        assert torch.equal(got.cpu(), want)


# --------------------------------------------------------------------------- G8: 16-bit probability rows (OPT, config 3)
G8_META, G8 = load("g8_lowprec")


def _sparse_row(V, idx, val, dtype=torch.float32):
    return torch.from_numpy(dense_from_sparse(V, idx, val))[None].to(dtype)


@pytest.mark.parametrize("case", G8_META["norm"], ids=[c["id"] for c in G8_META["norm"]])
def test_lowprec_norm_probs_golden(hip, case):
    """norm_logits on bf16 / fp16 rows at the real vocabularies, recorded from the reference: bit-exact (every value is a
    16-bit number), up to the reference's unspecified order inside runs of equal logits at the top-p cut."""
    dt = DT[case["dtype"]]
    x = logits_row(case["seed"], case["V"], case["scale"], dtype=dt)
    want = dense_from_sparse(case["V"], G8[case["id"] + "_idx"], G8[case["id"] + "_val"])
    got = hip.S.norm_logits(x.cuda(), case["T"], case["k"], case["p"])
    assert got.dtype == dt
    g = got.float().cpu().numpy()[0]
    if not case["tie_sensitive"]:
        np.testing.assert_array_equal(g, want)
    else:
        assert_rows_equal_up_to_tied_logits(g, want, (x.float() / case["T"]).to(dt).float().numpy()[0])


@pytest.mark.parametrize("case", G8_META["sample"], ids=[c["id"] for c in G8_META["sample"]])
def test_lowprec_sample_golden(hip, case):
    dt = DT[case["dtype"]]
    probs = _sparse_row(case["V"], G8[case["id"] + "_pidx"], G8[case["id"] + "_pval"], dt)
    noise = torch.from_numpy(G8[case["id"] + "_noise"].copy())
    tok = hip.S.sample(probs.cuda(), noise=hip.noise.ReplayNoise([("exp", noise)], "cuda"))
    assert int(tok) == case["token"]


@pytest.mark.parametrize("case", G8_META["max_fn"], ids=[c["id"] for c in G8_META["max_fn"]])
def test_lowprec_max_fn_golden(hip, case):
    dt = DT[case["dtype"]]
    p = _sparse_row(case["V"], G8[case["id"] + "_pidx"], G8[case["id"] + "_pval"], dt).cuda()
    q = _sparse_row(case["V"], G8[case["id"] + "_qidx"], G8[case["id"] + "_qval"], dt).cuda()
    want = dense_from_sparse(case["V"], G8[case["id"] + "_ridx"], G8[case["id"] + "_rval"])
    got = hip.S.max_fn(p - q)
    assert got.dtype == dt
    np.testing.assert_array_equal(got.float().cpu().numpy()[0], want)


@pytest.mark.parametrize("case", G8_META["trace"], ids=[c["id"] for c in G8_META["trace"]])
def test_lowprec_accept_resample_kernels_golden(hip, case):
    """The reference's loop over position-table models with 16-bit logits, replayed through the HIP kernels in
    SD_NORM_DT_* mode (norm rows, draft samples, accept scan, max_fn(p - q) residual, bonus sample): ids and accepted
    lengths of the recorded run.  Cases whose recorded run depends on the reference's unspecified tie order are only
    required to run to completion with valid tokens."""
    dt = DT[case["dtype"]]
    mode = hip.L.SD_NORM_DT_BF16 if dt == torch.bfloat16 else hip.L.SD_NORM_DT_F16
    rng = np.random.default_rng(case["table_seed"])
    V, S, L0, gamma = case["V"], case["S"], case["L"], case["gamma"]
    z = rng.standard_normal((S, V), dtype=np.float32) * 2.0
    eps = rng.standard_normal((S, V), dtype=np.float32) * 2.0
    prompt = rng.integers(3, V, size=(1, L0))
    q_hist = hip.S.norm_logits(torch.from_numpy(z).to(dt).cuda(), 1.0, case["top_k"], case["top_p"]).float().contiguous()
    p_hist = hip.S.norm_logits(torch.from_numpy(z + np.float32(case["sigma"]) * eps).to(dt).cuda(), 1.0, case["top_k"],
                               case["top_p"]).float().contiguous()
    nz = hip.noise.ReplayNoise(events(G8, case["id"]), "cuda")
    want = G8[case["id"] + "_out"]
    seq = torch.zeros(S + 8, dtype=torch.int32, device="cuda")
    seq[:L0] = torch.from_numpy(prompt[0].astype(np.int32)).cuda()
    host = list(prompt[0])
    T = L0 + case["max_len"]
    res = torch.zeros(C.sizeof(hip.L.SdAcceptResult), dtype=torch.uint8, device="cuda")
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    acc_len = []
    lib = hip.lib
    try:
        while len(host) < T:
            L = len(host)
            for i in range(gamma):
                e = nz.exponential(V)
                hip.L.check(lib.sd_sample(q_hist[L + i - 1].data_ptr(), V, e.data_ptr(), 0, 0, seq[L + i].data_ptr(),
                                          err.data_ptr(), mode, _st()))
            nz.skip_exponential(V)
            r, token = nz.uniforms(gamma, case["random_seed"])
            hip.L.check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), V, seq.data_ptr(), L, gamma,
                                           r.data_ptr(), 0, 0, res.data_ptr(), _st()))
            out = hip.L.SdAcceptResult.from_buffer_copy(res.cpu().numpy().tobytes())
            nz.realign(token, min(out.n_accepted + 1, gamma))
            e = nz.exponential(V)
            hip.L.check(lib.sd_resample(p_hist.data_ptr(), q_hist.data_ptr(), V, V, seq.data_ptr(), L, gamma,
                                        e.data_ptr(), 0, 0, res.data_ptr(), None, mode, _st()))
            out = hip.L.SdAcceptResult.from_buffer_copy(res.cpu().numpy().tobytes())
            assert not (out.flags & 2)
            acc_len.append(out.n_accepted)
            host = host + seq[L:L + out.n_accepted].cpu().tolist() + [out.next_token]
            if 2 in host[L0:]:
                host = host[:L0 + host[L0:].index(2) + 1]
                break
    except RuntimeError:
        if not case["tie_sensitive"]:
            raise
        return                                                    # the replayed noise no longer lines up: expected
    if not case["tie_sensitive"]:
        np.testing.assert_array_equal(np.array(host), want)
        assert acc_len == case["acc_len"]
    else:
        assert all(0 <= t < V for t in host)


# --------------------------------------------------------------------------- G10: the stand-alone filter on 16-bit rows
G10_META, G10 = load("g10_filter_lowprec")


@pytest.mark.parametrize("case", G10_META, ids=[c["id"] for c in G10_META])
def test_lowprec_top_k_top_p_filter_golden(hip, case):
    """sampling.utils.top_k_top_p_filter on a bf16 / fp16 tensor (sd_topk_topp_filter with its dtype mode):
    in place, returns its argument, and keeps exactly the set the reference kept (reference utils.py:152-179 run in the
    row dtype) - up to the reference's unspecified order inside a run of equal logits at the top-p cut."""
    dt = DT[case["dtype"]]
    x = logits_row(case["seed"], case["V"], case["scale"], dtype=dt)
    xd = x.cuda()
    y = hip.S.top_k_top_p_filter(xd, case["k"], case["p"])
    assert y is xd and y.dtype == dt
    g = y.float().cpu().numpy()[0]
    kept = np.nonzero(np.isfinite(g))[0]
    want = G10[case["id"] + "_kept"]
    z = x.float().numpy()[0]
    np.testing.assert_array_equal(g[kept], z[kept])              # kept logits are untouched
    wants = [want]
    if case.get("sum_order_sensitive"):
        # the cut of this row hinges on the last bit of torch's fp32 softmax denominator, i.e. on the order in which its
        # vectorised CPU kernel adds 50272 terms (make_golden.py: an exactly rounded softmax moves the cut by one token):
        # either of the two recorded sets is a faithful answer
        wants.append(G10[case["id"] + "_kept_exact_softmax"])

    def same(w):
        if not case["tie_sensitive"]:
            return np.array_equal(kept, w)
        return len(kept) == len(w) and np.array_equal(np.sort(z[kept]), np.sort(z[w]))   # same logit multiset: twins at the cut
    assert any(same(w) for w in wants), (len(kept), [len(w) for w in wants])
