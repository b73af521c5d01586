"""Prompt-lookup drafting, what needs no GPU: sampling.utils.lookup_propose against the reference definition on an exhaustive
sweep, the C entries' refusals in their order (they come before any launch), the Python ValueErrors, and the admissibility of
the fixed prompts / seeds of tests/test_gpu_lookup_parity.py, justified on tests/lookup_reference.py alone and printed."""
import itertools
import types

import numpy as np
import pytest
import torch

import lookup_reference as R
from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.sampling import prompt_lookup_sampling, prompt_lookup_sampling_batch
from llmspeculativesampling_amd.sampling.utils import lookup_propose

P = 0x1000                                                        # a placeholder pointer: every refusal comes before any use


def test_lookup_propose_equals_the_reference_on_every_short_sequence():
    """All sequences over a 3-token alphabet up to length 9, gamma in {1, 4}, N in {1, 3}, m in {1, N}: the longest match before
    a more recent one, the most recent among equals, an overlap with the key, m cutting a short match, wrap-around, L = 1."""
    n = 0
    seen = dict(longer_older=0, overlap=0, cut_by_m=0, wrap=0, none=0)
    for L in range(1, 10):
        for seq in itertools.product(range(3), repeat=L):
            for g, N in itertools.product((1, 4), (1, 3)):
                for m in sorted({1, N}):
                    d, k, c = R.propose(seq, g, N, m)
                    assert lookup_propose(list(seq), g, N, m) == (d.tolist(), k, c), (seq, g, N, m)
                    n += 1
                    seen["none"] += k == 0
                    seen["wrap"] += k > 0 and c + g > L
                    seen["overlap"] += k > 0 and c > L - k         # the match reaches into the key
                    seen["cut_by_m"] += m > 1 and k == 0 and R.propose(seq, g, N, 1)[1] > 0
                    seen["longer_older"] += k > 1 and any(seq[c2 - 1] == seq[L - 1] for c2 in range(c + 1, L))
    print(n, "cases;", seen)
    assert all(v > 0 for v in seen.values())
    assert lookup_propose([7], 4) == ([7, 7, 7, 7], 0, 0)          # L = 1: c = L - 1 = 0, the token repeated
    assert lookup_propose(torch.tensor([[1, 2, 3, 1, 2]]), 4, 3, 1) == ([3, 1, 2, 3], 2, 2)
    assert lookup_propose(np.array([5, 5, 5]), 3, 3, 1) == ([5, 5, 5], 2, 2)   # period 1, overlap with the key


def _propose(items=None, n_items=1, V=128, ld=128, gamma=4, nmax=3, nmin=1):
    items = (_lib.SdLookupItem * 16)(*[_lib.SdLookupItem(P, 5, P, P)] * 16) if items is None else items
    rc = _lib.lib.sd_lookup_propose(items, n_items, V, ld, gamma, nmax, nmin, None)
    return rc, _lib.lib.sd_last_error().decode()


def test_sd_lookup_propose_refusals_in_order():
    def refused(text, **kw):
        rc, msg = _propose(**kw)
        assert rc == _lib.SD_ERR_INVALID and msg.startswith("sd_lookup_propose: ") and text in msg, msg
    bad = (_lib.SdLookupItem * 2)(_lib.SdLookupItem(P, 5, P, P), _lib.SdLookupItem(P, 0, None, P))
    assert _lib.lib.sd_lookup_propose(None, 0, 0, 0, 0, 0, 0, None) == _lib.SD_ERR_INVALID
    assert "null argument" in _lib.lib.sd_last_error().decode()
    everything = dict(items=bad, n_items=17, V=0, ld=-1, gamma=17, nmax=9, nmin=0)
    refused("n_items 17 outside 1..16", **everything)
    everything["n_items"] = 2
    refused("gamma 17 outside 1..16", **everything)
    refused("gamma 0 outside 1..16", **{**everything, "gamma": 0})
    everything["gamma"] = 16
    refused("ngram_max 9 outside 1..8", **everything)
    refused("ngram_max 0 outside 1..8", **{**everything, "nmax": 0})
    everything["nmax"] = 8
    refused("ngram_min 0 outside 1..ngram_max 8", **everything)
    refused("ngram_min 4 outside 1..ngram_max 3", **{**everything, "nmax": 3, "nmin": 4})
    everything["nmin"] = 8
    refused("V 0 < 1", **everything)
    refused("ld 127 < V", **{**everything, "V": 128, "ld": 127})
    everything.update(V=128, ld=128)
    refused("item 1: null argument", **everything)
    bad[1].q_hist = P
    refused("item 1: L 0 < 1", **everything)
    refused("n_items 0 outside 1..16", n_items=0)


def _blocks(temperature=1.0, ws=None, rows=64):
    head = _lib.SdHeadScratch(logits=P, ld_logits=128, norm_mode=0)
    sampling = _lib.SdSampling(temperature=temperature, top_k=20, top_p=0.9, V=128, ld=128, eos_token_id=2)
    scratch = _lib.SdSpecScratch(draft=_lib.SdHeadScratch(), target=head, norm_workspace=ws, max_rows_per_forward=rows)
    return sampling, scratch


def test_sd_lookup_generate_refusals_follow_sd_spec_generate_with_the_draft_added():
    host = np.zeros(64, dtype=np.int32)

    def call(dev, gamma=4, nmax=3, nmin=1, **kw):
        sampling, scratch = _blocks(**kw)
        st = _lib.SdSeqState(host_seq=host.ctypes.data, len=5, T=20, max_iters=4, n_iters=-7, err=-7)
        rc = _lib.lib.sd_lookup_generate(dev, gamma, nmax, nmin, sampling, scratch, st, None, None)
        assert rc == _lib.SD_ERR_INVALID and (st.n_iters, st.err) == (-7, -7)
        msg = _lib.lib.sd_last_error().decode()
        assert msg.startswith("sd_lookup_generate: "), msg
        return msg
    ok = lambda draft=None: _lib.SdSpecStream(draft, P, P, P, P, P, P, P)
    assert "null argument" in call(_lib.SdSpecStream(None, None, P, P, P, P, P, P), gamma=0)
    assert "null argument" in call(None)
    assert "dev->draft must be NULL" in call(ok(P), gamma=0, nmax=0, temperature=0.0)
    assert "gamma 17 outside 1..16" in call(ok(), gamma=17, nmax=0, temperature=0.0)
    assert "ngram_max 0 outside 1..8" in call(ok(), nmax=0, nmin=0, temperature=0.0)
    assert "ngram_min 0 outside" in call(ok(), nmin=0, temperature=0.0)
    assert "temperature must be non-zero" in call(ok(), temperature=0.0, ws=P, rows=4)
    assert "a norm workspace of 4 rows" in call(ok(), ws=P, rows=4)


def test_sd_lookup_batch_generate_refusals():
    def call(streams, n=1, gamma=4, nmax=3, nmin=1, **kw):
        sampling, scratch = _blocks(**kw)
        log = _lib.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7)
        rc = _lib.lib.sd_lookup_batch_generate(streams, n, gamma, nmax, nmin, sampling, scratch, log, None, None)
        assert rc == _lib.SD_ERR_INVALID and (log.n_iters, log.err) == (-7, -7)
        msg = _lib.lib.sd_last_error().decode()
        assert msg.startswith("sd_lookup_batch_generate: "), msg
        return msg
    streams = (_lib.SdBatchStream * 2)()
    assert "null argument" in call(None)
    assert "n_streams 17 outside 1..16" in call(streams, n=17, gamma=0)
    assert "gamma 0 outside 1..16" in call(streams, gamma=0, nmax=9)
    assert "ngram_max 9 outside 1..8" in call(streams, nmax=9, nmin=0)
    assert "ngram_min 2 outside 1..ngram_max 1" in call(streams, nmax=1, nmin=2, temperature=0.0)
    assert "temperature must be non-zero" in call(streams, temperature=0.0)
    assert "stream 0: null pointer" in call(streams)
    for f in ("draft", "target", "seq", "q_hist", "p_hist", "err_words", "res_dev", "res_host", "host_seq"):
        setattr(streams[0], f, P)
    assert "stream 0: a draft session" in call(streams)


def test_python_entries_raise_value_error_before_a_model_is_touched():
    class Untouchable:
        tp_group = None
        cfg = types.SimpleNamespace(is_encoder_decoder=False)

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched: {name}")
    m, x = Untouchable(), torch.zeros((1, 4), dtype=torch.int64)
    for kw, text in ((dict(rng="host"), "device RNG"), (dict(rng=None), "device RNG"), (dict(temperature=0), "temperature"),
                     (dict(gamma=0), "gamma"), (dict(gamma=17), "gamma"), (dict(ngram_max=9), "ngram_max"),
                     (dict(ngram_max=0), "ngram_max"), (dict(ngram_min=0), "ngram_min"), (dict(ngram_max=2, ngram_min=3), "ngram_min")):
        with pytest.raises(ValueError, match=text):
            prompt_lookup_sampling(x, m, 2, None, 8, **kw)
        if "rng" not in kw:
            with pytest.raises(ValueError, match=text):
                prompt_lookup_sampling_batch([x], m, 2, None, 8, **kw)
    tp = types.SimpleNamespace(tp_group=object(), cfg=types.SimpleNamespace(is_encoder_decoder=False))
    encdec = types.SimpleNamespace(config=types.SimpleNamespace(is_encoder_decoder=True))
    for model, text in ((tp, "tensor-parallel"), (encdec, "encoder-decoder")):
        with pytest.raises(ValueError, match=text):
            prompt_lookup_sampling(x, model, 2, None, 8)
        with pytest.raises(ValueError, match=text):
            prompt_lookup_sampling_batch([x], model, 2, None, 8)


@pytest.mark.parametrize("case", list(R.PARITY_CASES))
def test_the_parity_cases_are_admissible_on_the_reference(case):
    """The prompt / seed of each token-for-token case gives, on the reference run with the reference Philox, at least one
    iteration of each kind the GPU test is there for; the final Philox position is (2 * gamma + 2) per iteration."""
    cfg, _, om = R.parity_model()
    ps, seed, top_k = R.PARITY_CASES[case]
    g = R.PARITY_GAMMA
    out, det = R.run(om, R.parity_prompt(cfg, ps), -1, R.PARITY_MAX_LEN, g, 1, top_k, 0, R.PARITY_NGRAM_MAX, R.PARITY_NGRAM_MIN,
                     R.CpuPhiloxNoise(seed, g))
    print(case, "acc_len", det["acc_len"], "match_len", det["match_len"], "src", det["src"], "wraps", det["wraps"])
    assert R.admissible(det, g, R.PARITY_NGRAM_MAX) == []
    assert det["draws"] == (2 * g + 2) * len(det["acc_len"]) and out.shape[1] >= 12 + R.PARITY_MAX_LEN
    assert sum(det["acc_len"]) + len(det["acc_len"]) == out.shape[1] - 12


# ---- the losslessness cases of tests/test_gpu_lookup_lossless.py, justified on the oracle and the reference proposer alone
@pytest.mark.parametrize("name", ["lookup_batch_fp32_filtered", "lookup_batch_bf16_plain", "lookup_single_fp32_filtered"])
def test_the_lossless_cases_are_admissible_and_sized(name):
    """The planted prompt is a fixed point of planting; the first iteration accepts at least one draft with probability >= 0.25
    and both with >= 0.05 (exact, from the tree's tables); the simulator without a defect fits the bar at the case's N, and each
    claimed defect exceeds it."""
    import lookup_lossless as K
    import lossless as LL
    cs = K.case(name)
    p_any, p_both, (drafted, k, c) = K.condition(cs.tree, cs.prompt)
    print(f"{name}: prompt {cs.prompt[0].tolist()}, first proposal {drafted} (match {k} at c = {c}); P[accepts >= 1] = {p_any:.3f}, "
          f"P[accepts both] = {p_both:.3f}; N {cs.N}, dof {cs.dof}, bar {cs.bar:.1f}, lambda_ref {cs.lam:.2f}")
    assert k >= 1 and p_any >= K.P_ANY and p_both >= K.P_BOTH
    x2, dof, outside = LL.x2_of(cs, K.simulate(cs.tree, cs.prompt, cs.N, np.random.default_rng(1)))
    print(f"  simulator, no defect: X2 {x2:.1f} on {dof} dof, {outside} outside")
    assert x2 < cs.bar and outside == 0
    for defect in K.CLAIMS[name]:
        x2, _, outside = LL.x2_of(cs, K.simulate(cs.tree, cs.prompt, cs.N, np.random.default_rng(1), defect))
        print(f"  simulator, {defect}: X2 {x2:.1f}, {outside} outside")
        assert x2 > cs.bar
