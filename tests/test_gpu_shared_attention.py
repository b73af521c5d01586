"""attn_shared_kernel (shared_attn.h) through engine.batch_forward(shared=(donor, keys)) and the prompt queue (`pytest -m gpu`):
two-layer random-weight models under SD_ATTN_SHARED=2, HIP against the same-dtype oracle (fp8 arena: the e4m3-emulating one,
scales folded in) judged against the fp32 oracle by the 1.5x rule.  The split of a pass is asked of sd_shared_attn_plan."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_probe as P
import oracle
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict
from prefill_probe_layouts import fold_scales, stream_scales
from sd_env import tunables
from test_gpu_attention_edges import hip  # noqa: F401  (the module's fixture)
from test_gpu_grouped_attention import _judge, _session
from test_gpu_production_parity import _assert_within_reference_error

pytestmark = pytest.mark.gpu

BASE = dict(arch="llama", vocab_size=512, intermediate_size=512, num_hidden_layers=2, max_position_embeddings=704, rms_norm_eps=1e-5)
MODELS = {"mha_d128": dict(BASE, hidden_size=512, num_attention_heads=4, num_key_value_heads=4),
          "g4_d64": dict(BASE, hidden_size=512, num_attention_heads=8, num_key_value_heads=2),
          "g8_d128": dict(BASE, hidden_size=1024, num_attention_heads=8, num_key_value_heads=1)}
CASES = [("mha_d128", "bf16", None), ("g4_d64", "fp16", "fp8"), ("g8_d128", "bf16", None)]
OWN, ROWS = (0, 70, 3), (9, 5, 1)     # keys of its own each stream holds behind the prefix; rows it forwards (15 rows, 4 groups)


def _streams(hip, name, dt, kvq, prefix, env):  # noqa: F811
    """The model, the donor prefilled with `prefix` tokens, three sessions that copied them and hold OWN further keys, their
    token buffers and ids (fp8: every arena with stream 0's scales)."""
    cfg, dtype = ModelConfig(**MODELS[name]), P.DTYPES[dt]
    sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 31, head_gain=2.0).items()}
    rng = np.random.default_rng(17)
    head = rng.integers(3, cfg.vocab_size, size=prefix)
    ids = [torch.from_numpy(np.concatenate([head, rng.integers(3, cfg.vocab_size, size=o + n)]))[None] for o, n in zip(OWN, ROWS)]
    seqs = [t[0].to(torch.int32).cuda() for t in ids]
    with tunables(env):
        m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, dtype), dtype=dtype)
        donor, *sess = [_session(m, cfg, 704, kvq) for _ in range(4)]
    donor.forward(seqs[0][:prefix], 0)
    for ses, sq, o in zip(sess, seqs, OWN):
        ses.copy_kv_from(donor, 0, prefix)
        ses.cache_len = prefix
        if o:
            ses.forward(sq[prefix:prefix + o], 0)
    return cfg, sd, m, donor, sess, seqs, ids


@pytest.mark.parametrize("prefix", [1, 65, 577])
@pytest.mark.parametrize("name,dt,kvq", CASES, ids=[f"{n}-{d}{'-fp8kv' if k else ''}" for n, d, k in CASES])
def test_two_layers_three_streams_behind_one_prefix(hip, name, dt, kvq, prefix):  # noqa: F811
    """G x 15 rows (two query tiles at G = 8), one stream of 8 + 1 rows whose suffix is the pass's own rows, one whose suffix
    crosses a 64-key block edge, prefixes off a block edge and (577) past one prefix split; each stream against its own oracle."""
    cfg, sd, m, donor, sess, seqs, ids = _streams(hip, name, dt, kvq, prefix, dict(SD_ATTN_SHARED=2))
    ps = C.c_int()
    P._lib.check(P._lib.lib.sd_shared_attn_plan(cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads, prefix, prefix + 75,
                                                sum(ROWS), 4, 0, None, C.byref(ps), None, None, None, None), "sd_shared_attn_plan")
    assert (ps.value > 1) == (prefix == 577), ps.value
    out = torch.split(hip.engine.batch_forward(sess, seqs, list(ROWS), list(ROWS), shared=(donor, prefix)).float().cpu(), list(ROWS))
    assert sess[0].shared_attn_launches() == cfg.num_hidden_layers
    o32 = oracle.RefCausalLM(cfg, sd)
    o16 = oracle.RefCausalLM(cfg, P.cast_sd(fold_scales(cfg, sd, stream_scales(0, cfg)) if kvq else sd, P.DTYPES[dt]), kv_quant=kvq)
    for i in range(3):
        _judge(f"stream {i}", out[i], (o32, o16), ids[i])


def test_refusals_and_passes_that_keep_their_route(hip):  # noqa: F811
    """shared_keys past a pos0, a donor of another model, an fp8 scale table other than the donor's: refused.  shared=None and
    SD_ATTN_SHARED=0 take the same launches (bit-identical logits, counter 0); so does a 65-key prefix under the default."""
    outs = []
    for env, shared in ((dict(SD_ATTN_SHARED=2), False), (dict(SD_ATTN_SHARED=0), True), ({}, True)):
        cfg, sd, m, donor, sess, seqs, ids = _streams(hip, "g4_d64", "fp16", "fp8", 65, env)
        outs.append(hip.engine.batch_forward(sess, seqs, list(ROWS), list(ROWS), shared=(donor, 65) if shared else None).clone())
        assert sess[0].shared_attn_launches() == 0, env
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    cfg, sd, m, donor, sess, seqs, ids = _streams(hip, "g4_d64", "fp16", "fp8", 65, dict(SD_ATTN_SHARED=2))
    sess[1].kv_scale.mul_(2.0)
    other = _streams(hip, "g4_d64", "fp16", "fp8", 65, {})[3]      # (the same shapes and scales: another model all the same)
    for msg, shared, ss in (("pos0", (donor, 66), [sess[0], sess[2]]), ("another model", (other, 65), [sess[0], sess[2]]),
                            ("scale table", (donor, 65), sess)):
        with pytest.raises(ValueError, match=msg):
            hip.engine.batch_forward(ss, [seqs[sess.index(s)] for s in ss], [1] * len(ss), [1] * len(ss), shared=shared)
        assert sess[0].shared_attn_launches() == 0, msg


def test_queue_with_a_shared_prefix_takes_the_route_end_to_end(hip, monkeypatch):  # noqa: F811
    """speculative_sampling_queue_logprobs(shared_prefix=40) (bf16, gamma = 4, two slots, four prompts behind 40 common tokens) under
    SD_ATTN_SHARED=2: target passes take the route, and the returned target log-probs agree with the oracles' scoring of the
    same outputs.  24 new tokens per prompt, as the grouped route's test scores: the rule compares two rms estimates, and over
    12 tokens their ratio moves by about a third either way (measured so: prompt 0 0.0305 against 0.0157 on the route and 0.0222
    against 0.0157 off it over 12 tokens, 0.0260 against 0.0175 and 0.0226 against 0.0229 over 24; prompts 1 - 3 pass at both)."""
    import llmspeculativesampling_amd.sampling as S
    tc, dc = ModelConfig(**MODELS["mha_d128"]), load_config("tiny-llama-draft")
    tsd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(tc, 3).items()}
    rng, lens = np.random.default_rng(6), [44, 41, 52, 47]
    head = rng.integers(3, tc.vocab_size, size=40)
    prompts = [torch.from_numpy(np.concatenate([head, rng.integers(3, tc.vocab_size, size=n - 40)]))[None].cuda() for n in lens]
    with tunables(SD_ATTN_SHARED=2):
        dm = hip.engine.SpecDecModel.from_state_dict(dc, P.cast_sd(make_state_dict(dc, 4), torch.bfloat16), dtype=torch.bfloat16)
        tm = hip.engine.SpecDecModel.from_state_dict(tc, P.cast_sd(tsd, torch.bfloat16), dtype=torch.bfloat16)
        sessions, new_session = [], tm.new_session
        monkeypatch.setattr(tm, "new_session", lambda *a, **kw: sessions.append(new_session(*a, **kw)) or sessions[-1])
        outs, lps = S.speculative_sampling_queue_logprobs(prompts, dm, tm, -1, None, 24, gamma=4, seeds=[70 + i for i in range(4)],
                                                                 slots=2, shared_prefix=40)
    assert sum(s.shared_attn_launches() for s in sessions) > 0
    lms = (oracle.RefCausalLM(tc, tsd), oracle.RefCausalLM(tc, P.cast_sd(tsd, torch.bfloat16)))
    for i, (out, lp, n) in enumerate(zip(outs, lps, lens)):
        ids = out.cpu().to(torch.int64)
        want = [torch.log_softmax(lm(ids, use_cache=False).logits[0].float(), -1)[n - 1:-1].gather(-1, ids[0, n:, None])[:, 0] for lm in lms]
        _assert_within_reference_error(P.errors(lp.float().cpu().reshape(-1), want[1], want[0]), f"prompt {i} target log-probs")
