"""attn_grouped_kernel (grouped_attn.h) through Session.forward (`pytest -m gpu`): attn_probe's planted keys on one-layer GQA
models under SD_ATTN_GROUPED=2, by test_gpu_attention_edges._run_causal - HIP against the same-dtype oracle (fp8 arena: the
e4m3-emulating one, scales folded in) judged against the fp32 oracle by the 1.5x rule, rows that may not see the marker
bit-identical to the filler run.  The split of a pass is asked of sd_grouped_attn_plan, never restated."""
import ctypes as C

import numpy as np
import pytest
import torch

import attn_probe as P
import oracle
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict
from prefill_probe_layouts import WIDE_MODELS, fold_scales, stream_scales
from sd_env import tunables
from test_gpu_attention_edges import Runner, _run_causal, hip  # noqa: F401  (hip: the module's fixture)
from test_gpu_production_parity import _assert_within_reference_error

pytestmark = pytest.mark.gpu

# attn_probe's construction: the TP-shard tile (8 heads over 1 KV head, D = 128) and 8 heads over 2 KV heads at D = 64
GQA_MODELS = {
    "llama_g8_d128": dict(P.MODELS["llama_gqa_d64"], hidden_size=1024, num_attention_heads=8, num_key_value_heads=1),
    "llama_g4_d64": dict(P.MODELS["llama_gqa_d64"], hidden_size=512, num_attention_heads=8, num_key_value_heads=2),
}
CASES = [("llama_gqa_d64", "bf16", None), ("llama_gqa_d64", "bf16", "fp8"), ("llama_g8_d128", "bf16", None),
         ("llama_g8_d128", "fp16", "fp8"), ("llama_g4_d64", "bf16", None)]
ROWS = [1, 5, 8, 9]               # a decode step, a gamma = 4 verify, a full group, two groups of 8 + 1
CONTEXTS = [200, 700]             # keys the last row sees: one split, several (asserted below)
# random weights, two layers (layer 1 reads what layer 0's attention wrote): G = 4, D = 128
TWO_LAYER = dict(arch="llama", vocab_size=512, hidden_size=1024, intermediate_size=512, num_hidden_layers=2,
                 num_attention_heads=8, num_key_value_heads=2, max_position_embeddings=640, rms_norm_eps=1e-5)


@pytest.fixture
def gqa_models(monkeypatch):
    for name, kw in dict(GQA_MODELS, **WIDE_MODELS).items():
        monkeypatch.setitem(P.MODELS, name, kw)


def _plan(cfg, s_max, groups):
    ns, ck = C.c_int(), C.c_int()
    P._lib.check(P._lib.lib.sd_grouped_attn_plan(cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads, s_max, groups, 0,
                                                 C.byref(ns), C.byref(ck), None), "sd_grouped_attn_plan")
    return ns.value, ck.value


def _layouts(cfg, n):
    out, splits = [], []
    for S in CONTEXTS:
        ns, ck = _plan(cfg, S, len(P.groups_of(n)))
        splits.append(ns)
        p0, last = S - n, n - 1
        keys = [(0, last, "key0"), (63, last, "block_edge"), (64, last, "block_edge"),
                (p0, 0, "own"), (S - 1, last, "own"),              # the causal diagonal of the first and the last row
                (p0 + 1, 0, "forbidden"), (S, last, "forbidden")]  # ... and its successor: a later row / the stale slot
        if ns > 1:
            keys += [(ck - 1, last, "chunk_edge"), (ck, last, "chunk_edge"), ((ns - 1) * ck, last, "chunk_edge")]
        out += [P.Layout(S, n, k, r, cls) for k, r, cls in dict.fromkeys(keys)]
    assert splits[0] == 1 and splits[1] > 1, splits
    return out


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name,dt,kvq", CASES, ids=[f"{n}-{d}{'-fp8kv' if k else ''}" for n, d, k in CASES])
def test_planted_key_at_every_block_split_and_causal_edge(hip, gqa_models, name, dt, kvq, n):  # noqa: F811
    """Query tiles of 2, 10, 16, 40, 64 and 32 rows (G x n); the marker at key 0, either side of a 64-key block edge and of a
    split edge, on the first and last row's own position, and just behind them (invisible: bit-identical to the filler run)."""
    cfg = P.probe_config(name)

    def check(r):                                                  # the route: one launch per layer of a gated pass
        r.run(P.Layout(100, n, 0, n - 1, "key0"))                  # (plants the context, by gated passes of its own)
        before = r.ses.grouped_attn_launches()
        r.run(P.Layout(100, n, 0, n - 1, "key0"))                  # nothing left to plant: the n-row pass alone
        assert r.ses.grouped_attn_launches() - before == cfg.num_hidden_layers == 1
    _run_causal(hip, "grouped", name, dt, _layouts(cfg, n), kvq=kvq, env=dict(SD_ATTN_GROUPED=2), check=check)


def test_only_gated_passes_take_the_route(hip, gqa_models):  # noqa: F811
    """The counter stays at 0 under SD_ATTN_GROUPED=0, under the default for a pass attn_kernel holds, for an MHA model, for
    a tree pass and for a pass the matrix-core prefill kernels take."""
    lay = P.Layout(300, 5, 0, 4, "key0")
    for env, name in ((dict(SD_ATTN_GROUPED=0), "llama_gqa_d64"), ({}, "llama_gqa_d64"), (dict(SD_ATTN_GROUPED=2), "llama_d128")):
        with tunables(env):
            r = Runner(hip, name, "bf16")
        r.run(lay)
        assert r.ses.grouped_attn_launches() == 0, (env, name)
    with tunables(SD_ATTN_GROUPED=2):
        tree = Runner(hip, "llama_gqa_d64", "bf16")
        wide = Runner(hip, "llama_gqa_d64_h512", "bf16")
    tree.run_tree(P.TreeLayout(150, 9, 150, 8, "ancestor"))        # (plants the 150 cached keys by gated passes)
    planted = tree.ses.grouped_attn_launches()
    tree.run_tree(P.TreeLayout(150, 9, 150, 8, "ancestor"))        # nothing left to plant: the tree pass alone
    assert tree.ses.grouped_attn_launches() == planted >= 1
    wide.ses.forward(wide._dev([P.F_TOK] * 81), 0, pos0=0)
    assert wide.ses.prefill_attn_launches() == 1 and wide.ses.grouped_attn_launches() == 0
    wide.run(lay)
    assert wide.ses.grouped_attn_launches() >= 1


def _session(m, cfg, max_seq, kvq, i=0):
    ses = m.new_session(max_seq, kv_dtype=kvq)
    if kvq:
        ses.kv_scale.copy_(stream_scales(i, cfg).to(ses.kv_scale.device))
        torch.cuda.synchronize()
    return ses


def _judge(label, got, lms, ids, past=None):
    """The last rows of `ids` (as many as `got` has): HIP against the same-dtype oracle, judged against the fp32 one."""
    truth, ref = (lm(ids, past_key_values=pk).logits[0, -got.shape[0]:].float() for lm, pk in zip(lms, past or (None, None)))
    _assert_within_reference_error(P.errors(got.float().cpu(), ref, truth), label)


@pytest.mark.parametrize("dt,kvq", [("bf16", None), ("fp16", "fp8")])
def test_two_layers_single_stream_and_batched_streams(hip, dt, kvq):  # noqa: F811
    """A 40-token prompt, a 5-row verify and a 1-row step; then one batch_forward over three sessions with 30, 600 (past one
    split: the 3-key stream's second chunk is empty) and 3 cached keys, each with its own fp8 scales and its own oracle."""
    cfg, dtype = ModelConfig(**TWO_LAYER), P.DTYPES[dt]
    sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 31, head_gain=2.0).items()}
    o32 = oracle.RefCausalLM(cfg, sd)
    o16 = [oracle.RefCausalLM(cfg, P.cast_sd(fold_scales(cfg, sd, stream_scales(i, cfg)) if kvq else sd, dtype), kv_quant=kvq)
           for i in range(3)]
    cached, n_new = (30, 600, 3), (5, 1, 5)
    ids = [torch.from_numpy(np.random.default_rng(9 + i).integers(3, cfg.vocab_size, size=(1, c + n))) for i, (c, n) in enumerate(zip(cached, n_new))]
    with tunables(SD_ATTN_GROUPED=2):
        m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, dtype), dtype=dtype)
        one = _session(m, cfg, 64, kvq)
        sess = [_session(m, cfg, 640, kvq, i) for i in range(3)]
    tok = ids[1][0, :46].to(torch.int32).cuda()
    one.forward(tok[:40], 0)
    _judge("verify", one.forward(tok[40:45], 5).clone(), (o32, o16[0]), ids[1][:, :45])
    _judge("step", one.forward(tok[45:46], 1).clone(), (o32, o16[0]), ids[1][:, :46])
    assert one.grouped_attn_launches() >= 3 * cfg.num_hidden_layers
    seqs = [t[0].to(torch.int32).cuda() for t in ids]
    for ses, sq, c in zip(sess, seqs, cached):
        ses.forward(sq[:c], 0)
    assert _plan(cfg, 601, 3)[0] > 1
    out = torch.split(hip.engine.batch_forward(sess, seqs, list(n_new), list(n_new)).float().cpu(), list(n_new))
    for i in range(3):
        _judge(f"stream {i}", out[i], (o32, o16[i]), ids[i])


def test_past_attn_kernels_lds_under_the_default_tunables(hip):  # noqa: F811
    """8 sessions x 9 rows (16 groups; a batched pass holds at most 80 rows) behind a shared 12100-token prompt: attn_kernel's
    4 splits cannot hold the pass (sd_attn_split, checked: SD_ERR_CAPACITY without the route), the default route runs it."""
    cfg = ModelConfig(**dict(WIDE_MODELS["llama_gqa_d64_h512"], num_key_value_heads=4, max_position_embeddings=12160))
    S0, n, B = 12100, 9, 8
    lds = C.c_long()
    assert P._lib.lib.sd_attn_split(cfg.head_dim, S0 + n, 2 * B, None, None, None, C.byref(lds)) == 0 and lds.value > 160 * 1024 - 512
    sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 31, head_gain=2.0).items()}
    ids = torch.from_numpy(np.random.default_rng(5).integers(3, cfg.vocab_size, size=(1, S0 + n)))
    m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, torch.bfloat16), dtype=torch.bfloat16)
    sess, seq = [m.new_session(S0 + 16) for _ in range(B)], ids[0].to(torch.int32).cuda()
    sess[0].forward(seq[:S0], 0)
    for ses in sess[1:]:
        ses.copy_kv_from(sess[0], 0, S0)
        ses.cache_len = S0
    assert sess[0].grouped_attn_launches() == 0
    out = hip.engine.batch_forward(sess, [seq] * B, [n] * B, [n] * B).float().cpu()
    assert sess[0].grouped_attn_launches() == 1 and _plan(cfg, S0 + n, 2 * B)[1] >= 768   # (>= 3 blocks per wave: the steady state)
    lms = (oracle.RefCausalLM(cfg, sd), oracle.RefCausalLM(cfg, P.cast_sd(sd, torch.bfloat16)))
    past = [[P.kv_rows(lm, ids, 0, S0)] for lm in lms]              # (one layer: its K / V rows depend on token and position alone)
    for i in (0, B - 1):
        _judge(f"session {i}", out[i * n:(i + 1) * n], lms, ids[:, S0:], past)


def test_speculative_sampling_logprobs_on_the_grouped_route(hip, monkeypatch):  # noqa: F811
    """The public entry (native loop, device RNG, bf16, gamma = 4) under SD_ATTN_GROUPED=2: the target session takes the route,
    and the returned target log-probs agree with the oracles' teacher-forced log-probs of the same output tokens."""
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import noise
    tc, dc = ModelConfig(**TWO_LAYER), load_config("tiny-llama-draft")
    tsd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(tc, 3).items()}
    prompt = torch.from_numpy(np.random.default_rng(6).integers(3, tc.vocab_size, size=(1, 20))).cuda()
    with tunables(SD_ATTN_GROUPED=2):
        dm = hip.engine.SpecDecModel.from_state_dict(dc, P.cast_sd(make_state_dict(dc, 4), torch.bfloat16), dtype=torch.bfloat16)
        tm = hip.engine.SpecDecModel.from_state_dict(tc, P.cast_sd(tsd, torch.bfloat16), dtype=torch.bfloat16)
        sessions, new_session = [], tm.new_session
        monkeypatch.setattr(tm, "new_session", lambda *a, **kw: sessions.append(new_session(*a, **kw)) or sessions[-1])
        out, lp = S.speculative_sampling(prompt, dm, tm, -1, None, 24, gamma=4, rng=noise.DeviceNoise(77), logprobs=True)
    assert len(sessions) == 1 and sessions[0].grouped_attn_launches() > 0
    ids = out.cpu().to(torch.int64)
    want = [torch.log_softmax(lm(ids, use_cache=False).logits[0].float(), -1)[19:-1].gather(-1, ids[0, 20:, None])[:, 0]
            for lm in (oracle.RefCausalLM(tc, tsd), oracle.RefCausalLM(tc, P.cast_sd(tsd, torch.bfloat16)))]
    _assert_within_reference_error(P.errors(lp[0].float().cpu(), want[1], want[0]), "target log-probs")
