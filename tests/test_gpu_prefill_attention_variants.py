"""attn_prefill_kernel<T, D, KV8> (`pytest -m gpu`): the fp8 arena at D = 128, D = 64 with either arena, and the 16-bit
arena at D = 128, bf16 and fp16 - planted keys at the kernel's own tile edges, the route (the session's
prefill-attention launch counter), the OPT arithmetic at D = 64 and a batched prefill whose streams carry different scales.

Scale folding, oracle, runner and bars are those of tests/attn_probe.py and test_gpu_attention_edges.py; the models are
attn_probe's at hidden 512 (prefill_probe_layouts.WIDE_MODELS: at hidden 256 a call is cut into passes of 64 rows and never
reaches the kernel - the route tests below would show it), registered in attn_probe's table for the length of a test (the
wide_models fixture); the layouts (tests/prefill_probe_layouts.py) are shown to discriminate by >= 20x the bar on the oracle
alone in test_prefill_probe_cpu.py.  No bar here is measured on the code under test: _assert_within_reference_error against the
same-dtype oracle (with the fp8 arena the e4m3-emulating one, the arena's scales folded in) and the fp32 oracle, and rows in
front of a forbidden key bit-identical to the filler run.

Oracle forwards are computed once per (model, dtype, arena, layout) and shared between the runs of a layout under
SD_PREFILL_ATTN=1 and =0 and between tests."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import oracle
import attn_probe as P
import prefill_probe_layouts as L
import test_gpu_attention_edges as E
from prefill_probe_layouts import wide_models  # noqa: F401  (fixture)
from test_gpu_attention_edges import Runner, _run_causal, _Stats, _Env, hip  # noqa: F401  (hip: the module's fixture)
from llmspeculativesampling_amd.config import load_config
from llmspeculativesampling_amd.synth import make_state_dict

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("wide_models")]


class _SharedOracle(P.ProbeOracle):
    """ProbeOracle whose layout forwards are kept (a layout runs under both settings of SD_PREFILL_ATTN; the results are
    only ever read)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._kept = {}

    def logits(self, lay, with_marker=True):
        key = (lay, with_marker)
        if key not in self._kept:
            self._kept[key] = super().logits(lay, with_marker)
        return self._kept[key]


_KEPT = {}                                                         # this file's oracles: (model, dtype, arena) -> _SharedOracle


@functools.lru_cache(maxsize=None)
def _sd(name):
    return P.probe_state_dict(name)                                # (seeded: the weights Runner builds its model from)


def _oracle(name, dt, kvq=None):
    key = (name, dt, kvq)
    if key not in _KEPT:
        _KEPT[key] = _SharedOracle(name, P.DTYPES[dt], kvq, sd=_sd(name))
    return _KEPT[key]


@pytest.fixture(autouse=True)
def _kept_oracles(monkeypatch):
    """_run_causal takes its oracles from its module's _oracle: give it this file's keeping ones for the length of a test."""
    monkeypatch.setattr(E, "_oracle", _oracle)


def _share_oracles(name, dt, kvq):
    return _oracle(name, "fp32"), _oracle(name, dt, kvq)


def _dev(tokens):
    return torch.from_numpy(np.asarray(tokens).astype(np.int32)).cuda()


# --------------------------------------------------------------------------- 1. planted keys on the new route
@pytest.mark.parametrize("name,dt,kvq", L.CASES, ids=L.CASE_IDS)
def test_prefill_variants_planted_key_at_every_tile_edge(hip, name, dt, kvq):
    """The 58 layouts of prefill_probe_layouts (one call of 81, 200 or 256 rows, logits of the last 64): marker at key 0, at
    pos0 - 1, at the first / last key of a 64-key V chunk, at a row's own position and at its successor for the first / last
    row of a 16-row group and of the logit tail, and in the stale slot behind the call.  Under SD_PREFILL_ATTN=1
    (attn_prefill_kernel) and again under =0 (attn_kernel's 8-row groups over the same rows: the layouts themselves hold)."""
    lays = L.layouts()
    _run_causal(hip, "prefill mfma", name, dt, lays, kvq=kvq, env=dict(SD_PREFILL_ATTN=1), tail=L.TAIL)
    _run_causal(hip, "prefill attn_kernel", name, dt, lays, kvq=kvq, env=dict(SD_PREFILL_ATTN=0), tail=L.TAIL)


# --------------------------------------------------------------------------- 2. route
def _fill(n):
    return _dev(np.full(n, P.F_TOK))


@pytest.mark.parametrize("name,dt,kvq", L.CASES, ids=L.CASE_IDS)
def test_route_counter_rises_by_one_per_layer_on_a_contiguous_call(hip, name, dt, kvq):
    """One 81-row call (contiguous: more than SD_MAX_ROWS = 80 rows) of a one-layer model raises
    Session.prefill_attn_launches() by exactly 1; with SD_PREFILL_ATTN=0, for a 31-row call and for an 80-row
    (non-contiguous) call it stays."""
    with _Env(SD_PREFILL_ATTN=1):
        r = Runner(hip, name, dt, kv_dtype=kvq)
        assert r.ses.prefill_attn_launches() == 0 and r.ses.max_rows >= 81
        r.ses.forward(_fill(81), 0, pos0=0)
        assert r.ses.prefill_attn_launches() == r.cfg.num_hidden_layers == 1
        r.ses.forward(_fill(81), 0, pos0=37)
        assert r.ses.prefill_attn_launches() == 2
        r.ses.forward(_fill(31), 0, pos0=0)
        r.ses.forward(_fill(80), 0, pos0=0)
        assert r.ses.prefill_attn_launches() == 2
        torch.cuda.synchronize()
    with _Env(SD_PREFILL_ATTN=0):
        r0 = Runner(hip, name, dt, kv_dtype=kvq, model=r.m)
        r0.ses.forward(_fill(81), 0, pos0=0)
        assert r0.ses.prefill_attn_launches() == 0
        torch.cuda.synchronize()


def test_route_counter_stays_on_tree_passes_and_outside_the_gate(hip):
    """A tree pass on an fp8 session (sd_session_forward_tree) and a head_dim-32 model's 81-row call keep attn_kernel."""
    with _Env(SD_PREFILL_ATTN=1):
        r = Runner(hip, "llama_gqa_d64_h512", "bf16", kv_dtype="fp8")
        for lay in (P.TreeLayout(150, 64, 150, 63, "ancestor"), P.TreeLayout(0, 40, 0, 39, "ancestor")):
            r.plant(P.tree_inputs(lay)[0], 0, lay.base)            # (the cached keys: a contiguous 150-row call, which counts)
            before = r.ses.prefill_attn_launches()
            r.run_tree(lay)
            assert r.ses.prefill_attn_launches() == before
        assert before == 1
        for kvq in (None, "fp8"):
            r32 = Runner(hip, "llama_d32_h512", "bf16", kv_dtype=kvq)
            assert r32.ses.max_rows >= 81                          # (one contiguous pass: only head_dim keeps it out)
            r32.ses.forward(_fill(81), 0, pos0=0)
            assert r32.ses.prefill_attn_launches() == 0
        torch.cuda.synchronize()


# --------------------------------------------------------------------------- 3. same probabilities from either kernel
@pytest.mark.parametrize("name,dt,kvq", [("llama_d128_h512", "bf16", "fp8"), ("llama_gqa_d64_h512", "bf16", None),
                                         ("llama_gqa_d64_h512", "bf16", "fp8"), ("llama_gqa_d64_h512", "fp16", "fp8")])
def test_either_kernel_gives_the_same_rows_within_the_reference_error(hip, name, dt, kvq):
    """The 64 tail logit rows of one 200-row call (pos0 = 37, the marker at a tail row's own position) under
    SD_PREFILL_ATTN=1 and =0: each within the file's rule of the oracle, and within tol16(e_ref) of each other - both kernels
    round the scores and the probabilities identically (k_scale first, then 1 / sqrt(D)), only the order of the P.V sum
    differs, so their distance is one more rounding of the attention output, far inside the reference's own error.  Not bit
    equality: the summation order differs by design (prefill_attn.h)."""
    o32, o16 = _share_oracles(name, dt, kvq)
    lay = P.Layout(237, 200, 37 + 190, 190, "own")
    truth, ref16 = o32.logits(lay)[-L.TAIL:], o16.logits(lay)[-L.TAIL:]
    got = {}
    for flag in (1, 0):
        with _Env(SD_PREFILL_ATTN=flag):
            r = Runner(hip, name, dt, kv_dtype=kvq)
            got[flag] = r.run(lay, L.TAIL)
            assert r.ses.prefill_attn_launches() == flag          # (the cached keys are planted in one 37-row call)
        st = _Stats(f"SD_PREFILL_ATTN={flag} {name} {dt} {kvq}")
        st.judge(got[flag], truth, ref16, lay)
    e_ref = float((ref16 - truth).abs().max())
    d = float((got[1] - got[0]).abs().max())
    print(f"{name} {dt} {kvq}: attn_prefill_kernel vs attn_kernel max {d:.4f}; reference error {e_ref:.4f}, bar {P.tol16(e_ref):.4f}")
    assert d <= P.tol16(e_ref), (name, dt, kvq, d, e_ref)


# --------------------------------------------------------------------------- 4. OPT arithmetic at D = 64
def _errors(got, ref16, truth, label):
    errs = P.errors(got, ref16, truth)
    print(f"{label}: |logit| max {float(truth.abs().max()):.2f}; max err hip {errs[0]:.4f} ref {errs[1]:.4f}; rms {errs[2]:.5f} / {errs[3]:.5f}")
    assert bool(torch.isfinite(got).all()), label
    E._assert_within_reference_error(errs, label)


def test_opt_arch_head_dim_64_two_layers(hip):
    """configs/tiny-opt-pre.json widened to hidden 512 / 8 heads (D = 64; hidden 256 stops at 64 rows per call), 2 layers, random bf16 weights: a 96-row call at
    pos0 = 0 (its last 8 logit rows), then a 5-row verify on top of it, against the bf16 oracle under the 1.5x rule against
    the fp32 truth.  OPT scores carry no 1 / sqrt(D) step after the product (q is pre-scaled); layer 1 reads its arena at
    the second layer's offset, and its K / V rows depend on layer 0's attention output, so the verify rows see what the
    prefill kernel wrote."""
    cfg = dataclasses.replace(load_config("tiny-opt-pre"), hidden_size=512, num_attention_heads=8, ffn_dim=512, word_embed_proj_dim=512)
    assert cfg.arch == "opt" and cfg.head_dim == 64 and cfg.num_hidden_layers == 2
    sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 23, head_gain=2.0).items()}
    sd["model.decoder.embed_tokens.weight"].mul_(0.25)             # tied head: logits of a few units (exact in bf16)
    sd["lm_head.weight"] = sd["model.decoder.embed_tokens.weight"]
    ids = torch.from_numpy(np.random.default_rng(5).integers(3, cfg.vocab_size, size=(1, 101)))
    with _Env(SD_PREFILL_ATTN=1):
        m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, torch.bfloat16), dtype=torch.bfloat16)
        ses = m.new_session(128)
        a = ses.forward(_dev(ids[0, :96]), 8).float().cpu().clone()
        assert ses.prefill_attn_launches() == 2
        b = ses.forward(_dev(ids[0, 96:]), 5).float().cpu().clone()
        assert ses.prefill_attn_launches() == 2
    o16, o32 = oracle.RefCausalLM(cfg, P.cast_sd(sd, torch.bfloat16)), oracle.RefCausalLM(cfg, sd)
    r16, r32 = o16(ids).logits.float()[0], o32(ids).logits.float()[0]
    _errors(a, r16[88:96], r32[88:96], "opt D = 64, 96-row prefill")
    _errors(b, r16[96:], r32[96:], "opt D = 64, 5-row verify")


# --------------------------------------------------------------------------- 5. batched prefill, one scale tensor per stream
def test_batched_prefill_fp8_each_stream_its_own_scales(hip):
    """engine.batch_prefill (RowTab contig == 2) over three fp8 sessions of a two-layer GQA D = 64 model with 40 / 33 / 90
    rows, each session with its own kv_scale tensor - the second with K's and V's scales swapped (a factor 4 in the scores
    and in the output where a group reads another stream's scales) - then one 1-row forward per session against ITS oracle
    (the bf16 oracle with the e4m3 arena emulation and that session's scales folded in) under the 1.5x rule against the fp32
    truth.  Layer 1's K / V rows of the prefill rows depend on layer 0's attention output, so the 1-row forward reads what
    attn_prefill_kernel made of every stream's scales.  The pass counts on its first session, once per layer."""
    cfg, sd, ids = L.batch_model()
    with _Env(SD_PREFILL_ATTN=1):
        m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, torch.bfloat16), dtype=torch.bfloat16)
        sess = []
        for i in range(3):
            ses = m.new_session(128, kv_dtype="fp8")
            ses.kv_scale.copy_(L.stream_scales(i, cfg).to(ses.kv_scale.device))
            sess.append(ses)
        torch.cuda.synchronize()
        seqs = [_dev(t[0]) for t in ids]
        hip.engine.batch_prefill(sess, seqs, list(L.BATCH_ROWS))
        assert [s.prefill_attn_launches() for s in sess] == [cfg.num_hidden_layers, 0, 0]
        got = [ses.forward(sq[n:n + 1], 1).float().cpu().clone() for ses, sq, n in zip(sess, seqs, L.BATCH_ROWS)]
    o32 = oracle.RefCausalLM(cfg, sd)
    for i, n in enumerate(L.BATCH_ROWS):
        o16 = oracle.RefCausalLM(cfg, P.cast_sd(L.fold_scales(cfg, sd, L.stream_scales(i, cfg)), torch.bfloat16), kv_quant="fp8")
        _errors(got[i], o16(ids[i]).logits.float()[0, n:], o32(ids[i]).logits.float()[0, n:], f"batched prefill, stream {i} ({n} rows)")
