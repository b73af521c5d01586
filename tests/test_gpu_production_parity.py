"""Round-3 parity tests at production shapes (`pytest -m gpu`), VERDICT r2 "next" item 1.

No bar in this file is set from a measurement of the HIP path:

* bf16 forwards are held to the rule "HIP's error against an fp32 forward of the same (bf16-valued) weights is at most
  1.5x the error of the reference's own bf16 arithmetic (the oracle run in bf16) against that fp32 forward" - at depths
  2, 8, 16 and at the full 40 layers of Llama-2-13b and OPT-13b.  Two correct bf16 evaluations that round in a different
  order sit at the same distance from the fp32 truth; a kernel that drops a rounding step, a k-step or a mask entry does
  not.  The factor 1.5 is the round-2 test's (depth 2); it is kept, not re-fitted.
* integer-valued operands make every dot product exact in fp32 in ANY summation order, so the MFMA GEMM kernels (every
  row-count class of the streaming kernel, gemm_bf16_mm, the balanced many-row kernel, all split-K folds) must
  reproduce an integer matmul bit for bit at the production shapes.
* a toy pair whose GEMMs are exact by construction (sparse few-bit weights) runs the whole native loop through the MFMA
  kernels, the MFMA attention and the fused epilogues token for token against the oracle.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle
from philox_replay import PhiloxOracleNoise
from llmspeculativesampling_amd.config import ModelConfig, load_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _host_sd(m):
    sd = {n: m._synth_get(n).cpu() for n in m._synth_names}
    if "model.decoder.embed_tokens.weight" in sd:                 # OPT's tied head (reference modeling_opt.py:833,840)
        sd["lm_head.weight"] = sd["model.decoder.embed_tokens.weight"]
    return sd


def _truth_errors(hip, cfg, seed, label, transform=None, prefill=23, verify=5, check_launches=None):
    """HIP bf16 forward and oracle bf16 forward against the oracle fp32 forward of the same bf16-valued weights:
    a `prefill`-row prefill, then a `verify`-row verify (gamma + 1 = 5 by default) whose logits are compared.  Returns the
    oracle's bf16 logits too.  check_launches(profile dict) may assert which launch classes the verify took."""
    n = prefill + verify
    max_pos = max(64, (n + 63) // 64 * 64)
    m = hip.engine.SpecDecModel.synthetic(cfg, seed=seed, dtype=torch.bfloat16, max_pos=max_pos, transform=transform)
    sd16 = _host_sd(m)
    ids = torch.from_numpy(np.random.default_rng(4).integers(3, cfg.vocab_size, size=(1, n)))
    ses = m.new_session(max_pos)
    ses.forward(ids[0, :prefill].to(torch.int32).cuda(), 0)
    if check_launches is not None:
        ses.profile(True)
    got = ses.forward(ids[0, prefill:n].to(torch.int32).cuda(), verify).cpu()
    if check_launches is not None:
        check_launches(ses.profile_read())
        ses.profile(False)
    del ses, m
    torch.cuda.empty_cache()
    o16 = oracle.RefCausalLM(cfg, sd16)
    r = o16(ids[:, :prefill])
    ref16 = o16(ids[:, prefill:n], past_key_values=r.past_key_values).logits.float()[0]
    del o16, r
    sd32 = {k: v.float() for k, v in sd16.items()}
    del sd16
    o32 = oracle.RefCausalLM(cfg, sd32)
    r = o32(ids[:, :prefill])
    truth = o32(ids[:, prefill:n], past_key_values=r.past_key_values).logits.float()[0]
    del o32, r, sd32
    e_hip, e_ref = float((got - truth).abs().max()), float((ref16 - truth).abs().max())
    rms_hip = float((got - truth).pow(2).mean().sqrt())
    rms_ref = float((ref16 - truth).pow(2).mean().sqrt())
    print(f"{label}: |logit| max {float(truth.abs().max()):.2f}; max err hip {e_hip:.4f} ref-bf16 {e_ref:.4f}; "
          f"rms hip {rms_hip:.5f} ref-bf16 {rms_ref:.5f}; hip vs ref-bf16 max {float((got - ref16).abs().max()):.4f}")
    return got, ref16, truth, (e_hip, e_ref, rms_hip, rms_ref)


def _assert_within_reference_error(errs, label):
    e_hip, e_ref, rms_hip, rms_ref = errs
    assert rms_hip <= 1.5 * rms_ref + 1e-3, (label, rms_hip, rms_ref)
    assert e_hip <= 1.5 * e_ref + 0.02, (label, e_hip, e_ref)


@pytest.mark.parametrize("depth", [2, 8, 16, 40])
def test_llama13b_shape_bf16_error_vs_fp32_truth_at_depth(hip, depth):
    """Llama-2-13b's layer shape (hidden 5120, 40 heads x 128, inter 13824, vocab 32000) at 2 / 8 / 16 / all 40 layers,
    bf16: the verify rows' logits after a 23-row prefill.  At every depth the HIP forward must be no further from the
    fp32 truth than 1.5x the reference's own bf16 arithmetic is (reference modeling_llama.py:405-457, 75-89; oracle
    models_ref.py).  This replaces reading the 40-layer "4 % of the logit scale" figure as a measured bar: that figure
    is what two bf16 evaluations 40 layers deep differ by, and this test shows the HIP one is not the outlier."""
    cfg = ModelConfig(arch="llama", vocab_size=32000, hidden_size=5120, intermediate_size=13824, num_hidden_layers=depth,
                      num_attention_heads=40, num_key_value_heads=40, max_position_embeddings=256, rms_norm_eps=1e-5)
    _, _, _, errs = _truth_errors(hip, cfg, seed=9, label=f"llama-13b shape, {depth} layers")
    _assert_within_reference_error(errs, f"depth {depth}")


def test_opt13b_config3_first_verify_vs_oracle_full_size(hip):
    """BASELINE configs[2] at its real shapes: opt-125m -> opt-13b, bf16 (ffn 20480, V 50272, LayerNorm + biases, learned
    positions + 2, tied head, logits kept in bf16: reference modeling_opt.py:160-278, 864-997).  A 23-token prompt and a
    5-row verify on the same synthetic weights: (i) target logits vs the fp32 truth under the 1.5x rule, (ii) the bf16
    probability rows norm_logits makes of them (T = 1, k = 20, p = 0.9; reference utils.py:182-210) against
    oracle.norm_logits of the oracle's bf16 logits: wherever the two bf16 logit rows agree on the top-20 set, the
    supports must be identical up to ties at the cut, and the draft's prefill + step likewise."""
    tcfg, dcfg = load_config("opt-13b"), load_config("opt-125m")

    def soft_head(name, t):
        # OPT ties its head to the (std 1) embedding table: at hidden 5120 that makes logits of several hundred and one-hot
        # probability rows, which would leave the probability-space check below with nothing to compare
        return t * 0.0625 if name.endswith("embed_tokens.weight") else t
    got, ref16, truth, errs = _truth_errors(hip, tcfg, seed=2, label="opt-13b", transform=soft_head)
    _assert_within_reference_error(errs, "opt-13b")
    # OPT's logits are bf16 values (modeling_opt.py:974): the HIP rows must already be rounded
    assert torch.equal(got, got.to(torch.bfloat16).float())
    p_hip = hip.S.norm_logits(got.cuda().to(torch.bfloat16), 1.0, 20, 0.9).float().cpu()
    for i in range(5):
        p_ref = oracle.norm_logits(ref16[i:i + 1].to(torch.bfloat16), 1.0, 20, 0.9)[0].float()
        p_self = oracle.norm_logits(got[i:i + 1].to(torch.bfloat16), 1.0, 20, 0.9)[0].float()
        # the HIP sampler on HIP's own logits is the oracle's sampler on those logits (ties at the top-p cut aside: G8)
        same = (p_hip[i] > 0) == (p_self > 0)
        assert int((~same).sum()) <= 2, (i, int((~same).sum()))
        on = same & (p_self > 0)
        assert float((p_hip[i][on] - p_self[on]).abs().max()) <= 2 ** -7 * float(p_self.max())
        # in probability space the same rule as for the logits: distance to the rows of the (bf16-rounded) fp32 truth
        p_true = oracle.norm_logits(truth[i:i + 1].to(torch.bfloat16), 1.0, 20, 0.9)[0].float()
        tv_hip = 0.5 * float((p_hip[i] - p_true).abs().sum())
        tv_ref = 0.5 * float((p_ref - p_true).abs().sum())
        print(f"opt-13b row {i}: TV to the truth's row: hip {tv_hip:.3f}, ref-bf16 {tv_ref:.3f}")
        assert tv_hip <= 1.5 * tv_ref + 0.05, (i, tv_hip, tv_ref)
    _, _, _, derrs = _truth_errors(hip, dcfg, seed=1, label="opt-125m", transform=soft_head)
    _assert_within_reference_error(derrs, "opt-125m")


# --------------------------------------------------------------------------- integer-exact MFMA GEMMs
GEMM_SHAPES = {                                                   # [N][K] of the per-layer GEMMs the bench configs run
    "13b_qkv": (15360, 5120), "13b_o": (5120, 5120), "13b_gate_up": (27648, 5120), "13b_down": (5120, 13824),
    "13b_lm_head": (32000, 5120), "68m_qkv": (2304, 768), "68m_lm_head": (32000, 768), "opt13b_fc1": (20480, 5120),
    "70b_down": (8192, 28672),
}


@pytest.mark.parametrize("shape", list(GEMM_SHAPES))
def test_mfma_gemm_is_integer_exact_at_production_shapes(hip, shape):
    """W in {-2..2}, X in {-4..4} (exact in bf16): every product and every partial sum is an integer below 2^24, so the
    fp32 result is the same in any summation order and the kernels - MFMA accumulation, in-workgroup fold, split-K slabs
    and their reduction - must equal an integer matmul bit for bit.  Row counts cover every dispatch class of
    sd_gemm_bf16: 1, 5 (decode / verify), 16, 17, 40, 60, 64 (stream-batched verify), 128 and 256 (prefill chunks); 145-256 rows
    are gemm_bf16_mm's k-slab form (mm_kernels.h) - 256 a full 256-row block, 145 / 150 / 177 / 200 / 241 ragged ones, whose X
    tiles past the pass are not copied and whose waves count their own LDS-DMA requests."""
    N, K = GEMM_SHAPES[shape]
    g = torch.Generator(device="cuda").manual_seed(N + K)
    W = torch.randint(-2, 3, (N, K), device="cuda", generator=g).to(torch.bfloat16)
    Wp = torch.empty_like(W)
    assert hip.lib.sd_pack_weight_bf16(W.data_ptr(), Wp.data_ptr(), N, K, _st()) == 0
    Wf = W.double()
    part = torch.empty(64 * 64 * N if N <= 8192 else 20 * 256 * N, dtype=torch.float32, device="cuda")
    for M in (1, 5, 16, 17, 40, 60, 64, 72, 80, 96, 127, 128, 132, 144, 145, 150, 177, 200, 241, 256):
        X = torch.randint(-4, 5, (M, K), device="cuda", generator=g).to(torch.bfloat16)
        Xt = torch.zeros((M + 15) // 16 * 16 * K, device="cuda", dtype=torch.bfloat16)
        assert hip.lib.sd_pack_activation_bf16(X.data_ptr(), Xt.data_ptr(), M, K, _st()) == 0
        out = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
        S = C.c_int(0)
        rc = hip.lib.sd_gemm_bf16(Wp.data_ptr(), Xt.data_ptr(), 1, M, N, K, part.data_ptr(), part.numel(), out.data_ptr(),
                                  C.byref(S), _st())
        assert rc == 0, hip.L.last_error() if hasattr(hip.L, "last_error") else rc
        want = (X.double() @ Wf.t()).float()
        assert torch.equal(out, want), (shape, M, S.value, float((out - want).abs().max()))
        if M <= 64:                                               # plain-row operand of the public entry (streaming kernel)
            out.fill_(float("nan"))
            assert hip.lib.sd_gemm_bf16(Wp.data_ptr(), X.data_ptr(), 0, M, N, K, part.data_ptr(), part.numel(),
                                        out.data_ptr(), None, _st()) == 0
            assert torch.equal(out, want), (shape, M, "row-major")


# --------------------------------------------------------------------------- token-exact run through the MFMA path
def _fewbit_sparse_sd(cfg: ModelConfig, seed: int, nnz: int = 4):
    """bf16 state dict whose GEMMs are exact in any summation order: every weight row has `nnz` non-zero entries, each
    +-2^j (one significant bit), so a dot product is a sum of `nnz` terms that are bf16 activations shifted by powers of
    two - exact in fp32 unless the terms are more than 15 binades apart.  Norm weights are exactly 1."""
    from llmspeculativesampling_amd.synth import param_shapes
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape, kind in param_shapes(cfg):
        if kind == "norm_w":
            a = np.ones(shape, dtype=np.float32)
        elif kind == "emb":
            a = rng.choice(np.array([-1.5, -1.0, -0.5, 0.5, 1.0, 1.5], dtype=np.float32), size=shape)
        else:
            rows, cols = shape
            a = np.zeros(shape, dtype=np.float32)
            idx = np.stack([rng.choice(cols, size=nnz, replace=False) for _ in range(rows)])
            mag = 2.0 ** rng.integers(-2, 1, size=(rows, nnz)) * (2.0 if kind == "head" else 1.0) / np.sqrt(nnz)
            mag = 2.0 ** np.round(np.log2(mag))
            a[np.arange(rows)[:, None], idx] = (mag * rng.choice([-1.0, 1.0], size=(rows, nnz))).astype(np.float32)
        sd[name] = torch.from_numpy(a).to(torch.bfloat16)
    return sd


def _perturb_fewbit(sd, seed, frac):
    """target = draft with a fraction of the matrix rows redrawn (keeps the few-bit sparse structure)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, t in sd.items():
        t = t.clone()
        if t.dim() == 2 and "embed" not in name:
            rows = np.nonzero(rng.random(t.shape[0]) < frac)[0]
            for r in rows:
                t[r] = t[r][torch.from_numpy(rng.permutation(t.shape[1]))]
        out[name] = t
    return out


TOKEN_EXACT_CASES = [("g4_a", 0.08, 4, 5), ("g2", 0.15, 2, 7), ("g4_c", 0.3, 4, 8)]


@pytest.mark.parametrize("wide", [False, True], ids=["h64", "h1024_seams"])
@pytest.mark.parametrize("name,frac,gamma,seed", TOKEN_EXACT_CASES, ids=[c[0] for c in TOKEN_EXACT_CASES])
def test_mfma_path_token_for_token_vs_oracle_on_exact_gemm_pair(hip, name, frac, gamma, seed, wide):
    """The bf16 engine (gemm_bf16_stream with the fused QKV / SiLU / head epilogues, the MFMA attention kernel, the
    native loop sd_spec_generate with device Philox) against the oracle's bf16 CPU run fed the same Philox variates,
    token for token, accept length for accept length.  Every fp32 test of this kind goes through gemm_f32_simple; here the
    pair is built so that bf16 rounding ORDER cannot separate the two implementations in the GEMMs (_fewbit_sparse_sd:
    dot products of 4 power-of-two-scaled terms are exact in any order), and the first prompt row - one key, softmax = 1,
    P.V = v - must come out bit for bit.
    What this does NOT make exact, measured with tools/diag_token_exact.py (round 3): attention's dense q.k and p.v sums
    are order-dependent, so from the fifth teacher-forced row on ~17 % of the logits of the two implementations differ, each
    by exactly one bf16 ulp.  Token-for-token identity over a bf16 trace therefore rests on sampling decisions not sitting
    within an ulp of a tie; of the four traces first written for this test, these three are identical and a fourth (same
    construction, seed 6) parts ways at its sixth token on such a tie - it was removed rather than re-seeded until green,
    and the statement "bf16 traces are token-exact" is NOT made: the production-shape guarantee is the error rule above.
    `wide` runs the same three traces at hidden 1024 / head_dim 128, i.e. through the default path of the 13b target: the
    fused attention + O launch, gemm_bf16_stream_xn (RMSNorm on load) and gemm_bf16_stream_fin (k-split down projection
    with the residual epilogue); they are identical to the oracle's as well."""
    V = 512
    # wide: hidden 1024 with head_dim 128 - the same construction through the fused attention + O launch, the
    # norm-on-load GEMMs and the k-split down projection with the residual epilogue (the default path of the 13b target)
    Hd, I, nh, nkv = (1024, 2048, 8, 4) if wide else (64, 128, 2, 1)
    dcfg = ModelConfig(arch="llama", vocab_size=V, hidden_size=Hd, intermediate_size=I, num_hidden_layers=1,
                       num_attention_heads=nh, num_key_value_heads=nh, max_position_embeddings=128, rms_norm_eps=1e-5)
    tcfg = ModelConfig(arch="llama", vocab_size=V, hidden_size=Hd, intermediate_size=I, num_hidden_layers=2,
                       num_attention_heads=nh, num_key_value_heads=nkv, max_position_embeddings=128, rms_norm_eps=1e-5)
    dsd = _fewbit_sparse_sd(dcfg, seed)
    tsd = _fewbit_sparse_sd(tcfg, seed + 100)
    # correlate the pair: the target shares the draft's embedding, first layer (its K / V rows are cut to the single KV
    # head) and head, with a fraction of rows redrawn
    shared = _perturb_fewbit(dsd, seed + 200, frac)
    hd = tcfg.head_dim
    for k, v in shared.items():
        if k in tsd and tsd[k].shape == v.shape:
            tsd[k] = v
        elif k in tsd and k.endswith(("k_proj.weight", "v_proj.weight")):
            tsd[k] = v[:hd * nkv]
    prompt = torch.from_numpy(np.random.default_rng(seed).integers(3, V, size=(1, 9)))
    kw = dict(gamma=gamma, top_k=20, top_p=0.9)
    want, wd = oracle.speculative_sampling(prompt, oracle.RefCausalLM(dcfg, dsd), oracle.RefCausalLM(tcfg, tsd), -1, None, 16,
                                           details=True, noise=PhiloxOracleNoise(hip.lib, 4242 + seed, gamma, _st), **kw)
    dm = hip.engine.SpecDecModel.from_state_dict(dcfg, dsd, dtype=torch.bfloat16)
    tm = hip.engine.SpecDecModel.from_state_dict(tcfg, tsd, dtype=torch.bfloat16)
    assert dm.fused and tm.fused                                  # the fused-epilogue MFMA route, not the fp32 kernels
    if wide:                                                      # ... and, at hidden 1024, the norm-on-load seams: of the target's
        ps = tm.new_session(32)                                   # 2 x 2 residual+norm launches only the final norm's is left
        ps.forward(prompt[0, :4].to(torch.int32).cuda(), 0)
        ps.profile(True)
        ps.forward(prompt[0, 4:9].to(torch.int32).cuda(), 5)
        assert ps.profile_read()["norm_residual"][1] == 1
        ps.profile(False)
    got, gd = hip.S.speculative_sampling(prompt.cuda(), dm, tm, -1, None, 16, details=True,
                                         rng=hip.noise.DeviceNoise(4242 + seed), **kw)
    print(name, "acc_len oracle", wd["acc_len"], "hip", gd["acc_len"])
    for cfg_, sd_, m_ in ((dcfg, dsd, dm), (tcfg, tsd, tm)):      # exact by construction: a single-row, single-key forward
        o0 = oracle.RefCausalLM(cfg_, sd_)(prompt[:, :1]).logits.float()[0]
        h0 = m_.new_session(16).forward(prompt[0, :1].to(torch.int32).cuda(), 1).cpu()
        assert torch.equal(h0, o0)
    np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    assert gd["acc_len"] == wd["acc_len"]
    assert gd["target_call_times"] == wd["target_call_times"]
    assert 0 < sum(wd["acc_len"]) < gamma * len(wd["acc_len"])    # the scenario has partial accepts (oracle's own run)
    # the Python-orchestrated loop (dense accept / resample kernels) agrees bit for bit too
    got2, gd2 = hip.S.speculative_sampling(prompt.cuda(), dm, tm, -1, None, 16, details=True, verbose=True,
                                           rng=hip.noise.DeviceNoise(4242 + seed), **kw)
    assert torch.equal(got, got2) and gd["acc_len"] == gd2["acc_len"]


def _llama13b_layers(depth):
    return ModelConfig(arch="llama", vocab_size=32000, hidden_size=5120, intermediate_size=13824, num_hidden_layers=depth,
                       num_attention_heads=40, num_key_value_heads=40, max_position_embeddings=256, rms_norm_eps=1e-5)


@pytest.mark.parametrize("verify", [5, 9], ids=["5rows", "9rows"])
def test_llama13b_shape_verify_at_bench_context_vs_fp32_truth(hip, verify):
    """the oracle check at the BENCH's context length.  2 layers of the 13b layer shape, a 200-row
    prefill (the gemm_bf16_mm prefill GEMMs, 25 attention groups) and then a 5-row and a 9-row verify at S = 205 / 209 - the
    fused attention + O launch with its write-through / counter hand-off (two row groups at 9 rows), both norm-on-load
    seams and the k-split down projection with the residual epilogue at 5 rows, the residual+norm launches at 9 - held to
    the fp32 truth under the 1.5x rule.  Until now that context was only ever compared with the unfused HIP path."""
    def launches(prof):
        # 5 rows: of 2 x 2 residual+norm launches only the final norm's is left (both seams normalise on load); the
        # attention class (2 launches = 2 layers) is the fused attention + O launch: the GEMM class has no O projection
        n_gemm = prof["gemm"][1]
        assert prof["attention"][1] == 2
        if verify <= 8:
            assert prof["norm_residual"][1] == 1 and n_gemm == 2 * 3 + 1, prof
        else:
            assert n_gemm == 2 * 3 + 1, prof                    # fused attention + O also at 9 rows (two row groups)
    _, _, _, errs = _truth_errors(hip, _llama13b_layers(2), seed=9, label=f"llama-13b shape, 200-row prefill, {verify}-row verify",
                                  prefill=200, verify=verify, check_launches=launches)
    _assert_within_reference_error(errs, f"S~200, {verify} rows")


@pytest.mark.parametrize("n_streams,gamma,arch", [(8, 4, "llama"), (12, 4, "llama"), (8, 2, "llama"), (8, 8, "llama"), (8, 8, "opt")],
                         ids=["40rows", "60rows", "g2_24rows", "g8_72rows", "opt_g8_72rows"])
def test_stream_batched_verify_13b_layer_shape_error_vs_fp32_truth(hip, n_streams, gamma, arch):
    """Throughput mode at the production layer shape: 8 / 12 streams x (gamma + 1) verify
    rows - 40 / 60 rows at gamma = 4, 24 rows at gamma = 2, 72 rows at gamma = 8 (config 4's sweep) - through a 2-layer model
    with Llama-2-13b's layer shape: the balanced many-row GEMM (gemm_bf16_rows) with its fused QKV / SiLU epilogues,
    per-stream attention groups (two per stream at 9 rows), batched prefill of the prompts - against the oracle run stream
    by stream.  Bar: per stream, the HIP logits' error against an fp32 forward of the same bf16-valued weights is at most
    1.5x the error of the reference's bf16 arithmetic (the rule of this file).  A pass carries at most the session's
    max_pass_rows: more streams than fit go through further passes of whole streams, as the native loop does - opt-13b's
    vocab of 50272 has no many-row lm_head kernel, so its 8 x 9 rows go as 7 + 1 streams."""
    cfg = _llama13b_layers(2) if arch == "llama" else _opt13b_layers(2)
    q = gamma + 1

    def soft_head(name, t):                                       # (OPT's tied head: see test_opt13b_config3_...)
        return t * 0.0625 if name.endswith("embed_tokens.weight") else t
    m = hip.engine.SpecDecModel.synthetic(cfg, seed=9, dtype=torch.bfloat16, max_pos=96, transform=soft_head if arch == "opt" else None)
    sd16 = _host_sd(m)
    sd32 = {k: v.float() for k, v in sd16.items()}
    o16, o32 = oracle.RefCausalLM(cfg, sd16), oracle.RefCausalLM(cfg, sd32)
    rng = np.random.default_rng(21)
    lens = [int(x) for x in rng.integers(9, 40, size=n_streams)]
    seqs = [torch.from_numpy(rng.integers(3, cfg.vocab_size, size=(L + q,)).astype(np.int32)).cuda() for L in lens]
    sessions = [m.new_session(96) for _ in lens]
    hip.engine.batch_prefill(sessions, seqs, lens)
    per_pass = max(1, sessions[0].max_pass_rows // q)
    got = torch.cat([hip.engine.batch_forward(sessions[a:a + per_pass], seqs[a:a + per_pass], [q] * len(sessions[a:a + per_pass]),
                                              [q] * len(sessions[a:a + per_pass])).cpu().clone()
                     for a in range(0, n_streams, per_pass)])
    worst = (0.0, 0.0)
    for i, (L, sq) in enumerate(zip(lens, seqs)):
        ids = sq[None].long().cpu()
        ref16 = o16(ids).logits.float()[0, L:L + q]
        truth = o32(ids).logits.float()[0, L:L + q]
        mine = got[q * i:q * i + q]
        e_hip, e_ref = float((mine - truth).abs().max()), float((ref16 - truth).abs().max())
        r_hip, r_ref = float((mine - truth).pow(2).mean().sqrt()), float((ref16 - truth).pow(2).mean().sqrt())
        worst = max(worst, (e_hip / max(e_ref, 1e-9), r_hip / max(r_ref, 1e-9)))
        assert r_hip <= 1.5 * r_ref + 1e-3, (i, L, r_hip, r_ref)
        assert e_hip <= 1.5 * e_ref + 0.02, (i, L, e_hip, e_ref)
    print(f"{n_streams} streams x {q} rows: worst (max-error ratio, rms ratio) HIP / reference-bf16 = ({worst[0]:.2f}, {worst[1]:.2f})")


def test_tp8_loopback_llama70b_shard_shape_fp8_kv_vs_fp32_truth(hip):
    """VERDICT r3 item 1(a) - BASELINE config 5 as far as ONE GPU allows: an 8-way tensor-parallel target at Llama-2-70b's
    layer shape (hidden 8192; per rank 8 of 64 query heads, 1 of 8 KV heads, 3584 of 28672 MLP columns; row-parallel
    O: K = 1024, down: K = 3584, both folded over the group), 2 layers, bf16 weights, fp8 (e4m3) KV arenas, all eight
    ranks in one process through the loopback group (the kernels and tp_reduce of the RCCL path; the all-reduce is an
    in-process rendezvous + sum kernel).  A 40-row prefill (the many-row GEMMs under TP) and a 5-row verify:
      * every rank's logits are bit-identical to every other rank's (same all-reduced sums everywhere);
      * the verify rows obey the rule of this file against an fp32 forward of the same weights (modeling_llama.py:225-234,
        292-393; oracle.RefCausalLM), where the reference arithmetic is the oracle run in bf16 WITH the same e4m3
        quantisation of new K / V rows (oracle models_ref._kv_fp8 - the fp8 arena has no reference counterpart, so the
        quantisation is part of the configuration, not of the error being judged);
      * the unsharded engine with an fp8 arena obeys the same rule (config 5's shape on one GPU, as the bench runs it);
      * each rank's arena holds its own KV head: e4m3 bytes equal to the unsharded engine's up to the last bit of a
        bf16 K / V value that sits on an e4m3 rounding boundary."""
    from llmspeculativesampling_amd import tp
    from test_gpu_native_parity import _run_ranks
    W = 8
    cfg = ModelConfig(arch="llama", vocab_size=32000, hidden_size=8192, intermediate_size=28672, num_hidden_layers=2,
                      num_attention_heads=64, num_key_value_heads=8, max_position_embeddings=128, rms_norm_eps=1e-5)
    full = hip.engine.SpecDecModel.synthetic(cfg, seed=17, dtype=torch.bfloat16, max_pos=64)
    sd16 = _host_sd(full)
    groups = tp.TPGroup.loopback(W)
    shards = [tp.shard_model(cfg, sd16, r, W, group=groups[r], dtype=torch.bfloat16, max_pos=64) for r in range(W)]
    lc = shards[0].cfg
    assert (lc.num_attention_heads, lc.num_key_value_heads, lc.intermediate_size, lc.head_dim, lc.hidden_size) == (8, 1, 3584, 128, 8192)
    ids = torch.from_numpy(np.random.default_rng(4).integers(3, cfg.vocab_size, size=(1, 45)))
    dev_ids = ids[0].to(torch.int32).cuda()
    sess = [m.new_session(64, kv_dtype="fp8") for m in shards]
    _run_ranks([lambda r=r: sess[r].forward(dev_ids[:40], 0) for r in range(W)])
    got = _run_ranks([lambda r=r: sess[r].forward(dev_ids[40:45], 5).clone() for r in range(W)])
    for r in range(1, W):
        assert torch.equal(got[r], got[0]), f"rank {r} differs from rank 0"
    fs = full.new_session(64, kv_dtype="fp8")
    fs.forward(dev_ids[:40], 0)
    got_full = fs.forward(dev_ids[40:45], 5).clone().cpu()
    kv_full = fs.kv.clone()
    tp_logits = got[0].cpu()
    kv_ranks = [s_.kv.clone() for s_ in sess]
    del sess, shards, groups, fs, full
    torch.cuda.empty_cache()
    o16 = oracle.RefCausalLM(cfg, sd16, kv_quant="fp8")
    r_ = o16(ids[:, :40])
    ref16 = o16(ids[:, 40:45], past_key_values=r_.past_key_values).logits.float()[0]
    del o16, r_
    sd32 = {k: v.float() for k, v in sd16.items()}
    del sd16
    o32 = oracle.RefCausalLM(cfg, sd32)
    r_ = o32(ids[:, :40])
    truth = o32(ids[:, 40:45], past_key_values=r_.past_key_values).logits.float()[0]
    del o32, r_, sd32
    for name, mine in (("tp8 loopback", tp_logits), ("unsharded", got_full)):
        e_hip, e_ref = float((mine - truth).abs().max()), float((ref16 - truth).abs().max())
        r_hip, r_ref = float((mine - truth).pow(2).mean().sqrt()), float((ref16 - truth).pow(2).mean().sqrt())
        print(f"70b shard shape, fp8 KV, {name}: |logit| max {float(truth.abs().max()):.2f}; max err hip {e_hip:.4f} ref {e_ref:.4f}; "
              f"rms hip {r_hip:.5f} ref {r_ref:.5f}")
        _assert_within_reference_error((e_hip, e_ref, r_hip, r_ref), name)
    # rank r's arena = KV head r of the unsharded arena: layer 0 depends on the embeddings alone, so its bytes must agree
    # except where a bf16 K / V value computed in another summation order straddles an e4m3 rounding boundary
    for r in range(W):
        assert tuple(kv_ranks[r].shape) == (2, 2, 1, 64, 128) and kv_ranks[r].dtype == torch.uint8
        mine, ref = kv_ranks[r][0, :, 0, :45], kv_full[0, :, r, :45]
        assert float((mine != ref).float().mean()) < 0.02, (r, float((mine != ref).float().mean()))
        a = mine.view(torch.float8_e4m3fn).float()
        b = ref.view(torch.float8_e4m3fn).float()
        assert bool(((a - b).abs() <= 0.126 * torch.maximum(a.abs(), b.abs()) + 2e-3).all())      # one e4m3 step at most




def test_fp16_many_row_passes_13b_layer_shape_vs_oracle(hip):
    """The fp16 instances (v_mfma_f32_16x16x32_f16) of the balanced many-row GEMM at every m-tile count it is built for - a
    132-row prefill chunk (9 m-tiles), then 72-, 40-, 24- and 100-row chunks (5, 3, 2 and 8 m-tiles) of ONE sequence at
    Llama-2-13b's layer shape, 2 layers - against the oracle's fp16 forward (what evaluation.py:185 loads): the last five
    logit rows of every chunk within 0.5 % of the logit scale (fp16's bar in tests/test_gpu_native_parity.py), and the fp16
    K / V rows of the last layer likewise."""
    cfg = _llama13b_layers(2)
    m = hip.engine.SpecDecModel.synthetic(cfg, seed=13, dtype=torch.float16, max_pos=384, gain=0.5)
    sd = _host_sd(m)
    om = oracle.RefCausalLM(cfg, sd)
    ses = m.new_session(384)
    ids = torch.from_numpy(np.random.default_rng(19).integers(3, cfg.vocab_size, size=(1, 368)))
    past, pos = None, 0
    for q in (132, 72, 40, 24, 100):
        chunk = ids[:, pos:pos + q]
        o = om(chunk, past_key_values=past)
        past = o.past_key_values
        got = ses.forward(chunk[0].to(torch.int32).cuda(), 5).cpu()
        want = o.logits.float()[0, -5:]
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        print(f"fp16, {q}-row chunk at position {pos}: |logit| max {scale:.2f}, max err {err:.4f}")
        assert err <= 0.005 * scale + 2e-3, (q, err, scale)
        pos += q
    k, v = ses.past_key_values()[1]
    ok, ov = past[1]
    assert float((k.float().cpu() - ok.float()).abs().max()) <= 0.01 * max(1.0, float(ok.float().abs().max()))
    assert float((v.float().cpu() - ov.float()).abs().max()) <= 0.01 * max(1.0, float(ov.float().abs().max()))


def _opt13b_layers(depth):
    return ModelConfig(arch="opt", vocab_size=50272, hidden_size=5120, ffn_dim=20480, num_hidden_layers=depth,
                       num_attention_heads=40, num_key_value_heads=40, max_position_embeddings=512, do_layer_norm_before=True)


@pytest.mark.parametrize("arch,rows", [("llama", 256), ("llama", 200), ("llama", 150), ("opt", 256), ("opt", 177)],
                         ids=["llama256", "llama200", "llama150", "opt256", "opt177"])
def test_prefill_pass_on_gemm_bf16_mm_vs_fp32_truth(hip, arch, rows):
    """Prefill passes past the balanced kernel's row count (145..256 rows) run their GEMMs on gemm_bf16_mm (mm_kernels.h: LDS-DMA
    stages, two in flight across one barrier per 64 columns of K, staggered wave halves) - QKV and gate/up (fc1) with the fused
    RoPE / KV-append and SiLU (ReLU + bias) epilogues on the block's accumulators, O / down (fc2) as k-slabs - at Llama-2-13b's
    and opt-13b's layer shapes, 2 layers, for full (256), ragged (200, 177) and barely-past-144 (150) row counts: ONE pass over
    `rows` prompt tokens, the logits of its last 8 rows under the file's rule (HIP error against the fp32 truth <= 1.5x the
    reference-bf16's own), the last layer's K / V rows within the bf16 bar of the oracle's, and the launch classes: no
    stand-alone QKV / activation epilogue launch is left in the pass."""
    cfg = _llama13b_layers(2) if arch == "llama" else _opt13b_layers(2)

    def soft_head(name, t):                                       # (OPT's tied head: see test_opt13b_config3_...)
        return t * 0.0625 if name.endswith("embed_tokens.weight") else t
    m = hip.engine.SpecDecModel.synthetic(cfg, seed=31, dtype=torch.bfloat16, max_pos=320, transform=soft_head if arch == "opt" else None)
    sd16 = _host_sd(m)
    ids = torch.from_numpy(np.random.default_rng(rows).integers(3, cfg.vocab_size, size=(1, rows)))
    ses = m.new_session(320)
    ses.profile(True)
    got = ses.forward(ids[0].to(torch.int32).cuda(), 8).cpu()
    prof = ses.profile_read()
    ses.profile(False)
    assert "qkv_rope_append" not in prof and "activation" not in prof, prof
    k_hip, v_hip = (t.float().cpu() for t in ses.past_key_values()[1])
    del ses, m
    torch.cuda.empty_cache()
    o16 = oracle.RefCausalLM(cfg, sd16)
    r16 = o16(ids)
    ref16 = r16.logits.float()[0, -8:]
    k_ref, v_ref = (t.float() for t in r16.past_key_values[1])
    del o16, r16
    o32 = oracle.RefCausalLM(cfg, {k: v.float() for k, v in sd16.items()})
    truth = o32(ids).logits.float()[0, -8:]
    del o32
    e_hip, e_ref = float((got - truth).abs().max()), float((ref16 - truth).abs().max())
    rms_hip, rms_ref = float((got - truth).pow(2).mean().sqrt()), float((ref16 - truth).pow(2).mean().sqrt())
    print(f"{arch} 13b shape, one {rows}-row pass: max err hip {e_hip:.4f} ref-bf16 {e_ref:.4f}; rms hip {rms_hip:.5f} ref-bf16 {rms_ref:.5f}")
    _assert_within_reference_error((e_hip, e_ref, rms_hip, rms_ref), f"{arch}, {rows}-row pass")
    for name, a, b in (("K", k_hip, k_ref), ("V", v_hip, v_ref)):
        assert a.shape[2] >= rows
        d = float((a[:, :, :rows] - b[:, :, :rows]).abs().max())
        assert d <= 0.04 * max(1.0, float(b.abs().max())), (name, d)


def test_prefill_pass_fp16_on_gemm_bf16_mm_vs_oracle(hip):
    """The fp16 instances (v_mfma_f32_16x16x32_f16) of gemm_bf16_mm: a 256-row and a 170-row pass of ONE sequence at the 13b
    layer shape against the oracle's fp16 forward (what evaluation.py:185 loads), last five logit rows within fp16's bar."""
    cfg = _llama13b_layers(2)
    m = hip.engine.SpecDecModel.synthetic(cfg, seed=13, dtype=torch.float16, max_pos=448, gain=0.5)
    om = oracle.RefCausalLM(cfg, _host_sd(m))
    ses = m.new_session(448)
    ids = torch.from_numpy(np.random.default_rng(23).integers(3, cfg.vocab_size, size=(1, 426)))
    past, pos = None, 0
    for q in (256, 170):
        chunk = ids[:, pos:pos + q]
        o = om(chunk, past_key_values=past)
        past = o.past_key_values
        got = ses.forward(chunk[0].to(torch.int32).cuda(), 5).cpu()
        want = o.logits.float()[0, -5:]
        scale, err = float(want.abs().max()), float((got - want).abs().max())
        print(f"fp16, {q}-row pass at position {pos}: |logit| max {scale:.2f}, max err {err:.4f}")
        assert err <= 0.005 * scale + 2e-3, (q, err, scale)
        pos += q


@pytest.mark.parametrize("kind", ["llama", "llama_gqa", "opt"])
def test_prefill_attention_on_the_matrix_cores_vs_fp32_truth_and_attn_kernel(hip, kind, monkeypatch):
    """Prefill passes of >= 32 rows of a head_dim-128 model take attn_prefill_kernel (prefill_attn.h: 16-row groups, P.V by
    MFMA over LDS-staged V read back transposed with ds_read_b64_tr_b16) instead of attn_kernel's 8-row groups.  Two passes of
    ONE sequence - 200 rows from position 0, then 100 rows on top of them (keys 0..299: five V chunks, a ragged last group of
    4 rows, a ragged last chunk) - for an MHA Llama, a GQA Llama (8 query heads on 2 KV heads) and an OPT shape (no score
    scaling after the product, biases): the last 8 logit rows of each pass under the file's rule against the fp32 truth, and
    against the same passes through attn_kernel (SD_PREFILL_ATTN=0) - same scores, same probabilities, only the order of the
    P.V sum differs: within two bf16 ulps of the logit scale (measured: one - a handful of logits round the other way)."""
    if kind == "opt":
        cfg = ModelConfig(arch="opt", vocab_size=4096, hidden_size=1024, ffn_dim=4096, num_hidden_layers=2, num_attention_heads=8,
                          num_key_value_heads=8, max_position_embeddings=512, do_layer_norm_before=True)
    else:
        cfg = ModelConfig(arch="llama", vocab_size=4096, hidden_size=1024, intermediate_size=2816, num_hidden_layers=2,
                          num_attention_heads=8, num_key_value_heads=2 if kind == "llama_gqa" else 8, max_position_embeddings=512,
                          rms_norm_eps=1e-5)
    ids = torch.from_numpy(np.random.default_rng(7).integers(3, cfg.vocab_size, size=(1, 300)))

    def soft_head(name, t):
        return t * 0.125 if name.endswith("embed_tokens.weight") and kind == "opt" else t

    def run(flag):
        monkeypatch.setenv("SD_PREFILL_ATTN", flag)
        m = hip.engine.SpecDecModel.synthetic(cfg, seed=17, dtype=torch.bfloat16, max_pos=320, transform=soft_head)
        ses = m.new_session(320)
        a = ses.forward(ids[0, :200].to(torch.int32).cuda(), 8).cpu().clone()
        b = ses.forward(ids[0, 200:].to(torch.int32).cuda(), 8).cpu().clone()
        kv = [t.float().cpu().clone() for t in ses.past_key_values()[1]]
        return m, a, b, kv
    m, a1, b1, kv1 = run("1")
    sd16 = _host_sd(m)
    del m
    _, a0, b0, kv0 = run("0")
    torch.cuda.empty_cache()
    o16, o32 = oracle.RefCausalLM(cfg, sd16), oracle.RefCausalLM(cfg, {k: v.float() for k, v in sd16.items()})
    r16, r32 = o16(ids).logits.float()[0], o32(ids).logits.float()[0]
    for name, new, old, lo, hi in (("200-row pass", a1, a0, 192, 200), ("100-row pass at 200", b1, b0, 292, 300)):
        ref16, truth = r16[lo:hi], r32[lo:hi]
        e_hip, e_ref = float((new - truth).abs().max()), float((ref16 - truth).abs().max())
        rms_hip, rms_ref = float((new - truth).pow(2).mean().sqrt()), float((ref16 - truth).pow(2).mean().sqrt())
        d_old = float((new - old).abs().max())
        print(f"{kind}, {name}: max err hip {e_hip:.4f} ref-bf16 {e_ref:.4f}; rms {rms_hip:.5f} / {rms_ref:.5f}; vs attn_kernel {d_old:.4f}")
        _assert_within_reference_error((e_hip, e_ref, rms_hip, rms_ref), f"{kind}, {name}")
        assert d_old <= 2.0 ** -6 * float(truth.abs().max()), (kind, name, d_old, float(truth.abs().max()))
    # layer 0's K / V rows do not depend on attention at all: bit-identical; layer 1's only through one bf16 rounding of layer 0
    for x1, x0 in zip(kv1, kv0):
        assert float((x1 - x0).abs().max()) <= 0.05 * max(1.0, float(x0.abs().max()))
