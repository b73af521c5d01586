"""attn_prefill_blocked_kernel<T, D, KV8> (`pytest -m gpu`): the matrix-core prefill attention with its score tile cut into
blocks of keys, which runs where attn_prefill_kernel's single tile no longer fits the LDS (past 2048 keys at D = 128, 2176 at
D = 64) and, under SD_PREFILL_ATTN_BLOCK=K, at any context.

  1. bit-equality with attn_prefill_kernel wherever both run (the kernel's contract: same scores, same probabilities, same
     order of every sum) - logits and the appended K / V rows, blocks of 64 and 128 keys;
  2. planted keys at the block edges (tests/prefill_block_layouts.py; shown to discriminate in test_prefill_blocked_cpu.py);
  3. past the tile limit, 2304 keys: the blocked kernel with the default block and the default route, against the oracle and
     against attn_kernel (SD_PREFILL_ATTN=0);
  4. a 6144-token prompt in 256-row passes - past the 5760 / 5888 keys at which such a pass used to end in a capacity error,
     where the default route hands a small launch to the blocked kernel - and a 5-row verify on top of it, against the oracle;
  5. the public loop (speculative_sampling) and sd_batch_prefill under a forced block of 64 keys against the default route.

Oracle, runner, bars and scale folding are those of tests/attn_probe.py, test_gpu_attention_edges.py and
prefill_probe_layouts.py; their MAX_SEQ is 1040, so the long-context tests give the runner and the oracle the arena length of
the model (registered for the length of a test, as the wide_models fixture does).  No bar is measured on
the code under test: bit equality, _assert_within_reference_error (HIP's error against the fp32 truth at most 1.5x the
same-dtype oracle's own) and attn_probe.tol16 of the reference's error between the two kernels."""
import functools

import numpy as np
import pytest
import torch

import oracle
import attn_probe as P
import prefill_block_layouts as B
import prefill_probe_layouts as L
from prefill_probe_layouts import wide_models  # noqa: F401  (fixture)
from test_gpu_attention_edges import Runner, _run_causal, _Stats, _Env, _sd, hip  # noqa: F401  (hip: the module's fixture)
from test_gpu_production_parity import _assert_within_reference_error
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict, perturb_state_dict

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("wide_models")]

DEFAULT = dict(SD_PREFILL_ATTN=1, SD_PREFILL_ATTN_BLOCK=0)         # the default route, whatever the caller's environment holds


def _dev(tokens):
    return torch.from_numpy(np.asarray(tokens).astype(np.int32)).cuda()


def _counts(ses):
    return ses.prefill_attn_launches(), ses.prefill_attn_blocked_launches()


# --------------------------------------------------------------------------- 1. the same bits as the single-tile kernel
BIT_CALLS = [(81, 37), (200, 0), (256, 37), (256, 700)]


@pytest.mark.parametrize("name,dt,kvq", B.CASES, ids=B.CASE_IDS)
def test_blocked_kernel_is_bit_identical_to_the_tile_kernel(hip, name, dt, kvq):
    """One call of 81 rows at pos0 37 (a ragged last group, one partial block), 200 at 0 (a ragged last V chunk), 256 at 37
    (a block edge inside a group's causal range) and 256 at 700 (S = 956 = 15 blocks of 64: blocks wholly past the early
    groups' range), the marker at the own position of a tail row: the 64 tail logit rows and layer 0's appended K / V rows
    under SD_PREFILL_ATTN_BLOCK=64 and =128 equal those under =0 bit for bit.  The blocked counter rises by one per layer per
    call under the forced setting and stays 0 under =0; the prefill counter counts either kernel."""
    got = {}
    for block in (0, 64, 128):
        with _Env(SD_PREFILL_ATTN=1, SD_PREFILL_ATTN_BLOCK=block):
            r = Runner(hip, name, dt, kv_dtype=kvq)
            assert r.cfg.num_hidden_layers == 1
            for n, pos0 in BIT_CALLS:
                lay = P.Layout(pos0 + n, n, pos0 + n - 10, n - 10, "own")
                t = P.layout_tokens(lay)
                r.plant(t, 0, pos0)
                r.plant(t, lay.S, lay.S + 1)
                before = _counts(r.ses)
                logits = r.run(lay, B.TAIL)
                after = _counts(r.ses)
                assert after[0] - before[0] == 1 and after[1] - before[1] == (1 if block else 0), (block, n, pos0, before, after)
                got[block, n, pos0] = (logits, r.ses.kv[0, :, :, pos0:pos0 + n, :].cpu().clone())
            if not block:
                assert r.ses.prefill_attn_blocked_launches() == 0
            torch.cuda.synchronize()
    for n, pos0 in BIT_CALLS:
        want = got[0, n, pos0]
        assert bool(torch.isfinite(want[0]).all()) and float(want[0].abs().max()) > 0
        for block in (64, 128):
            have = got[block, n, pos0]
            assert torch.equal(have[0], want[0]), (name, dt, kvq, block, n, pos0, float((have[0] - want[0]).abs().max()))
            assert torch.equal(have[1], want[1]), (name, dt, kvq, block, n, pos0, "appended K / V rows")


# --------------------------------------------------------------------------- 2. planted keys at the block edges
@pytest.mark.parametrize("name,dt,kvq", B.CASES, ids=B.CASE_IDS)
def test_blocked_kernel_planted_key_at_every_block_edge(hip, name, dt, kvq):
    """The 36 layouts of prefill_block_layouts under SD_PREFILL_ATTN_BLOCK=128: the marker at the last / first key of a
    block (the first key of the last, partial block among them), at a row's own position where that is a block's last or
    first key, at its successor and in the stale slot behind the call (rows in front bit-identical to the filler run)."""
    runners = []
    _run_causal(hip, "prefill blocked", name, dt, B.layouts(), kvq=kvq, env=dict(SD_PREFILL_ATTN=1, SD_PREFILL_ATTN_BLOCK=B.BLOCK),
                tail=B.TAIL, check=runners.append)
    assert len(runners) == 2
    for r in runners:                                              # every matrix-core launch of the run was the blocked kernel's
        n_all, n_blocked = _counts(r.ses)
        assert n_blocked == n_all >= len(B.layouts())


# --------------------------------------------------------------------------- long contexts: registry, runner, oracle
LONG_POS = 2560
LONG_MODELS = {f"{name}_p{LONG_POS}": dict(L.WIDE_MODELS[name], max_position_embeddings=LONG_POS)
               for name in ("llama_d128_h512", "llama_gqa_d64_h512")}


@pytest.fixture
def long_models(monkeypatch):
    """LONG_MODELS in attn_probe's registry for the length of one test (see prefill_probe_layouts.wide_models)."""
    for name, kw in LONG_MODELS.items():
        monkeypatch.setitem(P.MODELS, name, kw)


@functools.lru_cache(maxsize=None)
def _long_oracle(name, dt, kvq=None):
    return P.ProbeOracle(name, P.DTYPES[dt], kvq, sd=_sd(name), max_seq=P.probe_config(name).max_position_embeddings)


# --------------------------------------------------------------------------- 3. past the tile limit, default settings
LONG_CASES = [(f"{n}_p{LONG_POS}", d, k) for n, d, k in B.CASES]


def _route(hip, cfg, rows, s_max, block=0):
    """sd_prefill_attn_route on this device (cus = 0): 0 attn_kernel, 1 single tile, 2 blocked."""
    import ctypes as C
    k = C.c_int(-1)
    hip.engine.check(hip.lib.sd_prefill_attn_route(cfg.head_dim, cfg.num_attention_heads, rows, s_max, block, 0, C.byref(k)), "route")
    return k.value


@pytest.mark.parametrize("name,dt,kvq", LONG_CASES, ids=B.CASE_IDS)
def test_past_the_tile_limit_the_blocked_kernel_and_the_default_route(hip, long_models, name, dt, kvq):
    """2048 planted rows, then one 256-row call at pos0 = 2048 (S = 2304 keys: past 2048 at D = 128 and past 2176 at D = 64)
    with 64 tail logits; the marker at key 0, at key 2047 and at a tail row's own position.  Three settings: the default, the
    blocked kernel with the default block (SD_PREFILL_ATTN_BLOCK=256) and SD_PREFILL_ATTN=0.  The rows of each lie within the
    1.5x rule of the same-dtype oracle and the fp32 truth, and the blocked kernel's within tol16(e_ref) of the
    SD_PREFILL_ATTN=0 run of the same rows - both kernels round scores and probabilities identically, only the order of the
    P.V sum differs.  Route: under the forced block both counters rise by one (attn_kernel took such a pass before); under
    the default they follow sd_prefill_attn_route - these models launch 4 or 8 heads x 16 row groups, far fewer than two
    workgroups per CU, where the three sweeps measured 0.5-0.9x of attn_kernel's split keys, so the
    default keeps attn_kernel here and hands the pass to the blocked kernel only where attn_kernel cannot hold it
    (test_prompt_past_the_old_capacity_wall_and_a_verify_on_top); launches of two workgroups per CU and more take the blocked
    kernel by default (test_prefill_blocked_cpu.py pins the rule on the host, tools/prefill_attn_bench.py --sweep asserts it
    on the device)."""
    S, n = 2304, 256
    lays = [P.Layout(S, n, 0, n - 1, "key0"), P.Layout(S, n, 2047, n - 33, "last_cached"), P.Layout(S, n, 2048 + 250, 250, "own")]
    o32, o16 = _long_oracle(name, "fp32"), _long_oracle(name, dt, kvq)
    got = {}
    for tag, flag, block in (("default", 1, 0), ("blocked", 1, 256), ("attn_kernel", 0, 0)):
        st = _Stats(f"S = 2304, {tag} {name} {dt} {kvq}")
        with _Env(SD_PREFILL_ATTN=flag, SD_PREFILL_ATTN_BLOCK=block):
            r = Runner(hip, name, dt, kv_dtype=kvq, max_seq=P.probe_config(name).max_position_embeddings)
            assert r.ses.max_rows >= n
            kernel = _route(hip, r.cfg, n, S, block) if flag else 0
            assert kernel == (2 if block else 0 if r.cfg.num_attention_heads * 16 < 2 * torch.cuda.get_device_properties(0).multi_processor_count else 2)
            want = {0: (0, 0), 2: (1, 1)}[kernel]
            for lay in lays:
                t = P.layout_tokens(lay)
                r.plant(t, 0, S - n)
                r.plant(t, S, S + 1)
                before = _counts(r.ses)
                assert lay.S < r.max_seq                           # (Runner.run plants the stale slot behind the call)
                got[tag, lay] = r.run(lay, B.TAIL)
                after = _counts(r.ses)
                assert (after[0] - before[0], after[1] - before[1]) == want, (tag, lay, before, after)
                st.judge(got[tag, lay], o32.logits(lay)[-B.TAIL:], o16.logits(lay)[-B.TAIL:], lay)
            torch.cuda.synchronize()
        st.report()
    for lay in lays:
        e_ref = float((o16.logits(lay)[-B.TAIL:] - o32.logits(lay)[-B.TAIL:]).abs().max())
        for tag in ("blocked", "default"):
            d = float((got[tag, lay] - got["attn_kernel", lay]).abs().max())
            print(f"{name} {dt} {kvq} {lay}: {tag} vs attn_kernel max {d:.4f}; reference error {e_ref:.4f}, bar {P.tol16(e_ref):.4f}")
            assert d <= P.tol16(e_ref), (name, dt, kvq, lay, tag, d, e_ref)


# --------------------------------------------------------------------------- 4. past the old capacity wall
def _errors(got, ref16, truth, label):
    errs = P.errors(got, ref16, truth)
    print(f"{label}: |logit| max {float(truth.abs().max()):.2f}; max err hip {errs[0]:.4f} ref {errs[1]:.4f}; rms {errs[2]:.5f} / {errs[3]:.5f}")
    assert bool(torch.isfinite(got).all()), label
    _assert_within_reference_error(errs, label)


def _ref_tail_and_verify(lm, ids, n_prompt, n_tail):
    """Logits of the prompt's last n_tail rows and of the rows fed behind the prompt (a one-layer model: attn_probe.kv_rows)."""
    cut = n_prompt - n_tail
    a = lm(ids[:, cut:n_prompt], past_key_values=[P.kv_rows(lm, ids, 0, cut)])
    b = lm(ids[:, n_prompt:], past_key_values=a.past_key_values)
    return a.logits.float()[0], b.logits.float()[0]


WALL_POS, WALL_PROMPT = 6400, 6144


@pytest.mark.parametrize("base,dt,kvq", [("llama_d128_h512", "bf16", None), ("llama_gqa_d64_h512", "bf16", None),
                                         ("llama_d128_h512", "bf16", "fp8"), ("llama_gqa_d64_h512", "fp16", "fp8")],
                         ids=["d128-bf16", "gqa_d64-bf16", "d128-bf16-fp8kv", "gqa_d64-fp16-fp8kv"])
def test_prompt_past_the_old_capacity_wall_and_a_verify_on_top(hip, base, dt, kvq):
    """A 6144-token prompt through Session.forward (24 passes of 256 rows) on a one-layer hidden-512 model with 6400
    positions and random weights: a 256-row pass that reached past 5760 (D = 128) / 5888 (D = 64) keys used to end in
    SD_ERR_CAPACITY ("exceed the LDS score tile").  The last 8 logit rows, then the 5 rows of a verify step on top (attn_kernel,
    8 key splits), against the same-dtype oracle under the 1.5x rule against the fp32 truth; with the fp8 arena the oracle
    emulates e4m3 with the session's scales folded in.  Route (sd_prefill_attn_route; 4 or 8 heads are far fewer than two
    workgroups per CU): the 8 passes up to 2048 keys take the single tile, the passes behind them attn_kernel while its two key
    splits hold 256 rows, and the last ones - past 5760 keys at D = 128: two passes, past 5888 at D = 64: one - the blocked
    kernel."""
    cfg = ModelConfig(**dict(L.WIDE_MODELS[base], max_position_embeddings=WALL_POS))
    dtype = P.DTYPES[dt]
    sd = {k: v.to(torch.bfloat16).float() for k, v in make_state_dict(cfg, 37, head_gain=2.0).items()}
    ids = torch.from_numpy(np.random.default_rng(13).integers(3, cfg.vocab_size, size=(1, WALL_PROMPT + 5)))
    scales = L.stream_scales(0, cfg)
    with _Env(**DEFAULT):
        m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, dtype), dtype=dtype)
        ses = m.new_session(WALL_POS, kv_dtype=kvq)
        if kvq:
            ses.kv_scale.copy_(scales.to(ses.kv_scale.device))
            torch.cuda.synchronize()
        assert ses.max_rows == 256
        routes = [_route(hip, cfg, 256, 256 * k) for k in range(1, 25)]
        n_blocked = 2 if cfg.head_dim == 128 else 1
        assert routes == [1] * 8 + [0] * (16 - n_blocked) + [2] * n_blocked
        a = ses.forward(_dev(ids[0, :WALL_PROMPT]), 8).float().cpu().clone()
        assert _counts(ses) == (8 + n_blocked, n_blocked)
        b = ses.forward(_dev(ids[0, WALL_PROMPT:]), 5).float().cpu().clone()
        assert _counts(ses) == (8 + n_blocked, n_blocked)
    sd16 = P.cast_sd(L.fold_scales(cfg, sd, scales) if kvq else sd, dtype)
    ra16, rb16 = _ref_tail_and_verify(oracle.RefCausalLM(cfg, sd16, kv_quant=kvq), ids, WALL_PROMPT, 8)
    ra32, rb32 = _ref_tail_and_verify(oracle.RefCausalLM(cfg, sd), ids, WALL_PROMPT, 8)
    _errors(a, ra16, ra32, f"{base} {dt} {kvq}: last 8 rows of a 6144-token prompt")
    _errors(b, rb16, rb32, f"{base} {dt} {kvq}: 5-row verify at 6144 keys")


# --------------------------------------------------------------------------- 5. through the public interface
def test_speculative_sampling_is_byte_equal_under_a_forced_block(hip, monkeypatch):
    """speculative_sampling (native loop, device Philox, bf16) on a tiny Llama pair whose target qualifies (hidden 512,
    D = 128, 2 layers), a 150-token prompt, gamma = 4, 24 new tokens, under SD_PREFILL_ATTN_BLOCK=64 and =0: tokens, accepted
    lengths and the acceptance ratio are equal to the last bit (layer 1 reads what the prefill kernel wrote), and the target
    session's blocked counter is non-zero in the first run only."""
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import noise
    tc = ModelConfig(arch="llama", vocab_size=512, hidden_size=512, intermediate_size=512, num_hidden_layers=2,
                     num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=256, rms_norm_eps=1e-5)
    dc = load_config("tiny-llama-draft")
    tsd, dsd = make_state_dict(tc, 3), make_state_dict(dc, 4)
    prompt = torch.from_numpy(np.random.default_rng(6).integers(3, tc.vocab_size, size=(1, 150))).cuda()
    runs = {}
    for block in (64, 0):
        with _Env(SD_PREFILL_ATTN=1, SD_PREFILL_ATTN_BLOCK=block):
            dm = hip.engine.SpecDecModel.from_state_dict(dc, P.cast_sd(dsd, torch.bfloat16), dtype=torch.bfloat16)
            tm = hip.engine.SpecDecModel.from_state_dict(tc, P.cast_sd(tsd, torch.bfloat16), dtype=torch.bfloat16)
            sessions, new_session = [], tm.new_session
            monkeypatch.setattr(tm, "new_session", lambda *a, **kw: sessions.append(new_session(*a, **kw)) or sessions[-1])
            out, det = S.speculative_sampling(prompt, dm, tm, -1, None, 24, gamma=4, details=True, rng=noise.DeviceNoise(77))
            assert len(sessions) == 1
            runs[block] = (out.cpu(), list(det["acc_len"]), float(det["acc_rate"]), _counts(sessions[0]))
    assert runs[64][3][0] == runs[0][3][0] == tc.num_hidden_layers          # the prompt's one prefill pass, either kernel
    assert runs[64][3][1] == tc.num_hidden_layers and runs[0][3][1] == 0
    assert runs[64][0].shape[1] == 150 + 24
    assert torch.equal(runs[64][0], runs[0][0])
    assert runs[64][1] == runs[0][1] and runs[64][2] == runs[0][2]


def test_batched_prefill_is_bit_equal_under_a_forced_block(hip):
    """One sd_batch_prefill of three fp8 streams (40 / 33 / 90 rows, per-stream scales: prefill_probe_layouts.batch_model, a
    two-layer GQA D = 64 model) under SD_PREFILL_ATTN_BLOCK=64 and =0: the 1-row logits that follow - layer 1's K / V rows
    carry what the prefill attention computed - are equal bit for bit; the pass counts on its first session."""
    cfg, sd, ids = L.batch_model()
    got = {}
    for block in (64, 0):
        with _Env(SD_PREFILL_ATTN=1, SD_PREFILL_ATTN_BLOCK=block):
            m = hip.engine.SpecDecModel.from_state_dict(cfg, P.cast_sd(sd, torch.bfloat16), dtype=torch.bfloat16)
            sess = []
            for i in range(3):
                ses = m.new_session(128, kv_dtype="fp8")
                ses.kv_scale.copy_(L.stream_scales(i, cfg).to(ses.kv_scale.device))
                sess.append(ses)
            torch.cuda.synchronize()
            seqs = [_dev(t[0]) for t in ids]
            hip.engine.batch_prefill(sess, seqs, list(L.BATCH_ROWS))
            assert [_counts(s) for s in sess] == [(cfg.num_hidden_layers, cfg.num_hidden_layers if block else 0), (0, 0), (0, 0)]
            got[block] = [ses.forward(sq[n:n + 1], 1).float().cpu().clone() for ses, sq, n in zip(sess, seqs, L.BATCH_ROWS)]
    for a, b in zip(got[64], got[0]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
