"""The native autoregressive loop (sd_ar_batch_generate) on the GPU (`pytest -m gpu`): stream-batched runs against the CPU
oracle per stream (the device's Philox variates replayed into it, tests/philox_replay.py), the loop's in/out state through a
direct ctypes call, the single-stream route against the interpreter loop bit for bit in bf16, and the error path."""

import numpy as np
import pytest
import torch

import oracle
from philox_replay import PhiloxOracleNoise
from llmspeculativesampling_amd.config import ModelConfig, load_config
from llmspeculativesampling_amd.synth import make_state_dict

pytestmark = pytest.mark.gpu

# the small bf16 configuration of the native-parity tests (vocab wide enough for the head's tile maxima)
BF16_CFG = dict(arch="llama", vocab_size=8192, hidden_size=256, intermediate_size=704, num_hidden_layers=2,
                num_attention_heads=4, num_key_value_heads=2, max_position_embeddings=512, rms_norm_eps=1e-6)


@pytest.fixture(scope="module")
def hip():
    import types
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd import _lib, engine, noise
    return types.SimpleNamespace(S=S, lib=_lib.lib, L=_lib, engine=engine, noise=noise)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _prompts(V, lens, seed0=40):
    return [torch.from_numpy(np.random.default_rng(seed0 + i).integers(3, V, size=(1, n))) for i, n in enumerate(lens)]


def _oracle_runs(hip, cfg, sd, prompts, seeds, N, eos, kw):
    ref = oracle.RefCausalLM(cfg, sd)
    return [oracle.autoregressive_sampling(p, ref, N, eos, 1.0, kw["top_k"], kw["top_p"],
                                           noise=PhiloxOracleNoise(hip.lib, s, 1, _st)) for p, s in zip(prompts, seeds)]


def test_batched_streams_equal_the_oracle_per_stream(hip):
    """Four streams of 9 / 11 / 13 / 15 prompt tokens through shared passes, each against its own oracle run; the EOS is
    what the oracle's stream 1 generates at index 6, so at least that stream leaves the passes early."""
    cfg = load_config("tiny-llama-target")
    sd = make_state_dict(cfg, 21)
    prompts, seeds, N = _prompts(cfg.vocab_size, (9, 11, 13, 15)), [900 + i for i in range(4)], 20
    kw = dict(top_k=20, top_p=0.9)
    probe = _oracle_runs(hip, cfg, sd, prompts[1:2], seeds[1:2], N, -1, kw)[0]
    eos = int(probe[0, prompts[1].shape[1] + 6])
    wants = _oracle_runs(hip, cfg, sd, prompts, seeds, N, eos, kw)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    timing = {}
    outs = hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts], m, N, eos, seeds=seeds, _timing=timing, **kw)
    stopped = 0
    for p, want, got in zip(prompts, wants, outs):
        print("stream", p.shape[1], "oracle", want[0, p.shape[1]:].tolist(), "got", got[0, p.shape[1]:].tolist())
        assert got.dtype == torch.int64 and got.is_cuda
        stopped += int(want.shape[1] < p.shape[1] + N)
    for want, got in zip(wants, outs):
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    assert 1 <= stopped < 4
    # one entry per step: the streams in it never grow, the first step holds all four, the count is the longest stream's
    steps = timing["step"]
    assert len(steps) == max(w.shape[1] - p.shape[1] for w, p in zip(wants, prompts))
    assert steps[0][1] == 4 and all(a[1] >= b[1] >= 1 for a, b in zip(steps, steps[1:])) and all(ms > 0 for ms, _ in steps)
    assert sum(n for _, n in steps) == sum(w.shape[1] - p.shape[1] for w, p in zip(wants, prompts))


@pytest.mark.parametrize("N", [6, 1])
def test_sixteen_streams_on_opt_equal_the_oracle(hip, N):
    """The stream limit, on OPT (learned positions, LayerNorm, biases); N = 1: every stream finishes on the first step."""
    cfg = load_config("tiny-opt-pre")
    sd = make_state_dict(cfg, 33)
    prompts, seeds = _prompts(cfg.vocab_size, [5 + (3 * i) % 7 for i in range(16)], 70), [500 + i for i in range(16)]
    kw = dict(top_k=20, top_p=0.9)
    wants = _oracle_runs(hip, cfg, sd, prompts, seeds, N, -1, kw)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, sd, dtype=torch.float32)
    outs = hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts], m, N, -1, seeds=seeds, **kw)
    for p, want, got in zip(prompts, wants, outs):
        assert got.shape[1] == p.shape[1] + N
        np.testing.assert_array_equal(got.cpu().numpy(), want.numpy())
    if N == 1:
        with pytest.raises(ValueError, match="1..16 streams"):
            hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts] + [prompts[0].cuda()], m, N, -1, **kw)


class _Direct:
    """The arenas of n streams and a direct call of sd_ar_batch_generate on them."""

    def __init__(self, hip, m, prompts, seeds):
        self.hip, self.m, self.B = hip, m, len(prompts)
        self.kvs, self.seqs, self.hosts, self.errs = [], [], [], []
        self.arr = (hip.L.SdArStream * self.B)()
        for it, p, seed in zip(self.arr, prompts, seeds):
            L, cap = p.shape[1], p.shape[1] + 40
            kv, seq = hip.S._loop_common.open_stream(m, p[0], cap, cap, 1.0, 20, 0.9)
            host = np.zeros(cap, dtype=np.int32)
            host[:L] = p[0].numpy()
            err = torch.zeros(2, dtype=torch.int32, device="cuda")
            self.kvs.append(kv), self.seqs.append(seq), self.hosts.append(host), self.errs.append(err)
            it.session, it.seq, it.probs = kv._session.handle, seq.data_ptr(), kv._probs.data_ptr()
            it.err_words, it.host_seq = err.data_ptr(), host.ctypes.data
            it.len, it.cache_len, it.seed, it.draw = L, L - 1, seed, 0
        hip.engine.batch_prefill([kv._session for kv in self.kvs], self.seqs, [p.shape[1] - 1 for p in prompts])
        nb = hip.lib.sd_ar_block_bytes(self.B)
        self.dev_block = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        self.host_block = torch.zeros(nb, dtype=torch.uint8).pin_memory()

    def run(self, Ts, eos=-1):
        for it, T in zip(self.arr, Ts):
            it.T = T
        ses, kv = self.kvs[0]._session, self.kvs[0]
        L = self.hip.L
        sampling = L.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=self.m.cfg.vocab_size, ld=kv._probs.stride(0), eos_token_id=eos)
        head = L.SdHeadScratch(logits=ses.logits.data_ptr(), ld_logits=ses.logits.stride(0), norm_mode=self.m.norm_mode)
        log = L.SdArLog(n_steps=-1, err=-1)
        rc = self.hip.lib.sd_ar_batch_generate(self.arr, self.B, sampling, head, kv._norm_ws.data_ptr(), self.dev_block.data_ptr(),
                                               self.host_block.data_ptr(), log, _st(), None)
        return rc, log.n_steps, log.err


def test_direct_call_state_and_continuation(hip):
    """sd_ar_batch_generate through ctypes, two streams: draw, cache_len and steps after a call; host and device token
    buffers agree; a second call that continues from that state gives the tokens of one call with the larger T."""
    cfg = load_config("tiny-llama-target")
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, 21), dtype=torch.float32)
    prompts, seeds = _prompts(cfg.vocab_size, (7, 12), 60), [31, 32]
    a = _Direct(hip, m, prompts, seeds)
    first = [7 + 5, 12 + 3]
    assert a.run(first) == (0, 5, 0)
    for it, p, T, seq, host in zip(a.arr, prompts, first, a.seqs, a.hosts):
        gen = T - p.shape[1]
        assert (it.len, it.draw, it.cache_len, it.steps, it.done) == (T, gen, T - 1, gen, 1)
        assert host[:it.len].tolist() == seq[:it.len].tolist()
    final = [7 + 9, 12 + 11]
    assert a.run(final) == (0, 8, 0)
    b = _Direct(hip, m, prompts, seeds)
    assert b.run(final) == (0, 11, 0)
    for ia, ib, p, T, ha, hb, seq in zip(a.arr, b.arr, prompts, final, a.hosts, b.hosts, a.seqs):
        assert (ia.len, ia.draw, ia.cache_len) == (ib.len, ib.draw, ib.cache_len) == (T, T - p.shape[1], T - 1)
        assert ia.steps == T - first[0 if p.shape[1] == 7 else 1] and ib.steps == T - p.shape[1]
        assert ha[:T].tolist() == hb[:T].tolist() == seq[:T].tolist()
    assert a.run(final) == (0, 0, 0)                              # nothing left to do: no step, the state stays
    assert [it.len for it in a.arr] == final


@pytest.mark.parametrize("L", [24, 300], ids=["prompt24", "prompt300_two_prefill_chunks"])
def test_single_stream_native_loop_bit_equals_the_python_loop(hip, L):
    """bf16, the head's raw slab and tile maxima feeding the sampler: the native route against _native=False under the
    same seed - same prompt feeding (a 300-token prompt takes two prefill chunks), same draw order, identical ids."""
    cfg = ModelConfig(**BF16_CFG)
    m = hip.engine.SpecDecModel.from_state_dict(cfg, make_state_dict(cfg, 5, dtype=torch.bfloat16), dtype=torch.bfloat16)
    prompt = torch.from_numpy(np.random.default_rng(3).integers(3, cfg.vocab_size, size=(1, L))).cuda()
    kw = dict(top_k=20, top_p=0.9)
    na, nb = hip.noise.DeviceNoise(123), hip.noise.DeviceNoise(123)
    a = hip.S.autoregressive_sampling(prompt, m, 16, -1, rng=na, **kw)
    b = hip.S.autoregressive_sampling(prompt, m, 16, -1, rng=nb, _native=False, **kw)
    assert a.shape == (1, L + 16) and torch.equal(a, b)
    assert na.draw == nb.draw == 16
    assert len(set(a[0, L:].tolist())) > 4                        # (a run that really samples, not one repeated token)


def test_nan_in_the_final_norm_raises_norm_logits_error_on_both_loops(hip):
    cfg = load_config("tiny-llama-target")
    bad = {k: v.clone() for k, v in make_state_dict(cfg, 21).items()}
    bad["model.norm.weight"][3] = float("nan")
    m = hip.engine.SpecDecModel.from_state_dict(cfg, bad, dtype=torch.float32)
    prompts = _prompts(cfg.vocab_size, (9, 11), 60)
    for native in (True, False):
        with pytest.raises(RuntimeError, match="^norm logits error$"):
            hip.S.autoregressive_sampling(prompts[0].cuda(), m, 8, -1, top_k=20, top_p=0.9, rng=hip.noise.DeviceNoise(5),
                                          _native=native)
    with pytest.raises(RuntimeError, match="^norm logits error$"):
        hip.S.autoregressive_sampling_batch([p.cuda() for p in prompts], m, 8, -1, top_k=20, top_p=0.9, seeds=[5, 6])
    d = _Direct(hip, m, prompts, [5, 6])
    assert d.run([9 + 8, 11 + 8]) == (0, 1, 2)                    # one step ran, 'norm logits error'
    assert [it.len for it in d.arr] == [9, 11] and [it.draw for it in d.arr] == [0, 0]    # its tokens were not committed
    assert [e.tolist() for e in d.errs] == [[0, 0], [0, 0]]       # the hand-off launch cleared the words
