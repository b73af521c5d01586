"""Stream-batched speculative sampling ("throughput mode"): B independent prompt streams
decode in lockstep on one GPU and share every pass over the weights.  Each draft step is one forward over the B (or up
to 2B) new rows, each verify is one target forward over B*(gamma+1) rows: the bytes streamed per iteration are those of
ONE stream, the tokens produced are B times as many.

Every stream keeps its own KV arenas, probability arenas, token buffer and Philox stream, and runs exactly the
per-stream algorithm of reference sampling/speculative_sampling.py:1876-2076 (batch size 1 there, :1905): with the
same seeds the outputs equal those of B separate ``speculative_sampling(..., rng=DeviceNoise(seed))`` calls.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .._lib import lib, check, SdAcceptResult, SdBatchStream
from ..engine import as_specdec_model, _stream, check_token_ids, same_device, batch_prefill
from ..noise import DeviceNoise
from ._loop_common import LoopLog, accept_rates_f64, cut_after_new_eos, details_dict, open_stream, reseed_uniforms
from .autoregressive_sampling import ArRun
from .kvcache_model import KVCacheModel


@dataclass
class _Stream:
    draft: KVCacheModel
    target: KVCacheModel
    seq32: torch.Tensor
    err: torch.Tensor
    noise: DeviceNoise
    log: LoopLog
    prompt_len: int
    T: int
    ori_eos: int


class _Ms:                                                        # (bench.py reads e0.elapsed_time(e1))
    def __init__(self, ms):
        self.ms = ms

    def elapsed_time(self, _other):
        return self.ms


@torch.no_grad()
def speculative_sampling_batch(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id,
                               pad_token_id, max_len: int, gamma: int = 4, temperature: float = 1, top_k: int = 0,
                               top_p: float = 0, random_seed: int = None, details: bool = False,
                               seeds: Optional[Sequence[int]] = None, _timing: Optional[dict] = None):
    """B streams at once; ``prefixes[i]`` is (1, L_i) int64.  Returns a list of (1, len_i) tensors (and a list of
    ``details`` dicts with the reference's keys when ``details``).  Device Philox RNG, stream i seeded ``seeds[i]``."""
    draft_m, target_m = as_specdec_model(approx_model), as_specdec_model(target_model)
    same_device(draft_m, target_m)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    assert draft_m.cfg.vocab_size == V
    for pf in prefixes:
        check_token_ids(pf, V)
    B = len(prefixes)
    assert 1 <= B <= 16 and 1 <= gamma <= 16
    seeds = list(seeds) if seeds is not None else [int(torch.initial_seed()) + i for i in range(B)]
    res_sz = C.sizeof(SdAcceptResult)
    res_dev = torch.zeros((B, res_sz), dtype=torch.uint8, device=dev)
    res_host = torch.zeros((B, res_sz), dtype=torch.uint8).pin_memory()
    r_const = reseed_uniforms(random_seed, gamma, dev)
    max_iters = max(1, int(max_len)) + 1

    streams: List[_Stream] = []
    for i, pf in enumerate(prefixes):
        assert pf.shape[0] == 1, "input batch size must be 1"
        L = pf.shape[1]
        T = L + max_len
        cap = T + gamma + 2
        draft, _ = open_stream(draft_m, None, cap, 0, temperature, top_k, top_p)
        target, seq32 = open_stream(target_m, pf[0], cap, cap + 1, temperature, top_k, top_p)
        host = [int(t) for t in pf[0].tolist()]
        err = torch.zeros(3 * gamma + 1, dtype=torch.int32, device=dev)
        streams.append(_Stream(draft, target, seq32, err, DeviceNoise(seeds[i]),
                               LoopLog(host, cap, max_iters, gamma, q_fill=1.0), L, T, host.count(eos_token_id)))

    # prefill everything but the last prompt token, the B prompts packed into passes of up to 256 rows (engine.batch_prefill:
    # one pass over the weights serves several streams); the decode loop then starts with 1 new draft row and gamma+1 new
    # target rows per stream like every later iteration
    for side in ("draft", "target"):
        batch_prefill([getattr(s, side)._session for s in streams], [s.seq32 for s in streams],
                      [s.prompt_len - 1 for s in streams])

    # the lock-step loop itself runs inside libspecdec (sd_spec_batch_generate): per iteration gamma batched draft steps,
    # the verify passes, the batched accept + residual sample, one copy of the result blocks and one wait - the
    # interpreter sees the finished token buffers and the per-iteration statistics
    per_pass = streams[0].target._session.max_pass_rows
    norm_ws = torch.empty(lib.sd_norm_workspace_bytes(per_pass), dtype=torch.uint8, device=dev)
    cu = _stream()
    arr = (SdBatchStream * B)()
    for i, (it, s) in enumerate(zip(arr, streams)):
        it.draft, it.target = s.draft._session.handle, s.target._session.handle
        it.seq, it.q_hist, it.p_hist = s.seq32.data_ptr(), s.draft._probs.data_ptr(), s.target._probs.data_ptr()
        it.err_words = s.err.data_ptr()
        it.res_dev = res_dev.data_ptr() + i * res_sz
        it.res_host = res_host.data_ptr() + i * res_sz
        it.host_seq = s.log.host_seq.ctypes.data
        it.len, it.T, it.ori_eos_cnt = s.prompt_len, s.T, s.ori_eos
        it.draft_len = it.target_len = s.prompt_len - 1
        it.seed, it.draw = s.noise.seed, s.noise.draw
        it.acc_len_out, it.p_at_out, it.q_at_out = s.log.ptrs()[:3]
    n_log = max_iters * 2
    v_ms = np.zeros(n_log, dtype=np.float32)
    v_n = np.zeros(n_log, dtype=np.int32)
    v_ctx = np.zeros(n_log, dtype=np.float32)
    c_iters, c_err = C.c_int(0), C.c_int(0)
    d0, t0 = streams[0].draft._session, streams[0].target._session
    check(lib.sd_spec_batch_generate(arr, B, gamma, float(temperature), int(top_k or 0), float(top_p or 0.0), V,
                                     streams[0].draft._probs.stride(0), int(eos_token_id), int(random_seed or 0),
                                     r_const.data_ptr() if r_const is not None else None, draft_m.norm_mode,
                                     target_m.norm_mode, d0.logits.data_ptr(), d0.logits.stride(0), t0.logits.data_ptr(),
                                     t0.logits.stride(0), norm_ws.data_ptr(), per_pass,
                                     v_ms.ctypes.data, v_n.ctypes.data, v_ctx.ctypes.data, n_log, C.byref(c_iters),
                                     C.byref(c_err), cu), "sd_spec_batch_generate")
    if c_err.value:
        raise RuntimeError("s")
    if _timing is not None:
        for i in range(min(c_iters.value, n_log)):
            _timing.setdefault("verify", []).append((_Ms(float(v_ms[i])), None, int(v_n[i]), float(v_ctx[i])))
    outs, ds = [], []
    for it, s, pf in zip(arr, streams, prefixes):
        s.noise.seed, s.noise.draw = it.seed, it.draw
        s.draft._session.cache_len, s.target._session.cache_len = it.draft_len, it.target_len
        out = cut_after_new_eos(s.log.tokens(it.len), eos_token_id, s.ori_eos)
        outs.append(torch.tensor([out], dtype=torch.int64, device=pf.device))
        rate = accept_rates_f64(*s.log.ratios(it.calls))
        ds.append(details_dict(0, 0, 0, s.log.acc_len(it.calls), float(np.mean(rate)) if rate else 0.0, it.calls, it.calls,
                               target_model_time=0, target_pre_cache_time=0, target_post_prob_time=0))
    return (outs, ds) if details else outs


@torch.no_grad()
def autoregressive_sampling_batch(xs: Sequence[torch.Tensor], model, N: int, eos_token_id, temperature: float = 1,
                                  top_k: int = 0, top_p: float = 0, pad_token_id=None, *,
                                  seeds: Optional[Sequence[int]] = None, _timing: Optional[dict] = None):
    """``autoregressive_sampling`` for B streams at once: ``xs[i]`` is (1, L_i) int64, the result a list of (1, len_i)
    tensors.  The streams decode in lock-step and share every pass over the weights (sd_ar_batch_generate): each runs the
    algorithm of reference autoregressive_sampling.py:9-61 on its own Philox stream ``seeds[i]`` (default
    ``torch.initial_seed() + i``), so the outputs equal those of B ``autoregressive_sampling(..., rng=DeviceNoise(seed))``
    calls.  ``_timing["step"]`` receives (milliseconds, streams in the step) per step."""
    B = len(xs)
    if not 1 <= B <= 16:
        raise ValueError(f"autoregressive_sampling_batch takes 1..16 streams per call, not {B}")
    m = as_specdec_model(model)
    V = m.cfg.vocab_size
    for x in xs:
        assert x.dim() == 2 and x.shape[0] == 1 and x.shape[1] >= 1, "every stream is one (1, L) prompt"
        check_token_ids(x, V)
    seeds = list(seeds) if seeds is not None else [int(torch.initial_seed()) + i for i in range(B)]
    run = ArRun(m, temperature, top_k, top_p, eos_token_id)
    caps = [x.shape[1] + int(N) + 1 for x in xs]
    kvs, seqs = map(list, zip(*[open_stream(m, x[0], cap, cap, temperature, top_k, top_p) for x, cap in zip(xs, caps)]))
    # everything but the last prompt token, the prompts packed into shared passes; every step of the loop then feeds one
    # row per stream
    batch_prefill([kv._session for kv in kvs], seqs, [x.shape[1] - 1 for x in xs])
    for x, seed, kv, seq32 in zip(xs, seeds, kvs, seqs):
        run.add(kv, seq32, x[0].to(device="cpu", dtype=torch.int32).numpy(), x.shape[1] + int(N), DeviceNoise(seed))
    run.generate(timing=_timing is not None)
    if _timing is not None:
        _timing.setdefault("step", []).extend(run.steps)
    return [torch.from_numpy(run.tokens(i)).to(torch.int64).unsqueeze(0).to(x.device) for i, x in enumerate(xs)]
