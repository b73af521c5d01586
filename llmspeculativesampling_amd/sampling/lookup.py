"""Prompt-lookup drafting: speculative decoding without a draft model.

The draft of an iteration is a suffix match over the sequence itself (``sampling.utils.lookup_propose`` has the definition,
sd_lookup_propose the kernel): the most recent earlier occurrence of the last few tokens is found and the tokens that followed
it are proposed.  A lookup draft is a deterministic proposal, so its q row is one-hot, and the verify half of the iteration -
target forward, norm, accept scan, residual / bonus sample - is ``speculative_sampling``'s, launch for launch.  The output is
distributed as the target's own sampling whatever the lookup proposes; what the lookup decides is how many target passes it
takes.  Device Philox only; the loops run inside libspecdec (sd_lookup_generate, sd_lookup_batch_generate).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from .._lib import SD_LOOKUP_MAX_NGRAM, check, lib
from ..engine import _stream, as_specdec_model, check_token_ids
from ..noise import DeviceNoise
from ._loop_common import (LockstepStreams, details_dict, device_rng, make_noise, open_stream, sampling_block,
                           single_stream_native_call, spec_scratch, spec_stream, stream_seeds)

INFO_BYTES = 8                                                    # the proposer's two ints behind a stream's result block


def _check_arguments(target_model, gamma, temperature, ngram_max, ngram_min, rng="device") -> None:
    """What both entries refuse with ValueError before a model is touched."""
    if not device_rng(rng):
        raise ValueError('prompt lookup runs on the device RNG only: rng="device" (or a device noise object)')
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or float(temperature) == 0.0:
        raise ValueError(f"temperature: a non-zero number is required, not {temperature!r}")
    if isinstance(gamma, bool) or not isinstance(gamma, (int, np.integer)) or not 1 <= gamma <= 16:
        raise ValueError(f"gamma: 1..16 drafted tokens per iteration, not {gamma!r}")
    for name, v in (("ngram_max", ngram_max), ("ngram_min", ngram_min)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name}: an integer is required, not {v!r}")
    if not 1 <= ngram_max <= SD_LOOKUP_MAX_NGRAM:
        raise ValueError(f"ngram_max: 1..{SD_LOOKUP_MAX_NGRAM} tokens, not {ngram_max!r}")
    if not 1 <= ngram_min <= ngram_max:
        raise ValueError(f"ngram_min: 1..ngram_max ({ngram_max}) tokens, not {ngram_min!r}")
    if getattr(target_model, "tp_group", None) is not None:
        raise ValueError("prompt lookup is not available with a tensor-parallel target model")
    cfg = getattr(target_model, "cfg", None) or getattr(target_model, "config", None)
    if getattr(cfg, "is_encoder_decoder", False):
        raise ValueError("prompt lookup is not available with an encoder-decoder model")


@torch.no_grad()
def prompt_lookup_sampling(prefix: torch.Tensor, target_model, eos_token_id, pad_token_id, max_len: int, gamma: int = 4,
                           temperature: float = 1, top_k: int = 0, top_p: float = 0, ngram_max: int = 3, ngram_min: int = 1,
                           details: bool = False, *, rng="device"):
    """``speculative_sampling`` for a target without a draft model: every iteration drafts ``gamma`` tokens by prompt lookup
    (the longest match of the last ``ngram_min`` .. ``ngram_max`` tokens earlier in the sequence, the most recent among
    equals; ``sampling.utils.lookup_propose``) and verifies them in one target pass over gamma + 1 rows.  Output conventions,
    the EOS cut, the exceptions and the ``details`` dict are ``speculative_sampling``'s (``approx_time`` is the proposer's
    device time); ``details`` additionally carries ``match_len``, the match length of every iteration (0: nothing matched, the
    last token was repeated).  Philox draws per iteration: gamma + 1 reserved and unread, gamma accept uniforms, the residual /
    bonus sample - 2 * gamma + 2 in all, as ``speculative_sampling``.  ValueError before a model is touched: an ``rng`` that is
    not device Philox, a temperature of 0, ``gamma`` outside 1..16, n-gram bounds outside 1 <= ngram_min <= ngram_max <= 8, a
    tensor-parallel target, an encoder-decoder model."""
    _check_arguments(target_model, gamma, temperature, ngram_max, ngram_min, rng)
    assert prefix.shape[0] == 1, "input batch size must be 1"
    target_m = as_specdec_model(target_model)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    seq_len0 = prefix.shape[1]
    T = seq_len0 + max_len
    cap = T + gamma + 2
    host_seq = [int(t) for t in prefix[0].tolist()]
    if seq_len0 < T:
        try:
            check_token_ids(host_seq, V)
        except IndexError as e:
            print(e)
            raise RuntimeError("s") from e
    noise = make_noise(rng, dev)
    target, seq32 = open_stream(target_m, prefix[0], cap, cap + 1, temperature, top_k, top_p, noise)
    ld = target._probs.stride(0)
    q_hist = torch.empty((cap, ld), dtype=torch.float32, device=dev)
    match_len = np.zeros(max(1, T - seq_len0), dtype=np.int32)
    sampling = sampling_block(target._temperature, target._top_k, target._top_p, V, ld, eos_token_id)
    scratch = spec_scratch(target._session, target._session, target._norm_ws, target._session.max_rows)

    def call(res_dev, res_host, err_words, st):
        stream = spec_stream(None, target, seq32, err_words, res_dev.data_ptr(), res_host.data_ptr(), q_hist)
        check(lib.sd_lookup_generate(stream, gamma, ngram_max, ngram_min, sampling, scratch, st, match_len.ctypes.data, _stream()),
              "sd_lookup_generate")
    out_tokens, st, _, acc_len, acc_rate, (approx_time, target_time, other_time) = \
        single_stream_native_call(call, host_seq, T, gamma, eos_token_id, noise, dev, details, INFO_BYTES)
    calls = st.n_iters
    target._session.cache_len = st.target_len
    out = torch.tensor([out_tokens], dtype=torch.int64, device=prefix.device)
    if details:
        det = details_dict(approx_time, target_time, other_time, acc_len, float(np.mean(acc_rate)) if acc_rate else 0.0, calls, calls,
                           target_model_time=target_time, target_pre_cache_time=0, target_post_prob_time=0)
        det["match_len"] = match_len[:calls].tolist()
        return out, det
    return out


@torch.no_grad()
def prompt_lookup_sampling_batch(prefixes: Sequence[torch.Tensor], target_model, eos_token_id, pad_token_id, max_len: int,
                                 gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0, ngram_max: int = 3,
                                 ngram_min: int = 1, details: bool = False, seeds: Optional[Sequence[int]] = None):
    """B <= 16 streams in lock-step (sd_lookup_batch_generate): one proposer launch over the active streams per iteration,
    then the verify passes they share.  ``prefixes[i]`` is (1, L_i) int64; stream i runs on Philox stream ``seeds[i]`` (default
    ``torch.initial_seed() + i``) and equals ``prompt_lookup_sampling(prefixes[i], ..., rng=DeviceNoise(seeds[i]))``.  Returns
    the list of (1, len_i) outputs (and the list of ``details`` dicts, each with ``match_len``, when ``details``), as
    ``speculative_sampling_batch``.  The refusals are ``prompt_lookup_sampling``'s."""
    _check_arguments(target_model, gamma, temperature, ngram_max, ngram_min)
    try:
        B = len(prefixes)
    except TypeError:
        raise ValueError("prefixes: a sequence of (1, L) int64 prompts is required") from None
    if not 1 <= B <= 16:
        raise ValueError(f"prefixes: 1..16 streams decode at once, not {B}")
    if seeds is not None and len(seeds) != B:
        raise ValueError(f"seeds: {len(seeds)} seeds for {B} streams")
    target_m = as_specdec_model(target_model)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    for pf in prefixes:
        assert pf.shape[0] == 1, "input batch size must be 1"
        check_token_ids(pf, V)
    def open_slot(i, row, cap):
        """no draft session: the stream's own error words and the arena of its one-hot q rows"""
        target, seq32 = open_stream(target_m, row, cap, cap + 1, temperature, top_k, top_p)
        return (None, target, seq32, torch.zeros(3 * gamma + 1, dtype=torch.int32, device=dev),
                torch.empty((cap, target._probs.stride(0)), dtype=torch.float32, device=dev))
    # the B result blocks, then the B pairs of info ints
    table = LockstepStreams(prefixes, open_slot, dev, eos_token_id, max_len, gamma,
                            [DeviceNoise(seed) for seed in stream_seeds(seeds, B)], INFO_BYTES)
    t0 = table.streams[0].target
    match_len = [np.zeros(table.max_iters, dtype=np.int32) for _ in range(B)]
    ml = (C.c_void_p * B)(*[m.ctypes.data for m in match_len])
    check(lib.sd_lookup_batch_generate(table.arr, B, gamma, ngram_max, ngram_min,
                                       sampling_block(temperature, top_k, top_p, V, t0._probs.stride(0), eos_token_id),
                                       spec_scratch(t0._session, t0._session, table.norm_ws, table.per_pass), table.vlog.block, ml,
                                       _stream()),
          "sd_lookup_batch_generate")
    outs, ds = table.results(eos_token_id)
    for it, det, m in zip(table.arr, ds, match_len):
        det["match_len"] = m[:it.calls].tolist()
    return (outs, ds) if details else outs
