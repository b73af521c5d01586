"""Caller-side quality check of the reference harness (untimed there): mean target log-prob of the generated
suffix, reference evaluation.py:109-132 ``get_score`` (decoder-only branch).  One full target forward through the
engine; the log-softmax/gather/mean is three torch ops on the device (not part of the decode path).

``score_tokens`` is the native scoring pass (sd_score_sequence): per-token log-probabilities, ranks and top-N lists of a
sequence this call did not generate, without an S x V logit tensor; ``score_rows_torch`` states its definition in torch."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib
from .engine import _stream, as_specdec_model, check_token_ids


@torch.no_grad()
def get_score(output: torch.Tensor, target_model, input_len: int) -> torch.Tensor:
    m = as_specdec_model(target_model)
    if m.cfg.is_encoder_decoder:
        raise NotImplementedError("encoder-decoder scoring (reference evaluation.py:126-132) is out of scope")
    assert output.dim() == 2 and output.size(0) == 1
    S = output.size(1)
    check_token_ids(output, m.cfg.vocab_size)
    ses = m.new_session(S + 1)
    ids = output[0].to(device=m.device, dtype=torch.int32)
    logits = torch.empty((S, m.cfg.vocab_size), dtype=torch.float32, device=m.device)
    done = 0
    while done < S:                                   # all S rows of logits, max_rows at a time
        n = min(64, S - done)                         # logit rows per call
        ses.forward(ids[done:done + n], n, logits_out=logits[done:done + n])
        done += n
    logp = torch.log_softmax(logits[:-1], dim=-1)
    picked = torch.gather(logp, -1, output[0, 1:, None].to(m.device))
    return picked[input_len - 1:].mean()


def score_from_logprobs(logprobs: torch.Tensor) -> torch.Tensor:
    """get_score of an output whose decode call returned ``logprobs`` (``logprobs=True`` of the sampling functions,
    speculative_sampling_queue_logprobs): those are the target log-probabilities get_score gathers - the model's own, before
    temperature, top_k and top_p - so the score is their mean, and no second target pass runs."""
    return logprobs.to(torch.float32).mean()


class TokenScores(NamedTuple):
    """What score_tokens returns for the S - input_len scored tokens of a (1, S) sequence."""
    logprobs: torch.Tensor        # (1, S - input_len) float32: the target's log-probability of each token
    ranks: torch.Tensor           # (1, S - input_len) int32: its 1-based place among the row's ids (value descending, ties to the lower id)
    top_ids: torch.Tensor         # (S - input_len, top_n) int32: the first top_n ids of that order ...
    top_logprobs: torch.Tensor    # (S - input_len, top_n) float32: ... and their log-probabilities


@torch.no_grad()
def score_tokens(output: torch.Tensor, target_model, input_len: int = 1, top_n: int = 0) -> TokenScores:
    """Per-token target log-probabilities, ranks and top-``top_n`` alternatives of ``output[0, input_len:]`` (prompt log-probs
    with ``input_len=1``, re-scoring of another model's output, ``top_logprobs=N`` of the usual request formats): ONE native
    scoring pass (sd_score_sequence: the forward passes and one scoring launch behind each pass of logit rows, at most 80 logit
    rows alive at a time) and one synchronisation.  The scores are the model's own, before temperature, top_k and top_p, as
    ``logprobs=True`` of the sampling functions returns them; include/specdec.h has the definition."""
    if output.dim() != 2 or output.size(0) != 1:
        raise ValueError(f"score_tokens: one (1, S) sequence, not a tensor of shape {tuple(output.shape)}")
    S = output.size(1)
    if not 1 <= input_len <= S - 1:
        raise ValueError(f"score_tokens: input_len {input_len} outside 1..{S - 1}: a token is scored on the row of the one before it")
    if not 0 <= top_n <= _lib.SD_SCORE_MAX_TOP:
        raise ValueError(f"score_tokens: top_n {top_n} outside 0..{_lib.SD_SCORE_MAX_TOP}")
    m = as_specdec_model(target_model)
    check_token_ids(output, m.cfg.vocab_size)
    if getattr(m, "tp_group", None) is not None:
        raise ValueError("score_tokens is not available with a tensor-parallel target model")
    if m.cfg.is_encoder_decoder:
        raise NotImplementedError("encoder-decoder scoring (reference evaluation.py:126-132) is out of scope")
    dev, n = m.device, S - input_len
    ses = m.new_session(S - 1)
    ids = output[0].to(device=dev, dtype=torch.int32).contiguous()
    logprobs = torch.empty((1, n), dtype=torch.float32, device=dev)
    ranks = torch.empty((1, n), dtype=torch.int32, device=dev)
    top_ids = torch.empty((n, top_n), dtype=torch.int32, device=dev)
    top_logprobs = torch.empty((n, top_n), dtype=torch.float32, device=dev)
    out = _lib.SdScoreOut(logprobs.data_ptr(), ranks.data_ptr(), top_ids.data_ptr() if top_n else None,
                          top_logprobs.data_ptr() if top_n else None)
    _lib.check(_lib.lib.sd_score_sequence(ses.handle, ids.data_ptr(), S, input_len, top_n, ses.logits.data_ptr(), ses.logits.stride(0),
                                          ses.logits.shape[0], C.byref(out), _stream()), "sd_score_sequence")
    ses.cache_len = S - 1
    torch.cuda.current_stream().synchronize()
    return TokenScores(*(t.to(output.device) for t in (logprobs, ranks, top_ids, top_logprobs)))


def get_score_native(output: torch.Tensor, target_model, input_len: int) -> torch.Tensor:
    """``get_score`` by the native scoring pass: no S x V logit tensor and no library kernels on the way."""
    return score_tokens(output, target_model, input_len).logprobs.mean()


_ROW_DTYPES = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def score_rows_torch(logits: torch.Tensor, tokens: torch.Tensor, top_n: int, dt: int = 0):
    """The definition of sd_score_rows in torch, on CPU tensors: ``logits`` (R, V) fp32 rows, rounded to bf16 (dt 1) or fp16
    (dt 2) first as the kernel's mode does, ``tokens`` (R,) -> (logprob (R,) float32, rank (R,) int32, top_ids (R, top_n) int32,
    top_logprobs (R, top_n) float32).  float64 serves the log-sum only; the order is torch's stable descending sort."""
    x = logits.to(_ROW_DTYPES[dt]).to(torch.float32)
    R, V = x.shape
    tok = tokens.to(torch.int64)
    lse = torch.logsumexp(x.double(), dim=-1)
    void = ~torch.isfinite(lse)                                   # a NaN or +inf entry, or nothing but -inf
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices
    scored = (tok >= 0) & (tok < V) & ~void
    at = tok.clamp(0, V - 1)
    nan = float("nan")
    logprob = torch.where(scored, x.double().gather(-1, at[:, None])[:, 0] - lse, torch.full_like(lse, nan))
    place = (order == at[:, None]).to(torch.int32).argmax(dim=-1) + 1
    rank = torch.where(scored, place, torch.zeros_like(place))
    k = min(top_n, V)
    top_ids = torch.full((R, top_n), -1, dtype=torch.int64)
    top_lp = torch.full((R, top_n), nan, dtype=torch.float64)
    top_ids[:, :k] = order[:, :k]
    top_lp[:, :k] = x.double().gather(-1, order[:, :k]) - lse[:, None]
    top_ids[void] = -1
    top_lp[void] = nan
    return logprob.to(torch.float32), rank.to(torch.int32), top_ids.to(torch.int32), top_lp.to(torch.float32)
