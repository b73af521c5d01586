"""Host-side steps the decode-loop wrappers share (speculative_sampling, batch, multi, autoregressive_sampling): each
piece of reference semantics - the EOS rule, the reseed quirk, how the acceptance ratio is rounded - is written once."""
from __future__ import annotations

import ctypes as C
import math
from contextlib import contextmanager
from dataclasses import dataclass
from time import process_time_ns

import numpy as np
import torch

from .._lib import (LOGPROB_SLICE, LOGPROB_STREAMS, SD_EDIT_MAX_BIAS, SdAcceptResult, SdBatchStream, SdHeadScratch, SdLockstepLog,
                    SdLogitEdit, SdLogitEditBlock, SdLogprobBlock, SdLoopOpts, SdPenalty, SdPenaltyBlock, SdRowSampling, SdSampling,
                    SdSeqState, SdSpecScratch, SdSpecStream, lib)
from ..engine import batch_prefill
from ..noise import DeviceNoise, HostTorchNoise
from .grammar import (GRAMMAR_NEEDS_NATIVE, GrammarBinding, check_grammar_vocab, grammar_list, grammar_needs_target_rows)
from .kvcache_model import KVCacheModel


def make_noise(rng, device):
    if rng is None or rng == "host":
        return HostTorchNoise(device)
    if rng == "device":
        return DeviceNoise(seed=int(torch.initial_seed()))
    return rng


def cut_after_new_eos(tokens: list, eos_token_id, ori_eos_cnt: int) -> list:
    """EOS rule over the whole sequence (reference speculative_sampling.py:2033-2041): the prefix up to and including EOS
    number ``ori_eos_cnt + 1``; ``tokens`` itself (the same object) when no new EOS was produced."""
    seen = 0
    for idx, x in enumerate(tokens):
        if x == eos_token_id:
            seen += 1
            if seen == ori_eos_cnt + 1:
                return tokens[:idx + 1]
    return tokens


def reseed_uniforms(random_seed, n: int, device):
    """reseed-before-every-r quirk (:1976-1977): all r of a call are one and the same draw, whatever was accepted."""
    if not random_seed:
        return None
    g = torch.Generator().manual_seed(int(random_seed))
    return torch.rand(1, generator=g).repeat(n).to(device)


def accept_rates_f64(p_at, q_at) -> list:
    """min(1, p / q) as the python double ratio of two float32 values, like the reference's .item() division (:1966-1971)."""
    return np.minimum(1.0, np.asarray(p_at).astype(np.float64) / np.asarray(q_at).astype(np.float64)).tolist()


def accept_rates_f32_zero_q(p_at, q_at) -> list:
    """The width-w loop's form (:1597): fp32 division as p[...] / q[...], clamped to 1, and 0 where q is 0."""
    qa = np.asarray(q_at, dtype=np.float32).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.asarray(p_at, dtype=np.float32).ravel() / qa
    return [0 if q == 0 else (1 if a > 1 else a) for a, q in zip(ratio.tolist(), qa.tolist())]


def open_stream(model, prompt_row, cap: int, seq_len: int, temperature, top_k, top_p, noise=None):
    """One decode stream's device state: a KVCacheModel with arenas for ``cap`` positions and, when ``seq_len`` is not 0,
    an int32 token buffer of that length that starts with the prompt (else None)."""
    kv = KVCacheModel(model, temperature, top_k, top_p, max_seq=cap, noise=noise, full_history=False)
    kv._ensure(cap)
    if not seq_len:
        return kv, None
    dev = kv._model.device
    seq32 = torch.zeros(seq_len, dtype=torch.int32, device=dev)
    seq32[:len(prompt_row)] = prompt_row.to(device=dev, dtype=torch.int32)
    return kv, seq32


def open_spec_slot(draft_m, target_m, prompt_row, cap: int, gamma: int, temperature, top_k, top_p):
    """The device state of one lock-step speculative stream (or of one slot of the prompt queue): the two KVCacheModels with
    arenas for ``cap`` positions, the int32 token buffer (``cap + 1`` entries, starting with ``prompt_row``) and the
    3 * gamma + 1 error words."""
    draft, _ = open_stream(draft_m, None, cap, 0, temperature, top_k, top_p)
    target, seq32 = open_stream(target_m, prompt_row, cap, cap + 1, temperature, top_k, top_p)
    err = torch.zeros(3 * gamma + 1, dtype=torch.int32, device=target_m.device)
    return draft, target, seq32, err


def spec_stream(draft, target, seq32, err, res_dev: int, res_host: int, q_hist=None) -> SdSpecStream:
    """The device side of one speculative stream: sessions, token buffer, probability arenas, error words, result blocks.
    ``draft`` None (prompt lookup): no draft session, and ``q_hist`` is the arena of the one-hot q rows."""
    q_rows = draft._probs if draft is not None else q_hist
    return SdSpecStream(draft._session.handle if draft is not None else None, target._session.handle, seq32.data_ptr(),
                        q_rows.data_ptr(), target._probs.data_ptr(), err.data_ptr(), res_dev, res_host)


def bind_spec_slot(item, draft, target, seq32, err, res_dev: int, res_host: int, q_hist=None) -> None:
    """The device side of an SdBatchStream: its leading fields are an SdSpecStream's."""
    dev = spec_stream(draft, target, seq32, err, res_dev, res_host, q_hist)
    for name, _ in SdSpecStream._fields_:
        setattr(item, name, getattr(dev, name))


def sampling_block(temperature, top_k, top_p, V: int, ld: int, eos_token_id) -> SdSampling:
    """What a native loop samples with and stops on; ``None`` / 0 switch a filter off, no EOS is -1."""
    return SdSampling(float(temperature), int(top_k or 0), float(top_p or 0.0), int(V), int(ld),
                      -1 if eos_token_id is None else int(eos_token_id))


def _per_request(x) -> bool:
    return isinstance(x, (list, tuple)) or (isinstance(x, (np.ndarray, torch.Tensor)) and x.ndim > 0)


def row_sampling(n: int, what: str, temperature, top_k, top_p):
    """Per-request ``temperature`` / ``top_k`` / ``top_p`` of the lock-step loops: each a scalar (broadcast) or a sequence with
    one entry per ``what`` ("prompt", "stream"), ``n`` of them.  Returns ``None`` when all three are scalars - the call then
    is the scalar call as before, unchecked as before - else the ``n`` (temperature, top_k, top_p) triples; raises
    ValueError naming the parameter for a sequence of another length, a temperature of 0, a negative or non-integer top_k.
    Touches no model and no GPU."""
    given = {"temperature": temperature, "top_k": top_k, "top_p": top_p}
    if not any(_per_request(v) for v in given.values()):
        return None
    cols = {}
    for name, v in given.items():
        if not _per_request(v):
            cols[name] = [v] * n
            continue
        if len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} {what}s")
        cols[name] = [x.item() if isinstance(x, (np.generic, torch.Tensor)) else x for x in v]
    triples = []
    for i, (t, k, p) in enumerate(zip(cols["temperature"], cols["top_k"], cols["top_p"])):
        if isinstance(t, bool) or not isinstance(t, (int, float)) or float(t) == 0.0:
            raise ValueError(f"temperature: {what} {i}: a non-zero number is required, not {t!r}")
        k = 0 if k is None else k
        if isinstance(k, bool) or not isinstance(k, (int, float)) or k != int(k) or k < 0:
            raise ValueError(f"top_k: {what} {i}: an integer >= 0 is required, not {k!r}")
        if p is not None and (isinstance(p, bool) or not isinstance(p, (int, float))):
            raise ValueError(f"top_p: {what} {i}: a number is required, not {p!r}")
        triples.append((float(t), int(k), float(p or 0.0)))
    return triples


def row_sampling_array(triples):
    """The SdRowSampling array of row_sampling's triples (``None`` stays ``None``: a NULL ``row_params``)."""
    return None if triples is None else (SdRowSampling * len(triples))(*[SdRowSampling(*t) for t in triples])


def loop_opts(triples=None, lp=None, pb=None, eb=None):
    """The SdLoopOpts of one native loop call, from row_sampling's triples, a LogprobBlock, a PenaltyBlock and a LogitEditBlock,
    each of which may be ``None``: a NULL member.  All four ``None`` -> ``None``, the NULL block, so that a call with neutral
    keywords is the call that was made before the keywords existed.  The struct keeps the row_sampling_array alive; the three
    blocks stay with the caller."""
    if triples is None and lp is None and pb is None and eb is None:
        return None
    ptr = lambda b: C.pointer(b.block) if b is not None else None
    return SdLoopOpts(row_sampling_array(triples), ptr(lp), ptr(pb), ptr(eb))


def head_scratch(session) -> SdHeadScratch:
    """One model's logit rows (its session's) and the mode its rows are normalised in."""
    return SdHeadScratch(session.logits.data_ptr(), session.logits.stride(0), session.model.norm_mode)


def spec_scratch(draft_ses, target_ses, norm_ws, per_pass: int) -> SdSpecScratch:
    """The two heads' scratch, the norm workspace (a tensor or None) and the rows a target pass may carry."""
    return SdSpecScratch(head_scratch(draft_ses), head_scratch(target_ses), norm_ws.data_ptr() if norm_ws is not None else None,
                         int(per_pass))


class LockstepLog:
    """The per-iteration verify log of a lock-step loop: the host arrays and the SdLockstepLog that points at them."""

    def __init__(self, n_log: int):
        self.ms = np.zeros(n_log, dtype=np.float32)
        self.n = np.zeros(n_log, dtype=np.int32)
        self.ctx = np.zeros(n_log, dtype=np.float32)
        self.block = SdLockstepLog(self.ms.ctypes.data, self.n.ctypes.data, self.ctx.ctypes.data, n_log)

    def entries(self) -> list:
        """(milliseconds, streams, mean context) of every logged iteration."""
        return [(float(self.ms[i]), int(self.n[i]), float(self.ctx[i])) for i in range(min(self.block.n_iters, len(self.ms)))]


def lockstep_result(log: "LoopLog", n_tokens: int, calls: int, eos_token_id, ori_eos: int, device):
    """What a lock-step loop returns for one stream: the (1, len) int64 tokens, cut after the first new EOS, and the
    reference's ``details`` dict (no phase times: the streams share their passes)."""
    out = cut_after_new_eos(log.tokens(n_tokens), eos_token_id, ori_eos)
    rate = accept_rates_f64(*log.ratios(calls))
    det = details_dict(0, 0, 0, log.acc_len(calls), float(np.mean(rate)) if rate else 0.0, calls, calls,
                       target_model_time=0, target_pre_cache_time=0, target_post_prob_time=0)
    return torch.tensor([out], dtype=torch.int64, device=device), det


class LoopLog:
    """The host arrays one native loop call (or one stream of it) writes: the token buffer, the accepted length per
    iteration, ``per_iter`` logged p / q values per iteration and, when ``timed``, the two phases' milliseconds."""

    def __init__(self, tokens, seq_cap: int, max_iters: int, per_iter: int, q_fill: float, timed: bool = False):
        self.host_seq = np.zeros(seq_cap, dtype=np.int32)
        self.host_seq[:len(tokens)] = tokens
        self.per_iter = per_iter
        self.acc = np.zeros(max_iters, dtype=np.int32)
        self.p_at = np.zeros(max_iters * per_iter, dtype=np.float32)
        self.q_at = np.full(max_iters * per_iter, q_fill, dtype=np.float32)   # what a slot no iteration wrote divides by
        self.draft_ms = np.zeros(max_iters, dtype=np.float32) if timed else None
        self.target_ms = np.zeros(max_iters, dtype=np.float32) if timed else None

    def ptrs(self) -> tuple:
        """(acc_len, p_at, q_at, draft_ms, target_ms) as the native calls take them; the last two None when not timed."""
        ms = (self.draft_ms, self.target_ms)
        return tuple(a.ctypes.data if a is not None else None for a in (self.acc, self.p_at, self.q_at) + ms)

    def seq_state(self, n_tokens: int, T: int, ori_eos_cnt: int, cache_len: tuple, noise, max_iters: int) -> SdSeqState:
        """The in/out state of the one sequence this log belongs to: ``n_tokens`` of ``T`` so far, the (draft, target) cache
        lengths, the Philox position of ``noise``; the log pointers are this object's arrays."""
        st = SdSeqState(host_seq=self.host_seq.ctypes.data, len=n_tokens, T=T, ori_eos_cnt=ori_eos_cnt, draft_len=cache_len[0],
                        target_len=cache_len[1], seed=noise.seed, draw=noise.draw, max_iters=max_iters)
        st.acc_len_out, st.p_at_out, st.q_at_out, st.draft_ms_out, st.target_ms_out = self.ptrs()
        return st

    def tokens(self, n: int) -> list:
        return self.host_seq[:n].tolist()

    def acc_len(self, calls: int) -> list:
        return self.acc[:calls].tolist()

    def ratios(self, calls: int) -> tuple:
        return self.p_at[:calls * self.per_iter], self.q_at[:calls * self.per_iter]

    def phase_ns(self, calls: int) -> tuple:
        """(draft, target) device time: every entry truncated to whole nanoseconds, then summed; zeros when not timed."""
        if self.draft_ms is None:
            return 0, 0
        return tuple(int(sum(int(v * 1e6) for v in ms[:calls])) for ms in (self.draft_ms, self.target_ms))


def device_rng(rng) -> bool:
    """Whether ``rng`` selects the native device-RNG loops: "device", or a noise object that draws on the device."""
    return rng == "device" if isinstance(rng, str) else bool(getattr(rng, "on_device", False))


def logprobs_need_target_rows(target_m) -> None:
    """``logprobs=True`` reads the target's logit rows where a single-GPU forward leaves them: a tensor-parallel shard is refused."""
    if getattr(target_m, "tp_group", None) is not None:
        raise ValueError("logprobs=True is not available with a tensor-parallel target model")


class LogprobBlock:
    """The SdLogprobBlock of one native loop call: the device and pinned-host float slices (16 streams x 17 floats) and one host
    array per stream (per prompt in the queue) with the capacity of its token buffer, entry j = the target log-probability of
    the j-th token the call emitted for it."""

    def __init__(self, device, caps):
        n = LOGPROB_SLICE * LOGPROB_STREAMS
        self.dev = torch.zeros(n, dtype=torch.float32, device=device)
        self.host = torch.zeros(n, dtype=torch.float32).pin_memory()
        self.out = [np.zeros(max(1, int(c)), dtype=np.float32) for c in caps]
        self._ptrs = (C.c_void_p * len(self.out))(*[a.ctypes.data for a in self.out])
        self.block = SdLogprobBlock(self.dev.data_ptr(), self.host.data_ptr(), self._ptrs)

    def tensor(self, i: int, n: int, device) -> torch.Tensor:
        """The (1, n) float32 scores of stream i's first n new tokens (n: the output's length minus the prompt's)."""
        return torch.from_numpy(self.out[i][:max(0, n)].copy()).unsqueeze(0).to(device)


def penalty_triples(n: int, what: str, repetition_penalty, frequency_penalty, presence_penalty):
    """Per-request ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` of the native loops: each one value
    (broadcast) or a sequence with one entry per ``what`` ("prompt", "stream"), ``n`` of them.  Returns ``None`` for the three
    neutral scalars (1, 0, 0) - the call is then the call it was before - else the ``n`` (repetition, frequency,
    presence) triples; raises ValueError naming the parameter for a sequence of another length, a value that is not a finite
    number, a repetition penalty <= 0.  Touches no model and no GPU."""
    given = {"repetition_penalty": repetition_penalty, "frequency_penalty": frequency_penalty, "presence_penalty": presence_penalty}
    if not any(_per_request(v) for v in given.values()) and (repetition_penalty, frequency_penalty, presence_penalty) == (1.0, 0.0, 0.0) \
            and not any(isinstance(v, bool) for v in given.values()):
        return None
    cols = {}
    for name, v in given.items():
        if not _per_request(v):
            v = [v] * n
        elif len(v) != n:
            raise ValueError(f"{name}: {len(v)} entries for {n} {what}s")
        cols[name] = [x.item() if isinstance(x, (np.generic, torch.Tensor)) else x for x in v]
        for i, x in enumerate(cols[name]):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError(f"{name}: {what} {i}: a finite number is required, not {x!r}")
            if name == "repetition_penalty" and x <= 0:
                raise ValueError(f"repetition_penalty: {what} {i}: a value > 0 is required, not {x!r}")
    return [(float(r), float(f), float(p)) for r, f, p in zip(*cols.values())]


def penalties_need_target_rows(target_m) -> None:
    """Penalties edit the logit rows where a single-GPU forward leaves them: a tensor-parallel shard is refused."""
    if getattr(target_m, "tp_group", None) is not None:
        raise ValueError("repetition / frequency / presence penalties are not available with a tensor-parallel target model")


class PenaltyBlock:
    """The SdPenaltyBlock of one native loop call: the triples (one per stream, per prompt in the queue) and the device slab
    the edited logit rows of a pass go to - ``max_rows`` rows of V floats, 16-byte aligned with a stride that is a multiple
    of 4, so the norm launch keeps its two-kernel path."""

    def __init__(self, device, triples, V: int, max_rows: int):
        ld = (int(V) + 3) // 4 * 4
        self.rows = torch.empty((max(1, int(max_rows)), ld), dtype=torch.float32, device=device)
        self._params = (SdPenalty * len(triples))(*[SdPenalty(*t) for t in triples])
        self.block = SdPenaltyBlock(self.rows.data_ptr(), ld, self.rows.shape[0], self._params)


def _int_id(x):
    """A token id as a python int, or None for anything that is not an integer (bool included)."""
    if isinstance(x, torch.Tensor) and x.ndim == 0:
        x = x.item()
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        return None
    return int(x)


def _id_lists(n: int, what: str, name: str, v):
    """``allowed_token_ids`` / ``banned_token_ids``: None, a flat sequence of ids for every request, or a sequence with one
    sequence-or-None per request -> n lists-or-None."""
    if v is None:
        return [None] * n
    if isinstance(v, (np.ndarray, torch.Tensor)):
        v = v.tolist()
    if not isinstance(v, (list, tuple)):
        raise ValueError(f"{name}: a sequence of token ids, or one sequence (or None) per {what}, is required, not {v!r}")
    nested = lambda x: x is None or _per_request(x)
    try:                                                          # (a long flat list is recognised as one array, not entry by entry)
        arr = np.asarray(v)
        flat = arr.ndim == 1 and arr.dtype != object
    except ValueError:
        flat = False
    if flat and arr.dtype.kind in "iu":
        return [arr] * n                                          # (parsed: ids_of takes it as it is)
    if flat or not any(nested(x) for x in v):
        return [list(v)] * n
    if len(v) != n:
        raise ValueError(f"{name}: {len(v)} entries for {n} {what}s")
    out = []
    for i, x in enumerate(v):
        if not nested(x):
            raise ValueError(f"{name}: {what} {i}: a sequence of token ids or None is required, not {x!r}")
        out.append(None if x is None else list(x.tolist() if isinstance(x, (np.ndarray, torch.Tensor)) else x))
    return out


def allowed_mask_words(V: int, allowed=None, banned=()):
    """The sd_logit_edit mask of one request: (V + 31) // 32 uint32 words, bit ``t & 31`` of word ``t >> 5`` set = token t
    allowed.  ``allowed`` None means every id of [0, V); ``banned`` ids are cleared bits of the same mask; bits of ids >= V
    in the last word are clear."""
    bits = np.zeros(((V + 31) // 32) * 32, dtype=bool)
    if allowed is None:
        bits[:V] = True
    else:
        bits[np.asarray(allowed, dtype=np.int64)] = True
    if len(banned):
        bits[np.asarray(banned, dtype=np.int64)] = False
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def logit_edits(n: int, what: str, V, eos_token_id, logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_tokens=0):
    """Per-request ``logit_bias`` / ``allowed_token_ids`` / ``banned_token_ids`` / ``min_tokens`` of the native loops, ``n``
    requests called ``what`` ("prompt", "stream").  ``logit_bias``: one ``{id: bias}`` mapping for every request or a sequence
    with one mapping-or-None per request; the id lists: one flat sequence for every request or one sequence-or-None per
    request; ``min_tokens``: an int or one per request.  Returns ``None`` when everything is neutral - the call is then the
    call it was before - else one record per request: ``dict(bias_ids=int32 array ascending, bias_vals=float32 array,
    mask=uint32 words or None, min_tokens=int)``.  Raises ValueError naming the parameter and the request for a sequence of
    another length, a bias that is not a finite number, more than 1024 bias entries, an id that is not an integer or lies
    outside [0, V), min_tokens < 0, an allowed set that is empty once the banned ids are removed, or one that holds nothing but
    EOS while min_tokens > 0.  ``V`` None: the vocabulary is not known yet - the upper bound of the ids is not checked and the
    records carry no mask; the wrappers validate this way before they touch a model and finish the same records with
    ``bind_logit_edits`` once V is known, so every list is parsed once.  Touches no GPU."""
    if logit_bias is None or (hasattr(logit_bias, "items") and not isinstance(logit_bias, (list, tuple))):
        biases = [logit_bias] * n
    elif isinstance(logit_bias, (list, tuple)):
        if len(logit_bias) != n:
            raise ValueError(f"logit_bias: {len(logit_bias)} entries for {n} {what}s")
        biases = list(logit_bias)
    else:
        raise ValueError(f"logit_bias: a mapping of token id to bias, or one mapping (or None) per {what}, is required, not {logit_bias!r}")
    allowed, banned = _id_lists(n, what, "allowed_token_ids", allowed_token_ids), _id_lists(n, what, "banned_token_ids", banned_token_ids)
    if _per_request(min_tokens):
        if len(min_tokens) != n:
            raise ValueError(f"min_tokens: {len(min_tokens)} entries for {n} {what}s")
        mins = [x.item() if isinstance(x, (np.generic, torch.Tensor)) else x for x in min_tokens]
    else:
        mins = [min_tokens] * n

    def ids_of(name, i, xs):
        """-> the ids as a sorted array without repeats (a plain integer sequence is checked as one array)"""
        try:
            arr = np.asarray(xs) if len(xs) else np.zeros(0, dtype=np.int64)
        except (OverflowError, ValueError):
            arr = None
        if arr is None or arr.ndim != 1 or arr.dtype.kind not in "iu":
            for x in xs:
                if _int_id(x) is None:
                    raise ValueError(f"{name}: {what} {i}: token ids are integers, not {x!r}")
            arr = np.asarray([_int_id(x) for x in xs], dtype=object)
        bad = [int(t) for t in arr if t < 0 or t >= 2 ** 31] if arr.dtype == object else arr[(arr < 0) | (arr >= 2 ** 31)].tolist()
        if bad:
            raise ValueError(f"{name}: {what} {i}: token id {bad[0]} outside [0, {V if V is not None else 'V'})")
        return np.unique(arr.astype(np.int64))
    def bias_pairs(i, b):
        """-> the mapping's (id, bias) pairs, ascending by id"""
        keys, vals = (list(b.keys()), list(b.values())) if b else ([], [])
        if len(keys) > SD_EDIT_MAX_BIAS:
            raise ValueError(f"logit_bias: {what} {i}: {len(keys)} entries, at most {SD_EDIT_MAX_BIAS}")
        for t in keys:                                            # (one by one: a float key must not pass as its integer value)
            if _int_id(t) is None:
                raise ValueError(f"logit_bias: {what} {i}: token ids are integers, not {t!r}")
        if len(ids_of("logit_bias", i, keys)) != len(keys):
            raise ValueError(f"logit_bias: {what} {i}: a token id is listed twice")
        vals = [x.item() if isinstance(x, (np.generic, torch.Tensor)) else x for x in vals]
        for t, x in zip(keys, vals):
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
                raise ValueError(f"logit_bias: {what} {i}: token {t}: a finite number is required, not {x!r}")
        return sorted(zip((int(t) for t in keys), vals))
    records, neutral, parsed = [], True, {}
    masks = {}                                                    # one mask per pair of list objects: a list for all requests is built once
    for i in range(n):
        b = biases[i]
        if b is not None and not hasattr(b, "items"):
            raise ValueError(f"logit_bias: {what} {i}: a mapping of token id to bias or None is required, not {b!r}")
        if b and id(b) in parsed:                                 # (one mapping for every request is parsed once)
            pairs = parsed[id(b)]
        else:
            pairs = parsed[id(b)] = bias_pairs(i, b)
        m = mins[i]
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 0:
            raise ValueError(f"min_tokens: {what} {i}: an integer >= 0 is required, not {m!r}")
        key = (id(allowed[i]), id(banned[i]))
        if key not in masks:
            a = None if allowed[i] is None else ids_of("allowed_token_ids", i, allowed[i])
            d = ids_of("banned_token_ids", i, banned[i]) if banned[i] is not None else np.zeros(0, dtype=np.int64)
            left = np.setdiff1d(a, d) if a is not None else None   # (None: every id of [0, V) but d's)
            masked = a is not None or len(d) > 0
            masks[key] = (a, d, left, masked)
        a, d, left, masked = masks[key]
        neutral = neutral and not pairs and not masked and int(m) == 0
        records.append(dict(bias_ids=np.asarray([t for t, _ in pairs], dtype=np.int32),
                            bias_vals=np.asarray([float(x) for _, x in pairs], dtype=np.float32),
                            allowed=a, banned=d, left=left, mask=None, masked=masked, min_tokens=int(m)))
    if neutral:
        return None
    _check_left(records, what, None, eos_token_id)
    return records if V is None else bind_logit_edits(records, what, V, eos_token_id)


def _check_left(records, what: str, V, eos_token_id) -> None:
    """What the masks leave: refuses a request with no id left, or with EOS alone while min_tokens > 0.  V None: only the
    requests with an allowed list can be judged (banned ids alone empty nothing before the vocabulary is known)."""
    for i, r in enumerate(records):
        left, d, m = r["left"], r["banned"], r["min_tokens"]
        n_left = len(left) if left is not None else (V - len(d) if V is not None else None)
        if n_left == 0:
            raise ValueError(f"allowed_token_ids: {what} {i}: no token id is left once the banned ids are removed")
        if m > 0 and n_left == 1 and eos_token_id is not None and \
                (int(left[0]) == eos_token_id if left is not None else (0 <= eos_token_id < V and eos_token_id not in d)):
            raise ValueError(f"allowed_token_ids: {what} {i}: only EOS ({eos_token_id}) is allowed while min_tokens is {m}")


def bind_logit_edits(records, what: str, V: int, eos_token_id):
    """The second half of ``logit_edits``, once the vocabulary size is known: the upper bound of every id, what the banned ids
    leave of [0, V), and the mask words - on the arrays the first half parsed (requests that share their lists share the
    mask).  Completes and returns ``records``."""
    masks = {}
    for i, r in enumerate(records):
        for name, ids in (("logit_bias", r["bias_ids"]), ("allowed_token_ids", r["allowed"]), ("banned_token_ids", r["banned"])):
            if ids is not None and len(ids) and int(ids[-1]) >= V:     # (ascending)
                raise ValueError(f"{name}: {what} {i}: token id {int(ids[ids >= V][0])} outside [0, {V})")
    _check_left(records, what, V, eos_token_id)
    for r in records:
        key = (id(r["allowed"]), id(r["banned"]))
        if r["masked"] and key not in masks:
            masks[key] = allowed_mask_words(V, r["allowed"], r["banned"])
        r["mask"] = masks.get(key) if r["masked"] else None
    return records


def neutral_logit_edits(n: int):
    """``n`` records as ``logit_edits`` returns them, all neutral: what a call with a grammar and no edits of its own builds
    its edit block from (the masked rows need the block's slab)."""
    return [dict(bias_ids=np.zeros(0, dtype=np.int32), bias_vals=np.zeros(0, dtype=np.float32), allowed=None,
                 banned=np.zeros(0, dtype=np.int64), left=None, mask=None, masked=False, min_tokens=0) for _ in range(n)]


def edits_need_target_rows(target_m) -> None:
    """Logit edits act on the logit rows where a single-GPU forward leaves them: a tensor-parallel shard is refused."""
    if getattr(target_m, "tp_group", None) is not None:
        raise ValueError("logit_bias / allowed_token_ids / banned_token_ids / min_tokens are not available with a tensor-parallel "
                         "target model")


EDITS_NEED_NATIVE = ('logit_bias / allowed_token_ids / banned_token_ids / min_tokens need the native loop: rng="device" (or a device '
                     'noise object)')


class LogitEditBlock:
    """The SdLogitEditBlock of one native loop call: the records of ``logit_edits`` (one per stream, per prompt in the queue),
    every request's bias ids, bias values and mask words uploaded as ONE concatenated tensor per kind, and the device slab the
    edited logit rows of a pass go to, sized and aligned as PenaltyBlock's (``rows``: that block's slab, shared when a call has
    both - the launch writes the edit block's)."""

    def __init__(self, device, records, V: int, max_rows: int, rows=None):
        ld = (int(V) + 3) // 4 * 4
        self.rows = rows if rows is not None else torch.empty((max(1, int(max_rows)), ld), dtype=torch.float32, device=device)

        def upload(arrays, dtype):
            """-> the device address of every array (None for an absent / empty one) inside one tensor"""
            sizes = [0 if a is None else len(a) for a in arrays]
            if not sum(sizes):
                return None, [None] * len(arrays)
            host = np.concatenate([a for a in arrays if a is not None and len(a)]).astype(dtype)
            dev = torch.from_numpy(host.view(np.int32) if dtype == np.uint32 else host).to(device)
            offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
            return dev, [dev.data_ptr() + 4 * int(o) if k else None for o, k in zip(offs, sizes)]
        self._ids, ids = upload([r["bias_ids"] for r in records], np.int32)
        self._vals, vals = upload([r["bias_vals"] for r in records], np.float32)
        self._masks, masks = upload([r["mask"] for r in records], np.uint32)
        self._params = (SdLogitEdit * len(records))(*[SdLogitEdit(i, v, len(r["bias_ids"]), m, r["min_tokens"])
                                                      for r, i, v, m in zip(records, ids, vals, masks)])
        self.block = SdLogitEditBlock(self.rows.data_ptr(), self.rows.stride(0), self.rows.shape[0], self._params)


PENALTIES_NEED_NATIVE = 'repetition / frequency / presence penalties need the native loop: rng="device" (or a device noise object)'
LOGPROBS_NEED_NATIVE = 'logprobs=True needs the native loop: rng="device" (or a device noise object)'


def slab_rows(gamma: int = 0, streams: int = 1, per_pass: int = 0, *, ar_streams: int = None) -> int:
    """The rows of the slab a call's penalty and edit blocks write a pass's logit rows to: those of the loop's largest pass.  A
    speculative pass holds whole streams of gamma + 1 rows, as many as fit into ``per_pass`` rows, at least one and at most all
    ``streams`` (one stream: gamma + 1 whatever ``per_pass``); an autoregressive step holds one row of each of ``ar_streams``."""
    if ar_streams is not None:
        return int(ar_streams)
    return min(max(per_pass, gamma + 1), streams * (gamma + 1))


class AttachedOptions:
    """What ``RequestOptions.attach`` holds during one native call: the blocks ``lp`` / ``pb`` / ``eb`` (each may be None),
    ``members`` - loop_opts' four arguments; ``loop_opts`` is their SdLoopOpts, None when nothing is set - and
    ``grammar_states``, the sessions' device state caches (None without a grammar)."""

    def __init__(self, triples, lp, pb, eb, bound):
        self.lp, self.pb, self.eb = lp, pb, eb
        self.members = (triples, lp, pb, eb)
        self.grammar_states = bound.states if bound is not None else None

    @property
    def loop_opts(self):
        return loop_opts(*self.members)

    def logprob_tensor(self, i: int, n: int, device) -> torch.Tensor:
        return self.lp.tensor(i, n, device)


class RequestOptions:
    """The per-request options of one native loop call with ``n`` requests called ``what`` ("stream", "prompt"), from the
    keywords to the blocks of its sd_loop_opts, in three stages every wrapper goes through in this order: ``parse`` (no model,
    no GPU), the refusals ``require_native`` / ``require_target_rows`` / ``bind``, and ``attach`` around the native call.
    The fields keep the leaf parsers' results, None for a neutral option: ``sampling`` (row_sampling's triples), ``logprobs``,
    ``penalties`` (penalty_triples), ``edits`` (logit_edits' records), ``grammar`` (grammar_list)."""

    def __init__(self, n: int, what: str, eos_token_id, sampling=None, logprobs=False, penalties=None, edits=None, grammar=None):
        self.n, self.what, self.eos_token_id = n, what, eos_token_id
        self.sampling, self.logprobs, self.penalties, self.edits, self.grammar = sampling, logprobs, penalties, edits, grammar

    @classmethod
    def parse(cls, n: int, what: str, eos_token_id, *, sampling=None, logprobs=False, penalties=(1.0, 0.0, 0.0),
              edits=(None, None, None, 0), grammar=None) -> "RequestOptions":
        """``sampling``: the (temperature, top_k, top_p) of an entry that takes per-request sequences, else None; ``penalties``:
        (repetition, frequency, presence); ``edits``: (logit_bias, allowed_token_ids, banned_token_ids, min_tokens).  Parsed -
        and refused with the leaf parsers' ValueErrors - in the order sampling, penalties, edits, grammar."""
        return cls(n, what, eos_token_id, row_sampling(n, what, *sampling) if sampling is not None else None, logprobs,
                   penalty_triples(n, what, *penalties), logit_edits(n, what, None, eos_token_id, *edits),
                   grammar_list(n, what, grammar))

    def require_native(self, ok: bool, suffix: str) -> None:
        """The single-stream entries: an option that is set needs the native loop (``ok``); ``suffix`` names what else selects it."""
        for given, text in ((self.grammar is not None, GRAMMAR_NEEDS_NATIVE), (self.edits is not None, EDITS_NEED_NATIVE),
                            (self.penalties is not None, PENALTIES_NEED_NATIVE), (self.logprobs, LOGPROBS_NEED_NATIVE)):
            if given and not ok:
                raise ValueError(text + suffix)

    def require_target_rows(self, target_model) -> None:
        """Every option reads or edits the logit rows where a single-GPU forward leaves them: with one set, a tensor-parallel
        target is refused (``target_model`` as the caller passed it: nothing is converted or touched)."""
        for given, refuse in ((self.grammar is not None, grammar_needs_target_rows), (self.edits is not None, edits_need_target_rows),
                              (self.penalties is not None, penalties_need_target_rows), (self.logprobs, logprobs_need_target_rows)):
            if given:
                refuse(target_model)

    def bind(self, V: int) -> None:
        """Once the vocabulary is known: the ids' upper bound and the masks of the edits, the grammars' vocabulary."""
        if self.edits is not None:
            self.edits = bind_logit_edits(self.edits, self.what, V, self.eos_token_id)
        check_grammar_vocab(self.grammar, self.what, V)

    @contextmanager
    def attach(self, device, V: int, rows: int, logprob_caps, grammar_sessions, grammar_state_caps):
        """Builds the blocks of the call - ``rows``: slab_rows(...), which the penalty and the edit block share;
        ``logprob_caps``: the token capacity per request - and sets the grammars on ``grammar_sessions`` (the streams' target
        sessions; in the queue the slots', fewer than requests, which all have the one grammar) with state caches of
        ``grammar_state_caps`` ints.  Yields the AttachedOptions; the grammars come off again on exit, however the body ends."""
        lp = LogprobBlock(device, logprob_caps) if self.logprobs else None
        pb = PenaltyBlock(device, self.penalties, V, rows) if self.penalties is not None else None
        edits = self.edits
        if self.grammar is not None and edits is None:
            edits = neutral_logit_edits(self.n)                   # the masked rows need the edit block's slab
        eb = LogitEditBlock(device, edits, V, rows, pb.rows if pb is not None else None) if edits is not None else None
        bound = GrammarBinding(grammar_sessions, self.grammar[:len(grammar_sessions)], grammar_state_caps, device) \
            if self.grammar is not None else None
        try:
            yield AttachedOptions(self.sampling, lp, pb, eb, bound)
        finally:
            if bound is not None:
                bound.detach()


def stream_seeds(seeds, n: int) -> list:
    """The Philox seeds of ``n`` streams: ``seeds``, or ``torch.initial_seed() + i`` for stream i."""
    return list(seeds) if seeds is not None else [int(torch.initial_seed()) + i for i in range(n)]


@dataclass
class LockstepStream:
    draft: KVCacheModel          # None without a draft model
    target: KVCacheModel
    seq32: torch.Tensor
    err: torch.Tensor
    q_hist: torch.Tensor         # without a draft model: the arena of the one-hot q rows; else None (the draft's _probs)
    noise: DeviceNoise
    log: LoopLog
    prompt_len: int
    T: int
    ori_eos: int
    device: object               # the prompt's: where the output goes


class LockstepStreams:
    """The stream table of one lock-step speculative call (sd_spec_batch_generate, sd_lookup_batch_generate): a stream per
    prompt with its LoopLog, ``noises[i]`` and what the caller's ``open_slot(i, prompt_row, cap)`` opens for it - ``(draft,
    target, seq32, err, q_hist)`` with arenas for ``cap`` positions and 3 * gamma + 1 error words; prompt lookup has no draft
    model: ``draft`` None and an fp32 ``q_hist`` arena of the stream's own - everything but the last prompt token prefilled, and
    the SdBatchStream array ``arr`` bound to it.  ``info_bytes``: bytes per stream behind the B result blocks (stream i's
    block is at ``i * sizeof(SdAcceptResult)`` either way)."""

    def __init__(self, prefixes, open_slot, device, eos_token_id, max_len, gamma: int, noises, info_bytes: int = 0):
        B, res_sz = len(prefixes), C.sizeof(SdAcceptResult)
        self.res_dev = torch.zeros(B * (res_sz + info_bytes), dtype=torch.uint8, device=device)
        self.res_host = torch.zeros(B * (res_sz + info_bytes), dtype=torch.uint8).pin_memory()
        self.max_iters = max(1, int(max_len)) + 1
        self.streams = []
        for i, (pf, noise) in enumerate(zip(prefixes, noises)):
            assert pf.shape[0] == 1, "input batch size must be 1"
            L = pf.shape[1]
            T = L + max_len
            cap = T + gamma + 2
            host = [int(t) for t in pf[0].tolist()]
            self.streams.append(LockstepStream(*open_slot(i, pf[0], cap), noise, LoopLog(host, cap, self.max_iters, gamma, q_fill=1.0),
                                               L, T, host.count(eos_token_id), pf.device))
        drafted = self.streams[0].draft is not None
        # prefill everything but the last prompt token, the B prompts packed into passes of up to 256 rows (engine.batch_prefill:
        # one pass over the weights serves several streams); the decode loop then starts with 1 new draft row and gamma+1 new
        # target rows per stream like every later iteration
        for side in ("draft", "target") if drafted else ("target",):
            batch_prefill([getattr(s, side)._session for s in self.streams], [s.seq32 for s in self.streams],
                          [s.prompt_len - 1 for s in self.streams])
        self.arr = (SdBatchStream * B)()
        for i, (it, s) in enumerate(zip(self.arr, self.streams)):
            bind_spec_slot(it, s.draft, s.target, s.seq32, s.err, self.res_dev.data_ptr() + i * res_sz,
                           self.res_host.data_ptr() + i * res_sz, s.q_hist)
            it.host_seq = s.log.host_seq.ctypes.data
            it.len, it.T, it.ori_eos_cnt = s.prompt_len, s.T, s.ori_eos
            it.draft_len, it.target_len = s.prompt_len - 1 if drafted else 0, s.prompt_len - 1
            it.seed, it.draw = s.noise.seed, s.noise.draw
            it.acc_len_out, it.p_at_out, it.q_at_out = s.log.ptrs()[:3]
        self.per_pass = self.streams[0].target._session.max_pass_rows
        self.norm_ws = torch.empty(lib.sd_norm_workspace_bytes(self.per_pass), dtype=torch.uint8, device=device)
        self.vlog = LockstepLog(self.max_iters * 2)

    def results(self, eos_token_id) -> tuple:
        """After the loop: RuntimeError("s") for a logged error; else every stream's Philox position and cache lengths go back
        to its noise object and sessions, and the outputs and ``details`` dicts are returned (lockstep_result)."""
        if self.vlog.block.err:
            raise RuntimeError("s")
        outs, ds = [], []
        for it, s in zip(self.arr, self.streams):
            s.noise.seed, s.noise.draw = it.seed, it.draw
            if s.draft is not None:
                s.draft._session.cache_len = it.draft_len
            s.target._session.cache_len = it.target_len
            out, det = lockstep_result(s.log, it.len, it.calls, eos_token_id, s.ori_eos, s.device)
            outs.append(out)
            ds.append(det)
        return outs, ds


def single_stream_native_call(call, host_seq: list, T: int, gamma: int, eos_token_id, noise, device, timed: bool, info_bytes: int = 0):
    """One call of a single-stream native loop (sd_spec_generate, sd_lookup_generate): allocates the result pair (``info_bytes``
    more behind the block) and the 3 * gamma + 1 error words, builds the LoopLog and its SdSeqState, and runs the caller's
    ``call(res_dev, res_host, err_words, st)``, which makes the native call in its own module.  Returns ``(out_tokens, st, log,
    acc_len, acc_rate, (approx_time, target_time, other_time))``: the tokens cut after the first new EOS, the statistics, the
    two phases' device time (the reference's are host process_time deltas around generate() (:1937-1962); here the host only
    enqueues, so HIP events are reported) and the host CPU time.  The noise position is written back; any exception leaves as
    RuntimeError("s") (:2044-2046), the cause attached and printed."""
    seq_len0 = len(host_seq)
    ori_eos_cnt = host_seq.count(eos_token_id)
    nb = C.sizeof(SdAcceptResult) + info_bytes
    res_dev = torch.zeros(nb, dtype=torch.uint8, device=device)
    res_host = torch.zeros(nb, dtype=torch.uint8).pin_memory()
    err_words = torch.zeros(3 * gamma + 1, dtype=torch.int32, device=device)
    max_iters = max(1, T - seq_len0)
    log = LoopLog(host_seq, T + gamma + 2, max_iters, gamma, q_fill=1.0, timed=timed)
    st = log.seq_state(seq_len0, T, ori_eos_cnt, (0, 0), noise, max_iters)
    try:
        tick = process_time_ns()
        call(res_dev, res_host, err_words, st)
        other_time = process_time_ns() - tick            # host CPU time of the loop (enqueue + waits + bookkeeping)
        noise.seed, noise.draw = st.seed, st.draw
        raise_loop_error(st.err)
        acc_len = log.acc_len(st.n_iters)
        acc_rate = accept_rates_f64(*log.ratios(st.n_iters))
        times = (*log.phase_ns(st.n_iters), other_time)
        out_tokens = cut_after_new_eos(log.tokens(st.len), eos_token_id, ori_eos_cnt)
    except Exception as e:
        print(e)
        raise RuntimeError("s") from e
    return out_tokens, st, log, acc_len, acc_rate, times


def raise_loop_error(code: int) -> None:
    """The ``err`` a native loop leaves in its log / state block as the reference's exceptions (utils.py:224, :207)."""
    if code == 1:
        raise RuntimeError("prob error")
    if code == 2:
        raise RuntimeError("norm logits error")


def details_dict(approx_time, target_time, other_time, acc_len, acc_rate, target_calls, approx_calls, **more) -> dict:
    """The reference's ``details`` keys in its order; ``more``: the three target_* times of speculative_sampling."""
    return {"approx_time": approx_time, "target_time": target_time, "other_time": other_time, "acc_len": acc_len,
            "acc_rate": acc_rate, "target_call_times": target_calls, "approx_call_times": approx_calls, **more}
