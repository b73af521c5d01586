"""Stream-batched speculative sampling ("throughput mode"): B independent prompt streams
decode in lockstep on one GPU and share every pass over the weights.  Each draft step is one forward over the B (or up
to 2B) new rows, each verify is one target forward over B*(gamma+1) rows: the bytes streamed per iteration are those of
ONE stream, the tokens produced are B times as many.

Every stream keeps its own KV arenas, probability arenas, token buffer and Philox stream, and runs exactly the
per-stream algorithm of reference sampling/speculative_sampling.py:1876-2076 (batch size 1 there, :1905): with the
same seeds the outputs equal those of B separate ``speculative_sampling(..., rng=DeviceNoise(seed))`` calls.

``speculative_sampling_queue`` puts a prompt queue behind the same loop (continuous batching): any number of prompts share
up to 16 slots, and a stream that ends hands its slot to the next waiting prompt.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from .._lib import lib, check, SdAcceptResult, SdBatchStream, SdQueuePrompt
from ..engine import as_specdec_model, _stream, check_token_ids, same_device, batch_prefill
from ..noise import DeviceNoise
from ._loop_common import (LockstepLog, LockstepStreams, LoopLog, RequestOptions, bind_spec_slot, lockstep_result, open_spec_slot,
                           open_stream, reseed_uniforms, sampling_block, slab_rows, spec_scratch, stream_seeds)
from .grammar import TokenGrammar
from .autoregressive_sampling import ArRun


class _Ms:                                                        # (bench.py reads e0.elapsed_time(e1))
    def __init__(self, ms):
        self.ms = ms

    def elapsed_time(self, _other):
        return self.ms


@torch.no_grad()
def speculative_sampling_batch(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id,
                               pad_token_id, max_len: int, gamma: int = 4, temperature: float = 1, top_k: int = 0,
                               top_p: float = 0, random_seed: int = None, details: bool = False,
                               seeds: Optional[Sequence[int]] = None, _timing: Optional[dict] = None, *,
                               logprobs: bool = False, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0,
                               logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_tokens=0, grammar=None):
    """B streams at once; ``prefixes[i]`` is (1, L_i) int64.  Returns a list of (1, len_i) tensors (and a list of
    ``details`` dicts with the reference's keys when ``details``).  Device Philox RNG, stream i seeded ``seeds[i]``.
    ``temperature``, ``top_k`` and ``top_p`` each take one value for all streams or a sequence with one entry per stream
    (``T_i``, ``k_i``, ``p_i``; a scalar beside a sequence is broadcast): stream i equals ``speculative_sampling(prefixes[i],
    ..., temperature=T_i, top_k=k_i, top_p=p_i, rng=DeviceNoise(seeds[i]))``.  A sequence of another length, a temperature
    entry of 0 or a negative / non-integer top_k entry raises ValueError before a model is touched.  With three scalars the
    call is sd_spec_batch_generate's as before; any sequence is the ``row_params`` of its sd_loop_opts.
    ``logprobs``: the return value gains one last element, a list of float32 (1, len_i - L_i) tensors with the TARGET
    model's log-probability of every new token of stream i, as ``speculative_sampling(logprobs=True)`` defines it: the
    log-softmax of the raw target logits, before temperature, top_k and top_p - what the model says, not what the sampler
    drew from - cut where the tokens are cut (member ``logprobs`` of sd_loop_opts).
    ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` (neutral 1 / 0 / 0): each one value for all streams
    or one per stream, broadcast like ``temperature``; stream i equals ``speculative_sampling(prefixes[i], ...,
    repetition_penalty=r_i, frequency_penalty=f_i, presence_penalty=p_i, rng=DeviceNoise(seeds[i]))``
    (member ``penalties``; ``sampling.utils.apply_penalties`` has the definition).  A sequence of another length, a
    value that is not finite or a repetition penalty <= 0 raises ValueError before a model is touched.
    ``logit_bias`` (one ``{token id: bias}`` mapping for all streams, or a sequence with one mapping-or-None per stream),
    ``allowed_token_ids`` / ``banned_token_ids`` (one flat sequence of ids for all streams, or one sequence-or-None per stream)
    and ``min_tokens`` (an int, or one per stream): stream i equals ``speculative_sampling`` with its values
    (member ``edits``; ``sampling.utils.apply_logit_edits`` has the definition, ``speculative_sampling`` the
    refusals).
    ``grammar``: one ``sampling.grammar.TokenGrammar`` for all streams, or a sequence with one TokenGrammar-or-None per stream;
    stream i equals ``speculative_sampling(prefixes[i], ..., grammar=g_i, rng=DeviceNoise(seeds[i]))``.  Streams that share a
    grammar share its device tables; each has its own state cache (``_timing["grammar_states"]``: the device arrays, None for a
    stream without a grammar)."""
    try:
        opts = RequestOptions.parse(len(prefixes), "stream", eos_token_id, sampling=(temperature, top_k, top_p), logprobs=logprobs,
                                    penalties=(repetition_penalty, frequency_penalty, presence_penalty),
                                    edits=(logit_bias, allowed_token_ids, banned_token_ids, min_tokens), grammar=grammar)
    except TypeError:
        raise ValueError("prefixes: a sequence of (1, L) int64 prompts is required") from None
    opts.require_target_rows(target_model)
    draft_m, target_m = as_specdec_model(approx_model), as_specdec_model(target_model)
    same_device(draft_m, target_m)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    assert draft_m.cfg.vocab_size == V
    opts.bind(V)
    for pf in prefixes:
        check_token_ids(pf, V)
    B = len(prefixes)
    assert 1 <= B <= 16 and 1 <= gamma <= 16
    triples = opts.sampling or [(temperature, top_k, top_p)] * B
    r_const = reseed_uniforms(random_seed, gamma, dev)
    table = LockstepStreams(prefixes, lambda i, row, cap: (*open_spec_slot(draft_m, target_m, row, cap, gamma, *triples[i]), None),
                            dev, eos_token_id, max_len, gamma, [DeviceNoise(seed) for seed in stream_seeds(seeds, B)])
    streams = table.streams

    # the lock-step loop itself runs inside libspecdec (sd_spec_batch_generate): per iteration gamma batched draft steps,
    # the verify passes, the batched accept + residual sample, one copy of the result blocks and one wait - the
    # interpreter sees the finished token buffers and the per-iteration statistics
    d0, t0 = streams[0].draft._session, streams[0].target._session
    # (with per-stream parameters the block's own triple is not read: stream 0's stands in)
    args = (table.arr, B, gamma, sampling_block(*triples[0], V, streams[0].draft._probs.stride(0), eos_token_id),
            int(random_seed or 0), r_const.data_ptr() if r_const is not None else None,
            spec_scratch(d0, t0, table.norm_ws, table.per_pass), table.vlog.block, _stream())
    with opts.attach(dev, V, slab_rows(gamma, B, table.per_pass), [len(s.log.host_seq) for s in streams],
                     [s.target._session for s in streams], [s.T - s.prompt_len + gamma + 2 for s in streams]) as blocks:
        check(lib.sd_spec_batch_generate(*args, blocks.loop_opts), "sd_spec_batch_generate")
    if _timing is not None and blocks.grammar_states is not None:
        _timing["grammar_states"] = blocks.grammar_states
    outs, ds = table.results(eos_token_id)
    if _timing is not None:
        _timing.setdefault("verify", []).extend((_Ms(ms), None, n, ctx) for ms, n, ctx in table.vlog.entries())
    tail = ([blocks.logprob_tensor(i, o.shape[1] - s.prompt_len, o.device) for i, (o, s) in enumerate(zip(outs, streams))],) \
        if logprobs else ()
    if details:
        return (outs, ds, *tail)
    return (outs, *tail) if tail else outs


def _queue_arguments(prefixes, max_len, seeds, slots):
    """speculative_sampling_queue's argument checks (before a model or the GPU is touched); returns the per-prompt budgets."""
    if isinstance(slots, bool) or not isinstance(slots, int) or not 1 <= slots <= 16:
        raise ValueError(f"slots: 1..16 streams decode at once, not {slots!r}")
    try:
        N = len(prefixes)
    except TypeError:
        raise ValueError("prefixes: a sequence of (1, L) int64 prompts is required") from None
    if N < 1:
        raise ValueError("prefixes: at least one prompt is required")
    for i, pf in enumerate(prefixes):
        if not isinstance(pf, torch.Tensor) or pf.dim() != 2 or pf.shape[0] != 1 or pf.shape[1] < 1:
            raise ValueError(f"prefixes[{i}]: every prompt is one (1, L >= 1) tensor, got "
                             f"{tuple(pf.shape) if isinstance(pf, torch.Tensor) else type(pf).__name__}")
    if seeds is not None and len(seeds) != N:
        raise ValueError(f"seeds: {len(seeds)} seeds for {N} prompts")
    if isinstance(max_len, (int, np.integer)):
        return [int(max_len)] * N
    if len(max_len) != N:
        raise ValueError(f"max_len: {len(max_len)} budgets for {N} prompts")
    return [int(m) for m in max_len]


def _shared_prefix_argument(prefixes, shared_prefix) -> int:
    """speculative_sampling_queue_shared's check of ``shared_prefix`` (after _queue_arguments, before a model or the GPU is touched)."""
    if isinstance(shared_prefix, bool) or not isinstance(shared_prefix, (int, np.integer)) or shared_prefix < 0:
        raise ValueError(f"shared_prefix: a token count >= 0 is required, not {shared_prefix!r}")
    P = int(shared_prefix)
    shortest = min(pf.shape[1] for pf in prefixes)
    if P > shortest:
        raise ValueError(f"shared_prefix: {P} tokens, but the shortest prompt has {shortest}")
    if P:
        head = prefixes[0][0, :P].cpu()
        for i, pf in enumerate(prefixes[1:], 1):
            differ = (pf[0, :P].cpu() != head).nonzero()
            if differ.numel():
                raise ValueError(f"shared_prefix: prompt {i} differs from prompt 0 at position {int(differ[0])}: the first {P} tokens "
                                 "of every prompt must be the same")
    return P


@torch.no_grad()
def speculative_sampling_queue(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id, pad_token_id,
                               max_len, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                               random_seed: int = None, details: bool = False, seeds: Optional[Sequence[int]] = None,
                               slots: int = 8, prefill_chunk: int = 0, _timing: Optional[dict] = None):
    """Continuous batching: any number of prompts share ``slots`` lock-step streams (sd_spec_queue_generate).  Prompts are
    admitted in list order; a stream that ends at a new EOS or at its length (``max_len``: one int, or one per prompt) hands
    its slot to the next waiting prompt, whose prefill rides the passes the other streams run anyway - at most
    ``prefill_chunk`` prompt rows per pass (0: whatever room a pass has).  Prompt i runs on Philox stream ``seeds[i]``
    (default ``torch.initial_seed() + i``) from draw 0 wherever and whenever it is admitted: its tokens, ``acc_len`` and call
    counts equal those of ``speculative_sampling(prefixes[i], ..., max_len_i, rng=DeviceNoise(seeds[i]))``.  Returns the
    outputs in prompt order (and the ``details`` dicts of speculative_sampling_batch when ``details``).
    ``temperature``, ``top_k`` and ``top_p`` each take one value for all prompts or a sequence with one entry per prompt
    (``T_i``, ``k_i``, ``p_i``, the convention of ``max_len``; a scalar beside a sequence is broadcast): prompt i then equals
    ``speculative_sampling(prefixes[i], ..., temperature=T_i, top_k=k_i, top_p=p_i, rng=DeviceNoise(seeds[i]))``, whichever
    slot it decodes in and whatever its neighbours ask for.  A sequence of another length, a temperature entry of 0 or a
    negative / non-integer top_k entry raises ValueError before a model is touched.  With three scalars the call takes the
    scalar call as before; any sequence is the ``row_params`` of its sd_loop_opts.
    ``_timing`` receives "verify" entries as speculative_sampling_batch writes them, "iterations", "target_passes",
    "draft_passes", "extra_passes" (target passes that carried prompt rows only; "prefill_passes" of them ran while no
    stream was active), "prompt_rows" (target rows forwarded for prompts), "copied_rows" (0 here) and per prompt
    "admit_iter" / "finish_iter" (its first / last iteration).  speculative_sampling_queue_shared is this call for prompts
    that start with the same tokens."""
    return _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
                  random_seed, details, seeds, slots, prefill_chunk, _timing, 0)


@torch.no_grad()
def speculative_sampling_queue_shared(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id, pad_token_id,
                                      max_len, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                                      random_seed: int = None, details: bool = False, seeds: Optional[Sequence[int]] = None,
                                      slots: int = 8, prefill_chunk: int = 0, _timing: Optional[dict] = None,
                                      shared_prefix: int = 0):
    """speculative_sampling_queue with ``shared_prefix=P``: the first P tokens of every prompt are the same (a system prompt, a
    few-shot header; P <= the shortest prompt, checked token by token before a model is touched).  Their K / V rows depend on
    those tokens alone, so they go through each model once, into a donor pair of sessions, and an admitted prompt receives its
    first min(P, L_i - 1) rows as a copy of the donors' (sd_session_copy_kv) and forwards only the rest; the last prompt token is
    always fed as the first decode row.  The queue's contract holds unchanged - prompt i equals its speculative_sampling run -
    for 16-bit models up to the rounding a different pass shape for the prefix rows gives, which is the caveat the queue has
    anyway.  ``_timing``: "prompt_rows" includes the donor's rows, "copied_rows" is the number of KV rows copied per model
    summed over the prompts, and the donor's prefill passes count in "target_passes", "draft_passes", "extra_passes" and
    "prefill_passes", so a call compares with its ``shared_prefix=0`` twin.  With 0 (the default) there is no donor and the
    call is speculative_sampling_queue's, bit for bit and pass for pass.  ``temperature``, ``top_k`` and ``top_p`` take
    per-prompt sequences exactly as in speculative_sampling_queue: prompt i equals ``speculative_sampling(prefixes[i], ...,
    temperature=T_i, top_k=k_i, top_p=p_i, rng=DeviceNoise(seeds[i]))`` up to that caveat.  (A function of its own: the queue's parameter list
    is pinned by its tests.)"""
    return _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
                  random_seed, details, seeds, slots, prefill_chunk, _timing, shared_prefix)


@torch.no_grad()
def speculative_sampling_queue_logprobs(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id, pad_token_id,
                                        max_len, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                                        random_seed: int = None, details: bool = False, seeds: Optional[Sequence[int]] = None,
                                        slots: int = 8, prefill_chunk: int = 0, _timing: Optional[dict] = None,
                                        shared_prefix: int = 0):
    """speculative_sampling_queue_shared (``shared_prefix=0``: speculative_sampling_queue) that also returns, per prompt, the
    TARGET model's log-probability of every new token: ``(outs, logprobs)`` or ``(outs, details, logprobs)``, ``logprobs[i]`` a
    float32 (1, len_i - L_i) tensor on ``outs[i]``'s device, cut where the tokens are cut.  The score of a token is the
    log-softmax in fp32 of the target's raw logit row for the position before it, taken before temperature, top_k and top_p -
    what the model says, not what the sampler drew from - so ``logprobs[i].mean()`` is ``quality.get_score`` of output i
    without a second target pass.  Tokens, details and Philox positions are those of the call without scores
    (member ``logprobs`` of sd_loop_opts).  (A function of its own: the queues' parameter lists are pinned by their tests.)"""
    return _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
                  random_seed, details, seeds, slots, prefill_chunk, _timing, shared_prefix, logprobs=True)


@torch.no_grad()
def speculative_sampling_queue_requests(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id, pad_token_id,
                                        max_len, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                                        random_seed: int = None, details: bool = False, seeds: Optional[Sequence[int]] = None,
                                        slots: int = 8, prefill_chunk: int = 0, _timing: Optional[dict] = None,
                                        shared_prefix: int = 0, *, logprobs: bool = False, repetition_penalty=1.0,
                                        frequency_penalty=0.0, presence_penalty=0.0):
    """speculative_sampling_queue_shared with a request's whole sampling block: next to the per-prompt ``temperature`` /
    ``top_k`` / ``top_p``, ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` (neutral 1 / 0 / 0) each take
    one value for all prompts or one per prompt.  Prompt i then equals ``speculative_sampling(prefixes[i], ...,
    repetition_penalty=r_i, frequency_penalty=f_i, presence_penalty=p_i, rng=DeviceNoise(seeds[i]))``, whichever slot it decodes
    in and whatever its neighbours ask for: a slot changes penalties when it changes hands, and the prompt that counts as a
    request's prompt is its own (member ``penalties`` of sd_loop_opts; ``sampling.utils.apply_penalties`` has the definition).  A
    sequence of another length, a value that is not finite or a repetition penalty <= 0 raises ValueError before a model is
    touched.  ``logprobs=True`` returns what speculative_sampling_queue_logprobs returns: the scores stay what the model says,
    penalties or not.  (A function of its own: the queues' parameter lists are pinned by their tests.)"""
    return _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
                  random_seed, details, seeds, slots, prefill_chunk, _timing, shared_prefix, logprobs=logprobs,
                  penalties=(repetition_penalty, frequency_penalty, presence_penalty))


@torch.no_grad()
def speculative_sampling_queue_edits(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id, pad_token_id,
                                     max_len, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                                     random_seed: int = None, details: bool = False, seeds: Optional[Sequence[int]] = None,
                                     slots: int = 8, prefill_chunk: int = 0, _timing: Optional[dict] = None,
                                     shared_prefix: int = 0, *, logprobs: bool = False, repetition_penalty=1.0,
                                     frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None, allowed_token_ids=None,
                                     banned_token_ids=None, min_tokens=0):
    """speculative_sampling_queue_requests with the request fields that restrict what may be sampled: ``logit_bias`` (one
    ``{token id: bias}`` mapping for all prompts, or a sequence with one mapping-or-None per prompt), ``allowed_token_ids`` /
    ``banned_token_ids`` (one flat sequence of ids for all prompts, or one sequence-or-None per prompt) and ``min_tokens`` (an
    int, or one per prompt), as ``speculative_sampling`` describes them.  Prompt i equals ``speculative_sampling(prefixes[i],
    ..., rng=DeviceNoise(seeds[i]))`` with its values, whichever slot it decodes in: a slot changes its edits when it changes
    hands, and ``min_tokens`` counts the request's own output (member ``edits`` of sd_loop_opts; ``sampling.utils.apply_logit_edits``
    has the definition).  ValueError before a model is touched, as ``speculative_sampling`` lists them, naming the parameter
    and the prompt.  ``logprobs=True``: the scores stay what the model says.  (A function of its own:
    speculative_sampling_queue_requests' parameter list is pinned by its test, as the other queues' are.)"""
    return _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
                  random_seed, details, seeds, slots, prefill_chunk, _timing, shared_prefix, logprobs=logprobs,
                  penalties=(repetition_penalty, frequency_penalty, presence_penalty),
                  edits=(logit_bias, allowed_token_ids, banned_token_ids, min_tokens))


@torch.no_grad()
def speculative_sampling_queue_grammar(prefixes: Sequence[torch.Tensor], approx_model, target_model, eos_token_id, pad_token_id,
                                       max_len, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                                       random_seed: int = None, details: bool = False, seeds: Optional[Sequence[int]] = None,
                                       slots: int = 8, prefill_chunk: int = 0, _timing: Optional[dict] = None,
                                       shared_prefix: int = 0, *, logprobs: bool = False, repetition_penalty=1.0,
                                       frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None, allowed_token_ids=None,
                                       banned_token_ids=None, min_tokens=0, grammar=None):
    """speculative_sampling_queue_edits with ``grammar``: ONE ``sampling.grammar.TokenGrammar`` (or None) that every prompt's
    output must follow.  The grammar sits on the slots' target sessions, each slot with a state cache of its own, and a slot
    that changes hands starts again at the start state; prompt i equals ``speculative_sampling(prefixes[i], ..., grammar=grammar,
    rng=DeviceNoise(seeds[i]))`` with its other values, whichever slot it decodes in.  Per-prompt grammars in the queue are out
    of scope (``speculative_sampling_batch`` takes one per stream).  ``_timing["grammar_states"]``: the slots' device state
    caches.  (A function of its own: the queues' parameter lists are pinned by their tests.)"""
    if grammar is not None and not isinstance(grammar, TokenGrammar):
        raise ValueError(f"grammar: one TokenGrammar for all prompts (or None) is required, not {grammar!r}")
    return _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
                  random_seed, details, seeds, slots, prefill_chunk, _timing, shared_prefix, logprobs=logprobs,
                  penalties=(repetition_penalty, frequency_penalty, presence_penalty),
                  edits=(logit_bias, allowed_token_ids, banned_token_ids, min_tokens), grammar=grammar)


def _queue(prefixes, approx_model, target_model, eos_token_id, pad_token_id, max_len, gamma, temperature, top_k, top_p,
           random_seed, details, seeds, slots, prefill_chunk, _timing, shared_prefix, logprobs=False, penalties=(1.0, 0.0, 0.0),
           edits=(None, None, None, 0), grammar=None):
    """The prompt queue behind the public entry points (their docstrings have the contract)."""
    budgets = _queue_arguments(prefixes, max_len, seeds, slots)
    shared = _shared_prefix_argument(prefixes, shared_prefix)
    if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, int) or prefill_chunk < 0:
        raise ValueError(f"prefill_chunk: a row count >= 0 is required, not {prefill_chunk!r}")
    if not 1 <= gamma <= 16:
        raise ValueError(f"gamma: 1..16, not {gamma}")
    N = len(prefixes)
    opts = RequestOptions.parse(N, "prompt", eos_token_id, sampling=(temperature, top_k, top_p), logprobs=logprobs, penalties=penalties,
                                edits=edits, grammar=grammar)
    opts.require_target_rows(target_model)
    triples = opts.sampling
    if triples is not None:                                       # (a slot's KVCacheModel and the block's own triple are not read)
        temperature, top_k, top_p = triples[0]
    draft_m, target_m = as_specdec_model(approx_model), as_specdec_model(target_model)
    same_device(draft_m, target_m)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    assert draft_m.cfg.vocab_size == V
    opts.bind(V)
    for pf in prefixes:
        check_token_ids(pf, V)
    S = min(slots, N)
    seeds = stream_seeds(seeds, N)
    lens = [pf.shape[1] for pf in prefixes]
    cap = max(L + max(m, 0) for L, m in zip(lens, budgets)) + gamma + 2   # every slot holds the largest prompt of the call
    res_sz = C.sizeof(SdAcceptResult)
    res_dev = torch.zeros((S, res_sz), dtype=torch.uint8, device=dev)
    res_host = torch.zeros((S, res_sz), dtype=torch.uint8).pin_memory()
    r_const = reseed_uniforms(random_seed, gamma, dev)
    empty = torch.zeros(0, dtype=torch.int64)
    held = [open_spec_slot(draft_m, target_m, empty, cap, gamma, temperature, top_k, top_p) for _ in range(S)]
    slot_arr = (SdBatchStream * S)()
    for i, (it, (draft, target, seq32, err)) in enumerate(zip(slot_arr, held)):
        bind_spec_slot(it, draft, target, seq32, err, res_dev.data_ptr() + i * res_sz, res_host.data_ptr() + i * res_sz)
    # the prompts wait in pinned host memory: the loop copies one into its slot when it is admitted
    tokens = torch.cat([pf[0].to(device="cpu", dtype=torch.int32) for pf in prefixes]).pin_memory()
    offs = np.concatenate([[0], np.cumsum(lens)])
    logs, arr = [], (SdQueuePrompt * N)()
    for i, (it, pf, L, m) in enumerate(zip(arr, prefixes, lens, budgets)):
        host = tokens[offs[i]:offs[i + 1]].tolist()
        T = L + m
        log = LoopLog(host, max(L, T) + gamma + 2, max(1, m) + 1, gamma, q_fill=1.0)
        logs.append(log)
        it.tokens = tokens.data_ptr() + int(offs[i]) * 4
        it.L, it.T, it.ori_eos_cnt, it.seed = L, T, host.count(eos_token_id), int(seeds[i]) & 0xFFFFFFFFFFFFFFFF
        it.host_seq = log.host_seq.ctypes.data
        it.acc_len_out, it.p_at_out, it.q_at_out = log.ptrs()[:3]
    d0, t0 = held[0][0]._session, held[0][1]._session
    per_pass = t0.max_pass_rows
    norm_ws = torch.empty(lib.sd_norm_workspace_bytes(per_pass), dtype=torch.uint8, device=dev)
    vlog = LockstepLog(sum(max(1, m) + 1 for m in budgets))       # (an iteration has at least one stream in it)
    passes = (C.c_int * 6)()
    args = (slot_arr, S, cap, arr, N, prefill_chunk, gamma,
            sampling_block(temperature, top_k, top_p, V, held[0][0]._probs.stride(0), eos_token_id), int(random_seed or 0),
            r_const.data_ptr() if r_const is not None else None, spec_scratch(d0, t0, norm_ws, per_pass), vlog.block, passes, _stream())
    # the donors hold the shared rows a prompt can use: the longest prompt's last token is fed as a decode row like everyone's
    rows = min(shared, max(lens) - 1)
    donors, donor_passes = [None, None], [0, 0]                   # (draft, target) sessions and the passes of their prefill
    if rows > 0:
        head = tokens[:rows].to(dev)
        donors = [draft_m.new_session(rows), target_m.new_session(rows)]
        for side, ses in enumerate(donors):
            if ses.kv_fp8 and not torch.equal(ses.kv_scale, held[0][side]._session.kv_scale):
                raise ValueError("shared_prefix: the fp8 KV arenas of the donors and the slots have different scale tables")
            batch_prefill([ses], [head], [rows])
            donor_passes[side] = -(-rows // ses.max_rows)
    args += (*[ses.handle if ses else None for ses in donors], rows)
    states_cap = max(L + max(m, 0) for L, m in zip(lens, budgets)) - min(lens) + gamma + 2
    with opts.attach(dev, V, slab_rows(gamma, S, per_pass), [len(log.host_seq) for log in logs], [h[1]._session for h in held],
                     [states_cap] * S) as blocks:
        check(lib.sd_spec_queue_generate(*args, blocks.loop_opts), "sd_spec_queue_generate")
    if _timing is not None and blocks.grammar_states is not None:
        _timing["grammar_states"] = blocks.grammar_states
    passes[4] += rows                                             # the donor's target rows are prompt rows too
    if vlog.block.err:
        raise RuntimeError("s")
    if _timing is not None:
        _timing.setdefault("verify", []).extend((_Ms(ms), None, n, ctx) for ms, n, ctx in vlog.entries())
        _timing.update(iterations=vlog.block.n_iters, target_passes=passes[0] + donor_passes[1], draft_passes=passes[1] + donor_passes[0],
                       extra_passes=passes[2] + donor_passes[1], prefill_passes=passes[3] + donor_passes[1],
                       prompt_rows=passes[4], copied_rows=passes[5], admit_iter=[it.admit_iter for it in arr],
                       finish_iter=[it.finish_iter for it in arr])
    res = [lockstep_result(log, it.len, it.calls, eos_token_id, it.ori_eos_cnt, pf.device)
           for it, log, pf in zip(arr, logs, prefixes)]
    outs, ds = [r[0] for r in res], [r[1] for r in res]
    if logprobs:
        lps = [blocks.logprob_tensor(i, o.shape[1] - L, o.device) for i, (o, L) in enumerate(zip(outs, lens))]
        return (outs, ds, lps) if details else (outs, lps)
    return (outs, ds) if details else outs


@torch.no_grad()
def autoregressive_sampling_batch(xs: Sequence[torch.Tensor], model, N: int, eos_token_id, temperature: float = 1,
                                  top_k: int = 0, top_p: float = 0, pad_token_id=None, *,
                                  seeds: Optional[Sequence[int]] = None, _timing: Optional[dict] = None,
                                  logprobs: bool = False, repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0,
                                  logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_tokens=0, grammar=None):
    """``autoregressive_sampling`` for B streams at once: ``xs[i]`` is (1, L_i) int64, the result a list of (1, len_i)
    tensors.  The streams decode in lock-step and share every pass over the weights (sd_ar_batch_generate): each runs the
    algorithm of reference autoregressive_sampling.py:9-61 on its own Philox stream ``seeds[i]`` (default
    ``torch.initial_seed() + i``), so the outputs equal those of B ``autoregressive_sampling(..., rng=DeviceNoise(seed))``
    calls.  ``_timing["step"]`` receives (milliseconds, streams in the step) per step.  ``logprobs``: returns ``(outs,
    logprobs)``, a list of float32 (1, len_i - L_i) tensors with the model's log-probability of every new token: the
    log-softmax of its raw logits, before temperature, top_k and top_p - what the model says, not what the sampler drew from.
    ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` (neutral 1 / 0 / 0): each one value for all streams or
    one per stream; stream i equals ``autoregressive_sampling(xs[i], ..., rng=DeviceNoise(seeds[i]))`` with its values
    (member ``penalties`` of sd_loop_opts).  ``logit_bias`` / ``allowed_token_ids`` / ``banned_token_ids`` / ``min_tokens``: one
    value for all streams or one per stream, as ``speculative_sampling_batch`` takes them (member ``edits``).  ``grammar``: one
    ``sampling.grammar.TokenGrammar`` for all streams or one TokenGrammar-or-None per stream, as ``speculative_sampling_batch``
    takes it (``_timing["grammar_states"]``: the streams' device state caches)."""
    B = len(xs)
    if not 1 <= B <= 16:
        raise ValueError(f"autoregressive_sampling_batch takes 1..16 streams per call, not {B}")
    opts = RequestOptions.parse(B, "stream", eos_token_id, logprobs=logprobs,
                                penalties=(repetition_penalty, frequency_penalty, presence_penalty),
                                edits=(logit_bias, allowed_token_ids, banned_token_ids, min_tokens), grammar=grammar)
    opts.require_target_rows(model)
    m = as_specdec_model(model)
    V = m.cfg.vocab_size
    opts.bind(V)
    for x in xs:
        assert x.dim() == 2 and x.shape[0] == 1 and x.shape[1] >= 1, "every stream is one (1, L) prompt"
        check_token_ids(x, V)
    seeds = stream_seeds(seeds, B)
    run = ArRun(m, temperature, top_k, top_p, eos_token_id)
    caps = [x.shape[1] + int(N) + 1 for x in xs]
    kvs, seqs = map(list, zip(*[open_stream(m, x[0], cap, cap, temperature, top_k, top_p) for x, cap in zip(xs, caps)]))
    # everything but the last prompt token, the prompts packed into shared passes; every step of the loop then feeds one
    # row per stream
    batch_prefill([kv._session for kv in kvs], seqs, [x.shape[1] - 1 for x in xs])
    for x, seed, kv, seq32 in zip(xs, seeds, kvs, seqs):
        run.add(kv, seq32, x[0].to(device="cpu", dtype=torch.int32).numpy(), x.shape[1] + int(N), DeviceNoise(seed))
    run.generate(timing=_timing is not None, logprobs=logprobs, penalties=opts.penalties, edits=opts.edits, grammars=opts.grammar)
    if _timing is not None:
        _timing.setdefault("step", []).extend(run.steps)
        if run.grammar_states is not None:
            _timing["grammar_states"] = run.grammar_states
    outs = [torch.from_numpy(run.tokens(i)).to(torch.int64).unsqueeze(0).to(x.device) for i, x in enumerate(xs)]
    return (outs, [run.logprobs(i, x.device) for i, x in enumerate(xs)]) if logprobs else outs
