"""Drop-in for reference sampling/speculative_sampling.py:1876-2076 (``speculative_sampling``).

Same signature, return values, ``details`` keys, RNG draw order, EOS rule and exceptions.  The
loop body differs in mechanism only: tokens, both KV caches and both probability histories stay
on the device; each iteration is gamma x (draft forward, norm_probs, sample), one target forward
over gamma+1 rows, norm_probs, then one accept-scan + resample launch pair and a single
device->host read of the 208-byte result block.
"""
from __future__ import annotations

import ctypes as C
from time import process_time_ns

import numpy as np
import torch

from .._lib import lib, check, SdAcceptResult
from ..engine import as_specdec_model, _stream, check_token_ids, same_device
from ._loop_common import (RequestOptions, cut_after_new_eos, details_dict, device_rng, loop_opts, make_noise, open_stream,
                           reseed_uniforms, sampling_block, single_stream_native_call, slab_rows, spec_scratch, spec_stream)

_make_noise = make_noise                              # beam.py, multi.py and tests import it from here


@torch.no_grad()
def speculative_sampling(prefix: torch.Tensor, approx_model, target_model, eos_token_id, pad_token_id,
                         max_len: int, gamma: int = 4, temperature: float = 1, top_k: int = 0, top_p: float = 0,
                         verbose: bool = False, random_seed: int = None, details: bool = False, *, rng=None,
                         _event_logs=None, logprobs: bool = False, repetition_penalty: float = 1.0,
                         frequency_penalty: float = 0.0, presence_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None,
                         banned_token_ids=None, min_tokens=0, grammar=None):
    """reference speculative_sampling.py:1876-2076.

    ``rng`` (extension): "host" (default) draws every variate from torch's CPU generator in the
    reference's order, so token ids equal the reference's CPU path under the same seed; "device"
    uses on-device Philox (throughput mode); or a noise object from ``llmspeculativesampling_amd.noise``.

    ``logprobs`` (extension, native device-RNG loop only): the return value gains one last element, a float32 tensor
    (1, len(output) - len(prefix)) on the output's device with the TARGET model's log-probability of every new token:
    ``log_softmax`` in fp32 of the target's raw logit row for the position before it, taken before temperature, top_k and
    top_p - what the model says, not what the sampler drew from.  It is cut where the tokens are cut, and its mean is
    ``quality.get_score`` of the output without a second target pass (``quality.score_from_logprobs``).

    ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` (extension, native device-RNG loop only; neutral
    1 / 0 / 0): every draft and target logit row is edited on the device by the row's own history before it is normalised,
    as ``sampling.utils.apply_penalties`` defines it - the repetition penalty over prompt and output tokens (x / r for a
    positive logit, x * r otherwise), ``frequency * count`` and ``presence`` subtracted for tokens generated so far.  They
    change what the sampler draws from; ``logprobs`` stay what the model says.  ValueError before a model is touched for a
    value that is not finite, a repetition penalty <= 0, an interpreter path or a tensor-parallel target.

    ``logit_bias`` / ``allowed_token_ids`` / ``banned_token_ids`` / ``min_tokens`` (extension, native device-RNG loop only;
    neutral None / None / None / 0): the request fields that restrict what may be sampled, applied on the device to every
    draft and target logit row behind the penalties, as ``sampling.utils.apply_logit_edits`` defines it - a ``{token id:
    bias}`` mapping of at most 1024 entries is added, every id outside ``allowed_token_ids`` (None: all) or inside
    ``banned_token_ids`` becomes -inf, and so does ``eos_token_id`` until ``min_tokens`` tokens have been produced.
    ``logprobs`` stay what the model says.  ValueError before a model is touched for a bias that is not a finite number, more
    than 1024 entries, an id that is not an integer or lies outside the vocabulary, ``min_tokens < 0``, an allowed set that the
    banned ids empty or that holds nothing but EOS while ``min_tokens > 0``, an interpreter path or a tensor-parallel target.

    ``grammar`` (extension, native device-RNG loop only; a ``sampling.grammar.TokenGrammar`` or None): the output must follow
    the token automaton.  Every draft and target logit row is masked on the device, behind the logit edits, by the state the
    row's own output prefix leads to (``sampling.utils.apply_grammar``); the automaton advances on the device along the drafted
    tokens, so the output is distributed as the target's own sampling under the grammar.  ``logprobs`` stay what the model
    says.  ValueError before a model is touched for an interpreter path or a tensor-parallel target, and for a grammar built
    for another vocabulary once the model is known.
    """
    opts = RequestOptions.parse(1, "stream", eos_token_id, logprobs=logprobs,
                                penalties=(repetition_penalty, frequency_penalty, presence_penalty),
                                edits=(logit_bias, allowed_token_ids, banned_token_ids, min_tokens), grammar=grammar)
    opts.require_native(device_rng(rng) and not verbose, " and verbose=False")
    opts.require_target_rows(target_model)
    assert prefix.shape[0] == 1, "input batch size must be 1"
    draft_m, target_m = as_specdec_model(approx_model), as_specdec_model(target_model)
    if draft_m.cfg.is_encoder_decoder or target_m.cfg.is_encoder_decoder:
        raise NotImplementedError("encoder-decoder models are out of scope")
    same_device(draft_m, target_m)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    assert draft_m.cfg.vocab_size == V, "draft and target must share a vocabulary"
    assert 1 <= gamma <= 16
    opts.bind(V)

    seq_len0 = prefix.shape[1]
    T = seq_len0 + max_len
    cap = T + gamma + 2
    host_seq = [int(t) for t in prefix[0].tolist()]
    if seq_len0 < T:
        try:                                          # nn.Embedding's IndexError surfaces inside the reference's
            check_token_ids(host_seq, V)              # try block and leaves as RuntimeError('s') (:1933, :2044-2046)
        except IndexError as e:
            print(e)
            raise RuntimeError("s") from e
    noise = make_noise(rng, dev)
    draft, _ = open_stream(draft_m, None, cap, 0, temperature, top_k, top_p, noise)
    target, seq32 = open_stream(target_m, prefix[0], cap, cap + 1, temperature, top_k, top_p, noise)
    if getattr(noise, "on_device", False) and not verbose:
        return _native_device_loop(prefix, draft, target, seq32, host_seq, eos_token_id, T, gamma, random_seed, details,
                                   noise, _event_logs, opts)

    ori_eos_cnt = host_seq.count(eos_token_id)
    if _event_logs is not None:                       # bench.py: HIP-event brackets around every forward
        draft.event_log, target.event_log = _event_logs
    res_dev = torch.zeros(C.sizeof(SdAcceptResult), dtype=torch.uint8, device=dev)
    res_host = torch.zeros(C.sizeof(SdAcceptResult), dtype=torch.uint8).pin_memory()
    tok_host = torch.zeros(gamma + 2, dtype=torch.int32).pin_memory()
    serr = torch.zeros(gamma + 2, dtype=torch.int32, device=dev)
    q_hist, p_hist = draft._probs, target._probs
    ld = q_hist.stride(0)
    st = _stream()
    # p - q, max_fn and the residual draw run in the rows' dtype when both models keep 16-bit rows (OPT)
    res_mode = target_m.norm_mode if target_m.norm_mode == draft_m.norm_mode else 0
    res_dtype = target_m.probs_dtype if res_mode else torch.float32

    approx_time = target_time = other_time = 0
    approx_calls = target_calls = 0
    acc_rate, acc_len = [], []
    out_tokens = host_seq
    r_const = None
    try:
        while len(host_seq) < T:
            tick = process_time_ns()
            L = len(host_seq)
            # ---- draft: gamma steps, tokens never leave the device (kvcache_model.py:279-293)
            for i in range(gamma):
                draft.forward_sample(seq32, L + i, noise, serr[i])
            approx_calls += 1
            approx_time += process_time_ns() - tick
            tick = process_time_ns()
            # ---- target: one forward over the gamma+1 uncached rows (all rows on the first call)
            n_new = L + gamma - target.cache_len
            target.forward_rows(seq32, L + gamma, min(n_new, gamma + 1))
            # generate(x, 1) samples from the last row and throws the token away (kvcache_model.py:283):
            # the draw is part of the RNG contract even though its result is unused
            if noise.on_device:
                noise.next_draws(1)
            else:
                noise.skip_exponential(V, target_m.probs_dtype)
            target_calls += 1
            target_time += process_time_ns() - tick
            tick = process_time_ns()
            # ---- accept scan (speculative_sampling.py:1964-1991) + residual / bonus sample (:2005-2023)
            if noise.on_device:
                if random_seed:
                    # reseed-before-every-r quirk (:1976-1977): all r are one and the same draw and the
                    # stream restarts after it, whatever was accepted
                    noise.reseed(random_seed)
                    if r_const is None:
                        r_const = reseed_uniforms(random_seed, gamma, dev)
                    check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), ld, seq32.data_ptr(), L, gamma,
                                             r_const.data_ptr(), 0, 0, res_dev.data_ptr(), st), "sd_accept_scan")
                else:
                    check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), ld, seq32.data_ptr(), L, gamma,
                                             None, noise.seed, noise.next_draws(gamma), res_dev.data_ptr(), st),
                          "sd_accept_scan")
                check(lib.sd_resample(p_hist.data_ptr(), q_hist.data_ptr(), ld, V, seq32.data_ptr(), L, gamma, None,
                                      noise.seed, noise.next_draws(1), res_dev.data_ptr(), None, res_mode, st), "sd_resample")
            else:
                r, token = noise.uniforms(gamma, random_seed)
                check(lib.sd_accept_scan(p_hist.data_ptr(), q_hist.data_ptr(), ld, seq32.data_ptr(), L, gamma,
                                         r.data_ptr(), 0, 0, res_dev.data_ptr(), st), "sd_accept_scan")
                if token is not None:
                    # the reference stops drawing uniforms at the first reject: learn l, re-align the host stream
                    res_host.copy_(res_dev, non_blocking=True)
                    torch.cuda.current_stream().synchronize()
                    l_now = SdAcceptResult.from_buffer_copy(res_host.numpy().tobytes()).n_accepted
                    noise.realign(token, min(l_now + 1, gamma))
                e = noise.exponential(V, res_dtype)
                check(lib.sd_resample(p_hist.data_ptr(), q_hist.data_ptr(), ld, V, seq32.data_ptr(), L, gamma,
                                      e.data_ptr(), 0, 0, res_dev.data_ptr(), None, res_mode, st), "sd_resample")
            res_host.copy_(res_dev, non_blocking=True)
            tok_host.copy_(seq32[L:L + gamma + 2], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            res = SdAcceptResult.from_buffer_copy(res_host.numpy().tobytes())
            if bool(serr[:gamma].any()) or (res.flags & 2):
                raise RuntimeError("prob error")
            draft.check_errors(L - 1, L + gamma - 1)
            target.check_errors(L - 1, L + gamma)
            l, n, t = res.n_accepted, res.n, res.next_token
            for i in range(gamma):                    # statistic over all gamma drafted positions (:1966-1971)
                acc_rate.append(min(1.0, float(res.p_at[i]) / float(res.q_at[i])))
            acc_len.append(l)
            assert n >= L - 1, f"n {n}, prefix_len {L}"
            drafted = tok_host[:l].tolist()
            host_seq = host_seq + drafted + [t]
            draft.rollback(n + 1)
            target.rollback(n + 1 if l < gamma else n + 2)
            if verbose:
                print(f"accepted {l} of {gamma}: {drafted} + {t}")
            # ---- EOS rule over the whole sequence (:2033-2041)
            out_tokens = cut_after_new_eos(host_seq, eos_token_id, ori_eos_cnt)
            if out_tokens is not host_seq:            # a new EOS was produced
                break
            other_time += process_time_ns() - tick
    except Exception as e:                            # (:2044-2046); the cause stays attached to the traceback
        print(e)
        raise RuntimeError("s") from e

    out = torch.tensor([out_tokens], dtype=torch.int64, device=prefix.device)
    if verbose:
        print(f"generated tokens numbers {len(host_seq) - seq_len0}, acc len {acc_len}")
    if details:
        return out, details_dict(approx_time, target_time, other_time, acc_len, np.mean(acc_rate), target_calls, approx_calls,
                                 target_model_time=target.forward_time_dict["_model_time"],
                                 target_pre_cache_time=target.forward_time_dict["prepare_cache_time"],
                                 target_post_prob_time=target.forward_time_dict["norm_prob_time"])
    return out


def _native_device_loop(prefix, draft, target, seq32, host_seq, eos_token_id, T, gamma, random_seed, details, noise,
                        timing_log, opts):
    """Device-RNG mode: the loop itself runs inside libspecdec (sd_spec_generate): per iteration the gamma draft steps,
    the target forward, the accept scan and the resample are enqueued and the stream is waited on once, in native code;
    the interpreter only sees the finished sequence and the per-iteration statistics.  Same loop semantics as the
    Python-orchestrated path above (reference speculative_sampling.py:1934-2046)."""
    dev = target._model.device
    V = target._model.cfg.vocab_size
    seq_len0 = len(host_seq)
    r_const = reseed_uniforms(random_seed, gamma, dev)
    sampling = sampling_block(target._temperature, target._top_k, target._top_p, V, draft._probs.stride(0), eos_token_id)
    scratch = spec_scratch(draft._session, target._session, target._norm_ws, target._session.max_rows)
    with opts.attach(dev, V, slab_rows(gamma), [T + gamma + 2], [target._session], [T - seq_len0 + gamma + 2]) as blocks:
        def call(res_dev, res_host, err_words, st):
            stream = spec_stream(draft, target, seq32, err_words, res_dev.data_ptr(), res_host.data_ptr())
            check(lib.sd_spec_generate(stream, gamma, sampling, scratch, st, int(random_seed or 0),
                                       r_const.data_ptr() if r_const is not None else None, _stream(), loop_opts(*blocks.members)),
                  "sd_spec_generate")
        timed = timing_log is not None or details          # HIP-event brackets around the draft and the verify phase
        out_tokens, st, log, acc_len, acc_rate, (approx_time, target_time, other_time) = \
            single_stream_native_call(call, host_seq, T, gamma, eos_token_id, noise, dev, timed)
    calls = st.n_iters
    if timing_log is not None:
        Lc, tl = seq_len0, 0
        for i in range(calls):
            timing_log["draft_ms"].append(float(log.draft_ms[i]))
            timing_log["target"].append((float(log.target_ms[i]), Lc + gamma - tl, Lc + gamma))
            tl = Lc + acc_len[i]                             # n + 1 with n = L + l - 1
            Lc += acc_len[i] + 1
    draft._session.cache_len, target._session.cache_len = st.draft_len, st.target_len
    out = torch.tensor([out_tokens], dtype=torch.int64, device=prefix.device)
    tail = (blocks.logprob_tensor(0, len(out_tokens) - seq_len0, prefix.device),) if opts.logprobs else ()
    if details:
        # the verify phase is one fused launch chain (forward + norm_probs, no cache preparation): all of it is model time
        return (out, details_dict(approx_time, target_time, other_time, acc_len, np.mean(acc_rate), calls, calls,
                                  target_model_time=target_time, target_pre_cache_time=0, target_post_prob_time=0), *tail)
    return (out, *tail) if tail else out
