"""Drop-in for reference sampling/speculative_sampling.py:1379-1716 (``multi_speculative_sampling``), decoder-only,
``strategy="iid"``.

Each iteration ``width`` replicas of the draft sample their own gamma tokens, the target scores all of them, the replica
with the longest accepted run wins and both models continue from it.  Mechanism here: one KV arena, probability arena and
token buffer per replica; the width draft rows of a step and the width*(gamma+1) verify rows go through ONE pass over the
weights each (``sd_batch_forward`` + ``sd_norm_batch``), the replica scan is ``sd_accept_multi``, the residual / bonus
sample ``sd_multi_resample``, and where the reference re-materialises the cache with ``val.repeat(width, ...)``
(kvcache_model.py:180-192) and slices it with ``rollback(end, choice)`` (:390-396, 433-436) only the few positions
written in this iteration are copied from the winner's arenas to the others.

Under device RNG (``DeviceNoise``, not ``verbose``) the whole loop runs inside libspecdec (``sd_spec_multi_generate``): the
scan and the residual / bonus sample are one launch, the winner broadcast is one launch that reads ``choice`` from the
device result block, and the host waits once per iteration.  ``SD_MULTI_NATIVE=0`` (read per call) keeps the Python loop
below under device RNG too; the host-RNG modes always take it.

Same signature, return value, ``details`` keys, RNG draw order and EOS rule.  ``strategy="beam"`` (the reference's
default) and ``"acc_beam"`` rest on ``beam_sample_with_kv_cache`` (out of scope).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from time import process_time_ns

import numpy as np
import torch

from .. import _lib
from .._lib import lib, check, SdMultiItem, SdMultiReplica, SdMultiResult, SdNormRow, SpecDecError
from ..engine import as_specdec_model, batch_forward, _stream, MAX_ROWS_PER_FORWARD, check_token_ids, same_device
from ._loop_common import (LoopLog, accept_rates_f32_zero_q, cut_after_new_eos, details_dict, make_noise, open_stream,
                           raise_loop_error, reseed_uniforms, sampling_block, spec_scratch)


def _copy_positions(dst_ses, src_ses, lo: int, hi: int) -> None:
    """KV rows [lo, hi) of every layer / head from one replica's arena to another's (sd_session_copy_kv)."""
    if hi > lo:
        dst_ses.copy_kv_from(src_ses, lo, hi)


def _takes_native_loop(noise, verbose) -> bool:
    """The rule of speculative_sampling.py:84 plus the switch: device RNG, not verbose, SD_MULTI_NATIVE != 0 (read per call)."""
    return bool(getattr(noise, "on_device", False)) and not verbose and os.environ.get("SD_MULTI_NATIVE", "1") != "0"


def _check_native(rc: int) -> None:
    """check(), except that a refused argument (width / gamma / row limits) is an engine failure here, never swallowed."""
    if rc == _lib.SD_ERR_INVALID:
        raise SpecDecError("sd_spec_multi_generate: " + lib.sd_last_error().decode(errors="replace"))
    check(rc, "sd_spec_multi_generate")


@dataclass
class _MultiRun:
    """What both loops of one multi_speculative_sampling call share: the replicas and the call's parameters."""
    drafts: list
    targets: list
    seqs: list
    T: int
    gamma: int
    eos_token_id: int
    ori_eos: int
    random_seed: int
    sampling: tuple          # (temperature, top_k, top_p)
    norm_ws: torch.Tensor
    r_const: torch.Tensor


@dataclass
class _MultiResult:
    """What one sd_spec_multi_generate call left; ``rc`` and ``err`` are for the caller to raise on."""
    rc: int
    err: int
    tokens: list
    acc_len: list
    acc_rate: list
    calls: int
    approx_time: int
    target_time: int
    other_time: int


def _native_multi_loop(run: _MultiRun, host, cache_len, noise, timed):
    """Device-RNG mode: ONE call into libspecdec (sd_spec_multi_generate) runs every iteration - draft steps, verify passes,
    the fused scan + resample launch, the winner broadcast launch, one copy and one stream wait each - and the interpreter
    sees the finished sequence and the per-iteration statistics.  ``cache_len``: positions both models hold of ``host``."""
    drafts, targets, seqs, T, gamma = run.drafts, run.targets, run.seqs, run.T, run.gamma
    target_m, W = targets[0]._model, len(drafts)
    V, ld = target_m.cfg.vocab_size, drafts[0]._probs.stride(0)
    dev = target_m.device
    d_ses, t_ses = [m._session for m in drafts], [m._session for m in targets]
    reps = (SdMultiReplica * W)()
    for w in range(W):
        reps[w].draft, reps[w].target = d_ses[w].handle, t_ses[w].handle
        reps[w].seq, reps[w].q_hist, reps[w].p_hist = seqs[w].data_ptr(), drafts[w]._probs.data_ptr(), targets[w]._probs.data_ptr()
    nbytes = lib.sd_spec_multi_block_bytes(W, gamma)
    dev_block = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    host_block = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
    max_iters = max(1, T - len(host))
    log = LoopLog(host, T + gamma + 2, max_iters, W * gamma, q_fill=0.0, timed=timed)
    st = log.seq_state(len(host), T, int(run.ori_eos), (cache_len, cache_len), noise, max_iters)
    tick = process_time_ns()
    rc = lib.sd_spec_multi_generate(reps, W, gamma, seqs[0].numel(), sampling_block(*run.sampling, V, ld, run.eos_token_id),
                                    int(run.random_seed or 0), run.r_const.data_ptr() if run.r_const is not None else None,
                                    spec_scratch(d_ses[0], t_ses[0], run.norm_ws, t_ses[0].max_pass_rows), dev_block.data_ptr(),
                                    host_block.data_ptr(), st, _stream())
    other_time = process_time_ns() - tick                             # host CPU time of the call (enqueue + waits + bookkeeping)
    noise.seed, noise.draw = st.seed, st.draw
    for ses in d_ses:
        ses.cache_len = st.draft_len
    for ses in t_ses:
        ses.cache_len = st.target_len
    calls = st.n_iters
    n_acc = calls - 1 if calls and log.acc[calls - 1] < 0 else calls  # an iteration ended by an error word was not scanned
    return _MultiResult(rc, st.err, log.tokens(st.len), log.acc_len(n_acc),
                        accept_rates_f32_zero_q(*log.ratios(n_acc)), calls, *log.phase_ns(calls), other_time)


@torch.no_grad()
def multi_speculative_sampling(prefix: torch.Tensor, approx_model, target_model, eos_token_id, pad_token_id,
                               max_len: int, gamma: int = 4, width: int = 8, num_beams=None, strategy: str = "beam",
                               acc_rate_head=None, acc_rate_thres=0.4, temperature: float = 1, top_k: int = 0,
                               top_p: float = 0, verbose: bool = False, random_seed: int = None,
                               details: bool = False, *, rng=None):
    """reference speculative_sampling.py:1379-1716.  ``rng`` as in ``speculative_sampling``."""
    if strategy in ("beam", "acc_beam", "diverse"):
        raise NotImplementedError(f"strategy {strategy!r} needs beam_sample_with_kv_cache "
                                  "(reference kvcache_model.py:439-567), out of scope; use strategy='iid'")
    if strategy != "iid":
        raise RuntimeError("Strategy not implemented " + strategy)         # reference :1548
    assert prefix.shape[0] == 1, "input batch size must be 1"
    draft_m, target_m = as_specdec_model(approx_model), as_specdec_model(target_model)
    same_device(draft_m, target_m)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    assert draft_m.cfg.vocab_size == V, "draft and target must share a vocabulary"
    W = int(width)
    assert 1 <= W <= 16 and 1 <= gamma <= 16
    assert W * 2 <= MAX_ROWS_PER_FORWARD

    L0 = prefix.shape[1]
    T = L0 + max_len
    cap = T + gamma + 2
    host = [int(t) for t in prefix[0].tolist()]
    ori_eos = host.count(eos_token_id)
    noise = make_noise(rng, dev)
    on_dev = getattr(noise, "on_device", False)

    drafts = [open_stream(draft_m, None, cap, 0, temperature, top_k, top_p)[0] for _ in range(W)]
    targets, seqs = map(list, zip(*[open_stream(target_m, prefix[0], cap, cap + 1, temperature, top_k, top_p)
                                    for _ in range(W)]))
    d_ses, t_ses = [m._session for m in drafts], [m._session for m in targets]
    # the prompt but its last token goes through each model once; the other replicas get copies of those KV rows
    # (the reference runs the same rows width times, kvcache_model.py:156 with a (width, L) batch)
    if L0 > 1:
        d_ses[0].forward(seqs[0][:L0 - 1], 0)
        t_ses[0].forward(seqs[0][:L0 - 1], 0)
        for w in range(1, W):
            _copy_positions(d_ses[w], d_ses[0], 0, L0 - 1)
            _copy_positions(t_ses[w], t_ses[0], 0, L0 - 1)
    draft_len = target_len = L0 - 1

    norm_ws = torch.empty(lib.sd_norm_workspace_bytes(MAX_ROWS_PER_FORWARD), dtype=torch.uint8, device=dev)
    ld = drafts[0]._probs.stride(0)
    r_const = reseed_uniforms(random_seed, W * gamma, dev) if on_dev else None
    Tk, Kk, Pk = float(temperature), int(top_k or 0), float(top_p or 0.0)
    native = _takes_native_loop(noise, verbose)
    if not native:                                   # the Python loop's own buffers and tables
        n_err = 2 * gamma + (gamma + 1)              # draft norm / draft sample / target norm words per replica
        err = torch.zeros((W, n_err), dtype=torch.int32, device=dev)
        res_dev = torch.zeros(C.sizeof(SdMultiResult), dtype=torch.uint8, device=dev)
        res_host = torch.zeros(C.sizeof(SdMultiResult), dtype=torch.uint8).pin_memory()
        err_host = torch.zeros((W, n_err), dtype=torch.int32).pin_memory()
        q_ptr = [m._probs.data_ptr() for m in drafts]
        p_ptr = [m._probs.data_ptr() for m in targets]
        seq_ptr = [s.data_ptr() for s in seqs]
        ld_bytes = ld * 4
        err_ptr = err.data_ptr()
        cu = _stream()
        items = (SdMultiItem * W)()
        for w in range(W):
            items[w].p_hist, items[w].q_hist, items[w].seq = p_ptr[w], q_ptr[w], seq_ptr[w]
        res_mode = target_m.norm_mode if target_m.norm_mode == draft_m.norm_mode else 0

    acc_len, acc_rate = [], []
    approx_time = target_time = other_time = 0
    approx_calls = target_calls = 0
    out = host
    try:
        if len(host) < T:
            check_token_ids(host, V)                                   # nn.Embedding's IndexError, swallowed below
        if native and len(host) < T:
            run = _MultiRun(drafts, targets, seqs, T, gamma, eos_token_id, ori_eos, random_seed, (Tk, Kk, Pk), norm_ws, r_const)
            res = _native_multi_loop(run, host, draft_len, noise, details)
            out, acc_len, acc_rate, approx_calls, target_calls = res.tokens, res.acc_len, res.acc_rate, res.calls, res.calls
            approx_time, target_time, other_time = res.approx_time, res.target_time, res.other_time
            _check_native(res.rc)
            raise_loop_error(res.err)
            out = cut_after_new_eos(out, eos_token_id, ori_eos)        # EOS rule (:1688-1695)
        while not native and len(host) < T:
            L = len(host)
            tt = process_time_ns()
            d_lo, t_lo = draft_len, target_len
            # ---- gamma draft steps, all replicas per pass (kvcache_model.py:279-293 with multi = width)
            for i in range(gamma):
                n_new = L + i - draft_len
                for s in d_ses:
                    s.cache_len = draft_len
                logits = batch_forward(d_ses, seqs, [n_new] * W, [1] * W)
                if on_dev:
                    e_base, seed, draw0 = 0, noise.seed, noise.next_draws(W)
                else:
                    e = noise.exponential_rows(W, V, draft_m.probs_dtype)   # ONE (width, V) draw, like torch.multinomial
                    e_base, seed, draw0 = e.data_ptr(), 0, 0
                rows = (SdNormRow * W)()
                for w in range(W):
                    rows[w].probs_out = q_ptr[w] + (L + i - 1) * ld_bytes
                    rows[w].err = err_ptr + 4 * (w * n_err + i)
                    rows[w].exp_noise = (e_base + w * V * 4) if e_base else None
                    rows[w].philox_seed = seed
                    rows[w].draw_index = draw0 + w
                    rows[w].tok_out = seq_ptr[w] + 4 * (L + i)
                    rows[w].sample_err = err_ptr + 4 * (w * n_err + gamma + i)
                check(lib.sd_norm_batch(logits.data_ptr(), W, V, logits.stride(0), Tk, Kk, Pk, draft_m.norm_mode, rows, 1,
                                        norm_ws.data_ptr(), cu), "sd_norm_batch")
                draft_len = L + i
            approx_calls += 1
            approx_time += process_time_ns() - tt
            tt = process_time_ns()
            # ---- target over every replica's uncached rows (speculative_sampling.py:1560), <= max_pass_rows per pass
            n_new = L + gamma - target_len
            per_pass = max(1, t_ses[0].max_pass_rows // n_new)
            for a in range(0, W, per_pass):
                grp = list(range(a, min(W, a + per_pass)))
                for w in grp:
                    t_ses[w].cache_len = target_len
                logits = batch_forward([t_ses[w] for w in grp], [seqs[w] for w in grp], [n_new] * len(grp),
                                       [n_new] * len(grp))
                rows = (SdNormRow * (len(grp) * n_new))()
                k = 0
                for w in grp:
                    for r_ in range(n_new):
                        pos = L + gamma - n_new + r_
                        rows[k].probs_out = p_ptr[w] + pos * ld_bytes
                        rows[k].err = err_ptr + 4 * (w * n_err + 2 * gamma + min(r_, gamma))
                        k += 1
                check(lib.sd_norm_batch(logits.data_ptr(), k, V, logits.stride(0), Tk, Kk, Pk, target_m.norm_mode, rows, 0,
                                        norm_ws.data_ptr(), cu), "sd_norm_batch")
            # the target's own sample, drawn and thrown away by the reference (kvcache_model.py:283)
            if on_dev:
                noise.next_draws(W)
            else:
                noise.skip_exponential_rows(W, V, target_m.probs_dtype)
            target_calls += 1
            target_time += process_time_ns() - tt
            tt = process_time_ns()
            # ---- replica scan
            token = None
            if on_dev:
                if random_seed:
                    noise.reseed(random_seed)
                r_ptr, seed, draw = (r_const.data_ptr() if r_const is not None else None), noise.seed, \
                    noise.next_draws(W * gamma)
            else:
                r, token = noise.uniforms(W * gamma, random_seed)
                r_ptr, seed, draw = r.data_ptr(), 0, 0
            check(lib.sd_accept_multi(items, W, ld, L, gamma, r_ptr, seed, draw, res_dev.data_ptr(), cu),
                  "sd_accept_multi")
            res_host.copy_(res_dev, non_blocking=True)
            err_host.copy_(err, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            eh = err_host.numpy()
            if eh.any():
                if eh[:, gamma:2 * gamma].any():
                    raise RuntimeError("prob error")                   # reference utils.py:224
                raise RuntimeError("norm logits error")                # reference utils.py:207
            res = SdMultiResult.from_buffer_copy(res_host.numpy().tobytes())
            if not on_dev:
                noise.realign(token, res.n_uniform)
            choice, l, n = res.choice, res.chosen.n_accepted, res.chosen.n
            all_accept = bool(res.chosen.flags & 4)
            pa = np.ctypeslib.as_array(res.p_at).reshape(16, 16)[:W, :gamma].astype(np.float32)
            qa = np.ctypeslib.as_array(res.q_at).reshape(16, 16)[:W, :gamma].astype(np.float32)
            acc_rate.extend(accept_rates_f32_zero_q(pa, qa))           # replica by replica
            acc_len.append(l)
            # ---- residual / bonus sample on the winner's rows (:1645-1679)
            if on_dev:
                e_ptr, seed, draw = None, noise.seed, noise.next_draws(1)
            else:
                e1 = noise.exponential(V, target_m.probs_dtype if res_mode else torch.float32)
                e_ptr, seed, draw = e1.data_ptr(), 0, 0
            check(lib.sd_multi_resample(p_ptr[choice], q_ptr[choice], ld, V, seq_ptr[choice], gamma, e_ptr, seed, draw,
                                        res_dev.data_ptr(), res_mode, cu), "sd_multi_resample")
            res_host.copy_(res_dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            res = SdMultiResult.from_buffer_copy(res_host.numpy().tobytes())
            if res.chosen.flags & 2:
                out = host + [int(res.chosen.drafted[i]) for i in range(l)]    # output_prefix was already cut (:1641)
                raise RuntimeError("prob error")
            t = res.chosen.next_token
            host = host + [int(res.chosen.drafted[i]) for i in range(l)] + [int(t)]
            # ---- everyone continues from the winner: rollback(n+1 | n+2, choice) + the next forward's repeat()
            new_draft = min(L + gamma - 1, n + 1)
            new_target = L + gamma if all_accept else n + 1
            for w in range(W):
                if w != choice:
                    seqs[w][L:n + 2].copy_(seqs[choice][L:n + 2])
                    _copy_positions(d_ses[w], d_ses[choice], d_lo, new_draft)
                    _copy_positions(t_ses[w], t_ses[choice], t_lo, new_target)
            draft_len, target_len = new_draft, new_target
            other_time += process_time_ns() - tt
            out = cut_after_new_eos(host, eos_token_id, ori_eos)       # EOS rule (:1688-1695)
            if out is not host:                                        # a new EOS was produced
                break
    except SpecDecError:                                               # an engine failure is never swallowed
        raise
    except (RuntimeError, IndexError) as e:                            # 'norm logits error' / 'prob error' / a bad token id:
        print(e)                                                       # printed and swallowed like the reference (:1689-1690)

    result = torch.tensor([out], dtype=torch.int64, device=prefix.device)
    if verbose:
        print("approx model time", approx_time / 1e9)
        print("target model time", target_time / 1e9)
        print("other time", other_time / 1e9)
        print("acc len", np.mean(acc_len) if acc_len else 0.0, len(acc_len), acc_len)
    if details:
        return result, details_dict(approx_time, target_time, other_time, acc_len, np.mean(acc_rate) if acc_rate else 0.0,
                                    target_calls, approx_calls)
    return result
