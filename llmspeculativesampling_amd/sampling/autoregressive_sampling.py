"""Drop-in for reference sampling/autoregressive_sampling.py:8-61 (``autoregressive_sampling``)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .._lib import lib, check, SdArLog, SdArStream
from ..engine import as_specdec_model, _stream, check_token_ids
from ._loop_common import (RequestOptions, device_rng, head_scratch, loop_opts, make_noise, open_stream, raise_loop_error,
                           sampling_block, slab_rows)
from .kvcache_model import KVCacheModel


@torch.no_grad()
def autoregressive_sampling(x: torch.Tensor, model, N: int, eos_token_id: int, temperature: float = 1,
                            top_k: int = 0, top_p: float = 0, pad_token_id=None, *, rng=None, _native: bool = True,
                            logprobs: bool = False, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0,
                            presence_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
                            min_tokens=0, grammar=None):
    """reference autoregressive_sampling.py:9-61: exactly N tokens unless EOS is drawn (the EOS is kept).
    RNG contract: one ``sample`` per token.  With the device RNG the whole loop is one native call
    (sd_ar_batch_generate with one stream); ``_native=False`` keeps the interpreter loop below, which the host RNG
    and ReplayNoise always take (same tokens, same exceptions).
    ``logprobs`` (native loop only): returns ``(tokens, logprobs)``, a float32 tensor (1, len(tokens) - len(x)) with the
    model's log-probability of every new token - ``log_softmax`` in fp32 of the raw logit row it was sampled from, taken
    before temperature, top_k and top_p: what the model says, not what the sampler drew from.
    ``repetition_penalty`` / ``frequency_penalty`` / ``presence_penalty`` (native loop only; neutral 1 / 0 / 0): every logit row
    is edited on the device by its own history before it is normalised (``sampling.utils.apply_penalties``); ``logprobs`` stay
    what the model says.
    ``logit_bias`` / ``allowed_token_ids`` / ``banned_token_ids`` / ``min_tokens`` (native loop only; neutral None / None / None
    / 0): behind the penalties a ``{token id: bias}`` mapping is added, ids outside the allowed list or inside the banned list
    become -inf, and so does ``eos_token_id`` until ``min_tokens`` tokens have been produced
    (``sampling.utils.apply_logit_edits``).
    ``grammar`` (native loop only; a ``sampling.grammar.TokenGrammar`` or None): behind the edits every logit row is masked by
    the automaton state its output prefix leads to (``sampling.utils.apply_grammar``); the state advances on the device."""
    opts = RequestOptions.parse(1, "stream", eos_token_id, logprobs=logprobs,
                                penalties=(repetition_penalty, frequency_penalty, presence_penalty),
                                edits=(logit_bias, allowed_token_ids, banned_token_ids, min_tokens), grammar=grammar)
    opts.require_native(_native and device_rng(rng), ", not _native=False")
    opts.require_target_rows(model)
    assert x.shape[0] == 1
    m = as_specdec_model(model)
    dev = m.device
    V = m.cfg.vocab_size
    opts.bind(V)
    L0 = x.shape[1]
    check_token_ids(x, V)
    noise = make_noise(rng, dev)
    kv, seq32 = open_stream(m, x[0], L0 + N + 1, L0 + N + 1, temperature, top_k, top_p, noise)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    if _native and getattr(noise, "on_device", False):
        run = ArRun(m, temperature, top_k, top_p, eos_token_id)
        run.add(kv, seq32, x[0].to(device="cpu", dtype=torch.int32).numpy(), L0 + N, noise)
        run.generate(logprobs=logprobs, penalties=opts.penalties, edits=opts.edits, grammars=opts.grammar)
        out = torch.from_numpy(run.tokens(0)).to(torch.int64).unsqueeze(0).to(x.device)
        return (out, run.logprobs(0, x.device)) if logprobs else out
    n_out = 0
    # the EOS test needs each token on the host (autoregressive_sampling.py:55): one 4-byte read per step
    for i in range(N):
        S = L0 + i
        kv.forward_sample(seq32, S, noise, err)
        n_out += 1
        tok = int(seq32[S])
        kv.check_errors(S - 1, S)         # first, as the reference normalises before it samples (a NaN row sets both words)
        if int(err) != 0:
            raise RuntimeError("prob error")
        if tok == eos_token_id:
            break
    return seq32[:L0 + n_out].to(torch.int64).unsqueeze(0).to(x.device)


@dataclass
class _ArStream:
    kv: KVCacheModel
    seq32: torch.Tensor
    host: np.ndarray             # the host token buffer, T + 1 long
    err: torch.Tensor
    noise: object
    L: int
    T: int


class ArRun:
    """One call of sd_ar_batch_generate: the streams' table, the host token buffers and the 8-byte-per-stream hand-off
    blocks; shared by autoregressive_sampling (one stream) and sampling.batch.autoregressive_sampling_batch."""

    def __init__(self, model, temperature, top_k, top_p, eos_token_id):
        self.m = model
        self.args = (float(temperature), int(top_k or 0), float(top_p or 0.0))
        self.eos = -1 if eos_token_id is None else int(eos_token_id)
        self.streams = []                                         # _ArStream per add()
        self.steps = []                                           # (ms, n_streams) per step, filled by generate(timing=True)

    def add(self, kv: KVCacheModel, seq32: torch.Tensor, prompt: np.ndarray, T: int, noise) -> None:
        """A stream whose session holds ``kv.cache_len`` of the ``len(prompt)`` tokens in seq32 and is to reach T tokens."""
        host = np.zeros(T + 1, dtype=np.int32)
        host[:len(prompt)] = prompt
        err = torch.zeros(2, dtype=torch.int32, device=self.m.device)
        self.streams.append(_ArStream(kv, seq32, host, err, noise, len(prompt), int(T)))

    def generate(self, timing: bool = False, logprobs: bool = False, penalties=None, edits=None, grammars=None) -> None:
        """``penalties``: None, or one (repetition, frequency, presence) triple per stream (_loop_common.penalty_triples);
        ``edits``: None, or one record per stream (_loop_common.logit_edits); ``grammars``: None, or one TokenGrammar-or-None
        per stream (grammar.grammar_list) - ``self.grammar_states`` then holds each such stream's device state cache."""
        B = len(self.streams)
        if not 1 <= B <= 16:
            raise ValueError(f"autoregressive sampling takes 1..16 streams per call, not {B}")
        dev = self.m.device
        arr = (SdArStream * B)()
        for it, s in zip(arr, self.streams):
            it.session, it.seq, it.probs = s.kv._session.handle, s.seq32.data_ptr(), s.kv._probs.data_ptr()
            it.err_words, it.host_seq = s.err.data_ptr(), s.host.ctypes.data
            it.len, it.T, it.cache_len = s.L, s.T, s.kv._session.cache_len
            it.seed, it.draw = s.noise.seed, s.noise.draw
        nb = lib.sd_ar_block_bytes(B)
        dev_block = torch.zeros(nb, dtype=torch.uint8, device=dev)
        host_block = torch.zeros(nb, dtype=torch.uint8).pin_memory()
        kv0 = self.streams[0].kv
        norm_ws = kv0._norm_ws if B <= kv0._session.max_rows else None
        n_log = max(s.T - s.L for s in self.streams) if timing else 0
        ms = np.zeros(max(n_log, 1), dtype=np.float32)
        cnt = np.zeros(max(n_log, 1), dtype=np.int32)
        log = SdArLog(ms.ctypes.data if timing else None, cnt.ctypes.data if timing else None, n_log)
        args = (arr, B, sampling_block(*self.args, self.m.cfg.vocab_size, kv0._probs.stride(0), self.eos),
                head_scratch(kv0._session), norm_ws.data_ptr() if norm_ws is not None else None,
                dev_block.data_ptr(), host_block.data_ptr(), log, _stream())
        opts = RequestOptions(B, "stream", self.eos, None, logprobs, penalties, edits, grammars)
        with opts.attach(dev, self.m.cfg.vocab_size, slab_rows(ar_streams=B), [s.T + 1 for s in self.streams],
                         [s.kv._session for s in self.streams], [s.T - s.L + 2 for s in self.streams]) as blocks:
            self.blocks, self.grammar_states = blocks, blocks.grammar_states
            rc = lib.sd_ar_batch_generate(*args, loop_opts(*blocks.members))
        self.lens = []
        for it, s in zip(arr, self.streams):                      # the state the loop left, also after a failure
            s.kv._session.cache_len = it.cache_len
            s.noise.draw = it.draw
            self.lens.append(it.len)
        check(rc, "sd_ar_batch_generate")
        raise_loop_error(log.err)
        self.steps = [(float(ms[i]), int(cnt[i])) for i in range(min(log.n_steps, n_log))]

    def tokens(self, i: int) -> np.ndarray:
        return self.streams[i].host[:self.lens[i]]

    def logprobs(self, i: int, device) -> torch.Tensor:
        """generate(logprobs=True): the (1, new tokens) float32 scores of stream i."""
        return self.blocks.logprob_tensor(i, self.lens[i] - self.streams[i].L, device)
