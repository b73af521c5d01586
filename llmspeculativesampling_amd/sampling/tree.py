"""Token-tree speculative sampling: one target pass verifies a TREE of draft tokens, losslessly.

Every other loop of this package spends a target pass on a chain of gamma draft tokens.  Here the draft grows a tree of
shape ``branching = (b_1, .., b_D)`` below the last emitted token - every node of level d - 1 gets ``b_d`` children drawn
WITHOUT replacement from the draft's distribution there (``sd_tree_draw``) - level by level without forwarding a node twice
(``sd_session_forward_tree_from``), the target scores all nodes in one tree forward, and one launch walks the tree with the
recursive rejection rule (``sd_tree_accept``): a rejected child's mass leaves both working distributions before the next
sibling is tried, so the emitted tokens are distributed exactly as the target's own sampling (SpecInfer's multi-step
verification; recursive speculative decoding's without-replacement draw).  DESIGN.md, "Token-tree speculative sampling", has
the method, the noise order and the arena invariant; the loop runs inside libspecdec (``sd_tree_generate``).  Device Philox only.
"""
from __future__ import annotations

import ctypes as C
from time import process_time_ns

import numpy as np
import torch

from .._lib import SD_TREE_MAX_BRANCH, SD_TREE_MAX_NODES, SdTreeResult, SdTreeStream, check, lib
from ..engine import _stream, as_specdec_model, check_token_ids, same_device
from ..noise import DeviceNoise
from ._loop_common import (LoopLog, cut_after_new_eos, details_dict, device_rng, make_noise, raise_loop_error, sampling_block,
                           spec_scratch)

REQUEST_OPTIONS = ("logprobs", "repetition_penalty", "frequency_penalty", "presence_penalty", "logit_bias", "allowed_token_ids",
                   "banned_token_ids", "min_tokens", "grammar")


def tree_nodes(branching) -> int:
    """Nodes of a tree of shape ``branching`` (the root included); ValueError for a shape the kernels do not take: depth 0,
    a factor outside 1..8, more than 64 nodes."""
    try:
        bs = list(branching)
    except TypeError:
        raise ValueError(f"branching: a tuple of child counts per level is required, not {branching!r}") from None
    if not bs:
        raise ValueError("branching: at least one level is required (depth 0)")
    n = width = 1
    for d, b in enumerate(bs, 1):
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= b <= SD_TREE_MAX_BRANCH:
            raise ValueError(f"branching: level {d}: 1..{SD_TREE_MAX_BRANCH} children per node, not {b!r}")
        width *= int(b)
        n += width
        if n > SD_TREE_MAX_NODES:
            raise ValueError(f"branching: {tuple(bs)} has more than {SD_TREE_MAX_NODES} nodes")
    return n


def _check_arguments(target_model, approx_model, branching, temperature, rng, options) -> int:
    """What the call refuses with ValueError before a model is touched; returns the node count."""
    n = tree_nodes(branching)
    if rng is not None and not device_rng(rng):
        raise ValueError('tree_speculative_sampling runs on the device RNG only: rng="device" (or a device noise object), '
                         "not a host-noise provider")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or float(temperature) == 0.0:
        raise ValueError(f"temperature: a non-zero number is required, not {temperature!r}")
    for name in options:
        what = "a request option of the chain loops" if name in REQUEST_OPTIONS else "not an argument"
        raise ValueError(f"{name}: {what}; tree_speculative_sampling does not take it (penalties, logit edits, grammars and "
                         "logprobs are served by speculative_sampling)")
    for m in (approx_model, target_model):
        if getattr(m, "tp_group", None) is not None:
            raise ValueError("tree_speculative_sampling is not available with a tensor-parallel model")
        if getattr(m, "kv_dtype", None) is not None:
            raise ValueError("tree_speculative_sampling is not available with an fp8 KV arena")
    return n


@torch.no_grad()
def tree_speculative_sampling(prefix: torch.Tensor, approx_model, target_model, eos_token_id, pad_token_id, max_len: int,
                              branching=(3, 2, 1), temperature: float = 1, top_k: int = 0, top_p: float = 0,
                              random_seed: int = None, details: bool = False, *, rng=None, **request_options):
    """Speculative decoding over a draft token tree; the output is distributed as ``autoregressive_sampling``'s.

    ``branching``: child slots per node, level by level; at most 8 per node and 64 nodes with the root
    (``(1,) * gamma`` is a chain).  ``rng``: None or "device" (Philox seeded with ``random_seed``, else ``torch.initial_seed()``)
    or a device noise object; a host-noise provider is refused.  Output conventions, the EOS cut, the exceptions and the
    ``details`` keys (``acc_len``: accepted depth per iteration, ``target_call_times``, ``approx_call_times``, ...) are
    ``speculative_sampling``'s; ``acc_rate`` is the mean accepted depth over the tree's depth.  One function serves one
    stream: the batch and queue forms, request options, tensor-parallel models and fp8 KV arenas are refused with ValueError
    before a model is touched, as are a ``branching`` of depth 0, a factor outside 1..8 or more than 64 nodes.
    """
    n_nodes = _check_arguments(target_model, approx_model, branching, temperature, rng, request_options)
    assert prefix.shape[0] == 1, "input batch size must be 1 (the batch and queue forms are not built)"
    draft_m, target_m = as_specdec_model(approx_model), as_specdec_model(target_model)
    if draft_m.cfg.is_encoder_decoder or target_m.cfg.is_encoder_decoder:
        raise NotImplementedError("encoder-decoder models are out of scope")
    same_device(draft_m, target_m)
    dev = target_m.device
    V = target_m.cfg.vocab_size
    assert draft_m.cfg.vocab_size == V, "draft and target must share a vocabulary"
    shape = [int(b) for b in branching]
    D = len(shape)
    L0 = prefix.shape[1]
    T = L0 + max_len
    host = [int(t) for t in prefix[0].tolist()]
    if L0 >= T:
        out = torch.tensor([host], dtype=torch.int64, device=prefix.device)
        return (out, details_dict(0, 0, 0, [], 0.0, 0, 0)) if details else out
    try:
        check_token_ids(host, V)
    except IndexError as e:
        print(e)
        raise RuntimeError("s") from e
    noise = DeviceNoise(seed=int(random_seed if random_seed is not None else torch.initial_seed())) if rng is None \
        else make_noise(rng, dev)
    ori_eos = host.count(eos_token_id)

    cap = T + D + n_nodes + 2
    d_ses, t_ses = draft_m.new_session(cap), target_m.new_session(cap)
    tok32 = prefix[0].to(device=dev, dtype=torch.int32)
    if L0 > 1:                                                          # the prompt but its last token: the root is a tree row
        d_ses.forward(tok32[:L0 - 1], 0)
        t_ses.forward(tok32[:L0 - 1], 0)
    ld = (V + 3) // 4 * 4
    tokens = torch.full((SD_TREE_MAX_NODES,), -1, dtype=torch.int32, device=dev)
    tokens[0] = tok32[L0 - 1]
    q_rows = torch.empty((SD_TREE_MAX_NODES, ld), dtype=torch.float32, device=dev)
    p_rows = torch.empty((SD_TREE_MAX_NODES, ld), dtype=torch.float32, device=dev)
    work = torch.empty(2 * V, dtype=torch.float32, device=dev)
    err = torch.zeros(2 * SD_TREE_MAX_NODES, dtype=torch.int32, device=dev)
    path = torch.zeros(SD_TREE_MAX_NODES, dtype=torch.int32, device=dev)
    res_dev = torch.zeros(C.sizeof(SdTreeResult), dtype=torch.uint8, device=dev)
    res_host = torch.zeros(C.sizeof(SdTreeResult), dtype=torch.uint8).pin_memory()
    norm_ws = torch.empty(lib.sd_norm_workspace_bytes(SD_TREE_MAX_NODES), dtype=torch.uint8, device=dev)
    stream = SdTreeStream(d_ses.handle, t_ses.handle, tokens.data_ptr(), q_rows.data_ptr(), p_rows.data_ptr(), work.data_ptr(),
                          err.data_ptr(), path.data_ptr(), res_dev.data_ptr(), res_host.data_ptr())
    max_iters = max(1, T - L0)
    log = LoopLog(host, T + D + 2, max_iters, 1, q_fill=1.0, timed=details)
    st = log.seq_state(L0, T, ori_eos, (L0 - 1, L0 - 1), noise, max_iters)
    st.p_at_out = st.q_at_out = None
    tick = process_time_ns()
    rc = lib.sd_tree_generate(stream, (C.c_int32 * D)(*shape), D, sampling_block(temperature, top_k, top_p, V, ld, eos_token_id),
                              spec_scratch(d_ses, t_ses, norm_ws, SD_TREE_MAX_NODES), st, _stream())
    other_time = process_time_ns() - tick
    noise.seed, noise.draw = st.seed, st.draw
    d_ses.cache_len, t_ses.cache_len = st.draft_len, st.target_len
    check(rc, "sd_tree_generate")
    try:
        raise_loop_error(st.err)
    except RuntimeError as e:                                           # (speculative_sampling.py:2044-2046)
        print(e)
        raise RuntimeError("s") from e
    calls = st.n_iters
    out_tokens = cut_after_new_eos(log.tokens(st.len), eos_token_id, ori_eos)
    out = torch.tensor([out_tokens], dtype=torch.int64, device=prefix.device)
    if details:
        acc_len = log.acc_len(calls)
        approx_time, target_time = log.phase_ns(calls)
        return out, details_dict(approx_time, target_time, other_time, acc_len, float(np.mean(acc_len)) / D if acc_len else 0.0,
                                 calls, calls, target_model_time=target_time, target_pre_cache_time=0, target_post_prob_time=0)
    return out
