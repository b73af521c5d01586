"""sd_loop_opts, the native loops' optional block: what needs no GPU - the members are refused behind the entry's own refusals,
in the members' order (row_params, logprobs, penalties, edits), under the name of the entry that was called, before anything is
written or launched; a NULL block and a block of four NULLs are one call; the Python helper that builds the block.  The lock-step
batch entry reaches the block on placeholder pointers (its own refusals read no session), so it carries the order.  (The layout
and the entries' argument lists: test_abi_cpu.py; the two loops that refuse row_params read their sessions first:
test_gpu_row_sampling.py.)"""
import ctypes as C

import torch

from llmspeculativesampling_amd import _lib
from llmspeculativesampling_amd.sampling import _loop_common as LC

P = 0x1000                                                        # a placeholder pointer: every refusal comes before any use
GAMMA = 4


def _batch(opts, gamma=GAMMA):
    """sd_spec_batch_generate on one placeholder stream -> (status, message, what the log holds afterwards)."""
    head = _lib.SdHeadScratch(logits=P, ld_logits=128, norm_mode=0)
    sampling = _lib.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=128, ld=128, eos_token_id=2)
    scratch = _lib.SdSpecScratch(draft=head, target=head, norm_workspace=None, max_rows_per_forward=64)
    log = _lib.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7)
    streams = (_lib.SdBatchStream * 1)()
    rc = _lib.lib.sd_spec_batch_generate(streams, 1, gamma, sampling, 0, None, scratch, log, None, opts)
    return rc, _lib.lib.sd_last_error().decode(), (log.n_iters, log.err)


def _refused(opts, text, **kw):
    rc, msg, log = _batch(opts, **kw)
    assert rc == _lib.SD_ERR_INVALID and msg.startswith("sd_spec_batch_generate: ") and text in msg, msg
    assert log == (-7, -7)                                        # nothing was written, nothing ran


def test_members_are_refused_in_their_order_under_the_called_entry_s_name():
    """A block that is wrong in every member is refused for the first; mended member by member, for the next."""
    keep = []                                                     # (the arrays the blocks point to)

    def array(t, *items):
        keep.append((t * len(items))(*items))
        return keep[-1]
    outs = array(C.c_void_p, P)
    rows = lambda T, k: array(_lib.SdRowSampling, _lib.SdRowSampling(T, k, 0.9))
    lp_bad, lp_ok = _lib.SdLogprobBlock(P, None, outs), _lib.SdLogprobBlock(P, P, outs)
    pens = lambda r: array(_lib.SdPenalty, _lib.SdPenalty(r, 0.0, 0.5))
    pb_bad, pb_ok = _lib.SdPenaltyBlock(P, 127, 64, pens(1.0)), _lib.SdPenaltyBlock(P, 128, 64, pens(1.0))
    eb_bad = _lib.SdLogitEditBlock(P, 128, GAMMA, array(_lib.SdLogitEdit, _lib.SdLogitEdit(None, None, 0, None, 3)))   # one row short
    opts = lambda rp, lp, pb, eb: _lib.SdLoopOpts(rp, C.pointer(lp), C.pointer(pb), C.pointer(eb))
    _refused(opts(rows(0.0, 20), lp_bad, pb_bad, eb_bad), "stream 0: temperature must be non-zero")
    _refused(opts(rows(1.0, -1), lp_bad, pb_bad, eb_bad), "stream 0: top_k -1 is negative")
    _refused(opts(rows(1.0, 20), lp_bad, pb_bad, eb_bad), "logprobs: null pointer")
    _refused(opts(None, lp_bad, pb_bad, eb_bad), "logprobs: null pointer")
    _refused(opts(None, _lib.SdLogprobBlock(P, P, array(C.c_void_p, None)), pb_bad, eb_bad), "logprobs: logprob_out[0] is null")
    _refused(opts(rows(1.0, 20), lp_ok, pb_bad, eb_bad), "penalties: ld 127 < V 128")
    _refused(_lib.SdLoopOpts(None, None, C.pointer(pb_bad), C.pointer(eb_bad)), "penalties: ld 127 < V 128")
    _refused(opts(None, lp_ok, _lib.SdPenaltyBlock(P, 128, 64, pens(0.0)), eb_bad), "stream 0: repetition penalty 0 must be > 0")
    _refused(opts(rows(1.0, 20), lp_ok, pb_ok, eb_bad), f"edits: a slab of {GAMMA} rows, the largest pass has {GAMMA + 1}")
    _refused(_lib.SdLoopOpts(edits=C.pointer(eb_bad)), f"edits: a slab of {GAMMA} rows")
    # the entry's own refusals come first, whatever the block holds
    _refused(opts(rows(0.0, 20), lp_bad, pb_bad, eb_bad), "bad arguments", gamma=17)


def test_a_null_block_and_a_block_of_four_nulls_are_one_call():
    for opts in (None, _lib.SdLoopOpts()):
        _refused(opts, "bad arguments", gamma=0)
    # ... also behind the entry's own refusals: the queue's last one names a slot's sessions
    head = _lib.SdHeadScratch(logits=P, ld_logits=128, norm_mode=0)
    sampling = _lib.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=128, ld=128, eos_token_id=2)
    scratch = _lib.SdSpecScratch(draft=head, target=head, norm_workspace=None, max_rows_per_forward=64)
    log = _lib.SdLockstepLog(max_iters_log=0, n_iters=-7, err=-7)
    slots, prompts = (_lib.SdBatchStream * 2)(), (_lib.SdQueuePrompt * 2)()
    said = []
    for opts in (None, _lib.SdLoopOpts(), _lib.SdLoopOpts(logprobs=C.pointer(_lib.SdLogprobBlock()))):
        assert _lib.lib.sd_spec_queue_generate(slots, 2, 64, prompts, 2, 0, GAMMA, sampling, 0, None, scratch, log, None, None, None,
                                               None, 0, opts) == _lib.SD_ERR_INVALID
        said.append(_lib.lib.sd_last_error().decode())
    assert said == ["sd_spec_queue_generate: slot 0: null pointer"] * 3 and (log.n_iters, log.err) == (-7, -7)


def test_the_helper_builds_null_for_nothing_and_keeps_its_array_alive(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    assert LC.loop_opts() is None and LC.loop_opts(None, None, None, None) is None
    triples = [(1.0, 20, 0.9), (0.7, 0, 0.0)]
    o = LC.loop_opts(triples)
    assert isinstance(o, _lib.SdLoopOpts) and not o.logprobs and not o.penalties and not o.edits
    assert [(r.top_k, round(r.temperature, 6)) for r in o.row_params[:2]] == [(20, 1.0), (0, 0.7)]
    lp = LC.LogprobBlock("cpu", [8, 8])
    pb = LC.PenaltyBlock("cpu", [(1.2, 0.0, 0.0)] * 2, 64, 5)
    o = LC.loop_opts(None, lp, pb)
    assert not o.row_params and not o.edits
    assert C.addressof(o.logprobs.contents) == C.addressof(lp.block) and C.addressof(o.penalties.contents) == C.addressof(pb.block)
    assert o.penalties.contents.max_rows == 5 and o.penalties.contents.ld == 64
