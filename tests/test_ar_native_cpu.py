"""Host-side checks of the native autoregressive loop (sd_ar_batch_generate): ABI of the two entry points and of
sd_ar_stream, the size of the hand-off block, argument refusal before any launch, and which loop autoregressive_sampling
takes.  No GPU needed."""
import ctypes as C
import inspect
import re

import pytest


def test_ar_symbols_are_exported_and_declared():
    """(Argument counts and classes against the header: test_abi_cpu.py.)"""
    from llmspeculativesampling_amd import _lib
    bound, raw = {n: res for n, res, _ in _lib.SYMBOLS}, C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "sd_ar_block_bytes") and hasattr(raw, "sd_ar_batch_generate")
    assert bound["sd_ar_block_bytes"] is C.c_size_t and bound["sd_ar_batch_generate"] is C.c_int


def test_ar_stream_layout_matches_the_header():
    from llmspeculativesampling_amd import _lib
    assert [f for f, _ in _lib.SdArStream._fields_] == ["session", "seq", "probs", "err_words", "host_seq", "len", "T", "cache_len",
                                                       "seed", "draw", "done", "steps"]
    assert C.sizeof(_lib.SdArStream) == 80


def test_ar_block_bytes():
    """8 bytes per stream ({int32 token, int32 flags}), rounded up to a multiple of 16; 0 outside 1..16 streams."""
    from llmspeculativesampling_amd import _lib
    for n in range(1, 17):
        assert _lib.lib.sd_ar_block_bytes(n) == (8 * n + 15) // 16 * 16
    assert [_lib.lib.sd_ar_block_bytes(n) for n in (-1, 0, 17)] == [0, 0, 0]


def _call(lib, table, n, log, without="", opts=None):
    """sd_ar_batch_generate on placeholder buffers; ``without`` names a block to hand over as NULL."""
    from llmspeculativesampling_amd import _lib
    p = C.addressof((C.c_char * 256)())
    sampling = _lib.SdSampling(temperature=1.0, top_k=20, top_p=0.9, V=128, ld=128, eos_token_id=2)
    head = _lib.SdHeadScratch(logits=None if without == "logits" else p, ld_logits=128, norm_mode=0)
    block = None if without == "block" else p
    return lib.sd_ar_batch_generate(table, n, None if without == "sampling" else sampling, None if without == "head" else head,
                                    None, block, block, None if without == "log" else log, None, opts)


def test_ar_generate_refuses_bad_arguments_before_any_launch():
    from llmspeculativesampling_amd import _lib
    lib = _lib.lib
    log = _lib.SdArLog(n_steps=-7, err=-7)
    table = (_lib.SdArStream * 16)()
    for n in (0, 17, -1):
        assert _call(lib, table, n, log) == _lib.SD_ERR_INVALID
        assert re.search(r"n_streams -?\d+ outside 1\.\.16", lib.sd_last_error().decode())
    assert _call(lib, None, 2, log) == _lib.SD_ERR_INVALID and b"sd_ar_batch_generate: null" in lib.sd_last_error()
    for block in ("sampling", "head", "logits", "block", "log"):
        assert _call(lib, table, 2, log, without=block) == _lib.SD_ERR_INVALID
        assert b"sd_ar_batch_generate: null" in lib.sd_last_error()
    # a table entry without its pointers
    assert _call(lib, table, 1, log) == _lib.SD_ERR_INVALID and b"stream 0: null pointer" in lib.sd_last_error()
    # two streams, the second not prefilled up to its last token (placeholder pointers: the refusal comes before any use)
    for it in table[:2]:
        it.session = it.seq = it.probs = it.err_words = it.host_seq = 0x1000
        it.len, it.T, it.cache_len = 9, 12, 8
    table[1].cache_len = 5
    assert _call(lib, table, 2, log) == _lib.SD_ERR_INVALID
    assert b"stream 1" in lib.sd_last_error() and b"prefilled" in lib.sd_last_error()
    table[1].cache_len = 9                                        # a cache longer than the sequence
    assert _call(lib, table, 2, log) == _lib.SD_ERR_INVALID and b"stream 1: cache_len 9 of 9" in lib.sd_last_error()
    # the entry's own refusals come before anything in opts, and an empty block is a NULL one
    bad = _lib.SdLoopOpts(row_params=(_lib.SdRowSampling * 2)(), penalties=C.pointer(_lib.SdPenaltyBlock()))
    for opts in (bad, _lib.SdLoopOpts()):
        assert _call(lib, table, 2, log, opts=opts) == _lib.SD_ERR_INVALID and b"stream 1: cache_len 9 of 9" in lib.sd_last_error()
        assert _call(lib, table, 17, log, opts=opts) == _lib.SD_ERR_INVALID and b"n_streams 17 outside" in lib.sd_last_error()
    assert (log.n_steps, log.err) == (-7, -7)                     # nothing was written, nothing ran
    with pytest.raises(ValueError, match="sd_ar_batch_generate"):
        _lib.check(_lib.SD_ERR_INVALID, "sd_ar_batch_generate")


def test_python_entry_points():
    import llmspeculativesampling_amd.sampling as S
    from llmspeculativesampling_amd.sampling.autoregressive_sampling import ArRun
    assert callable(S.autoregressive_sampling_batch) and "autoregressive_sampling_batch" in S.__all__
    sig = inspect.signature(S.autoregressive_sampling)
    assert sig.parameters["_native"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["_native"].default is True
    sig = inspect.signature(S.autoregressive_sampling_batch)
    assert list(sig.parameters)[:8] == ["xs", "model", "N", "eos_token_id", "temperature", "top_k", "top_p", "pad_token_id"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seeds", "_timing"))
    for n in (0, 17):                                             # refused before a model or a GPU is touched
        with pytest.raises(ValueError, match="1..16 streams"):
            S.autoregressive_sampling_batch([None] * n, None, 4, 2)
    run = ArRun(None, 1, 0, 0, None)
    assert run.eos == -1 and run.args == (1.0, 0, 0.0)
    with pytest.raises(ValueError, match="1..16 streams"):
        run.generate()
