"""Host-side checks of the native autoregressive loop (sd_ar_batch_generate): ABI of the two entry points and of
sd_ar_stream, the size of the hand-off block, argument refusal before any launch, and which loop autoregressive_sampling
takes.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sd_ar_block_bytes", "sd_ar_batch_generate"]


def _header():
    return open(os.path.join(ROOT, "include", "specdec.h")).read()


def _declared_arg_count(name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", _header(), re.S)
    assert m, name
    return len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])


def test_ar_symbols_are_exported_and_declared():
    from llmspeculativesampling_amd import _lib
    bound = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        fn = getattr(_lib.lib, name)
        res, args = bound[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
        assert len(args) == _declared_arg_count(name), name
    assert bound["sd_ar_block_bytes"][0] is C.c_size_t and bound["sd_ar_batch_generate"][0] is C.c_int


def test_ar_stream_layout_matches_the_header():
    """Field order and C types are read from the header's struct; offsets follow from the x86-64 rules (natural alignment)."""
    from llmspeculativesampling_amd import _lib
    body = re.search(r"typedef struct \{([^}]*)\}\s*sd_ar_stream;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []                                                   # (name, size)
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"((?:const\s+)?[A-Za-z_0-9]+)\s+(.*)", decl, re.S).groups()
        for nm in names.split(","):
            nm = nm.strip()
            ptr = nm.startswith("*")
            size = 8 if ptr else {"int32_t": 4, "int": 4, "uint64_t": 8, "float": 4}[ctype]
            fields.append((nm.lstrip("*").strip(), size))
    assert [f for f, _ in fields] == ["session", "seq", "probs", "err_words", "host_seq", "len", "T", "cache_len", "seed",
                                      "draw", "done", "steps"]
    assert [f for f, _ in _lib.SdArStream._fields_] == [f for f, _ in fields]
    off = 0
    for name, size in fields:
        off = (off + size - 1) // size * size
        d = getattr(_lib.SdArStream, name)
        assert (d.offset, d.size) == (off, size), name
        off += size
    assert C.sizeof(_lib.SdArStream) == (off + 7) // 8 * 8 == 80


def test_ar_block_bytes():
    """8 bytes per stream ({int32 token, int32 flags}), rounded up to a multiple of 16; 0 outside 1..16 streams."""
    from llmspeculativesampling_amd import _lib
    for n in range(1, 17):
        assert _lib.lib.sd_ar_block_bytes(n) == (8 * n + 15) // 16 * 16
    assert [_lib.lib.sd_ar_block_bytes(n) for n in (-1, 0, 17)] == [0, 0, 0]


def _call(lib, table, n, z):
    buf = (C.c_char * 256)()
    p = C.addressof(buf)
    return lib.sd_ar_batch_generate(table, n, 1.0, 20, 0.9, 128, 128, 2, 0, p, 128, None, p, p, None, None, 0, C.byref(z),
                                    C.byref(z), None)


def test_ar_generate_refuses_bad_arguments_before_any_launch():
    from llmspeculativesampling_amd import _lib
    lib = _lib.lib
    z = C.c_int(-7)
    table = (_lib.SdArStream * 16)()
    for n in (0, 17, -1):
        assert _call(lib, table, n, z) == _lib.SD_ERR_INVALID
        assert re.search(r"n_streams -?\d+ outside 1\.\.16", lib.sd_last_error().decode())
    assert _call(lib, None, 2, z) == _lib.SD_ERR_INVALID and b"sd_ar_batch_generate: null" in lib.sd_last_error()
    assert lib.sd_ar_batch_generate(table, 2, 1.0, 20, 0.9, 128, 128, 2, 0, None, 128, None, None, None, None, None, 0, None,
                                    None, None) == _lib.SD_ERR_INVALID
    # a table entry without its pointers
    assert _call(lib, table, 1, z) == _lib.SD_ERR_INVALID and b"stream 0: null pointer" in lib.sd_last_error()
    # two streams, the second not prefilled up to its last token (placeholder pointers: the refusal comes before any use)
    for it in table[:2]:
        it.session = it.seq = it.probs = it.err_words = it.host_seq = 0x1000
        it.len, it.T, it.cache_len = 9, 12, 8
    table[1].cache_len = 5
    assert _call(lib, table, 2, z) == _lib.SD_ERR_INVALID
    assert b"stream 1" in lib.sd_last_error() and b"prefilled" in lib.sd_last_error()
    table[1].cache_len = 9                                        # a cache longer than the sequence
    assert _call(lib, table, 2, z) == _lib.SD_ERR_INVALID and b"stream 1: cache_len 9 of 9" in lib.sd_last_error()
    assert z.value == -7                                          # nothing was written, nothing ran
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
