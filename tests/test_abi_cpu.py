"""The whole of include/specdec.h against the ctypes binding (_lib.SYMBOLS, _lib.C_STRUCTS) and the built library: every
prototype by return class, argument count and argument class, every struct by field order, offsets, sizes and sizeof.  No GPU."""
import ctypes as C

import abi_header
from llmspeculativesampling_amd import _lib

PROTOS, STRUCTS = abi_header.parse()


def test_every_declared_symbol_is_bound_and_exported():
    print(f"{len(PROTOS)} prototypes, {len(STRUCTS)} structs")
    assert len(PROTOS) >= 82 and len(STRUCTS) >= 24
    bound = [n for n, _, _ in _lib.SYMBOLS]
    assert len(bound) == len(set(bound)) and set(bound) == set(PROTOS), set(bound) ^ set(PROTOS)
    raw = C.CDLL(_lib.LIB_PATH)
    assert [n for n in PROTOS if not hasattr(raw, n)] == []


def test_every_prototype_matches_its_binding():
    for name, res, args in _lib.SYMBOLS:
        fn = getattr(_lib.lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert (abi_header.ctypes_class(res), [abi_header.ctypes_class(a) for a in args]) == PROTOS[name][:2], name
        for base, t in zip(PROTOS[name][2], args):                # a typed pointer names the struct the header names
            if base in _lib.C_STRUCTS and hasattr(t, "contents"):
                assert t._type_ is _lib.C_STRUCTS[base], (name, base)


def test_every_struct_matches_its_ctypes_class():
    assert set(_lib.C_STRUCTS) == set(STRUCTS), set(_lib.C_STRUCTS) ^ set(STRUCTS)
    for name, cls in _lib.C_STRUCTS.items():
        assert ([(f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_], C.sizeof(cls)) == STRUCTS[name], name


def test_spec_generate_takes_the_shared_blocks():
    """The single-stream loop is one call on the blocks the other loops take, plus the device side of its one stream."""
    assert not [n for n in PROTOS if n in ("sd_spec_create", "sd_spec_destroy", "sd_spec_timing", "sd_spec_last_times",
                                           "sd_spec_iteration")]
    assert PROTOS["sd_spec_generate"] == ("i32", ["ptr", "i32", "ptr", "ptr", "ptr", "u64", "ptr", "ptr", "ptr"],
                                          ["sd_spec_stream", "int", "sd_sampling", "sd_spec_scratch", "sd_seq_state", "uint64_t",
                                           "float", "void", "sd_loop_opts"])
    fields = ["draft", "target", "seq", "q_hist", "p_hist", "err_words", "res_dev", "res_host"]
    assert STRUCTS["sd_spec_stream"] == ([(f, 8 * i, 8) for i, f in enumerate(fields)], 64)
    assert C.sizeof(_lib.SdSpecStream) == 64 and [f for f, _ in _lib.SdSpecStream._fields_] == fields
    # ... which are the eight leading fields of sd_batch_stream, at the same offsets
    assert STRUCTS["sd_batch_stream"][0][:8] == STRUCTS["sd_spec_stream"][0]
    assert [(f, getattr(_lib.SdBatchStream, f).offset) for f in fields] == [(f, getattr(_lib.SdSpecStream, f).offset) for f in fields]


# what each loop entry took before its optional blocks moved into sd_loop_opts (ABI 6: sd_spec_generate, sd_spec_batch_generate,
# sd_spec_queue_generate_shared, sd_ar_batch_generate): argument classes and base types
LOCKSTEP_TAIL = [("ptr", "sd_sampling"), ("u64", "uint64_t"), ("ptr", "float"), ("ptr", "sd_spec_scratch"), ("ptr", "sd_lockstep_log")]
BEFORE_OPTS = {
    "sd_spec_generate": [("ptr", "sd_spec_stream"), ("i32", "int"), ("ptr", "sd_sampling"), ("ptr", "sd_spec_scratch"),
                         ("ptr", "sd_seq_state"), ("u64", "uint64_t"), ("ptr", "float"), ("ptr", "void")],
    "sd_spec_batch_generate": [("ptr", "sd_batch_stream"), ("i32", "int"), ("i32", "int"), *LOCKSTEP_TAIL, ("ptr", "void")],
    "sd_spec_queue_generate": [("ptr", "sd_batch_stream"), ("i32", "int"), ("i32", "int"), ("ptr", "sd_queue_prompt"), ("i32", "int"),
                               ("i32", "int"), ("i32", "int"), *LOCKSTEP_TAIL, ("ptr", "int"), ("ptr", "void"), ("ptr", "sd_session"),
                               ("ptr", "sd_session"), ("i32", "int")],
    "sd_ar_batch_generate": [("ptr", "sd_ar_stream"), ("i32", "int"), ("ptr", "sd_sampling"), ("ptr", "sd_head_scratch"), ("ptr", "void"),
                             ("ptr", "void"), ("ptr", "void"), ("ptr", "sd_ar_log"), ("ptr", "void")],
}


def test_loop_entries_end_in_the_options_block():
    """One optional block, sd_loop_opts, is the last argument of each of the four loop entries; in front of it every entry takes
    exactly what it took before the block existed.  Four pointers, 32 bytes, header and binding agreeing."""
    members = ["row_params", "logprobs", "penalties", "edits"]
    assert STRUCTS["sd_loop_opts"] == ([(f, 8 * i, 8) for i, f in enumerate(members)], 32)
    cls = _lib.C_STRUCTS["sd_loop_opts"]
    assert cls is _lib.SdLoopOpts and C.sizeof(cls) == 32
    assert [(f, getattr(cls, f).offset, t._type_) for f, t in cls._fields_] == \
        [(f, 8 * i, t) for i, (f, t) in enumerate(zip(members, (_lib.SdRowSampling, _lib.SdLogprobBlock, _lib.SdPenaltyBlock,
                                                                 _lib.SdLogitEditBlock)))]
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name, before in BEFORE_OPTS.items():
        _, classes, bases = PROTOS[name]
        assert list(zip(classes, bases)) == before + [("ptr", "sd_loop_opts")], name
        assert bound[name][-1]._type_ is _lib.SdLoopOpts and len(bound[name]) == len(before) + 1, name
    # no other entry takes the block, and the suffixed entries of ABI 6 are gone from header, binding and library
    assert sorted(n for n, (_, _, bases) in PROTOS.items() if "sd_loop_opts" in bases) == sorted(BEFORE_OPTS)
    raw = C.CDLL(_lib.LIB_PATH)
    removed = [loop + tail for loop in BEFORE_OPTS for tail in ("_logprobs", "_penalties", "_edits")] + \
        ["sd_spec_batch_generate_rows", "sd_spec_queue_generate_rows", "sd_spec_queue_generate_shared"]
    assert len(removed) == 15
    for name in removed:
        assert name not in PROTOS and name not in bound and not hasattr(raw, name), name
