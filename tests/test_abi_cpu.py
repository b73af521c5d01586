"""The whole of include/specdec.h against the ctypes binding (_lib.SYMBOLS, _lib.C_STRUCTS) and the built library: every
prototype by return class, argument count and argument class, every struct by field order, offsets, sizes and sizeof.  No GPU."""
import ctypes as C

import abi_header
from llmspeculativesampling_amd import _lib

PROTOS, STRUCTS = abi_header.parse()


def test_every_declared_symbol_is_bound_and_exported():
    print(f"{len(PROTOS)} prototypes, {len(STRUCTS)} structs")
    assert len(PROTOS) >= 83 and len(STRUCTS) >= 23
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
