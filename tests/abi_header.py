"""include/specdec.h read as an ABI, next to the same view of the ctypes binding.  The classes are what the x86-64 calling
convention tells apart: "ptr", "i32" (int, int32_t, unsigned, enums), "long", "f32", "u64" (uint64_t and size_t: one ctypes type)."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "specdec.h")
SCALARS = {"int": ("i32", 4), "int32_t": ("i32", 4), "unsigned": ("i32", 4), "float": ("f32", 4), "long": ("long", 8),
           "uint64_t": ("u64", 8), "size_t": ("u64", 8)}


def _declarators(decl):
    """'const float *p, *q' / 'float p_at[16]' -> the base type and (name, pointer depth, array length or 0) per name."""
    first, *rest = [d.strip() for d in decl.split(",")]
    words = re.findall(r"\w+", re.sub(r"\[\w+\]|\bconst\b|\bstruct\b", " ", first))
    base = " ".join(words[:-1])
    return base, [(re.findall(r"\w+", d.split("[")[0])[-1], d.count("*"), int((re.findall(r"\[(\w+)\]", d) or [0])[0]))
                  for d in [first] + rest]


def parse(path=HEADER):
    """-> (prototypes {name: (return class, [argument classes], [argument base types])}, structs {name: (fields, sizeof)})."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    sized = {name: (4, 4) for name in re.findall(r"typedef enum\s*\{[^}]*\}\s*(\w+)\s*;", text)}      # name -> (size, alignment)
    sized.update({name: (size, size) for name, (_, size) in SCALARS.items()})
    text = re.sub(r"(typedef )?enum\s*\{[^}]*\}\s*\w*\s*;", " ", text)
    structs = {}
    for body, name in re.findall(r"typedef struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields, off, align = [], 0, 1
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, names = _declarators(decl)
            for field, stars, arr in names:
                sz, al = (8, 8) if stars else sized[base]
                off = (off + al - 1) // al * al
                fields.append((field, off, sz * (arr or 1)))
                off += sz * (arr or 1)
                align = max(align, al)
        sized[name] = ((off + align - 1) // align * align, align)
        structs[name] = (fields, sized[name][0])
    text = re.sub(r"typedef struct[^;{]*(\{[^{}]*\})?[^;]*;", " ", text)

    def cls(base, stars, arr=0):
        return "ptr" if stars or arr else "i32" if sized[base] == (4, 4) and base not in SCALARS else SCALARS[base][0]

    protos = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(sd_\w+)\s*\(([^()]*)\)\s*;", text):
        rbase, [(_, rstars, _)] = _declarators(ret + " _")
        argv = [] if args.strip() in ("", "void") else [_declarators(a) for a in args.split(",")]
        protos[name] = (cls(rbase, rstars), [cls(b, *n[0][1:]) for b, n in argv], [b for b, _ in argv])
    return protos, structs


def ctypes_class(t):
    """The class of a ctypes restype / argtype."""
    pointer = t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents")
    return "ptr" if pointer else {C.c_int: "i32", C.c_uint: "i32", C.c_long: "long", C.c_float: "f32", C.c_uint64: "u64"}[t]
