"""include/aptai_hip.h as ctypes sees it: prototypes, struct layouts and integer constants, parsed from the header itself so
that Python holds no second copy of the C ABI.  The reader knows the few forms the header uses and raises AbiError, naming the
symbol or field, on anything else: an unknown type is never given a default."""
from __future__ import annotations

import collections
import ctypes
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aptai_hip.h")

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
            "double": ctypes.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "int32_t", "uint8_t"}

Abi = collections.namedtuple("Abi", "prototypes structs constants")   # name -> (restype, [argtypes]) | [(field, type)] | int

# one top-level item of the header after comments and preprocessor lines are gone
_ITEM = re.compile(r"""\s*(?:
      typedef\s+struct\s*\{(?P<sbody>[^{}]*)\}\s*(?P<sname>\w+)\s*;
    | (?:typedef\s+)?enum\s*\{(?P<ebody>[^{}]*)\}\s*\w*\s*;
    | (?P<ret>[\w\s*]+?)\b(?P<fn>\w+)\s*\((?P<params>[^()]*)\)\s*;
    | extern\s*"C"\s*\{ | \}
    )""", re.X)


class AbiError(ValueError):
    pass


def _ctype(decl: str, what: str, structs=()):
    """ctypes type of a C type written without its declarator: every pointer is c_void_p, except char* which is c_char_p."""
    toks = [t for t in decl.replace("*", " * ").split() if t != "const"]
    base, stars = (toks[0], toks[1:]) if toks else ("", [])
    if any(s != "*" for s in stars) or (base not in _POINTEES and base not in structs) or (not stars and base not in _SCALARS):
        raise AbiError(f"{what}: unknown type '{' '.join(decl.split())}'")
    if not stars:
        return _SCALARS[base]
    return ctypes.c_char_p if (base, len(stars)) == ("char", 1) else ctypes.c_void_p


def _int(expr: str, what: str) -> int:
    """An integer literal or `a << b`, with or without parentheses."""
    m = re.fullmatch(r"\(?\s*(-?\w+)\s*(?:<<\s*(\w+))?\s*\)?", expr.strip())
    try:
        return int(m.group(1), 0) << int(m.group(2) or "0", 0)
    except (AttributeError, ValueError):
        raise AbiError(f"{what}: '{expr.strip()}' is not an integer constant") from None


def _fields(body: str, sname: str, structs) -> list:
    out = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        first, *more = (p.strip() for p in decl.split(","))
        m = re.fullmatch(r"(.*?)(\w+(?:\[\w+\])?)", first)
        if m is None or ("*" in m.group(1) and more):     # `int* a, b` declares a pointer and an int: not written here
            raise AbiError(f"{sname}: cannot read the declaration '{decl}'")
        for declarator in [m.group(2)] + more:
            d = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", declarator)
            if d is None:
                raise AbiError(f"{sname}: cannot read the declarator '{declarator}' in '{decl}'")
            t = _ctype(m.group(1), f"{sname}.{d.group(1)}", structs)
            out.append((d.group(1), t * _int(d.group(2), f"{sname}.{d.group(1)}") if d.group(2) else t))
    return out


def parse(text: str) -> Abi:
    prototypes, structs, constants = {}, {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*)$", text, flags=re.M):   # `#define NAME` alone is a guard
        constants[m.group(1)] = _int(m.group(2), m.group(1))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).rstrip()
    pos = 0
    while pos < len(text):
        m = _ITEM.match(text, pos)
        if m is None:
            raise AbiError(f"cannot read the header at '{' '.join(text[pos:pos + 80].split())}'")
        pos = m.end()
        if m.group("sname"):
            structs[m.group("sname")] = _fields(m.group("sbody"), m.group("sname"), structs)
        elif m.group("ebody") is not None:
            for entry in filter(None, (e.strip() for e in m.group("ebody").split(","))):
                name, _, value = (s.strip() for s in entry.partition("="))
                constants[name] = _int(value, name)
        elif m.group("fn"):
            fn, params = m.group("fn"), m.group("params").strip()
            args = []
            for p in ([] if params == "void" else params.split(",")):
                pm = re.fullmatch(r"(.*?)(\w+)", p.strip(), flags=re.S)
                if pm is None or not pm.group(1).strip():
                    raise AbiError(f"{fn}: cannot read the parameter '{' '.join(p.split())}'")
                args.append(_ctype(pm.group(1), f"{fn}({pm.group(2)})", structs))
            prototypes[fn] = (_ctype(m.group("ret"), f"{fn} return", structs), args)
    return Abi(prototypes, structs, constants)


@functools.lru_cache(maxsize=None)
def header() -> Abi:
    """The project's header, parsed once per process."""
    with open(HEADER) as f:
        return parse(f.read())
