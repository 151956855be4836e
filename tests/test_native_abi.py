"""The ctypes tables and shared constants of ``ops/native.py`` against the
C headers that declare the native ABI (``csrc/hsio_abi.h``,
``csrc/hsgpu_abi.h``, ``csrc/hsgpu_hooks.h``).

No compiler and no library: the headers are restricted to prototypes over
scalars and pointers plus anonymous enums of integer constants, which the
small parser below reads; it raises on anything else.
"""

import ctypes
import os
import re

import pytest

from hipsnapshot.ops import native

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "hipsnapshot", "csrc")

SCALARS = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
           "uint64_t": ctypes.c_uint64, "double": ctypes.c_double}

_TYPE = r"(?:const\s+)?(\w+)((?:\s*\*(?:\s*const\b)?)*)"
_PARAM = re.compile(rf"^{_TYPE}\s*(\w+)$")
_PROTO = re.compile(rf"^{_TYPE}\s*(\w+)\s*\((.*)\)$", re.S)
_ENUM = re.compile(r"^enum\s*\{(.*)\}$", re.S)
_ENUMERATOR = re.compile(r"^(\w+)\s*=\s*(\d+)$")


def _ctype(base, stars):
    """A header type as (base, pointer depth)."""
    depth = stars.count("*")
    if base not in SCALARS and base not in ("void", "char"):
        raise ValueError(f"unknown type {base!r}")
    return base, depth


def parse_header(name):
    """(includes, {constant: value}, {function: (return type, [param types])})
    of one header; raises ValueError on any statement it does not understand."""
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r"//[^\n]*", "", text)
    if "/*" in text:
        raise ValueError(f"{name}: block comments are not supported")
    includes = re.findall(r'^#include\s+[<"]([^>"]+)[>"]\s*$', text, re.M)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)           # guards, includes
    text = re.sub(r'extern\s+"C"\s*\{', "", text, count=1)
    consts, funcs = {}, {}
    for stmt in (s.strip() for s in text.split(";")):
        if not stmt or stmt == "}":                            # `}` closes extern "C"
            continue
        m = _ENUM.match(stmt)
        if m:
            for item in (i.strip() for i in m.group(1).split(",")):
                e = _ENUMERATOR.match(item)
                if not e or e.group(1) in consts:
                    raise ValueError(f"{name}: bad enumerator {item!r}")
                consts[e.group(1)] = int(e.group(2))
            continue
        m = _PROTO.match(stmt)
        if not m:
            raise ValueError(f"{name}: cannot parse {stmt!r}")
        base, stars, fn, params = m.groups()
        args = []
        for p in (q.strip() for q in params.split(",")) if params.strip() else ():
            pm = _PARAM.match(" ".join(p.split()))
            if not pm:
                raise ValueError(f"{name}: {fn}: cannot parse parameter {p!r}")
            args.append(_ctype(pm.group(1), pm.group(2)))
        if fn in funcs:
            raise ValueError(f"{name}: {fn} declared twice")
        funcs[fn] = (_ctype(base, stars), args)
    return includes, consts, funcs


def allowed_ctypes(ctype, is_return=False):
    """The ctypes declarations a header type may have."""
    base, depth = ctype
    if depth == 0:
        if base == "void" and is_return:
            return [None]
        return [SCALARS[base]]                                 # KeyError: void / char by value
    if base == "void":
        if depth != 1:
            raise ValueError("void** is not supported")
        return [ctypes.c_void_p]
    if base == "char":
        pointee = ctypes.c_char_p
        exact = pointee if depth == 1 else ctypes.POINTER(pointee)
        if depth > 2:
            raise ValueError("char*** is not supported")
    else:
        if depth != 1:
            raise ValueError(f"{base}** is not supported")
        exact = ctypes.POINTER(SCALARS[base])
    return [exact, ctypes.c_void_p]


HSIO = parse_header("hsio_abi.h")
HSGPU = parse_header("hsgpu_abi.h")
HOOKS = parse_header("hsgpu_hooks.h")


def test_headers_include_only_stdint_and_each_other():
    assert HSIO[0] == ["stdint.h"]
    assert HSGPU[0] == ["stdint.h"]
    assert HOOKS[0] == ["hsgpu_abi.h"]


def test_tables_name_exactly_the_headers_functions():
    assert set(native.HSIO_ABI) == set(HSIO[2])
    assert set(native.HSGPU_ABI) == set(HSGPU[2])
    hooks = set(HOOKS[2])
    assert hooks and not hooks & (set(native.HSIO_ABI) | set(native.HSGPU_ABI))
    assert not hooks & set(HSGPU[2]), "a hook is also declared in hsgpu_abi.h"
    assert not HOOKS[1], "shared constants belong in hsgpu_abi.h"


def test_hsgpu_has_one_error_getter():
    # one message channel for the whole library: hsg_last_error
    exported = set(HSGPU[2]) | set(HOOKS[2])
    assert [fn for fn in sorted(exported) if fn.endswith("_last_error")] == ["hsg_last_error"]


@pytest.mark.parametrize("table,funcs", [(native.HSIO_ABI, HSIO[2]), (native.HSGPU_ABI, HSGPU[2])],
                         ids=["hsio", "hsgpu"])
def test_every_signature_matches_its_prototype(table, funcs):
    bad = []
    for fn, (ret, params) in funcs.items():
        restype, argtypes = table[fn]
        if restype not in allowed_ctypes(ret, is_return=True)[:1]:
            bad.append(f"{fn}: returns {ret}, declared {restype}")
        if len(argtypes) != len(params):
            bad.append(f"{fn}: {len(params)} parameters, {len(argtypes)} declared")
            continue
        for k, (p, a) in enumerate(zip(params, argtypes)):
            if a not in allowed_ctypes(p):
                bad.append(f"{fn}: parameter {k} is {p}, declared {a}")
    assert not bad, "\n".join(bad)


def test_hooks_use_only_supported_types():
    for ret, params in HOOKS[2].values():
        allowed_ctypes(ret, is_return=True)
        for p in params:
            allowed_ctypes(p)


def test_shared_constants_match():
    hsio = {"HSIO_DIRECT": native.IO_DIRECT, "HSIO_SYNC": native.IO_SYNC,
            "HSIO_MKDIRS": native.IO_MKDIRS, "HSIO_APPEND": native.IO_APPEND,
            "HSIO_NODE_SHIFT": native.IO_NODE_SHIFT}
    hsgpu = {"HSG_DRAIN_SYNC": native.DRAIN_SYNC, "HSG_DRAIN_HASH": native.DRAIN_HASH,
             "HSG_DRAIN_DIRECT": native.DRAIN_DIRECT,
             "HSG_DRAIN_HASH_LOW_PRIO": native.DRAIN_HASH_LOW_PRIO,
             "HSG_DRAIN_NICE_SHIFT": native.DRAIN_NICE_SHIFT,
             "HSG_DRAIN_PARKED_SHIFT": native.DRAIN_PARKED_SHIFT,
             "HSG_DRAIN_NUM_STATS": len(native.NativeDrain.STATS),
             "HSG_DRAIN_MSG_BYTES": native.DRAIN_MSG_BYTES,
             "HSG_RESTORE_NUM_STATS": len(native.NativeRestore.STATS),
             "HSG_RESTORE_MSG_BYTES": native.RESTORE_MSG_BYTES,
             "HSG_CODEC_RAW": native.CODEC_RAW, "HSG_CODEC_HSZ": native.CODEC_HSZ}
    # equality of the whole mappings: a constant added to a header needs its
    # Python counterpart here
    assert HSIO[1] == hsio
    assert HSGPU[1] == hsgpu


def test_drain_flags_are_built_from_the_shared_bits():
    f = native.NativeDrain.flags
    assert f(True, False, False, True, 0) == HSGPU[1]["HSG_DRAIN_SYNC"]
    assert f(False, True, False, True, 0) == HSGPU[1]["HSG_DRAIN_HASH"]
    assert f(False, False, True, True, 0) == HSGPU[1]["HSG_DRAIN_DIRECT"]
    assert f(False, False, False, False, 0) == HSGPU[1]["HSG_DRAIN_HASH_LOW_PRIO"]
    assert f(False, False, False, True, 5) == 5 << HSGPU[1]["HSG_DRAIN_NICE_SHIFT"]
