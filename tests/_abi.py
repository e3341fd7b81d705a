"""C prototypes against the binding's signature table (_lib.SIGNATURES): the
one parser of the headers and the one comparison, for tests/test_abi.py and
the tests that pin single rows."""
from __future__ import annotations

import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracingtherestofyourlife_amd", "csrc")
PUBLIC_HEADERS = {"include/rtp.h": 40, "include/rtp_mesh.h": 4, "include/rtp_adaptive.h": 8}  # prototypes of each


def source(path: str) -> str:
    """A header's text without its comments and preprocessor lines (path: from the repository's root)."""
    src = open(os.path.join(ROOT, path)).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return re.sub(r"^[ \t]*#[^\n]*", "", src, flags=re.M)


def prototypes(*paths: str) -> dict:
    """The rtp_* functions the headers declare, in their order: name ->
    (return type, [argument declarations])."""
    protos = {}
    for path in paths:
        for ret, name, args in re.findall(r"([\w\s\*]+?)\b(rtp_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", source(path)):
            args = [a.strip() for a in args.split(",")]
            protos[name] = (" ".join(ret.split()), [] if args == ["void"] else args)
    return protos


def c_class(decl: str):
    """(base type, pointer depth) of a C argument declaration `type name` or `type name[n]`."""
    ctype, array = re.fullmatch(r"(.*?)\b\w+\s*(\[\d*\])?", decl).groups()
    words = [w for w in ctype.replace("*", " ").split() if w != "const"]
    return words[0], ctype.count("*") + (1 if array else 0)


def agrees(ct, base: str, depth: int, plain_c: bool = False) -> bool:
    """The ctypes type `ct` against a C declaration of `base` with `depth`
    stars.  plain_c: the internal headers' `int` is a type too (the public
    headers use the fixed-width names only)."""
    from raytracingtherestofyourlife_amd import _lib

    scalars = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
               "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
    by_value = ["int32_t", "uint32_t", "int64_t", "float"]
    if plain_c:
        scalars["int"] = ctypes.c_int
        by_value.append("int")
    structs = {"rtp_camera": _lib.RtpCamera, "rtp_view": _lib.RtpView, "rtp_scene_desc": _lib.RtpSceneDesc,
               "rtp_stats": _lib.RtpStats, "rtp_pixel_aux": _lib.RtpPixelAux, "rtp_render_state": _lib.RtpRenderState,
               "rtp_direct_desc": _lib.RtpDirectDesc, "rtp_denoise_params": _lib.RtpDenoiseParams,
               "rtp_ff_info": _lib.RtpFfInfo, "rtp_refine_params": _lib.RtpRefineParams}
    if depth == 0:
        return base in by_value and ct is scalars[base]
    if base in structs:  # a typed pointer, never void*
        return depth == 1 and ct is ctypes.POINTER(structs[base])
    if ct is ctypes.c_void_p:
        return True
    if ct is ctypes.c_char_p:
        return base == "char" and depth == 1
    if isinstance(ct, type) and issubclass(ct, ctypes._Pointer):
        if depth > 1:
            return agrees(ct._type_, base, depth - 1, plain_c)
        # the pointee the header names; rtp_context and void have no mirror and must be c_void_p
        return ct._type_ is scalars.get(base)
    return False


def disagreements(protos: dict, rows: dict, plain_c: bool = False) -> list:
    """Every row against its prototype: the return class, the argument count
    and each argument's class (exact scalar; pointer kind and pointee)."""
    returns = {"rtp_status": ctypes.c_int32, "int32_t": ctypes.c_int32, "const char*": ctypes.c_char_p, "void": None}
    if plain_c:
        returns.update({"int": ctypes.c_int, "int64_t": ctypes.c_int64})
    bad = []
    for name, (restype, argtypes) in rows.items():
        if name not in protos:
            bad.append(f"{name}: no prototype")
            continue
        ret, args = protos[name]
        if ret not in returns or restype is not returns[ret]:
            bad.append(f"{name}: returns {ret}, table {restype}")
        if len(argtypes) != len(args):
            bad.append(f"{name}: {len(args)} arguments, table {len(argtypes)}")
            continue
        bad += [f"{name}: argument {k} `{decl}`, table {ct}" for k, (decl, ct) in enumerate(zip(args, argtypes))
                if not agrees(ct, *c_class(decl), plain_c)]
    return bad
