"""The check of a header under include/ against the table of ``_lib.HEADERS`` that binds it, written once: how a C
declaration maps to ctypes, the parser of a header's declarations, and ``check_header``, which the ``test_the_prototype*``
test of every family calls with what is the family's own: its names in order and its doctored declarations."""
import ctypes
import os
import re

from connectome_gnn_amd import _lib

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")

_HEADER_STRUCTS = {"cgnn_tiles": _lib.CgnnTiles, "cgnn_l0src": _lib.CgnnL0Src, "cgnn_bn_tail": _lib.CgnnBnTail,
                   "cgnn_dw_jobs": _lib.CgnnDwJobs, "cgnn_adam_jobs": _lib.CgnnAdamJobs,
                   "cgnn_gather_jobs": _lib.CgnnGatherJobs, "cgnn_reduce_jobs": _lib.CgnnReduceJobs}
_HEADER_SCALARS = {"int": _lib.I32, "int32_t": _lib.I32, "int64_t": _lib.I64, "uint64_t": _lib.U64,
                   "float": _lib.F32, "double": _lib.F64}


def _header_ctype(decl: str, is_return: bool = False):
    """The ctypes type of one C parameter (or return type) as include/cgnn.h writes it."""
    words = decl.replace("*", " * ").split()
    if "*" not in words:
        base = [w for w in words if w != "const"][0]
        return ctypes.c_int if (is_return and base == "int") else _HEADER_SCALARS[base]
    base = [w for w in words[:words.index("*")] if w != "const"][0]
    if base == "char":
        return ctypes.c_char_p
    return ctypes.POINTER(_HEADER_STRUCTS[base]) if base in _HEADER_STRUCTS else _lib.DevPtr


def declared(text: str) -> dict:
    """name -> (restype, [argtypes]) of every ``cgnn_*`` function that the header ``text`` declares, in its order."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    rows = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?\*?)\s*\b(cgnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        rows[name] = (_header_ctype(ret, True), [_header_ctype(p) for p in params])
    return rows


def read(name: str) -> str:
    return open(os.path.join(INCLUDE, name)).read()


def check_header(name: str, table: dict, order: list, doctored) -> str:
    """Everything that ties ``include/<name>`` to ``table``, the family's table in ``_lib``; returns the header's text.

    ``table`` is the registry's entry ``_lib.HEADERS[name]``, the very object; the header's declarations are the table,
    return type and every argument type, and both are in ``order``; cgnn.h includes the
    header; the loaded library exports every name with the table's restype and argtypes; no name is in the table of
    any other header of the registry; and each ``(old, new)`` of ``doctored`` -- a widened integer, a dropped parameter
    -- is text of the header whose replacement parses to something else, so that a parser that matches nothing, or
    reads no types, cannot pass."""
    hdr = read(name)
    assert _lib.HEADERS[name] is table
    assert declared(hdr) =={k: (r, list(a)) for k, (r, a) in table.items()}
    assert list(table) == list(declared(hdr)) == list(order)
    assert f'#include "{name}"' in read("cgnn.h")
    lib = _lib.load()
    for fn_name, (res, args) in table.items():
        fn = getattr(lib, fn_name)
        assert fn.restype is res and list(fn.argtypes) == list(args), fn_name
    for other, rows in _lib.HEADERS.items():
        assert other == name or not set(table) & set(rows), (name, other)
    assert doctored, "a comparison that is never shown a wrong header proves nothing"
    for old, new in doctored:
        assert old in hdr and declared(hdr.replace(old, new)) != declared(hdr), old
    return hdr
