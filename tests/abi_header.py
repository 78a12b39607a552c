"""``include/gmr_hip.h`` as the host tests read it: a prototype's parameters as the ctypes types ``_lib.py`` must declare, a typedef struct's
field names, a ``#define``'s value."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gmr_hip.h")
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}


def read() -> str:
    with open(HEADER) as f:
        return f.read()


def _plain(text: str) -> str:
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def ctype_of(decl: str):
    """the ctypes type of one C parameter declaration: ``int *x`` is a count that comes back (``POINTER(c_int)``), every other pointer an
    address (``c_void_p``), a scalar its own type"""
    decl = decl.strip()
    if "*" in decl:
        return C.POINTER(C.c_int) if re.match(r"int\s*\*", decl) else C.c_void_p
    return SCALARS[decl.split()[0]]


def parameters(hdr: str, symbol: str):
    """the parameter list of ``int symbol(...);`` as ctypes types"""
    m = re.search(r"\bint " + symbol + r"\(([^;]*)\);", hdr)
    assert m, symbol
    return [ctype_of(p) for p in _plain(m.group(1)).split(",")]


def fields(hdr: str, name: str):
    """the field names of ``typedef struct { ... } name``, in order"""
    body = _plain(re.search(r"typedef struct \{([^}]*)\} " + name, hdr).group(1))
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"\[.*\]", "", x).strip(" *") for x in re.sub(r"^(const\s+)?\w+\s+", "", decl).split(",")]
    return out


def define(hdr: str, name: str):
    """the value of ``#define name value``: a whole number where it is one, the text otherwise; ``None`` when there is no such line"""
    m = re.search(r"^#define " + name + r"[ \t]+(\S+)", hdr, flags=re.M)
    if m is None:
        return None
    try:
        return int(m.group(1), 0)
    except ValueError:
        return m.group(1)
