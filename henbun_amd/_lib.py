"""ctypes binding of libhenbun_hip.so, derived from include/henbun_hip.h.

This is the module that stands where the reference has `tf_wraps.py` + the
TensorFlow runtime (reference Henbun/tf_wraps.py:26-48, model.py:265-266): the
only way numerics happen in henbun_amd.  There is NO fallback: if the shared
library is missing the import-time loader raises, and a call that returns a
non-zero status raises `HipBackendError`.

The header is the one statement of the C ABI.  Every `.hip` file includes it,
so the compiler holds the definitions to it; this module reads the same text:
`parse_prototypes` gives the argument and return types of every entry point
(and with them the arity that `_Lib.call` enforces), `parse_constants` the
enumerators and integer macros that `hip_ops` uses.  A new entry point is
declared in the header, defined in csrc/ and wrapped in hip_ops.py; nothing is
added here.  tests/test_abi_cpu.py has a C++ compiler confirm that the parser
reads the header the way the compiler does.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import c_char_p, c_double, c_int, c_long, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhenbun_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "henbun_hip.h"))


class HipBackendError(RuntimeError):
    """A libhenbun_hip.so entry point returned a non-zero status."""


# ---- the header's text -> signatures and constants ---------------------------
# A parameter whose text contains `*` is a pointer; every other parameter, and every return, must be listed here.
_ARG_TYPES = {"int": c_int, "long": c_long, "double": c_double, "uint64_t": c_uint64, "unsigned long long": c_uint64}
_RET_TYPES = {"int": c_int, "long": c_long, "const char*": c_char_p}
_TYPE_WORDS = {"int", "long", "double", "float", "char", "short", "unsigned", "signed", "const", "void"}
_PROTOTYPE = re.compile(r"\s*([A-Za-z_][\w\s\*]*?)\b(hb_\w+)\s*\(([^()]*)\)\s*")
_ENUM = re.compile(r"\benum\s*\{([^{}]*)\}\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(HB_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", re.M)


def _uncomment(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _arg_type(param, proto):
    if "*" in param:
        return c_void_p
    words = [w for w in param.split() if w != "const"]
    # the last word is the parameter's name: `unsigned long long` without one must not be read as `unsigned long`
    ctype = _ARG_TYPES.get(" ".join(words[:-1])) if words and words[-1] not in _TYPE_WORDS else None
    if ctype is None:
        raise ValueError("henbun_hip.h: cannot bind parameter %r of `%s`" % (param.strip(), proto))
    return ctype


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every `RET hb_name(ARGS);` in a header's text.  Whatever is left of the text once
    comments, preprocessor lines, enum bodies and the extern "C" wrapper are gone must be such a prototype, and every
    type in it one of the few the ABI uses: anything else raises ValueError naming the prototype."""
    text = re.sub(r"^[ \t]*#.*$", " ", _uncomment(text), flags=re.M)
    text = re.sub(r'\bextern\s+"C"\s*\{', " ", _ENUM.sub(" ", text)).replace("}", " ")
    out = {}
    for stmt in text.split(";"):
        if not stmt.strip():
            continue
        proto = " ".join(stmt.split())
        m = _PROTOTYPE.fullmatch(stmt)
        if m is None:
            raise ValueError("henbun_hip.h: not a prototype of an hb_ entry point: `%s`" % proto)
        ret, name, params = m.groups()
        restype = _RET_TYPES.get(re.sub(r"\s*\*\s*", "*", " ".join(ret.split())))
        if restype is None:
            raise ValueError("henbun_hip.h: cannot bind the return type of `%s`" % proto)
        if name in out:
            raise ValueError("henbun_hip.h: `%s` is declared twice" % name)
        params = params.strip()
        out[name] = (restype, [] if params in ("", "void") else [_arg_type(p, proto) for p in params.split(",")])
    return out


def parse_constants(text):
    """{name: int} of every enumerator of the `enum { ... };` blocks (explicit values, previous + 1, expressions over
    earlier enumerators) and of every integer `#define HB_*` in a header's text."""
    text = _uncomment(text)
    out = {name: int(value, 0) for name, value in _DEFINE.findall(text)}
    for body in _ENUM.findall(text):
        value = -1
        for item in filter(None, (s.strip() for s in body.split(","))):
            name, eq, expr = (s.strip() for s in item.partition("="))
            try:
                if not re.fullmatch(r"[A-Za-z_]\w*", name) or (eq and not re.fullmatch(r"[\w\s()|&^~+\-*<>]+", expr)):
                    raise ValueError(item)
                # integer arithmetic over the enumerators read so far: no other name resolves
                value = int(eval(expr, {"__builtins__": {}}, out)) if eq else value + 1
            except Exception:
                raise ValueError("henbun_hip.h: cannot read the enumerator `%s`" % item) from None
            out[name] = value
    return out


@functools.lru_cache(maxsize=None)
def _header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError:
        raise ImportError("henbun_amd: %s is missing: the ctypes binding is derived from it." % HEADER_PATH) from None


@functools.lru_cache(maxsize=None)
def constants():
    """Every enumerator and integer macro of include/henbun_hip.h (HB_EW_*, HB_KERN_*, ..., HB_ABI_VERSION).  Reads the
    header only: the library need not be built."""
    return parse_constants(_header())


def declared_symbols():
    """Every symbol include/henbun_hip.h declares (used by the ABI tests)."""
    return list(parse_prototypes(_header()))


class _Lib:
    def __init__(self, path: str):
        if not os.path.exists(path):
            raise ImportError(
                "henbun_amd: %s is missing.  Build it with `python -m henbun_amd._build` "
                "(hipcc, gfx950).  There is no CPU fallback." % path
            )
        signatures = parse_prototypes(_header())
        # PyTorch (device memory / streams) ships its own libamdhip64.so: it must be the HIP runtime of the process.
        # Loading this library first would pull in /opt/rocm's copy, and kernels launched through that second runtime
        # see no device ("no ROCm-capable device is detected" when henbun_amd was imported before torch).
        import torch  # noqa: F401

        self._dll = ctypes.CDLL(path)
        self._fns = {}  # name -> (function, number of parameters)
        for name, (restype, argtypes) in signatures.items():
            fn = getattr(self._dll, name)
            fn.argtypes = argtypes
            fn.restype = restype
            self._fns[name] = (fn, len(argtypes))
        if self.raw("hb_version")() != constants()["HB_ABI_VERSION"]:
            raise ImportError("henbun_amd: ABI version mismatch in " + path)

    def raw(self, name):
        return self._fns[name][0]

    def last_error(self) -> str:
        s = self._fns["hb_last_error_string"][0]()
        return s.decode() if s else ""

    def call(self, name, *args):
        """Call an int-returning entry point; raise on a non-zero status.  cdecl lets surplus arguments through
        unnoticed, so the count is held to the prototype's here."""
        fn, nargs = self._fns[name]
        if len(args) != nargs:
            raise TypeError("%s takes %d arguments (%d given)" % (name, nargs, len(args)))
        rc = fn(*args)
        if rc != 0:
            raise HipBackendError("%s failed (status %d): %s" % (name, rc, self.last_error()))
        return 0


_lib = None


def lib() -> _Lib:
    """The loaded backend (loads on first use; raises ImportError if absent)."""
    global _lib
    if _lib is None:
        _lib = _Lib(LIB_PATH)
    return _lib
