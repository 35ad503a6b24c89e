"""ctypes binding of libmvs_hip.so (the C ABI declared in include/mvs_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C mvsformer_amd/csrc`` and is the ONLY
compute path of this package: there is no PyTorch or CPU fallback, so a missing library is a hard error.

``import torch`` must precede the ``CDLL`` call: torch's wheel bundles its own HIP runtime under the same
SONAME (libamdhip64.so.7) and the dynamic loader then binds our library to that already-loaded runtime, so the
``hipStream_t`` handles torch hands us belong to the runtime that launches our kernels.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_void_p

import torch  # noqa: F401  (load order, see above)

from . import switches as sw

_HERE = os.path.dirname(os.path.abspath(__file__))
# MVS_HIP_LIB: diagnostics only - another BUILD of the same library (tests/test_hip_multistream.py's variants); never a fallback
LIB_PATH = sw.text("MVS_HIP_LIB") or os.path.join(_HERE, "libmvs_hip.so")
HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "mvs_hip.h")

P, I, F, L, Dbl = c_void_p, c_int, c_float, c_int64, c_double
_SCALARS = {"int": I, "float": F, "int64_t": L, "double": Dbl}


def _ctype(decl: str, fn: str, result: bool = False):
    """One parameter (``const float* x``, ``int64_t n``, ``mvs_stream_t stream``) or result type of ``fn`` -> its ctypes type.
    Anything outside the header's small vocabulary raises: a guessed width would hand a kernel a corrupted argument."""
    words = decl.replace("*", " * ").split()
    if result and words == ["const", "char", "*"]:
        return c_char_p
    if not result and ("*" in words or words[:1] == ["mvs_stream_t"]):
        return P
    words = [w for w in words if w != "const"]
    ctype = _SCALARS.get(" ".join(words if result or len(words) == 1 else words[:-1]))      # a parameter's last word is its name
    if ctype is None:
        raise TypeError("include/mvs_hip.h: %s: no ctypes mapping for %r" % (fn, decl.strip()))
    return ctype


def parse_header(text: str):
    """The text of include/mvs_hip.h -> ``{name: (restype, [argtypes])}`` of every ``mvs_*`` prototype and ``{MVS_*: value}`` of every
    integer ``#define``.  Struct members hold no parentheses and are passed over; every other declaration must be a prototype."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MVS_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r'^[ \t]*#[^\n]*|extern\s+"C"\s*\{', " ", text, flags=re.M)
    signatures = {}
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue
        m = re.fullmatch(r"\s*([^()]*?)\b(mvs_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m is None:
            raise TypeError("include/mvs_hip.h: cannot read the declaration %r" % " ".join(stmt.split()))
        res, fn, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[fn] = (_ctype(res, fn, result=True), [_ctype(p, fn) for p in params])
    return signatures, defines


# name -> (restype, argtypes) and the integer macros, read from the header itself: there is no second copy to drift
SIGNATURES, DEFINES = parse_header(open(HEADER_PATH).read())
# the scene-preparation entries (csrc/scene_prep.hip) have a header of their own, bound the same way; mvs_hip.h's table stands as it was
SCENE_HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "mvs_scene_prep.h")
SCENE_SIGNATURES, SCENE_DEFINES = parse_header(open(SCENE_HEADER_PATH).read())
ABI_VERSION = DEFINES["MVS_ABI_VERSION"]
ADAM_HYPER_STRIDE = DEFINES["MVS_ADAM_HYPER_STRIDE"]         # lr, weight_decay, beta1, beta2, eps, maximize, 0, 0


class AdamTensor(ctypes.Structure):
    """``MvsAdamTensor`` of include/mvs_hip.h."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("n", ctypes.c_int64)]


class AdamEntry(ctypes.Structure):
    """``MvsAdamEntry`` of include/mvs_hip.h: a tensor of the multi-group table."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("group", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class WgradJob(ctypes.Structure):
    """``MvsWgradJob`` of include/mvs_hip.h."""
    _fields_ = [("A", ctypes.c_void_p), ("Bt", ctypes.c_void_p), ("dW", ctypes.c_void_p)] + \
               [(n, ctypes.c_int) for n in ("nbatch", "CA", "CB", "CBout", "Dp", "Hp", "Wp", "Db", "Hb", "Wb", "sd", "shw", "taps", "reserved")]


_lib = None


class MvsHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load (once) and return the library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MvsHipError(
            "%s is missing: the HIP path has not been built (run `python -c \"import __graft_entry__ as g; g.build()\"` "
            "or `make -C mvsformer_amd/csrc`).  mvsformer_amd has no CPU/PyTorch fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(SCENE_SIGNATURES.items()):
        fn = getattr(lib, name)          # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    got = lib.mvs_version()
    if got != ABI_VERSION:
        raise MvsHipError("libmvs_hip.so ABI version %d, binding expects %d — rebuild" % (got, ABI_VERSION))
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().mvs_last_error()
        raise MvsHipError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))
