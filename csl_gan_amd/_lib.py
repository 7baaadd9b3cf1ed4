"""ctypes binding of libcslgan_hip.so, read from include/cslgan.h.

The header is the one table of the C ABI: at import this module parses its prototypes into EXPORTS and the restype / argtypes of
every entry, and its `#define CSLGAN_X <integer>` lines and enum bodies into the constants below.  A type the mapping does not
know raises at import (never a silent `int`).  Only the three descriptor structs are restated by hand (tests/test_abi.py holds
their layout to the compiler's).  Adding an entry: prototype in the header, definition in a .hip file of build.SOURCES — nothing here.

The product path has no CPU fallback for CUDA/HIP tensors: if the shared library is missing
or fails to load, :func:`lib` raises immediately.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSLGAN_LIB_PATH") or os.path.join(_HERE, "libcslgan_hip.so")      # override: kernel experiments
HEADER_PATH = os.path.join(_HERE, "..", "include", "cslgan.h")


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def parse_constants(text):
    """{name without CSLGAN_: int} of every `#define CSLGAN_X <integer>` and every `NAME = <integer>` of an enum body."""
    text = _strip_comments(text)
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+CSLGAN_(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, flags=re.M)
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        found += re.findall(r"\bCSLGAN_(\w+)\s*=\s*(-?(?:0[xX][0-9a-fA-F]+|\d+))\b", body)
    return {name: int(value, 0) for name, value in found}


try:
    with open(HEADER_PATH) as _f:
        _HEADER = _f.read()
except OSError as e:
    raise FileNotFoundError("csl_gan_amd binds libcslgan_hip.so from its header, which is not at %s (%s)" % (HEADER_PATH, e)) from None

_K = parse_constants(_HEADER)
ABI_VERSION = _K["ABI_VERSION"]
MAX_SEGS, MAX_CLIP_LAYERS, MAX_CLIP_JOBS = _K["MAX_SEGS"], _K["MAX_CLIP_LAYERS"], _K["MAX_CLIP_JOBS"]
MAX_WGRAD_BLOCKS, NORM_PARTIAL_BLOCKS = _K["MAX_WGRAD_BLOCKS"], _K["NORM_PARTIAL_BLOCKS"]
ACT_NONE, ACT_LRELU02, ACT_RELU, ACT_TANH = _K["ACT_NONE"], _K["ACT_LRELU02"], _K["ACT_RELU"], _K["ACT_TANH"]
COMPUTE_F32, COMPUTE_BF16, COMPUTE_BF16X3 = _K["COMPUTE_F32"], _K["COMPUTE_BF16"], _K["COMPUTE_BF16X3"]


class SegsT(C.Structure):
    _fields_ = [
        ("n_seg", C.c_int32), ("_pad", C.c_int32),
        ("inp", C.c_void_p * MAX_SEGS), ("out", C.c_void_p * MAX_SEGS), ("noise", C.c_void_p * MAX_SEGS),
        ("len", C.c_int64 * MAX_SEGS), ("row_stride", C.c_int64 * MAX_SEGS), ("rows", C.c_int64 * MAX_SEGS), ("call_counter", C.c_void_p),
    ]


class AdaptiveClipT(C.Structure):
    _fields_ = [
        ("n_layers", C.c_int32), ("n_mat", C.c_int32), ("n_jobs", C.c_int32), ("_pad", C.c_int32),
        ("sq_adapt", C.c_void_p * MAX_CLIP_LAYERS), ("sq_rows", C.c_void_p * MAX_CLIP_LAYERS), ("mat_layer", C.c_int32 * MAX_CLIP_LAYERS),
        ("job_dst", C.c_void_p * MAX_CLIP_JOBS), ("job_first", C.c_int64 * MAX_CLIP_JOBS), ("job_layer", C.c_int32 * MAX_CLIP_JOBS),
        ("job_count", C.c_int32 * MAX_CLIP_JOBS), ("job_scale", C.c_float * MAX_CLIP_JOBS),
    ]


class ConvT(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("N", "H", "W", "C", "K", "R", "S", "stride", "pad", "compute", "P", "Q")] + [("split_ws", C.c_void_p), ("split_ws_floats", C.c_int64), ("gn_part", C.c_void_p), ("gn_groups", C.c_int32), ("in_relu", C.c_int32), ("in_scale", C.c_void_p), ("in_shift", C.c_void_p)]


_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
_STRUCTS = {"cslgan_segs_t": SegsT, "cslgan_conv_t": ConvT, "cslgan_adaptive_clip_t": AdaptiveClipT}


def _argtype(entry, param):
    words = param.replace("*", " * ").replace("[", " [").split()
    if "*" in words or words[-1].startswith("["):        # a pointer or array: the three descriptors by type, anything else opaque
        struct = _STRUCTS.get(words[1] if words[0] == "const" else words[0])
        return C.POINTER(struct) if struct else C.c_void_p
    if words[0] == "const":
        words = words[1:]
    ctype = " ".join(words[:-1] if len(words) > 1 else words)        # the last word is the parameter's name
    if ctype not in _SCALARS:
        raise TypeError("%s: parameter '%s' has type '%s', which the binding does not map" % (entry, param, ctype))
    return _SCALARS[ctype]


def parse_prototypes(text):
    """{entry: (restype, argtypes)} of every `<type> cslgan_xxx(...);` of a header text, in header order."""
    protos = {}
    for ret, entry, params in re.findall(r"^[ \t]*([\w \t*]+?)[ \t]*\b(cslgan_\w+)\s*\(([^()]*)\)\s*;", _strip_comments(text), flags=re.M):
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise TypeError("%s: return type '%s' is not one the binding maps" % (entry, ret))
        params = " ".join(params.split())
        protos[entry] = (_RETURNS[ret], [] if params in ("void", "") else [_argtype(entry, p.strip()) for p in params.split(",")])
    return protos


PROTOTYPES = parse_prototypes(_HEADER)
EXPORTS = list(PROTOTYPES)

_lib = None


class HipLibraryMissing(RuntimeError):
    pass


def lib():
    """Load (once) and return the C-ABI library; raises HipLibraryMissing if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            "libcslgan_hip.so not found at %s — build it with `python -m csl_gan_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for device tensors." % LIB_PATH)
    # torch first: its bundled HIP runtime must be the one already mapped when our library's
    # libamdhip64 dependency is resolved (two HIP runtimes in one process cannot share a device context)
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.cslgan_version() != ABI_VERSION:
        raise HipLibraryMissing("libcslgan_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().cslgan_last_error().decode(errors="replace")
        raise RuntimeError("cslgan %s failed (%d): %s" % (what, rc, msg))
