"""ctypes binding of libmmdfn_hip.so (the C ABI declared in include/mmdfn_hip.h).

There is no CPU fallback: if the library is missing, stale or a kernel returns
an error, the product path raises.
"""
import ctypes
import os
import re

import torch

from . import build as _build

_F = ctypes.c_float


class HipLibraryError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def _ctype(text, decl):
    """ctypes type of one parameter or return type as the header spells it: anything with ``*`` is a pointer."""
    if "*" in text:
        return ctypes.c_void_p
    text = text.strip()
    words = [w for w in text.split() if w != "const"]
    if "[" in text or not words:
        raise HipLibraryError("cannot split the declaration '%s' of include/mmdfn_hip.h" % decl)
    if words[0] == "struct" or words[0].startswith("mmdfn_"):
        raise HipLibraryError("'%s' is passed by value in '%s': the binding takes structs by pointer only" % (text, decl))
    if words[0] not in _SCALARS or len(words) > 2:      # [type] or [type, name]
        raise HipLibraryError("unknown scalar type '%s' in '%s'" % (text, decl))
    return _SCALARS[words[0]]


def parse_header(text):
    """(argtypes, restypes) by symbol name for every ``mmdfn_*(...)`` declaration of the C header ``text``.  Strict: a
    declaration it cannot read raises HipLibraryError; no type is ever guessed."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    argtypes, restypes = {}, {}
    for stmt in re.split(r"[;{}]", text):
        if not re.search(r"\bmmdfn_\w+\s*\(", stmt):
            continue
        decl = " ".join(stmt.split())
        m = re.fullmatch(r"(\w[\w\s*]*?)\s*\b(mmdfn_\w+)\s*\(([^()]*)\)", decl)
        if m is None:
            raise HipLibraryError("cannot split the declaration '%s' of include/mmdfn_hip.h" % decl)
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        restypes[name] = _ctype(ret, decl)
        argtypes[name] = [_ctype(p, decl) for p in params]
    return argtypes, restypes


# name -> argtypes / return type, read from the header that build._digest() already stamps the library with
with open(os.path.join(_build.INCLUDE, "mmdfn_hip.h")) as _f:
    SIGNATURES, RESTYPES = parse_header(_f.read())

ABI_VERSION = 23


class AdamState(ctypes.Structure):
    """Mirror of ``mmdfn_adam_state`` (include/mmdfn_hip.h): FlatAdam's step state, 64 bytes of device memory."""
    _fields_ = [("step", ctypes.c_int32), ("enabled", ctypes.c_int32), ("skip_nonfinite", ctypes.c_int32),
                ("skipped", ctypes.c_int32), ("last_skipped", ctypes.c_int32),
                ("lr", _F), ("weight_decay", _F), ("max_norm", _F), ("grad_norm", _F), ("scale", _F),
                ("bc1", _F), ("bc2_sqrt", _F), ("reserved", ctypes.c_int32 * 4)]


def adam_state_word(name):
    """Index of field ``name`` in the block viewed as 16 four-byte words."""
    return getattr(AdamState, name).offset // 4


_libs = {}
_tuning = os.environ.get("MMDFN_TUNING_LIB", "0") == "1"


def set_tuning(flag):
    """Select the -DMMDFN_TUNING build (lib/libmmdfn_hip_tuning.so) for subsequent calls; returns the previous setting.
    Only tools/ and the variant-forcing kernel tests do this (also: MMDFN_TUNING_LIB=1 in the environment).  It is the
    one library that honours the MMDFN_* ablation / tiling switches; the production library has none compiled in."""
    global _tuning
    prev, _tuning = _tuning, bool(flag)
    return prev


def lib():
    """Load (once) and return the shared library; raises if unavailable."""
    handle = _libs.get(_tuning)
    if handle is not None:
        return handle
    tuning = _tuning
    path = _build.TUNING_LIBPATH if tuning else _build.LIBPATH
    if _build.is_stale(tuning):
        # missing or built from other sources (digest stamp): rebuild in place when a compiler is at hand (the GPU box
        # has hipcc).  A library that does not match the sources is never loaded.
        try:
            _build.build(verbose=False, tuning=tuning)
        except Exception as e:
            raise HipLibraryError(
                "%s is missing or stale (source digest mismatch) and could not be rebuilt (%s): run `python -m "
                "mm_dfn_amd.build` (needs hipcc); the MI355X path has no CPU fallback" % (path, e)) from e
    handle = ctypes.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise HipLibraryError("%s lacks symbol %s (stale build?)" % (os.path.basename(path), name)) from e
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    if handle.mmdfn_abi_version() != ABI_VERSION:
        raise HipLibraryError("%s ABI version mismatch" % os.path.basename(path))
    _libs[tuning] = handle
    return handle


def riders_context():
    """An empty rider context (include/mmdfn_hip.h mmdfn_riders_bytes): zeroed host memory that the rider entry points stage
    work in and the GRU launches given it take work from."""
    return ctypes.create_string_buffer(int(query("mmdfn_riders_bytes")))


def ptr(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != 0:
        raise HipLibraryError("%s failed with code %d" % (what, rc))


def _miscall(name, nargs):
    if name not in SIGNATURES:
        return HipLibraryError("%s is not declared in include/mmdfn_hip.h" % name)
    return HipLibraryError("%s takes %d arguments, got %d" % (name, len(SIGNATURES[name]), nargs))


def query(name, *args):
    """Value of entry point ``name`` (a size or a predicate: *_workspace, *_bytes, *_supported, ...).  ctypes takes surplus
    arguments in silence, so the count is checked against the header before the library is entered."""
    argtypes = SIGNATURES.get(name)
    if argtypes is None or len(args) != len(argtypes):
        raise _miscall(name, len(args))
    return getattr(_libs.get(_tuning) or lib(), name)(*args)


def call(name, *args, allow=()):
    """Run entry point ``name`` after the same count check; raises unless it returns 0 or a code in ``allow``.  Returns the
    code.  (Not written through ``query``: a Python frame per launch is what the eager step is made of.)"""
    argtypes = SIGNATURES.get(name)
    if argtypes is None or len(args) != len(argtypes):
        raise _miscall(name, len(args))
    rc = getattr(_libs.get(_tuning) or lib(), name)(*args)
    if rc != 0 and rc not in allow:
        raise HipLibraryError("%s failed with code %d" % (name, rc))
    return rc


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipLibraryError("the MM-DFN HIP path needs tensors on an MI355X device (got %s); "
                                  "there is no CPU fallback" % t.device)


def ptr_array(tensors):
    """Host array of device pointers (one per group) for the grouped entry points."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def int_array(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def long_array(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def float_array(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def require_f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise HipLibraryError("the MM-DFN HIP kernels are fp32 (got %s)" % t.dtype)
