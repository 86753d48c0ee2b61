"""The C-ABI library loads and exports every symbol include/mmdfn_hip.h declares (no compute)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "mmdfn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|int64_t)\s+(mmdfn_\w+)\s*\(", text)))


def test_header_declares_symbols():
    syms = declared_symbols()
    assert "mmdfn_propagate" in syms and "mmdfn_adj_build" in syms and len(syms) >= 5


def test_library_exports_every_declared_symbol():
    from mm_dfn_amd import build
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    handle = ctypes.CDLL(build.LIBPATH)
    for s in declared_symbols():
        assert hasattr(handle, s), "missing export %s" % s
    from mm_dfn_amd import _hip
    assert handle.mmdfn_abi_version() == _hip.ABI_VERSION


def test_binding_table_matches_header():
    from mm_dfn_amd import _hip
    assert sorted(_hip.SIGNATURES.keys()) == declared_symbols()


def test_arg_counts_match_header():
    from mm_dfn_amd import _hip
    text = open(os.path.join(ROOT, "include", "mmdfn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, args in re.findall(r"\bint\s+(mmdfn_\w+)\s*\(([^)]*)\)", text):
        n = 0 if args.strip() in ("", "void") else len(args.split(","))
        assert n == len(_hip.SIGNATURES[name]), name


def test_header_parser_on_synthetic_text():
    from ctypes import c_float, c_int, c_int64, c_void_p
    from mm_dfn_amd import _hip
    text = """
    #include <stdint.h>
    extern "C" {
    /* not a declaration: int mmdfn_in_comment(int a);  and a mention of mmdfn_named(here) */
    typedef struct mmdfn_adam_state { int32_t step; float lr; } mmdfn_adam_state;
    int64_t mmdfn_bytes(void);
    int mmdfn_empty();
    int mmdfn_spread(const float* x,
                     int64_t n,   /* rows */
                     int32_t k, float
                     scale,
                     void* stream);
    int mmdfn_pointers(const float* const* groups, mmdfn_adam_state* st, const mmdfn_adam_state* cst, double* partials,
                       const double* p2, const void* const* planes, int* count);
    int64_t mmdfn_wide(int64_t n, int k, const int64_t big);
    }
    """
    args, res = _hip.parse_header(text)
    assert sorted(args) == ["mmdfn_bytes", "mmdfn_empty", "mmdfn_pointers", "mmdfn_spread", "mmdfn_wide"]
    assert args["mmdfn_bytes"] == [] and res["mmdfn_bytes"] is c_int64
    assert args["mmdfn_empty"] == [] and res["mmdfn_empty"] is c_int
    assert args["mmdfn_spread"] == [c_void_p, c_int64, c_int, c_float, c_void_p] and res["mmdfn_spread"] is c_int
    assert args["mmdfn_pointers"] == [c_void_p] * 7
    assert args["mmdfn_wide"] == [c_int64, c_int, c_int64] and res["mmdfn_wide"] is c_int64


@pytest.mark.parametrize("decl, named", [
    ("int mmdfn_bad(const float* x, unsigned n, void* stream);", "unsigned n"),          # a scalar type the binding does not know
    ("int mmdfn_bad(double x);", "double x"),
    ("int mmdfn_bad(size_t n);", "size_t n"),
    ("double mmdfn_bad(int n);", "double"),                                              # ... as the return type
    ("int mmdfn_bad(mmdfn_adam_state st, void* stream);", "mmdfn_adam_state st"),        # a struct by value
    ("int mmdfn_bad(struct mmdfn_adam_state st);", "struct mmdfn_adam_state st"),
    ("int mmdfn_bad(int n[4]);", "mmdfn_bad"),                                           # declarations it cannot split
    ("int mmdfn_bad(int (*fn)(int), void* stream);", "mmdfn_bad"),
])
def test_header_parser_is_strict(decl, named):
    from mm_dfn_amd import _hip
    with pytest.raises(_hip.HipLibraryError) as e:
        _hip.parse_header("int mmdfn_good(int n);\n" + decl + "\n")
    assert named in str(e.value) and "mmdfn_bad" in str(e.value)


def test_binding_types_of_real_symbols():
    """Written out by hand from the text of include/mmdfn_hip.h: every type class and both return types."""
    from ctypes import c_float as F, c_int as I, c_int64 as L, c_void_p as P
    from mm_dfn_amd import _hip
    want = {
        "mmdfn_abi_version": ([], I),
        "mmdfn_riders_bytes": ([], L),
        "mmdfn_lstm_pointwise_fwd": ([P, P, P, P, L, I, P], I),
        "mmdfn_adam_step": ([P, P, P, P, L, F, F, F, F, F, I, P], I),
        "mmdfn_adam_step_state": ([P, P, P, P, L, P, F, F, F, P], I),          # const mmdfn_adam_state* st
        "mmdfn_adam_prepare": ([P, P, I, F, F, P], I),                         # mmdfn_adam_state*, const double*
        "mmdfn_grad_sumsq": ([P, L, P, I, P, P], I),                           # double* partials, int* nparts
        "mmdfn_tfn_workspace": ([L, I, I, I, I, I], L),
        "mmdfn_keep_flags": ([P, L, F, P, P], I),
        "mmdfn_gru_seq_fwd": ([I, P, P, P, P, P, P, P, I, P, P], I),           # const float* const*, const int*
        "mmdfn_adj_build_kind": ([P] * 11 + [I] * 5 + [F, I, P], I),
        "mmdfn_weight_planes_workspace": ([I, I], L),
    }
    for name, (argtypes, restype) in want.items():
        assert _hip.SIGNATURES[name] == argtypes, name
        assert _hip.RESTYPES[name] is restype, name
    assert sorted(_hip.RESTYPES) == sorted(_hip.SIGNATURES)


@pytest.mark.parametrize("helper", ["call", "query"])
def test_wrong_argument_count_never_enters_the_library(helper, monkeypatch):
    """ctypes runs f(-3, 7, 9) against argtypes = [c_int]: a call to the wrong sibling of a pair that differs by one argument
    (mmdfn_adj_build / _kind, ...) would launch.  The count is checked first, before the library is even loaded."""
    from mm_dfn_amd import _hip

    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_hip, "lib", entered)
    monkeypatch.setattr(_hip, "_libs", {})
    band = [None] * 8 + [0, 1, 0, 0, 0, 0, None]                # the 15 arguments of mmdfn_adj_build_band
    for args in (band + [None], band[:-1]):
        with pytest.raises(_hip.HipLibraryError) as e:
            getattr(_hip, helper)("mmdfn_adj_build_band", *args)
        assert "mmdfn_adj_build_band" in str(e.value) and "15" in str(e.value) and str(len(args)) in str(e.value)
    with pytest.raises(_hip.HipLibraryError):
        getattr(_hip, helper)("mmdfn_no_such_entry")


def test_call_checks_the_return_code():
    """mmdfn_adj_build_band returns -1 on its first line for B = 0 / null pointers, before any HIP call."""
    from mm_dfn_amd import build, _hip
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    band = [None] * 8 + [0, 1, 0, 0, 0, 0, None]
    with pytest.raises(_hip.HipLibraryError) as e:
        _hip.call("mmdfn_adj_build_band", *band)
    assert str(e.value) == "mmdfn_adj_build_band failed with code -1"
    assert _hip.call("mmdfn_adj_build_band", *band, allow=(-1,)) == -1
    with pytest.raises(_hip.HipLibraryError):
        _hip.call("mmdfn_adj_build_band", *band, allow=(-2,))
    assert _hip.query("mmdfn_adj_build_band", *band) == -1
    assert _hip.query("mmdfn_abi_version") == _hip.ABI_VERSION
    assert _hip.query("mmdfn_adam_state_bytes") == 64


def test_library_keeps_no_writable_state_of_its_own():
    """The C ABI is re-entrant: the production library defines no writable data symbol (nm class b / B / d / D) beyond the
    toolchain's own (reserved names: __hip_* code-object registration, _DYNAMIC, ...), the kernel handles (demangled names end
    in ')') and the per-kernel attribute memo of mmdfn_allow_big_lds."""
    import shutil
    import subprocess
    from mm_dfn_amd import build
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    nm = "/opt/rocm/llvm/bin/llvm-nm"
    if not os.path.exists(nm):
        nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm here")
    out = subprocess.run([nm, "-C", "--defined-only", build.LIBPATH], check=True, capture_output=True, text=True).stdout
    state = []
    for line in out.splitlines():
        parts = line.split(None, 2)
        if len(parts) < 3 or parts[1] not in "bBdD":
            continue
        name = parts[2]
        if re.match(r"_[_A-Z]|DW\.ref\.", name) or name.endswith(")") or name.startswith("mmdfn_allow_big_lds<"):
            continue
        state.append(name)
    assert not state, "writable host state in %s: %s" % (os.path.basename(build.LIBPATH), state)


def test_cpu_tensors_fail_loudly():
    import torch
    from mm_dfn_amd import ops, _hip
    from mm_dfn_amd.layout import DialogueLayout
    lay = DialogueLayout([3, 2], 3, "cpu")
    with pytest.raises(_hip.HipLibraryError):
        ops.build_adjacency(torch.randn(3, 5, 8), [3, 2])
