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
