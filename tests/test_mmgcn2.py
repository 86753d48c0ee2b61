"""MM_GCN2 and the arccos graph kind without a device: state-dict keys against the reference's, the constructions that are
refused, the new entry points' argument checks (no compute)."""
import ctypes
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# how the reference constructs it (model.py:956-958)
DEFAULT = dict(nfeat=200, nlayers=64, nhidden=100, nclass=6, dropout=0.4, lamda=0.5, alpha=0.1, variant=True,
               return_feature=True, use_residue=True)


def test_state_dict_keys_and_shapes_match_the_reference():
    from mm_dfn_amd import MM_GCN2
    want = [line.split() for line in open(os.path.join(GOLD, "state_dict_keys_mmgcn2.txt")) if line.strip()]
    with torch.device("meta"):
        m = MM_GCN2(**DEFAULT)
    got = [[k] + [str(d) for d in v.shape] for k, v in m.state_dict().items()]
    assert got == want
    assert len(got) == 64 + 6 and got[0] == ["convs.0.weight", "200", "100"] and got[-1] == ["fcs.2.bias", "100"]


@pytest.mark.parametrize("kw", [dict(new_graph=True), dict(modals='al'), dict(return_feature=False)])
def test_unsupported_constructions_raise(kw):
    from mm_dfn_amd import MM_GCN2
    cfg = dict(DEFAULT, nlayers=2)
    cfg.update(kw)
    with pytest.raises(NotImplementedError, match=r"model_mm\.py"):
        MM_GCN2(**cfg)


def test_gcnii_lyc_without_adjacency_still_refuses_new_graph():
    from mm_dfn_amd import GCNII_lyc
    m = GCNII_lyc(8, 1, 8, 6, 0.0, 0.5, 0.1, True, True, True, new_graph=True)
    with pytest.raises(NotImplementedError, match=r"model_GCN\.py"):
        m(torch.randn(3, 8), [3], None)


def test_build_adjacency_refuses_an_unknown_kind():
    from mm_dfn_amd import ops
    with pytest.raises(ValueError, match="kind"):
        ops.build_adjacency(torch.randn(1, 3, 8), [3], kind="cosine")


def test_binding_table_lists_the_kind_entry_points():
    from mm_dfn_amd import _hip
    for name in ("mmdfn_adj_build", "mmdfn_adj_build_bwd"):
        old, new = _hip.SIGNATURES[name], _hip.SIGNATURES[name + "_kind"]
        assert new == old[:-1] + [ctypes.c_int, old[-1]]           # today's argument list plus `int kind` in front of the stream
    assert _hip.ABI_VERSION == 23


def test_entry_points_refuse_other_kinds_before_any_launch():
    """kind outside {0, 1} is an argument error (-1), checked before anything is enqueued: null pointers are never read."""
    from mm_dfn_amd import build
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    from mm_dfn_amd import _hip
    handle = ctypes.CDLL(build.LIBPATH)
    for name, nptr in (("mmdfn_adj_build_kind", 11), ("mmdfn_adj_build_bwd_kind", 19)):
        fn = getattr(handle, name)
        fn.argtypes, fn.restype = _hip.SIGNATURES[name], ctypes.c_int
        for kind in (-1, 2, 7):
            assert fn(*([None] * nptr), 1, 1, 4, 8, 4, 1.0, kind, None) == -1, (name, kind)
