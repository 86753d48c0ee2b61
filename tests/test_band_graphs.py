"""The window and speaker-chain graphs of new_graph=True without a device: the float64 restatement of both graphs against the
reference's own matrices (tests/golden/band_graphs.npz, written by tests/golden/make_golden_band_graphs.py), key construction
against plain Python loops, state-dict keys, the refusals and the binding table (no compute on a device).

Errors are max |x - x64| / max |x64|.  The reference's error against the restatement is the yardstick of the device tests
(test_band_graphs_gpu.py); here it must be below 1e-4 -- an off-by-one band or a chain mix-up moves entries by far more."""
import ctypes

import pytest
import torch

from band_graph_ref import (WINDOW_CASES, WINDOW_WIDTH, band_graph, case, err, load_gold, pack_keys, speaker_keys_loop,
                            window_keys_loop)

CFG = dict(nfeat=40, nlayers=2, nhidden=20, nclass=6, dropout=0.0, lamda=0.5, alpha=0.2, variant=True, return_feature=True,
           use_residue=True)


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def graph_cases(gold):
    for n, lengths in enumerate(WINDOW_CASES):
        c = case(gold, "win/%d/" % n)
        assert c["lengths"] == lengths
        yield "window %s" % lengths, c, window_keys_loop(lengths), WINDOW_WIDTH
    for n in range(2):
        c = case(gold, "spk/%d/" % n)
        yield "speaker batch %d %s" % (n, c["lengths"]), c, speaker_keys_loop(c["qmask"], c["lengths"]), 1


def test_restatement_against_the_reference_matrices(gold):
    seen = 0
    for name, c, pairs, width in graph_cases(gold):
        r64 = band_graph(c["x"].double(), c["lengths"], pairs, width)
        r32 = band_graph(c["x"], c["lengths"], pairs, width)
        e_ref, e32 = err(c["adj"], r64["adj"]), err(r32["adj"], r64["adj"])
        print("%-40s reference %.3e  float32 restatement %.3e" % (name, e_ref, e32))
        assert e_ref < 1e-4, name
        assert torch.equal(c["adj"] != 0, r64["adj"] != 0), name             # the same edge set, entry for entry
        seen += 1
    assert seen == 5


def test_window_edge_set_is_the_band_of_half_width_20(gold):
    c = case(gold, "win/1/")                         # [21, 22, 23]: the last fully dense tile, the first zero entries
    A = c["adj"]
    assert bool((A[:21, :21] != 0).all())
    assert float(A[21, 21 + 21]) == 0.0 and float(A[21, 21 + 20]) != 0.0
    assert int((A[21:43, 21:43] == 0).sum()) == 2 and int((A[43:, 43:] == 0).sum()) == 6
    assert float(A[:21, 21:].abs().max()) == 0.0     # block-diagonal over dialogues


def test_window_keys_against_a_loop():
    from mm_dfn_amd import ops
    for lengths in WINDOW_CASES + [[129, 4]]:
        keys = ops.window_keys(lengths, torch.device("cpu"))
        assert keys.dtype == torch.int32 and torch.equal(keys, pack_keys(window_keys_loop(lengths)))
    assert ops.window_keys([3, 2], torch.device("cpu")) is ops.window_keys([3, 2], torch.device("cpu"))      # cached


def test_window_keys_inside_an_index_scope_are_private_and_retargeted():
    from mm_dfn_amd import ops
    from mm_dfn_amd.layout import IndexScope
    shared = ops.window_keys([3, 2], torch.device("cpu"))
    scope = IndexScope()
    with scope:
        keys = ops.window_keys([3, 2], torch.device("cpu"))
        assert keys is not shared and keys is ops.window_keys([3, 2], torch.device("cpu"))
    scope.retarget([2, 3])
    assert keys.tolist() == [0, 1, 0, 1, 2] and shared.tolist() == [0, 1, 2, 0, 1]


def test_speaker_keys_against_a_loop(gold):
    from mm_dfn_amd import ops
    for n in range(2):
        c = case(gold, "spk/%d/" % n)
        want = pack_keys(speaker_keys_loop(c["qmask"], c["lengths"]))
        got = ops.speaker_keys(c["qmask"], c["lengths"])
        assert got.dtype == torch.int32 and torch.equal(got, want), n
        other = c["qmask"].clone()
        for i, L in enumerate(c["lengths"]):
            other[i, L:] = -3.0                    # the padded positions are never read
        assert torch.equal(ops.speaker_keys(other, c["lengths"]), want)
        assert torch.equal(ops.speaker_keys(c["qmask"].long(), c["lengths"]), want)
    c = case(gold, "spk/1/")                       # P = 3: speakers 1 and 2 share chain 1
    pairs = speaker_keys_loop(c["qmask"], c["lengths"])
    L0 = c["lengths"][0]
    spk = c["qmask"][0, :L0].argmax(1).tolist()
    assert [ch for ch, _ in pairs[:L0]] == [0 if s == 0 else 1 for s in spk] and {1, 2} <= set(spk)
    with pytest.raises(ValueError, match="qmask"):
        ops.speaker_keys(c["qmask"][:, :2], c["lengths"])


def test_state_dict_keys_do_not_depend_on_new_graph():
    from mm_dfn_amd import GCNII, GCNII_lyc
    for cls in (GCNII, GCNII_lyc):
        with torch.device("meta"):
            a, b = cls(**CFG, new_graph=True, reason_flag=True), cls(**CFG, new_graph=False, reason_flag=True)
        assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]


def test_refusals():
    from mm_dfn_amd import GCNII, GCNII_lyc, _hip, ops
    x = torch.randn(5, 40)
    qmask = torch.zeros(2, 3, 2)
    g = GCNII(**CFG, new_graph=True)
    with pytest.raises(ValueError, match="qmask"):
        g(x, [3, 2], None)
    with pytest.raises(ValueError, match="qmask"):
        g(x, [3, 2])
    with pytest.raises(_hip.HipLibraryError):
        g(x, [3, 2], qmask)
    lyc = GCNII_lyc(**CFG, new_graph=True)
    with pytest.raises(_hip.HipLibraryError):
        lyc.message_passing_relation_graph(x, [3, 2])
    with pytest.raises(_hip.HipLibraryError):
        lyc.message_passing_directed_speaker(x, [3, 2], qmask)
    with pytest.raises(_hip.HipLibraryError):
        ops.build_band_adjacency(x, [3, 2], ops.window_keys([3, 2], torch.device("cpu")), 20)
    with pytest.raises(NotImplementedError, match=r"model_GCN\.py") as info:
        lyc(x, [3, 2], None)
    assert "model_GCN.py" in str(info.value) and "message_passing_relation_graph" in str(info.value)
    with pytest.raises(ValueError, match="kind"):
        ops.build_adjacency(torch.randn(1, 3, 8), [3], kind="window")      # the sparse graphs are no kind of build_adjacency


def test_binding_table_lists_the_band_entry_point():
    from mm_dfn_amd import _hip
    P, I = ctypes.c_void_p, ctypes.c_int
    assert _hip.SIGNATURES["mmdfn_adj_build_band"] == [P] * 8 + [I] * 6 + [P]
    assert _hip.ABI_VERSION == 23
