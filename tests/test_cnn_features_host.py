"""CPU: the host-side contract of CNNFeatureExtractor and the K18 entry points (csrc/cnn_features.hip): state_dict keys against
the reference's, the frozen pretrained table, every refusal (constructor, forward, the entry points' -1 before any HIP call),
the float64 restatement of the module (tests/cnn_features_ref.py) against the reference's goldens, and DailyDialogueDataset +
collate_fn on a synthetic pickle."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cnn_features_ref as CR
from mm_dfn_amd import CNNFeatureExtractor, _hip, cnn_features, data, synthetic

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _keys(path):
    with open(path) as f:
        return [(ln.split()[0], tuple(int(d) for d in ln.split()[1:])) for ln in f if ln.strip()]


def test_state_dict_keys_and_shapes_match_the_reference():
    m = CNNFeatureExtractor(60, 100, 100, 50, (3, 4, 5), 0.5)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _keys(os.path.join(GOLD, "state_dict_keys_cnn_features.txt"))
    assert m.feature_dim == 100 and m.dropout.p == 0.5 and m.kernel_sizes == (3, 4, 5)
    assert isinstance(m.embedding, torch.nn.Embedding) and isinstance(m.convs[0], torch.nn.Conv1d)
    wide = CNNFeatureExtractor(10, 300, 64, 64, [1, 2, 7, 8], 0.0)
    assert tuple(wide.fc.weight.shape) == (64, 256) and tuple(wide.convs[3].weight.shape) == (64, 300, 8)


def test_pretrained_embeddings_are_frozen():
    m = CNNFeatureExtractor(60, 100, 100, 50, (3, 4, 5), 0.5)
    assert m.embedding.weight.requires_grad
    vec = np.random.RandomState(0).randn(60, 100)
    m.init_pretrained_embeddings_from_numpy(vec)
    assert not m.embedding.weight.requires_grad and m.embedding.weight.dtype == torch.float32
    assert torch.equal(m.embedding.weight, torch.from_numpy(vec).float())
    assert list(m.state_dict())[0] == "embedding.weight"
    assert [k for k, p in m.named_parameters() if not p.requires_grad] == ["embedding.weight"]


@pytest.mark.parametrize("args, word", [
    ((60, 102, 100, 50, (3, 4, 5), 0.0), "embedding_dim"), ((60, 308, 100, 50, (3,), 0.0), "embedding_dim"),
    ((60, 0, 100, 50, (3,), 0.0), "embedding_dim"), ((60, 100, 100, 0, (3,), 0.0), "filters"),
    ((60, 100, 100, 65, (3,), 0.0), "filters"), ((60, 100, 100, 50, (), 0.0), "kernel sizes"),
    ((60, 100, 100, 50, (1, 2, 3, 4, 5), 0.0), "kernel sizes"), ((60, 100, 100, 50, (3, 9), 0.0), "K <= 8"),
    ((60, 100, 100, 50, (0,), 0.0), "K <= 8")])
def test_constructor_refusals_name_the_limit(args, word):
    with pytest.raises(NotImplementedError, match="CNNFeatureExtractor") as e:
        CNNFeatureExtractor(*args)
    assert word in str(e.value)


@pytest.mark.parametrize("shape, word", [((3, 2, 4), "max(kernel_sizes) <= num_words <= 512"), ((3, 2, 513), "num_words <= 512"),
                                         ((0, 2, 12), "rows >= 1"), ((3, 0, 12), "rows >= 1")])
def test_forward_refusals_name_the_limit(shape, word):
    """The launch-time part of the envelope raises NotImplementedError before the device is asked for anything (CPU tensors)."""
    m = CNNFeatureExtractor(60, 100, 100, 50, (3, 4, 5), 0.0)
    with pytest.raises(NotImplementedError, match="CNNFeatureExtractor") as e:
        m(torch.zeros(*shape), torch.ones(shape[1], shape[0]))
    assert word in str(e.value)
    with pytest.raises(NotImplementedError, match="cnn_pool") as e:
        cnn_features.cnn_pool(torch.zeros(shape[0] * shape[1], shape[2], dtype=torch.int64), m.embedding.weight,
                              [c.weight for c in m.convs], [c.bias for c in m.convs], torch.ones(shape[0] * shape[1]))
    assert word in str(e.value)


def test_cpu_tensors_raise():
    m = CNNFeatureExtractor(60, 100, 100, 50, (3, 4, 5), 0.0)
    with pytest.raises(_hip.HipLibraryError):
        m(torch.zeros(3, 2, 12), torch.ones(2, 3))
    with pytest.raises(_hip.HipLibraryError):
        cnn_features.cnn_pool(torch.zeros(2, 12, dtype=torch.int64), m.embedding.weight, [c.weight for c in m.convs],
                              [c.bias for c in m.convs], torch.ones(2))


def test_header_declares_the_entry_points_and_the_abi_stays_23():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert _hip.ABI_VERSION == 23
    assert _hip.SIGNATURES["mmdfn_cnn_pool_fwd"] == [P] * 8 + [L] + [I] * 5 + [P, P]
    assert _hip.SIGNATURES["mmdfn_cnn_pool_bwd"] == [P] * 6 + [L] + [I] * 5 + [P, P]
    assert _hip.SIGNATURES["mmdfn_cnn_table_keys"] == [P] * 3 + [L] + [I] * 4 + [P, P]
    assert _hip.SIGNATURES["mmdfn_cnn_table_bwd"] == [P] * 6 + [L] + [I] * 4 + [P, P]
    assert _hip.SIGNATURES["mmdfn_cnn_tile_words"] == [] and _hip.SIGNATURES["mmdfn_cnn_rows_per_group"] == []
    assert _hip.RESTYPES["mmdfn_cnn_planes_bytes"] is L and _hip.RESTYPES["mmdfn_cnn_table_entries"] is L


def test_refused_calls_return_minus_one_before_any_device_call():
    """One violation per call, never a valid call: nothing may launch here (no device needed)."""
    from mm_dfn_amd import build
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    P = ctypes.c_void_p(4096)                                   # a non-null value that is never dereferenced
    arr = lambda n=3: (ctypes.c_void_p * n)(*[4096] * n)        # host arrays: these ARE read, their entries are not
    ks = _hip.int_array([3, 4, 5])
    assert _hip.query("mmdfn_cnn_tile_words") >= 1 and _hip.query("mmdfn_cnn_rows_per_group") >= 1
    assert _hip.query("mmdfn_cnn_planes_bytes", 100, 50, 3, ks) == 12 * 4 * 4 * 3 * 64 * 16
    assert _hip.query("mmdfn_cnn_table_entries", 7, 50, 3, ks) == 7 * 150 * 5
    fwd = lambda rows, W, V, D, F, n_k, k, tok=P, w=None: _hip.call(
        "mmdfn_cnn_pool_fwd", tok, P, arr() if w is None else w, arr(), P, P, P, P, rows, W, V, D, F, n_k, k, None, allow=(-1,))
    bwd = lambda rows, W, V, D, F, n_k, k: _hip.call("mmdfn_cnn_pool_bwd", P, P, P, P, arr(), arr(), rows, W, V, D, F, n_k, k,
                                                     None, allow=(-1,))
    bad = [(0, 12, 60, 100, 50, 3, ks), (2, 4, 60, 100, 50, 3, ks), (2, 513, 60, 100, 50, 3, ks), (2, 12, 0, 100, 50, 3, ks),
           (2, 12, 60, 102, 50, 3, ks), (2, 12, 60, 308, 50, 3, ks), (2, 12, 60, 100, 0, 3, ks), (2, 12, 60, 100, 65, 3, ks),
           (2, 12, 60, 100, 50, 0, ks), (2, 12, 60, 100, 50, 5, _hip.int_array([1, 2, 3, 4, 5])),
           (2, 12, 60, 100, 50, 3, _hip.int_array([3, 9, 5])), (2, 12, 60, 100, 50, 3, _hip.int_array([3, 0, 5])),
           (2, 12, 60, 100, 50, 3, None)]
    for a in bad:
        assert fwd(*a) == -1, a
        assert bwd(*a) == -1, a
    assert fwd(2, 12, 60, 100, 50, 3, ks, tok=None) == -1
    assert fwd(2, 12, 60, 100, 50, 3, ks, w=(ctypes.c_void_p * 3)(4096, None, 4096)) == -1
    assert _hip.query("mmdfn_cnn_planes_bytes", 102, 50, 3, ks) == -1
    assert _hip.call("mmdfn_cnn_table_keys", P, P, None, 2, 12, 60, 50, 3, ks, None, allow=(-1,)) == -1
    assert _hip.call("mmdfn_cnn_table_bwd", P, P, P, arr(), P, None, 2, 60, 100, 50, 3, ks, None, allow=(-1,)) == -1
    assert _hip.call("mmdfn_cnn_table_bwd", P, P, P, arr(), P, P, 0, 60, 100, 50, 3, ks, None, allow=(-1,)) == -1


@pytest.mark.parametrize("name", sorted(n for n, c in CR.MODEL_CASES.items() if not c["lstm"]))
def test_float64_restatement_reproduces_the_reference_goldens(name):
    """module_forward (what the GPU tests compare with) against the reference's own outputs: features, loss, gradients.  (Case c
    adds the LSTMModel, whose restatement tests/test_lstm_model_host.py checks.)"""
    g = np.load(os.path.join(GOLD, "cnn_features.npz"), allow_pickle=False)
    seed = int(g["seed"])
    c = CR.MODEL_CASES[name]
    x, qmask, umask, label, weight, G, pretrained = CR.model_inputs(name, seed + 1)
    sd = synthetic.seeded_state_dict(CNNFeatureExtractor(*c["args"]).state_dict(), seed)
    if c["frozen"]:
        sd["embedding.weight"] = torch.from_numpy(pretrained)
    P = {k: v.double().requires_grad_(not (c["frozen"] and k == "embedding.weight")) for k, v in sd.items()}
    feats, _, _ = CR.module_forward(P, x, umask)
    loss = (feats * G.double()).sum()
    loss.backward()
    assert np.abs(feats.detach().numpy() - g[name + "/features"]).max() < 1e-4
    assert abs(loss.item() - float(g[name + "/loss"])) < 1e-5
    assert (name + "/digest/embedding.weight" in g.files) == (not c["frozen"])
    for k, prm in P.items():
        if prm.grad is None:
            continue
        want = g[name + "/digest/" + k]
        assert abs(CR.digest(prm.grad)[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
        if k in CR.MODEL_GRAD_ROWS:
            rows = g[name + "/grad/" + k]
            assert np.abs(prm.grad[::CR.MODEL_GRAD_ROWS[k]].numpy() - rows).max() / np.abs(rows).max() < 2e-4, k
    assert CR.model_decidable({k: v.detach().float() for k, v in P.items()}, x, umask)


def test_daily_dialogue_dataset_and_collate(tmp_path):
    path = data.write_synthetic_dailydialog_pickle(str(tmp_path / "dd.pkl"), lengths=(3, 1, 2), n_words=12, vocab_size=60)
    ds = data.DailyDialogueDataset("train", path)
    assert len(ds) == 3 and len(data.DailyDialogueDataset("test", path)) == 1 and len(data.DailyDialogueDataset("valid", path)) == 1
    tokens, qmask, umask, label, conv = ds[0]
    assert tuple(tokens.shape) == (3, 12) and tokens.dtype == torch.float32 and tuple(qmask.shape) == (3, 2)
    assert umask.dtype == torch.float32 and tuple(umask.shape) == (3,) and label.dtype == torch.int64 and conv == "conv000"
    assert ((qmask.sum(1) == 1).all()) and float(tokens.max()) < 60 and float(tokens.min()) >= 0
    batch = ds.collate_fn([ds[i] for i in range(3)])
    x, q, um, lab, ids = batch
    assert tuple(x.shape) == (3, 3, 12) and x.dtype == torch.float32            # time-major
    assert tuple(q.shape) == (3, 3, 2)
    assert tuple(um.shape) == (3, 3) and tuple(lab.shape) == (3, 3) and lab.dtype == torch.int64      # batch-major
    assert um.tolist() == [[1, 1, 1], [1, 0, 0], [1, 1, 0]]
    assert ids == ["conv000", "conv001", "conv002"]
    assert float(x[1:, 1].abs().max()) == 0.0 and float(x[2, 2].abs().max()) == 0.0 and float(q[1:, 1].abs().max()) == 0.0
    assert torch.equal(x[:, 0], ds[0][0]) and torch.equal(lab[2, :2], ds[2][3])
    with pytest.raises(ValueError):
        data.DailyDialogueDataset("dev", path)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=ds.collate_fn)
    assert [tuple(b[0].shape) for b in loader] == [(3, 2, 12), (2, 1, 12)]
