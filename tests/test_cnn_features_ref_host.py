"""The instrument of tests/test_cnn_feature_kernels_gpu.py is right and bites (CPU only): the float64 reference of
tests/cnn_features_ref.py equals torch's float64 embedding -> conv1d -> relu -> max_pool1d and its autograd; a reference with one
tap removed, or one argmax shifted by one, fails the derived bounds; the generated cases are decidable."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import cnn_features_ref as R

KS = (3, 4, 5)


def torch_reference(case):
    tok = torch.from_numpy(case.tokens)
    table = torch.from_numpy(case.table).double().requires_grad_(True)
    ws = [torch.from_numpy(w).double().requires_grad_(True) for w in case.weights]
    bs = [torch.from_numpy(b).double().requires_grad_(True) for b in case.biases]
    emb = F_.embedding(tok, table).transpose(1, 2)
    pooled = torch.cat([F_.max_pool1d(torch.relu(F_.conv1d(emb, w, b)), emb.shape[2] - w.shape[2] + 1).squeeze(2)
                        for w, b in zip(ws, bs)], 1)
    pooled = pooled * torch.from_numpy(case.mask).double()[:, None]
    (pooled * torch.from_numpy(case.d_pooled).double()).sum().backward()
    return pooled.detach().numpy(), table.grad.numpy(), [w.grad.numpy() for w in ws], [b.grad.numpy() for b in bs]


@pytest.fixture(scope="module")
def case():
    return R.random_case(3, 9, 8, 5, KS, mask=[1, 0, 1])


def test_reference_equals_torch_float64(case):
    fwd = R.forward(case.tokens, case.table, case.weights, case.biases, case.mask)
    bwd = R.backward(case.tokens, case.table, case.weights, fwd.argmax, case.d_pooled)
    pooled, dtable, dws, dbs = torch_reference(case)
    np.testing.assert_allclose(fwd.pooled, pooled, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(bwd.d_table, dtable, rtol=1e-12, atol=1e-13)
    for i in range(len(KS)):
        np.testing.assert_allclose(bwd.d_weights[i], dws[i], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(bwd.d_biases[i], dbs[i], rtol=1e-12, atol=1e-13)
    assert (fwd.argmax[1] == -1).all() and (fwd.pooled[1] == 0).all()
    assert ((fwd.argmax >= 0) == (fwd.pooled > 0)).all()


def test_lowest_index_wins_a_tie():
    """Two windows with the same content: the reference reports the first, as torch's max_pool1d does."""
    rs = np.random.RandomState(0)
    tokens, table, weights, biases, mask, _ = R.random_inputs(rs, 1, 8, 9, 4, 3, (2,))
    tokens[0] = [1, 2, 3, 1, 2, 4, 1, 2]
    fwd = R.forward(tokens, table, weights, biases, mask)
    emb = F_.embedding(torch.from_numpy(tokens), torch.from_numpy(table).double()).transpose(1, 2)
    conv = torch.relu(F_.conv1d(emb, torch.from_numpy(weights[0]).double(), torch.from_numpy(biases[0]).double()))
    _, idx = F_.max_pool1d(conv, 7, return_indices=True)
    want = np.where(fwd.pooled[0] > 0, idx[0, :, 0].numpy(), -1)
    assert (fwd.argmax[0] == want).all()


def test_a_missing_tap_fails_the_bound(case):
    fwd = R.forward(case.tokens, case.table, case.weights, case.biases, case.mask)
    R.check("self", fwd.pooled, fwd.pooled, fwd.bound)
    for i, K in enumerate(KS):
        for k in range(K):
            bad = R.forward(case.tokens, case.table, case.weights, case.biases, case.mask, skip_tap=(i, k))
            with pytest.raises(AssertionError):
                R.check("tap %d of size %d removed" % (k, K), bad.pooled, fwd.pooled, fwd.bound)


def test_a_shifted_argmax_fails_the_bound(case):
    fwd = R.forward(case.tokens, case.table, case.weights, case.biases, case.mask)
    bwd = R.backward(case.tokens, case.table, case.weights, fwd.argmax, case.d_pooled)
    F = case.weights[0].shape[0]
    r, col = [(r, c) for r in (0, 2) for c in range(F) if 0 <= fwd.argmax[r, c] < case.tokens.shape[1] - KS[0]][0]
    bad = R.backward(case.tokens, case.table, case.weights, fwd.argmax, case.d_pooled, shift=(r, col))
    with pytest.raises(AssertionError):
        R.check("dW with one window shifted", bad.d_weights[0], bwd.d_weights[0], bwd.bw[0])
    with pytest.raises(AssertionError):
        R.check("dEmb with one window shifted", bad.d_table, bwd.d_table, bwd.bt)


def test_generated_cases_are_decidable(case):
    cases = [case, R.random_case(2, 37, 100, 50, KS), R.onehot_case(12, 8, 3, (2, 8), 5, 1),
             R.planted_case(40, 8, 4, KS, lambda K: 0), R.planted_case(40, 8, 4, KS, lambda K: 40 - K)]
    for c in cases:
        ks = tuple(w.shape[2] for w in c.weights)
        fwd = R.forward(c.tokens, c.table, c.weights, c.biases, c.mask)
        assert R.decidable(c.tokens, c.mask, fwd, ks), c.name
    for c, t in ((cases[3], 0), (cases[4], 37)):
        fwd = R.forward(c.tokens, c.table, c.weights, c.biases, c.mask)
        assert (fwd.argmax[:, 0] == t).all(), (c.name, fwd.argmax[:, 0])


def test_undecidable_inputs_are_recognised():
    """Two windows of different content whose values differ by one ulp of one term: the predicate says no."""
    rs = np.random.RandomState(1)
    tokens, table, weights, biases, mask, _ = R.random_inputs(rs, 1, 5, 5, 4, 1, (2,))
    tokens[0] = [0, 1, 4, 2, 3]
    table[:] = np.abs(table)
    weights[0][:] = np.abs(weights[0])
    biases[0][:] = 0
    table[4] = -table[4]                                              # the windows that hold token 4 lose
    table[2] = table[0]
    table[3] = table[1]
    table[3, 0] = np.nextafter(table[1, 0], np.float32(4.0))          # window (2, 3) is one ulp of one term above window (0, 1)
    fwd = R.forward(tokens, table, weights, biases, mask)
    assert fwd.argmax[0, 0] == 3
    assert not R.decidable(tokens, mask, fwd, (2,))


def test_ties_are_decided_by_content_not_by_the_bits_of_a_product():
    """first_same names the lowest window of equal content; forward reports it even where the later copy has the larger bits."""
    tokens = np.array([[1, 2, 3, 1, 2, 4, 1, 2], [5, 5, 5, 5, 5, 5, 5, 5]])
    assert R.first_same(tokens, 2).tolist() == [[0, 1, 2, 0, 4, 5, 0], [0] * 7]
    assert R.first_same(tokens, 8).tolist() == [[0], [0]]
    rs = np.random.RandomState(3)
    _, table, weights, biases, mask, _ = R.random_inputs(rs, 2, 8, 9, 4, 3, (2,))
    fwd = R.forward(tokens, table, weights, biases, mask)
    assert set(fwd.argmax[1].tolist()) <= {0, -1}
    assert all(t in (-1, 0, 1, 2, 4, 5) for t in fwd.argmax[0].tolist())
