"""Float64 reference, derived elementwise bounds, the decidability predicate and the case generators for the fused
embed-conv-maxpool kernels (csrc/cnn_features.hip, K18).  Everything here runs on the CPU.

    conv_i[r, t, f] = b_i[f] + sum_{k < K_i} sum_c W_i[f, c, k] E[tok[r, t + k], c],     0 <= t <= W - K_i
    pooled[r, i F + f] = max_t relu(conv_i[r, t, f]);  argmax = the LOWEST t attaining it (first_same: by content), -1 where the maximum is <= 0
    rows whose mask is 0: pooled 0, argmax -1

The bound, in the convention of tests/dense_product_ref.py (u = 2^-24):   |got - want| <= (n + 16) u S + 2^-126.
Forward: n = K_i D and S = sum |E| |W| + |b| per window; max and ReLU are 1-Lipschitz, so the pooled bound is the largest window
bound of that (row, filter).  Gradients: n = the number of non-zero terms of that gradient element, S the sum of their magnitudes.

decidable(): the comparison of argmax is exact only if no rounding can change which window wins.  For every (row, size, filter)
the float64 gap between the best window and the best competitor exceeds twice the forward bound; a competitor is a window with
DIFFERENT content (windows with the same tokens in the same order tie exactly and give identical gradients: no conflict) or
"no window at all" (value 0: the ReLU floor).  The case generators return only inputs on which EVERY element is decidable -- a
condition on the inputs, asserted on the CPU; no element is excluded on the GPU side.  Seeds are searched upward from 0.
"""
import collections

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126

Case = collections.namedtuple("Case", "name tokens table weights biases mask d_pooled seed")
Forward = collections.namedtuple("Forward", "pooled argmax bound conv")
Backward = collections.namedtuple("Backward", "d_weights d_biases d_table bw bb bt")


def windows(tokens, table, w, b):
    """(conv, S) in float64, (rows, W - K + 1, F) each: the pre-activation of every window and its sum of magnitudes."""
    E = np.asarray(table, np.float64)[np.asarray(tokens)]            # (rows, W, D)
    w64, b64 = np.asarray(w, np.float64), np.asarray(b, np.float64)
    F, D, K = w64.shape
    T = E.shape[1] - K + 1
    conv = np.zeros((E.shape[0], T, F)) + b64
    S = np.zeros((E.shape[0], T, F)) + np.abs(b64)
    for k in range(K):
        conv += E[:, k:k + T] @ w64[:, :, k].T
        S += np.abs(E[:, k:k + T]) @ np.abs(w64[:, :, k]).T
    return conv, S


def first_same(tokens, K):
    """(rows, W - K + 1) int: for every window start t the LOWEST start whose K tokens are the same in the same order.  Windows of
    equal content tie exactly in exact arithmetic; the matrix products above need not give them equal bits (a library may sum
    the rows of a product in different orders), so the winner of such a tie is taken from the CONTENT, never from the values."""
    tokens = np.asarray(tokens)
    T = tokens.shape[1] - K + 1
    wins = np.stack([tokens[:, t:t + K] for t in range(T)], 1)                  # (rows, T, K)
    same = (wins[:, :, None, :] == wins[:, None, :, :]).all(3)                   # (rows, T, T)
    return same.argmax(2)                                                        # the first True of every row


def forward(tokens, table, weights, biases, mask, skip_tap=None):
    """Forward(pooled, argmax, bound, conv): (rows, n_k F) float64 / int / float64, conv = the per-size window values.
    ``skip_tap`` = (i, k): leave tap k of size i out (a faulty instrument for the host test)."""
    mask = np.asarray(mask)
    pooled, argmax, bound, convs = [], [], [], []
    for i, (w, b) in enumerate(zip(weights, biases)):
        w = np.array(w, np.float64)
        if skip_tap is not None and skip_tap[0] == i:
            w[:, :, skip_tap[1]] = 0.0
        conv, S = windows(tokens, table, w, b)
        K, D = w.shape[2], w.shape[1]
        best = conv.max(1)
        arg = first_same(tokens, K)[np.arange(conv.shape[0])[:, None], conv.argmax(1)]
        live = (best > 0) & (mask[:, None] != 0)
        pooled.append(np.where(live, best, 0.0))
        argmax.append(np.where(live, arg, -1))
        bound.append(np.where(mask[:, None] != 0, (K * D + 16) * U * S.max(1), 0.0) + TINY)
        convs.append(conv)
    return Forward(np.concatenate(pooled, 1), np.concatenate(argmax, 1).astype(np.int64), np.concatenate(bound, 1), convs)


def backward(tokens, table, weights, argmax, d_pooled, shift=None):
    """Backward(d_weights, d_biases, d_table, bw, bb, bt): float64 gradients of sum(pooled * d_pooled) through the windows
    ``argmax`` names, and their elementwise bounds.  ``shift`` = (r, column): read that one window one position further (a faulty
    instrument for the host test)."""
    tokens = np.asarray(tokens)
    E = np.asarray(table, np.float64)
    V, D = E.shape
    rows, W = tokens.shape
    F = weights[0].shape[0]
    g = np.asarray(d_pooled, np.float64)
    dws, dbs, bws, bbs = [], [], [], []
    dt, St, nt = np.zeros((V, D)), np.zeros((V, D)), np.zeros((V, D))
    for i, w in enumerate(weights):
        w64 = np.asarray(w, np.float64)
        K = w64.shape[2]
        dw, Sw, nw = np.zeros(w64.shape), np.zeros(w64.shape), np.zeros(w64.shape)
        db, Sb, nb = np.zeros(F), np.zeros(F), np.zeros(F)
        for r in range(rows):
            for f in range(F):
                t = int(argmax[r, i * F + f])
                gv = g[r, i * F + f]
                if t < 0:
                    continue
                if shift is not None and shift == (r, i * F + f):
                    t = min(t + 1, W - K)
                db[f] += gv
                Sb[f] += abs(gv)
                nb[f] += gv != 0
                for k in range(K):
                    e = E[tokens[r, t + k]]
                    dw[f, :, k] += gv * e
                    Sw[f, :, k] += np.abs(gv * e)
                    nw[f, :, k] += (gv * e) != 0
                    term = gv * w64[f, :, k]
                    dt[tokens[r, t + k]] += term
                    St[tokens[r, t + k]] += np.abs(term)
                    nt[tokens[r, t + k]] += term != 0
        dws.append(dw)
        dbs.append(db)
        bws.append((nw + 16) * U * Sw + TINY)
        bbs.append((nb + 16) * U * Sb + TINY)
    return Backward(dws, dbs, dt, bws, bbs, (nt + 16) * U * St + TINY)


def decidable(tokens, mask, fwd, kernel_sizes):
    """True iff, for every live (row, size, filter), the best window beats every competitor by more than twice the forward bound."""
    tokens = np.asarray(tokens)
    rows, W = tokens.shape
    F = fwd.pooled.shape[1] // len(kernel_sizes)
    for i, K in enumerate(kernel_sizes):
        conv = fwd.conv[i]
        T = W - K + 1
        wins = np.stack([tokens[:, t:t + K] for t in range(T)], 1)        # (rows, T, K)
        for r in range(rows):
            if mask[r] == 0:
                continue
            same = (wins[r][:, None, :] == wins[r][None, :, :]).all(2)     # (T, T): equal content
            for f in range(F):
                col = i * F + f
                t = int(conv[r, :, f].argmax())
                best = conv[r, t, f]
                others = np.maximum(conv[r, ~same[t], f], 0.0)
                rival = max(float(others.max()) if others.size else 0.0, 0.0)
                margin = 2.0 * fwd.bound[r, col]
                if best > 0:
                    if best - rival <= margin:
                        return False
                elif best >= -margin:          # every window negative: must stay negative under rounding
                    return False
    return True


def _full(rs, *shape):
    """Unit Gaussians as float32 with full mantissas, kept away from zero (dense_product_ref._full)."""
    v = rs.randn(*shape).astype(np.float32)
    small = np.abs(v) < 2.0 ** -6
    v[small] = np.float32(1.37109375) * np.where(rs.rand(*shape) < 0.5, -1, 1).astype(np.float32)[small]
    return v


def random_inputs(rs, rows, W, V, D, F, kernel_sizes, mask=None):
    tokens = rs.randint(0, V, size=(rows, W)).astype(np.int64)
    table = _full(rs, V, D)
    weights = [_full(rs, F, D, K) for K in kernel_sizes]
    biases = [_full(rs, F) for _ in kernel_sizes]
    mask = np.ones(rows, np.float32) if mask is None else np.asarray(mask, np.float32)
    d_pooled = _full(rs, rows, len(kernel_sizes) * F)
    return tokens, table, weights, biases, mask, d_pooled


def search(name, build, kernel_sizes, max_seed=2000):
    """The first seed from 0 upward for which ``build(RandomState(seed))`` -> (tokens, table, weights, biases, mask, d_pooled) is
    decidable everywhere, as a Case."""
    for seed in range(max_seed):
        tokens, table, weights, biases, mask, d_pooled = build(np.random.RandomState(seed))
        fwd = forward(tokens, table, weights, biases, mask)
        if decidable(tokens, mask, fwd, kernel_sizes):
            return Case(name, tokens, table, weights, biases, mask, d_pooled, seed)
    raise AssertionError("%s: no decidable input among %d seeds" % (name, max_seed))


def distinct_tokens(rs, rows, W, V):
    """Every row a random arrangement of W different ids: no two windows of a row share a token at the same offset."""
    assert W <= V
    return np.stack([rs.permutation(V)[:W] for _ in range(rows)]).astype(np.int64)


def random_case(rows, W, D, F, kernel_sizes, V=23, mask=None, negative_filter=None):
    """``negative_filter`` = f: that filter of every size gets a bias of -1e4, so that none of its windows is positive."""
    name = "r%d_w%d_d%d_f%d_k%s_v%d" % (rows, W, D, F, "".join(str(k) for k in kernel_sizes), V)

    def build(rs):
        out = random_inputs(rs, rows, W, V, D, F, kernel_sizes, mask)
        if negative_filter is not None:
            for b in out[3]:
                b[negative_filter] = np.float32(-1e4)
        return out
    return search(name, build, kernel_sizes)


def onehot_case(W, D, F, kernel_sizes, c, k, V=23):
    """One non-zero table column (c) and one non-zero tap (k; the last tap of a shorter size) per size, bias 0, distinct tokens in
    a row: every window value is ONE product, so n = 1 and a missing piece product is tens of bounds away (the argument of
    tests/dense_product_ref.py)."""
    def build(rs):
        _, table, weights, biases, mask, d_pooled = random_inputs(rs, 2, W, V, D, F, kernel_sizes)
        col = table[:, c].copy()
        table[:] = 0.0
        table[:, c] = col
        for w, K in zip(weights, kernel_sizes):
            tap = w[:, c, min(k, K - 1)].copy()
            w[:] = 0.0
            w[:, c, min(k, K - 1)] = tap
        return distinct_tokens(rs, 2, W, V), table, weights, [np.zeros_like(b) for b in biases], mask, d_pooled
    return search("onehot_c%d_k%d" % (c, k), build, kernel_sizes)


def onehot_weights_case(D, K, F, n_sizes, first, W=20, V=32):
    """A dense table and ONE non-zero tap per filter: filter j of size i (all sizes K) holds pair number first + F i + j (modulo
    D K) of the sweep (c, k) = divmod(pair, K); bias 0, distinct tokens in a row.  Every window value is one product."""
    kernel_sizes = (K,) * n_sizes

    def build(rs):
        _, table, weights, biases, mask, d_pooled = random_inputs(rs, 2, W, V, D, F, kernel_sizes)
        for i, w in enumerate(weights):
            full = w.copy()
            w[:] = 0.0
            for j in range(F):
                c, k = divmod((first + F * i + j) % (D * K), K)
                w[j, c, k] = full[j, c, k]
        return distinct_tokens(rs, 2, W, V), table, weights, [np.zeros_like(b) for b in biases], mask, d_pooled
    return search("onehot_w_first%d" % first, build, kernel_sizes)


def onehot_forward_bound(case):
    """The forward bound of a one-product case with n = 1 instead of K D: 17 u |E W| per window, the largest of the (row, filter)."""
    out = []
    for w, b in zip(case.weights, case.biases):
        _, S = windows(case.tokens, case.table, w, b)
        out.append(17 * U * S.max(1) + TINY)
    return np.concatenate(out, 1)


def planted_case(W, D, F, kernel_sizes, place, V=23, again=None):
    """A random case (2 rows) in which filter 0 of the FIRST size has its maximum at window t = place(K): the id V - 1 occurs only
    in that window (all K of its tokens), and its embedding is 4 sign(sum_k W_0[0, :, k]) plus a little noise, so the window's
    value is about 4 sum_c |sum_k W_0[0, c, k]|.  ``again``: a second, identical window at again(K) (an exact tie)."""
    K = kernel_sizes[0]

    def build(rs):
        tokens, table, weights, biases, mask, d_pooled = random_inputs(rs, 2, W, V, D, F, kernel_sizes)
        tokens[tokens == V - 1] = 0
        for t in [place(K)] + ([] if again is None else [again(K)]):
            tokens[:, t:t + K] = V - 1
        table[V - 1] = np.float32(4.0) * np.sign(weights[0][0].sum(1)).astype(np.float32) + table[V - 1] * np.float32(0.01)
        return tokens, table, weights, biases, mask, d_pooled
    return search("planted_w%d_t%d" % (W, place(K)), build, kernel_sizes)


def check(name, got, want, bound):
    """Elementwise |got - want| <= bound over every element; prints and returns the worst ratio."""
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s: not finite" % name
    ratio = float((np.abs(got - want) / bound).max()) if got.size else 0.0
    print("RATIO %s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: error / bound = %.3f" % (name, ratio)
    return ratio


# ---- the module: CNNFeatureExtractor (reference model.py:1410-1443) and its golden cases ---------------------------------------
# name -> constructor arguments (vocab_size, embedding_dim, output_size, filters, kernel_sizes, dropout), x (num_utt, batch,
# num_words), utterances per dialogue, whether the table is a frozen pretrained one, whether an LSTMModel(100, 100, 32, 6 classes)
# and MaskedNLLLoss follow (as case a of tests/lstm_model_ref.py).  tests/golden/make_golden_cnn_features.py writes the
# reference's outputs for exactly these.
MODEL_CASES = {
    "a": dict(args=(60, 100, 100, 50, (3, 4, 5), 0.0), x=(5, 3, 12), lengths=[5, 3, 1], frozen=False, lstm=False),
    "b": dict(args=(40, 300, 100, 50, (3, 4, 5), 0.0), x=(2, 2, 7), lengths=[2, 1], frozen=True, lstm=False),
    "c": dict(args=(60, 100, 100, 50, (3, 4, 5), 0.0), x=(5, 3, 12), lengths=[5, 3, 1], frozen=False, lstm=True),
}
LSTM_ARGS = (100, 100, 32)          # D_m, D_e, D_h of case c's LSTMModel
N_CLASSES = 6
# rows of the stored gradients (every k-th row; the digests cover every parameter in full)
MODEL_GRAD_ROWS = {"embedding.weight": 4, "convs.0.weight": 5, "convs.2.weight": 5, "fc.weight": 4}


def model_inputs(name, seed):
    """x (num_utt, batch, num_words) token ids AS FLOATS (the reference's dataset delivers them so), qmask (L, B, 2), umask (B, L),
    label (B, L) int64, class weights (C), G (L, B, output_size) > 0, scaled by 1 / G.numel(): the cotangent of cases a / b (their
    "loss" is sum(features G), a mean of order 1 without cancellation, features being >= 0),
    pretrained (V, D) float32 vectors (used by the frozen case).  Utterances beyond a dialogue's length are all-zero ids."""
    import torch
    c = MODEL_CASES[name]
    L, B, W = c["x"]
    V, D, out = c["args"][0], c["args"][1], c["args"][2]
    rs = np.random.RandomState(seed)
    x = rs.randint(0, V, size=(L, B, W)).astype(np.float32)
    umask = np.zeros((B, L), np.float32)
    for b, n in enumerate(c["lengths"]):
        umask[b, :n] = 1.0
        x[n:, b] = 0.0
    qmask = np.zeros((L, B, 2), np.float32)
    qmask[:, :, 0] = 1.0
    label = rs.randint(0, N_CLASSES, size=(B, L)).astype(np.int64)
    weight = rs.uniform(0.5, 1.5, size=(N_CLASSES,)).astype(np.float32)
    G = (np.abs(rs.standard_normal((L, B, out))) / (L * B * out)).astype(np.float32)
    pretrained = (rs.standard_normal((V, D)) / np.sqrt(D)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, qmask, umask, label, weight, G)) + (pretrained,)


def module_forward(params, x, umask, keep=None, p=0.0, prefix=""):
    """CNNFeatureExtractor.forward in the dtype of ``params`` (state_dict keys) with torch's CPU ops; ``keep``: 0 / 1 flags of the
    dropout on the pooled block (rows, n_k F), scaled by 1 / (1 - p).  Returns (features (L, B, out), pooled, fc pre-activation)."""
    import torch
    import torch.nn.functional as F_
    dt = params[prefix + "embedding.weight"].dtype
    L, B, W = x.shape
    emb = F_.embedding(x.long().view(-1, W), params[prefix + "embedding.weight"]).transpose(1, 2)
    pooled = []
    i = 0
    while prefix + "convs.%d.weight" % i in params:
        conv = torch.relu(F_.conv1d(emb, params[prefix + "convs.%d.weight" % i], params[prefix + "convs.%d.bias" % i]))
        pooled.append(conv.max(2)[0])
        i += 1
    pooled = torch.cat(pooled, 1)
    if keep is not None:
        pooled = pooled * keep.to(dt).view(-1)[:pooled.numel()].view(pooled.shape) * (1.0 / (1.0 - p) if p < 1.0 else 0.0)
    pre = pooled @ params[prefix + "fc.weight"].t() + params[prefix + "fc.bias"]
    mask = umask.to(dt).t().unsqueeze(2)
    return torch.relu(pre).view(L, B, -1) * mask, pooled, pre


def model_decidable(params, x, umask):
    """The max-pool comparisons of a module case are decidable (decidable() above) on the rows the mask keeps."""
    ks, ws, bs = [], [], []
    i = 0
    while "convs.%d.weight" % i in params:
        ws.append(params["convs.%d.weight" % i].detach().numpy())
        bs.append(params["convs.%d.bias" % i].detach().numpy())
        ks.append(ws[-1].shape[2])
        i += 1
    tokens = x.long().view(-1, x.shape[2]).numpy()
    mask = umask.t().reshape(-1).numpy()
    fwd = forward(tokens, params["embedding.weight"].detach().numpy(), ws, bs, mask)
    return decidable(tokens, mask, fwd, ks)


def digest(g):
    """tests/test_oracle_golden._digest's format."""
    g = g.detach().double().reshape(-1)
    return np.array([g.sum().item(), g.abs().sum().item(), (g * g).sum().item()])
