"""Float64 reference, derived elementwise bound, structured input families and a numpy model of the bf16-piece arithmetic for the
dense projection kernels (csrc/linear.hip, linear_split.hip, linear_small.hip, linear_planes.hip).

Everything here runs on the CPU.  tests/test_dense_product_ref_host.py proves the instrument (the model passes, a model with one
piece product removed or two k indices swapped does not); tests/test_dense_products_gpu.py points it at the kernels.

The bound, with u = 2^-24, per output element:

    |got - want| <= (n + 16) u S + 2^-126,        S = |X| |W|^T + |bias| + |base|

n = the number of non-zero terms the element's contraction sums (1 for a one-hot operand, K otherwise, K + K2 with a second
segment): the convention of tests/test_fusion_kernels_gpu.py.  Of the 16, two are the products the piece forms leave out
(a2b3 + a3b2 + a3b3 <= 2^-23 |a||b| per product, csrc/bf16_pieces.h); the rest covers the bias / addend / mask roundings of the
epilogue.  ReLU is 1-Lipschitz, so the bound holds behind the activation as well.  No element is excluded.

Why a one-hot family: (K + 16) u S is a worst case over K roundings, so at K = 100 .. 200 a kernel that drops a third-order piece
product (2^-16 relative per product) still passes it on dense inputs.  With ONE product per output element n is 1, the bound is
17 u |x w|, and any missing piece product is tens of bounds away; sweeping the non-zero over every k also checks the k mapping of
every fragment layout one index at a time."""
import collections

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126

Case = collections.namedtuple("Case", "name X W bias n")   # X (R, K), W (N, K), bias (N,) float32; n: terms per output element

# the six piece products (0-based piece of a, piece of b) in the order of six() in csrc/bf16_pieces.h, smallest first
PRODUCTS = collections.OrderedDict([("a3b1", (2, 0)), ("a2b1", (1, 0)), ("a2b2", (1, 1)), ("a1b3", (0, 2)), ("a1b2", (0, 1)),
                                    ("a1b1", (0, 0))])
THIRD_ORDER = ("a1b3", "a2b2", "a3b1")


def _full(rs, *shape):
    """Unit Gaussians as float32 (full mantissas), kept away from zero so that every third piece stays a normal number."""
    v = rs.randn(*shape).astype(np.float32)
    small = np.abs(v) < 2.0 ** -6
    v[small] = np.float32(1.37109375) * np.where(rs.rand(*shape) < 0.5, -1, 1).astype(np.float32)[small]
    return v


def to_bf16(v):
    """Truncate float32 values to what a bf16 holds exactly (pieces two and three become zero)."""
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _onehot(rs, rows, K, values=None):
    m = np.zeros((rows, K), np.float32)
    r = np.arange(rows)
    m[r, r % K] = _full(rs, rows) if values is None else values
    return m


def families(R, K, N, seed, expand=True, only=None):
    """Yield the named input families as Case tuples.  ``expand``: the one-hot X has max(R, K) rows, so that every k is hit (its R
    is then X.shape[0]); ``only``: restrict to these family names ('onehot' selects all three one-hot cases)."""
    rs = np.random.RandomState(seed)
    zero = np.zeros(N, np.float32)

    def want(name):
        return only is None or name in only

    Ro = max(R, K) if expand else R
    if want("onehot"):
        yield Case("onehot", _onehot(rs, Ro, K), _full(rs, N, K), zero, 1)
        yield Case("onehot_w", _full(rs, R, K), _onehot(rs, N, K), zero, 1)       # mirrored: W rows one-hot, X dense
        yield Case("bf16x", _onehot(rs, Ro, K, to_bf16(_full(rs, Ro))), _full(rs, N, K), zero, 1)
    if want("samesign"):
        yield Case("samesign", np.abs(_full(rs, R, K)), np.abs(_full(rs, N, K)), np.abs(_full(rs, N)), K)
    if want("cancel"):
        # X columns equal in pairs, W columns of the even outputs in +- pairs: want is exactly 0 there while S is a full K-term sum
        X = _full(rs, R, K)
        W = _full(rs, N, K)
        X[:, 1::2] = X[:, 0:2 * (K // 2):2]
        W[0::2, 1::2] = -W[0::2, 0:2 * (K // 2):2]
        yield Case("cancel", X, W, zero, K)
    if want("graded"):
        sr = (2.0 ** rs.randint(-20, 21, size=(R, 1))).astype(np.float32)
        sc = (2.0 ** rs.randint(-20, 21, size=(N, 1))).astype(np.float32)
        yield Case("graded", _full(rs, R, K) * sr, _full(rs, N, K) * sc, _full(rs, N) * sc[:, 0], K)
    if want("dropout"):
        X = _full(rs, R, K) * (rs.rand(R, K) < 0.5).astype(np.float32) * np.float32(2.0)
        X[::5] = 0.0                                                                # some all-zero rows
        W = _full(rs, N, K)
        W[N // 2] = 0.0                                                             # one all-zero weight row
        yield Case("dropout", X, W, _full(rs, N), K)


def want_and_bound(X, W, bias, base, n):
    """(want, bound) in float64 of X W^T + bias + base; bias / base may be None.  A second segment is passed concatenated along k."""
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64)
    want = X64 @ W64.T
    S = np.abs(X64) @ np.abs(W64).T
    if bias is not None:
        want = want + np.asarray(bias, np.float64)
        S = S + np.abs(np.asarray(bias, np.float64))
    if base is not None:
        want = want + np.asarray(base, np.float64)
        S = S + np.abs(np.asarray(base, np.float64))
    return want, (n + 16) * U * S + TINY


def worst_ratio(got, want, bound):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), "not finite"
    return float((np.abs(got - want) / bound).max())


def check(name, got, want, bound):
    """Elementwise |got - want| <= bound over every element; prints and returns the worst ratio."""
    ratio = worst_ratio(got, want, bound)
    print("RATIO %s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: error / bound = %.3f" % (name, ratio)
    return ratio


def cut(x):
    """The three bf16 pieces of float32 values by truncation (csrc/bf16_pieces.h): x = p1 + p2 + p3 up to O(2^-24 x)."""
    x = np.array(x, np.float32)
    pieces = []
    for _ in range(3):
        p = to_bf16(x)
        pieces.append(p)
        x = (x - p).astype(np.float32)                  # (exact in float32)
    return pieces


def emulate(X, W, drop=None, swap_k=None, step=16):
    """X W^T as the piece kernels form it: truncating cut, the six products in the order of six(), each product's ``step``-wide
    k-step (16; 32 in the weight-gradient kernels) added to a float32 accumulator (the exact sum of the step, rounded once).
    ``drop``: a name of PRODUCTS to leave out; ``swap_k`` = (k1, k2): exchange these two k indices of W only (a fragment-layout
    fault)."""
    X, W = np.asarray(X, np.float32), np.array(W, np.float32)
    if swap_k is not None:
        k1, k2 = swap_k
        W[:, [k1, k2]] = W[:, [k2, k1]]
    a, b = cut(X), cut(W)
    acc = np.zeros((X.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, X.shape[1], step):
        for name, (i, j) in PRODUCTS.items():
            if name == drop:
                continue
            term = a[i][:, k0:k0 + step].astype(np.float64) @ b[j][:, k0:k0 + step].astype(np.float64).T
            acc = (acc.astype(np.float64) + term).astype(np.float32)
    return acc
