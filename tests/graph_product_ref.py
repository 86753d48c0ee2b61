"""Float64 references, derived elementwise bounds and structured input families for the graph propagation kernels: K6 and its
transpose (csrc/propagate.hip, propagate_split.hip), K6' (csrc/tile_dot.hip and its bf16-piece form) and the fused K6 + K7 strip
launch (csrc/gcn_small.hip).

Everything here runs on the CPU.  tests/test_graph_product_ref_host.py proves the instrument (a float32 evaluation of every
operation passes every family; the same evaluation with one cross term dropped, two k columns swapped, a tile transposed, a
clamped row left unmasked, a padding NaN let in, eight contraction columns left out or the residual operands exchanged does not);
tests/test_graph_products_gpu.py points it at the kernels.

The bounds, with u = 2^-24, per output element and with no element left out (the convention of tests/dense_product_ref.py):

    K6, K6^T   |got - A H| <= (n + 16) u (|A| |H|) + 2^-126         n = the non-zeros of the row of A (of A^T)
    K6' tile   |got - X Y^T| <= (K + 16) u (|X| |Y|^T)              (+ |old| inside the bracket in accumulate mode)
    K6' cross  |got - (X_m.Y_n + X_n.Y_m)| <= (2 K + 16) u (|X_m|.|Y_n| + |X_n|.|Y_m|)
    fused      chained through hi -> P = [hi | h0] W -> pre -> out, see fused_reference().

The adjacency families:

    perm      every tile row p holds ONE non-zero, at column (p + s) mod L; s = shift + 5 i + m moves with the dialogue i and the
              modality m, so over a length list it sweeps the columns; no cross terms.  n = 1: the bound is 17 u |a h|, every k of
              every fragment layout is checked one index at a time and a missing bf16-piece product is tens of bounds away.
    cross     zero tiles, dense cross diagonals (n = M - 1).
    dense     util.random_block_adjacency: non-symmetric tiles + cross, so A^T != A.
    samesign  all-positive A (the callers pair it with an all-positive H): no cancellation hides a dropped term.
    graded    the dense family with tile rows and columns scaled by powers of two, 2^-20 .. 2^20 in all.

Operands of the kernels sit in wider buffers whose other columns are NaN (wide()): the strided ldh / ldo forms.  The output view is
pre-filled with NaN; it must come back finite and the columns outside it must keep their bits (check_wide())."""
import collections
import functools

import numpy as np
import torch

from dense_product_ref import TINY, U, _full, worst_ratio
from mm_dfn_amd.layout import DialogueLayout, pair_list
from util import random_block_adjacency

FAMILIES = ("perm", "cross", "dense", "samesign", "graded")

Adjacency = collections.namedtuple("Adjacency", "lengths M family tiles cross dense tile_list")
# tiles: flat float32 block-tile storage (padding columns L .. ld-1 zero or NaN); cross: (npairs, N) float32; dense: (MN, MN) float64;
# tile_list: the L x L float32 tiles, dialogue-major then modality (what BlockTileAdjacency.from_parts takes)


def check(name, got, want, bound):
    """Elementwise |got - want| <= bound over every element; prints and returns the worst ratio."""
    ratio = worst_ratio(got, want, bound)
    print("RATIO %s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: error / bound = %.3f" % (name, ratio)
    return ratio


def layout(lengths, M):
    return DialogueLayout.get(list(lengths), M, torch.device("cpu"))


def _seed(lengths, M, family):
    return (sum((i + 1) * L for i, L in enumerate(lengths)) * 31 + 7 * M + FAMILIES.index(family)) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=12)
def adjacency(lengths, M, family, nan_pad=False, shift=0):
    """Block adjacency of ``family`` over the dialogue ``lengths`` (a tuple) and M modalities.  ``nan_pad``: the padding columns
    L .. ld-1 of every tile row are NaN (they are not data and must never reach a product)."""
    assert family in FAMILIES, family
    lengths = tuple(int(L) for L in lengths)
    lay = layout(lengths, M)
    N = lay.N
    rs = np.random.RandomState(_seed(lengths, M, family))
    if family in ("dense", "samesign", "graded"):
        _, _, tl, cr = random_block_adjacency(_seed(lengths, M, family), list(lengths), M, "cpu")
        tile_list = [t.numpy().copy() for t in tl]
        cross = cr.numpy().copy()
        if family == "samesign":
            tile_list = [np.abs(t) for t in tile_list]
            cross = np.abs(cross)
        if family == "graded":
            for t in tile_list:
                L = t.shape[0]
                t *= (2.0 ** rs.randint(-10, 11, size=(L, 1))).astype(np.float32)
                t *= (2.0 ** rs.randint(-10, 11, size=(1, L))).astype(np.float32)
            cross *= (2.0 ** rs.randint(-20, 21, size=cross.shape)).astype(np.float32)
    elif family == "perm":
        tile_list = []
        for i, L in enumerate(lengths):
            for m in range(M):
                t = np.zeros((L, L), np.float32)
                p = np.arange(L)
                t[p, (p + shift + 5 * i + m) % L] = _full(rs, L)
                tile_list.append(t)
        cross = np.zeros((lay.npairs, N), np.float32)
    else:
        tile_list = [np.zeros((L, L), np.float32) for L in lengths for _ in range(M)]
        cross = _full(rs, lay.npairs, N).reshape(lay.npairs, N)
    tiles = np.zeros(lay.tile_elems, np.float32)
    dense = np.zeros((M * N, M * N), np.float64)
    it = iter(tile_list)
    for i, L in enumerate(lengths):
        ld, base, r0 = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        for m in range(M):
            t = next(it)
            view = tiles[base + m * L * ld: base + (m + 1) * L * ld].reshape(L, ld)
            view[:, :L] = t
            if nan_pad:
                view[:, L:] = np.nan
            dense[m * N + r0:m * N + r0 + L, m * N + r0:m * N + r0 + L] = t
    ar = np.arange(N)
    for k, (m, n) in enumerate(pair_list(M)):
        dense[m * N + ar, n * N + ar] = cross[k]
        dense[n * N + ar, m * N + ar] = cross[k]
    for a in (tiles, cross, dense):
        a.setflags(write=False)
    return Adjacency(lengths, M, family, tiles, cross, dense, tile_list)


def features(family, rows, d, seed):
    """The (rows, d) float32 operand that goes with an adjacency family: full-mantissa unit Gaussians, all-positive for 'samesign',
    rows scaled by powers of two for 'graded'."""
    rs = np.random.RandomState(seed)
    H = _full(rs, rows, d)
    if family == "samesign":
        H = np.abs(H)
    if family == "graded":
        H = H * (2.0 ** rs.randint(-20, 21, size=(rows, 1))).astype(np.float32)
    return H


def wide(view, left=4, right=8):
    """``view`` (R, d) as a column slice of a NaN-filled (R, left + d + right) float32 buffer: returns (buffer, slice).  left and
    right are multiples of 4, so that the slice keeps the kernels' 16-byte alignment."""
    view = np.asarray(view, np.float32)
    buf = np.full((view.shape[0], left + view.shape[1] + right), np.nan, np.float32)
    buf[:, left:left + view.shape[1]] = view
    return buf, slice(left, left + view.shape[1])


def check_wide(buf_after, cols, buf_before=None):
    """The view of a NaN pre-filled output buffer is finite; every column outside it still holds the bits it held before (NaN
    fill when ``buf_before`` is None).  Returns the view."""
    after = np.asarray(buf_after, np.float32)
    before = np.full(after.shape, np.nan, np.float32) if buf_before is None else np.asarray(buf_before, np.float32)
    outside = np.ones(after.shape[1], bool)
    outside[cols] = False
    assert np.array_equal(after[:, outside].view(np.uint32), before[:, outside].view(np.uint32)), "written outside the view"
    assert np.isfinite(after[:, cols]).all(), "not finite inside the view"
    return after[:, cols]


# ---- K6 and its transpose ------------------------------------------------------------------------------------------------------
def propagate_reference(adj, H, transpose=False):
    """(want, bound) of out = A H (A^T H) in float64."""
    A = adj.dense.T if transpose else adj.dense
    H64 = np.asarray(H, np.float64)
    n = (A != 0).sum(1, keepdims=True)
    return A @ H64, (n + 16) * U * (np.abs(A) @ np.abs(H64)) + TINY


PropagateCase = collections.namedtuple("PropagateCase", "adj H want bound")


@functools.lru_cache(maxsize=24)
def propagate_case(lengths, M, family, d, transpose=False, nan_pad=True, shift=0):
    """Adjacency, operand, reference and bound of one K6 case, computed once and shared by the tests that run it on several kernels."""
    adj = adjacency(tuple(lengths), M, family, nan_pad, shift)
    H = features(family, adj.dense.shape[0], d, _seed(lengths, M, family) + d)
    want, bound = propagate_reference(adj, H, transpose)
    for a in (H, want, bound):
        a.setflags(write=False)
    return PropagateCase(adj, H, want, bound)


# ---- K6' -----------------------------------------------------------------------------------------------------------------------
OUTER_FAMILIES = ("dense", "samesign", "graded", "onehot")


def outer_operands(family, rows, K, seed):
    """(X, Y) float32 (rows, K) of a K6' case: 'dense' Gaussians, 'samesign' all-positive, 'graded' rows scaled by 2^-20 .. 2^20,
    'onehot' X rows with one non-zero at k = row mod K (one product per tile element: the k mapping, one index at a time)."""
    assert family in OUTER_FAMILIES, family
    rs = np.random.RandomState(seed)
    X, Y = _full(rs, rows, K), _full(rs, rows, K)
    if family == "samesign":
        X, Y = np.abs(X), np.abs(Y)
    if family == "graded":
        X = X * (2.0 ** rs.randint(-20, 21, size=(rows, 1))).astype(np.float32)
        Y = Y * (2.0 ** rs.randint(-20, 21, size=(rows, 1))).astype(np.float32)
    if family == "onehot":
        keep = np.zeros((rows, K), np.float32)
        keep[np.arange(rows), np.arange(rows) % K] = 1.0
        X = X * keep
    return X, Y


def outer_reference(lengths, M, X, Y, old_tiles=None, old_cross=None):
    """K6' in float64: [(offset, L, ld, want (L, L), bound (L, L))] per stored tile in storage order, and (want, bound) of the
    (npairs, N) cross diagonals.  ``old_tiles`` / ``old_cross``: accumulate mode, reference = old + new with |old| inside S."""
    lay = layout(tuple(lengths), M)
    N, K = lay.N, X.shape[1]
    X64, Y64 = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    tiles = []
    for i, L in enumerate(lay.lengths):
        ld, base, r0 = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        for m in range(M):
            x, y = X64[m * N + r0:m * N + r0 + L], Y64[m * N + r0:m * N + r0 + L]
            want, S = x @ y.T, np.abs(x) @ np.abs(y).T
            off = base + m * L * ld
            if old_tiles is not None:
                old = np.asarray(old_tiles[off:off + L * ld], np.float64).reshape(L, ld)[:, :L]
                want, S = want + old, S + np.abs(old)
            tiles.append((off, L, ld, want, (K + 16) * U * S))
    cw = np.zeros((lay.npairs, N))
    cS = np.zeros((lay.npairs, N))
    for k, (m, n) in enumerate(pair_list(M)):
        xm, xn, ym, yn = (a[b * N:(b + 1) * N] for a in (X64, Y64) for b in (m, n))
        cw[k] = (xm * yn).sum(1) + (xn * ym).sum(1)
        cS[k] = (np.abs(xm) * np.abs(yn)).sum(1) + (np.abs(xn) * np.abs(ym)).sum(1)
    if old_cross is not None:
        cw, cS = cw + np.asarray(old_cross, np.float64), cS + np.abs(np.asarray(old_cross, np.float64))
    return tiles, (cw, (2 * K + 16) * U * cS)


def check_outer(name, dtiles, dcross, ref, padding_zero=True):
    """All tiles and cross diagonals of a K6' result against outer_reference(); returns (worst tile ratio, worst cross ratio)."""
    tiles, (cw, cb) = ref
    dtiles = np.asarray(dtiles, np.float32)
    worst = 0.0
    for off, L, ld, want, bound in tiles:
        got = dtiles[off:off + L * ld].reshape(L, ld)
        worst = max(worst, worst_ratio(got[:, :L], want, bound + (bound == 0) * TINY))
        if padding_zero and ld > L:
            assert not got[:, L:].any(), "%s: tile padding columns are not exact zeros" % name
    print("RATIO %s.tiles %.3f" % (name, worst))
    assert worst <= 1.0, "%s tiles: error / bound = %.3f" % (name, worst)
    cworst = 0.0
    if cw.size:
        cworst = check(name + ".cross", np.asarray(dcross, np.float32).reshape(cw.shape), cw, cb)
    return worst, cworst


# ---- the fused K6 + K7 layer ---------------------------------------------------------------------------------------------------
FusedCase = collections.namedtuple("FusedCase", "adj z h0 W q mk theta alpha ms")
FusedRef = collections.namedtuple("FusedRef", "hi e_hi pre e_pre out b_out mask mm sure left_out")
LEFT_OUT_CAP = 1e-3        # at most 0.1 % of a case's elements may sit within e_pre of the ReLU's kink


@functools.lru_cache(maxsize=8)
def fused_case(lengths, M, H, variant="plain", nan_pad=True):
    """The input recipe of tests/test_gcn_small_gpu.py: uniform(-1, 1) tiles and cross, unit Gaussian z and h0, W ~ 0.2 N(0, 1),
    theta = ln 1.25, alpha = 0.1; 'q+mask' and 'strided' add a Gaussian q and a keep mask of rate 0.7 scaled by 1 / 0.7.  The
    scalars are the float32 values the kernel receives."""
    adj = adjacency(tuple(lengths), M, "dense", nan_pad)
    R = adj.dense.shape[0]
    rs = np.random.RandomState(_seed(lengths, M, "dense") + H)
    t = lambda *sh: rs.randn(*sh).astype(np.float32)
    z, h0, W = t(R, H), t(R, H), t(2 * H, H) * np.float32(0.2)
    q = t(R, H) if variant != "plain" else None
    mk = (rs.uniform(size=(R, H)) > 0.3).astype(np.float32) if variant != "plain" else None
    f32 = lambda v: float(np.float32(v))
    return FusedCase(adj, z, h0, W, q, mk, f32(np.log(0.5 / 2 + 1)), f32(0.1), f32(1.0 / 0.7) if mk is not None else 1.0)


def fused_reference(case):
    """hi, pre, out = relu(pre) m ms + q and the gate mask (pre > 0) m ms in float64, with the chained bounds

        e_hi  = (n + 16) u |A| |z| + 2^-126
        e_P   = (2H + 16) u |[hi | h0]| |W| + e_hi |W[:H]|
        e_pre = theta e_P + (1 - theta)(1 - alpha) e_hi + 8 u (|theta P| + (1 - theta)((1 - alpha) |hi| + alpha |h0|))
        out   : e_pre m ms + 4 u |out| on every element (ReLU is 1-Lipschitz);
        mask  : exact wherever |pre| > e_pre (``sure``); ``left_out`` = the share of elements where that does not hold."""
    A = case.adj.dense
    z, h0, W = (np.asarray(a, np.float64) for a in (case.z, case.h0, case.W))
    H = z.shape[1]
    th, al = case.theta, case.alpha
    n = (A != 0).sum(1, keepdims=True)
    hi = A @ z
    e_hi = (n + 16) * U * (np.abs(A) @ np.abs(z)) + TINY
    P = hi @ W[:H] + h0 @ W[H:]
    e_P = (2 * H + 16) * U * (np.abs(hi) @ np.abs(W[:H]) + np.abs(h0) @ np.abs(W[H:])) + e_hi @ np.abs(W[:H])
    pre = th * P + (1 - th) * ((1 - al) * hi + al * h0)
    e_pre = th * e_P + (1 - th) * (1 - al) * e_hi + 8 * U * (np.abs(th * P) + (1 - th) * ((1 - al) * np.abs(hi) + al * np.abs(h0)))
    mm = np.ones_like(pre) if case.mk is None else np.asarray(case.mk, np.float64) * case.ms
    out = np.maximum(pre, 0.0) * mm + (0.0 if case.q is None else np.asarray(case.q, np.float64))
    b_out = e_pre * mm + 4 * U * np.abs(out) + TINY
    sure = np.abs(pre) > e_pre
    return FusedRef(hi, e_hi, pre, e_pre, out, b_out, (pre > 0) * mm, mm, sure, 1.0 - float(sure.mean()))


def check_fused(name, ref, hi, out, mask):
    """hi and out on every element, the gate mask exactly on the elements whose ReLU decision the bound settles; the share of the
    others is capped.  Returns the three worst ratios (the mask's is 0 or inf) and the left-out share."""
    assert ref.left_out <= LEFT_OUT_CAP, "%s: %.4f %% of the elements sit within e_pre of zero" % (name, 100 * ref.left_out)
    r_hi = check(name + ".hi", hi, ref.hi, ref.e_hi)
    r_out = check(name + ".out", out, ref.out, ref.b_out)
    mask = np.asarray(mask, np.float64)
    assert np.isfinite(mask).all(), "%s: gate mask not finite" % name
    wrong = int(((mask != ref.mask) & ref.sure).sum())
    print("RATIO %s.mask %.3f (left out %.4f %%)" % (name, float("inf") if wrong else 0.0, 100 * ref.left_out))
    assert wrong == 0, "%s: %d gate-mask elements differ where |pre| > e_pre" % (name, wrong)
    assert ((mask == 0) | (mask == ref.mm)).all(), "%s: a gate-mask element is neither 0 nor m ms" % name
    return r_hi, r_out, 0.0, ref.left_out
