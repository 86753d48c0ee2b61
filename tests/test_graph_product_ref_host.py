"""The instrument of tests/test_graph_products_gpu.py proved on the CPU (tests/graph_product_ref.py): a plain float32 numpy
evaluation of K6, K6^T, K6' and the fused layer passes the bound of every input family; the same evaluation with one of the faults
a kernel of this family can have fails at least one family; the fused layer's ReLU decisions that the bound leaves open stay under
the cap for every case the GPU test runs."""
import numpy as np
import pytest
import torch

import graph_product_ref as G
from mm_dfn_amd.layout import BlockTileAdjacency, pair_list

LENGTHS = (1, 15, 16, 17, 33, 5)        # every padding width ld - L in 0 .. 3, a tile over two 16-row fragments
M = 3
D = 36


def model_propagate(adj, H, transpose=False, fault=None):
    """out = A H (A^T H) tile by tile in float32, reading the block-tile STORAGE (padding included, masked the way a kernel has to
    mask it).  ``fault`` names one defect, applied to the second dialogue's first modality (a 15-row tile with one padding column):
    'drop_cross', 'swap_k', 'transposed_tile', 'clamped_row', 'padding'."""
    lay = G.layout(adj.lengths, adj.M)
    N, Mm = lay.N, adj.M
    H = np.asarray(H, np.float32)
    out = np.zeros_like(H)
    for i, L in enumerate(lay.lengths):
        ld, base, r0 = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        for m in range(Mm):
            hit = fault is not None and i == 1 and m == 0
            stored = adj.tiles[base + m * L * ld: base + (m + 1) * L * ld].reshape(L, ld)
            T = stored[:, :L].copy()
            if transpose != (hit and fault == "transposed_tile"):
                T = T.T.copy()
            if hit and fault == "swap_k":
                T[:, [2, 9]] = T[:, [9, 2]]
            rows = slice(m * N + r0, m * N + r0 + L)
            o = T @ H[rows]
            if hit and fault == "clamped_row":
                o[L - 1] = T[L - 2] @ H[rows]                       # the last row computed from the row its address was clamped to
            if hit and fault == "padding":
                o[0] = o[0] + stored[0, L] * H[rows][L - 1]         # column L of the storage row against the clamped H row
            for k, (a, b) in enumerate(pair_list(Mm)):
                if m in (a, b):
                    n = b if m == a else a
                    if hit and fault == "drop_cross" and n == Mm - 1:
                        continue
                    o = o + adj.cross[k, r0:r0 + L, None] * H[n * N + r0:n * N + r0 + L]
            out[rows] = o
    return out


def _propagate_passes(family, transpose, fault):
    adj = G.adjacency(LENGTHS, M, family, True)
    H = G.features(family, M * sum(LENGTHS), D, 11)
    want, bound = G.propagate_reference(adj, H, transpose)
    try:
        G.check("%s.%s" % (family, fault), model_propagate(adj, H, transpose, fault), want, bound)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("transpose", [False, True])
def test_float32_propagate_passes_every_family(transpose):
    for family in G.FAMILIES:
        assert _propagate_passes(family, transpose, None), family


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("fault", ["drop_cross", "swap_k", "transposed_tile", "clamped_row", "padding"])
def test_faulty_propagate_fails_some_family(fault, transpose):
    failed = [family for family in G.FAMILIES if not _propagate_passes(family, transpose, fault)]
    assert failed, "no family notices '%s'" % fault
    # and the families built for a fault do notice it
    if fault in ("swap_k", "transposed_tile", "clamped_row"):
        assert "perm" in failed and "dense" in failed
    if fault == "drop_cross":
        assert "cross" in failed and "samesign" in failed
    if fault == "padding":
        assert len(failed) == len(G.FAMILIES)           # a NaN is a NaN whatever it meets


def test_padding_fault_needs_the_nan_padding():
    """With zero padding the same fault is invisible: that is why the GPU cases poison the padding."""
    adj = G.adjacency(LENGTHS, M, "dense", False)
    H = G.features("dense", M * sum(LENGTHS), D, 11)
    want, bound = G.propagate_reference(adj, H)
    G.check("zero-padding", model_propagate(adj, H, False, "padding"), want, bound)


def test_adjacency_parts_are_the_dense_matrix():
    for family in G.FAMILIES:
        adj = G.adjacency(LENGTHS, M, family, False)
        lay = G.layout(LENGTHS, M)
        bta = BlockTileAdjacency(lay, torch.from_numpy(adj.tiles.copy()), torch.from_numpy(adj.cross.copy()))
        assert np.array_equal(bta.to_dense().double().numpy(), adj.dense), family
        packed = BlockTileAdjacency.from_parts(lay, [torch.from_numpy(t) for t in adj.tile_list], torch.from_numpy(adj.cross.copy()))
        assert np.array_equal(packed.tiles.numpy(), adj.tiles), family
        nan = G.adjacency(LENGTHS, M, family, True)
        assert np.isnan(nan.tiles).sum() == sum(M * L * (((L + 3) & ~3) - L) for L in LENGTHS)
        assert np.array_equal(nan.dense, adj.dense)
    perm = G.adjacency(LENGTHS, M, "perm", False)
    assert ((perm.dense != 0).sum(1) == 1).all() and ((perm.dense != 0).sum(0) == 1).all()
    dense = G.adjacency(LENGTHS, M, "dense", False).dense
    assert not np.array_equal(dense, dense.T)


def test_wide_buffers():
    v = np.arange(12, dtype=np.float32).reshape(3, 4)
    buf, cols = G.wide(v)
    assert buf.shape == (3, 16) and np.array_equal(buf[:, cols], v) and np.isnan(buf[:, :4]).all() and np.isnan(buf[:, 8:]).all()
    assert np.array_equal(G.check_wide(buf, cols), v)
    spoilt = buf.copy()
    spoilt[1, 9] = 0.0
    with pytest.raises(AssertionError):
        G.check_wide(spoilt, cols)
    spoilt = buf.copy()
    spoilt[2, 5] = np.nan
    with pytest.raises(AssertionError):
        G.check_wide(spoilt, cols)


# ---- K6' -----------------------------------------------------------------------------------------------------------------------
def model_outer(lengths, Mm, X, Y, old=None, fault=None):
    """dtiles / dcross of K6' in float32; fault 'short_k': the last 8 columns of the contraction left out of the tiles,
    'short_k_cross': of the cross diagonals, 'drop_cross': the second term of the cross diagonal left out."""
    lay = G.layout(lengths, Mm)
    N, K = lay.N, X.shape[1]
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    Kt = K - 8 if fault == "short_k" else K
    Kc = K - 8 if fault == "short_k_cross" else K
    dt = np.zeros(lay.tile_elems, np.float32) if old is None else old[0].copy()
    for i, L in enumerate(lay.lengths):
        ld, base, r0 = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        for m in range(Mm):
            x, y = X[m * N + r0:m * N + r0 + L, :Kt], Y[m * N + r0:m * N + r0 + L, :Kt]
            dt[base + m * L * ld: base + (m + 1) * L * ld].reshape(L, ld)[:, :L] += x @ y.T
    dc = np.zeros((lay.npairs, N), np.float32) if old is None else old[1].copy()
    for k, (m, n) in enumerate(pair_list(Mm)):
        xm, xn, ym, yn = (a[b * N:(b + 1) * N, :Kc] for a in (X, Y) for b in (m, n))
        dc[k] += (xm * yn).sum(1) + (0 if fault == "drop_cross" else (xn * ym).sum(1))
    return dt, dc


def _outer_passes(family, K, fault, accumulate=False):
    rows = M * sum(LENGTHS)
    X, Y = G.outer_operands(family, rows, K, 5)
    old = None
    if accumulate:
        lay = G.layout(LENGTHS, M)
        rs = np.random.RandomState(6)
        old = (rs.randn(lay.tile_elems).astype(np.float32) * 8, rs.randn(lay.npairs, lay.N).astype(np.float32) * 8)
    ref = G.outer_reference(LENGTHS, M, X, Y, *(old or (None, None)))
    try:
        G.check_outer("%s.%s" % (family, fault), *model_outer(LENGTHS, M, X, Y, old, fault), ref, padding_zero=not accumulate)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("K", [36, 208])
def test_float32_outer_passes_every_family(K, accumulate):
    for family in G.OUTER_FAMILIES:
        assert _outer_passes(family, K, None, accumulate), family


@pytest.mark.parametrize("fault", ["short_k", "short_k_cross", "drop_cross"])
def test_faulty_outer_fails_some_family(fault):
    failed = [family for family in G.OUTER_FAMILIES if not _outer_passes(family, 208, fault)]
    assert "dense" in failed and "samesign" in failed, failed


def test_outer_padding_must_be_zero():
    X, Y = G.outer_operands("dense", M * sum(LENGTHS), D, 5)
    ref = G.outer_reference(LENGTHS, M, X, Y)
    dt, dc = model_outer(LENGTHS, M, X, Y)
    lay = G.layout(LENGTHS, M)
    dt[int(lay.tile_base_host[1]) + 15] = 1e-30                      # the padding column of the first row of a 15-row tile
    with pytest.raises(AssertionError):
        G.check_outer("padding", dt, dc, ref)


# ---- the fused layer -----------------------------------------------------------------------------------------------------------
# the cases of tests/test_graph_products_gpu.py (the GPU test imports this list)
FUSED_CASES = [((1,), 3, 100), ((31, 32, 33), 3, 100), ((110, 64, 97, 5), 3, 100), ((128, 2), 2, 64), ((50, 20), 1, 100),
               ((110,) * 9, 3, 100), ((17, 96), 3, 96), ((40,), 3, 4), ((33, 1, 32, 128, 127, 65), 3, 100), ((16, 17, 15), 2, 36)]
# where mmdfn_prop_layer_fwd answers -2 and the two launches run: M = 4, max_len = 129, a grid of 4 128 strips
FUSED_TWO_LAUNCH_CASES = [((20, 7), 4, 100), ((129, 5), 3, 100), ((128,) + (1,) * 343, 3, 100)]


def model_fused(case, fault=None):
    f = np.float32
    hi = model_propagate(case.adj, case.z)
    a, b = (case.h0, hi) if fault == "swap_residual" else (hi, case.h0)
    P = hi @ case.W[:hi.shape[1]] + case.h0 @ case.W[hi.shape[1]:]
    th, al = f(case.theta), f(case.alpha)
    pre = th * P + (f(1) - th) * ((f(1) - al) * a + al * b)
    mm = np.ones_like(pre) if case.mk is None else case.mk * f(case.ms)
    out = np.maximum(pre, 0) * mm + (0 if case.q is None else case.q)
    return hi, out.astype(f), ((pre > 0) * mm).astype(f)


@pytest.mark.parametrize("variant", ["plain", "q+mask"])
@pytest.mark.parametrize("lengths,Mm,H", FUSED_CASES + FUSED_TWO_LAUNCH_CASES)
def test_float32_fused_layer_passes_and_relu_cap_holds(lengths, Mm, H, variant):
    case = G.fused_case(lengths, Mm, H, variant)
    ref = G.fused_reference(case)
    print("LEFT_OUT %s M=%d H=%d: %d of %d" % (list(lengths)[:6], Mm, H, int((~ref.sure).sum()), ref.sure.size))
    assert ref.left_out <= G.LEFT_OUT_CAP
    G.check_fused("fused", ref, *model_fused(case))


def test_fused_layer_with_the_residual_operands_exchanged_fails():
    case = G.fused_case((31, 32, 33), 3, 100, "q+mask")
    ref = G.fused_reference(case)
    hi, out, mask = model_fused(case, "swap_residual")
    G.check("hi", hi, ref.hi, ref.e_hi)                              # (hi itself is not touched by this fault)
    with pytest.raises(AssertionError):
        G.check_fused("fused", ref, hi, out, mask)
    with pytest.raises(AssertionError):
        G.check("out", out, ref.out, ref.b_out)


def test_fused_layer_mask_is_held_exactly():
    case = G.fused_case((31, 32, 33), 3, 100, "q+mask")
    ref = G.fused_reference(case)
    hi, out, mask = model_fused(case)
    r, c = np.argwhere(ref.sure & (ref.mm > 0))[0]
    mask[r, c] = 0.0 if mask[r, c] else np.float32(case.ms)          # one decided ReLU unit flipped in the mask alone
    with pytest.raises(AssertionError):
        G.check_fused("fused", ref, hi, out, mask)
