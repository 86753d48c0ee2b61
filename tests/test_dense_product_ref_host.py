"""CPU: the instrument of tests/test_dense_products_gpu.py, proven before it is pointed at the device.

dense_product_ref.emulate restates the bf16-piece arithmetic of csrc/bf16_pieces.h in numpy (truncating cut, six products, float32
accumulation per 16-wide k-step).  Against the float64 reference and the bound (n + 16) u S of dense_product_ref the full model
must pass every input family with room to spare, and a model with ONE piece product removed, or with two k indices of the weight
exchanged, must fail the one-hot family by a wide margin at every contraction width.  The two thresholds (<= 0.5 and > 4) sit
between what was measured on the CPU with these seeds: 0.46 at worst for the full model (one-hot, K = 600; <= 0.24 on the dense
families), 23.9 for the weakest removal (a third-order product at K = 8)."""
import pytest

import dense_product_ref as D

WIDTHS = [8, 36, 100, 200, 600]
R, N = 64, 48


@pytest.fixture(scope="module")
def cases():
    return {K: list(D.families(R, K, N, seed=K)) for K in WIDTHS}


def ratio(case, **fault):
    want, bound = D.want_and_bound(case.X, case.W, None, None, case.n)
    return D.worst_ratio(D.emulate(case.X, case.W, **fault), want, bound)


@pytest.mark.parametrize("K", WIDTHS)
def test_the_full_model_passes_every_family(cases, K):
    names = [c.name for c in cases[K]]
    assert names == ["onehot", "onehot_w", "bf16x", "samesign", "cancel", "graded", "dropout"]
    for case in cases[K]:
        r = ratio(case)
        print("RATIO emulate[K=%d] %s %.3f" % (K, case.name, r))
        assert r <= 0.5, (K, case.name, r)


@pytest.mark.parametrize("K", WIDTHS)
def test_every_removed_product_fails_the_one_hot_family(cases, K):
    onehot = cases[K][0]
    assert onehot.name == "onehot" and onehot.X.shape[0] == max(R, K)          # every k carries the non-zero of some row
    assert ((onehot.X != 0).sum(1) == 1).all() and (onehot.X != 0).any(0).all()
    for name in D.PRODUCTS:
        r = ratio(onehot, drop=name)
        print("RATIO emulate[K=%d] onehot without %s %.1f" % (K, name, r))
        assert r > 4.0, (K, name, r)


@pytest.mark.parametrize("K", WIDTHS)
def test_the_mirrored_and_bf16_cases_see_the_products_they_can(cases, K):
    """W one-hot, X dense: the same six products fail it.  X exactly bf16 (a2 = a3 = 0): the products of a1 fail it, the others are
    zero there, which is why the family has both."""
    mirrored, bf16x = cases[K][1], cases[K][2]
    for name in D.PRODUCTS:
        assert ratio(mirrored, drop=name) > 4.0, (K, name)
    for name in ("a1b1", "a1b2", "a1b3"):
        assert ratio(bf16x, drop=name) > 4.0, (K, name)
    for name in ("a2b1", "a2b2", "a3b1"):
        assert ratio(bf16x, drop=name) == ratio(bf16x), (K, name)


@pytest.mark.parametrize("K", WIDTHS)
def test_a_swapped_k_pair_fails_the_one_hot_family(cases, K):
    onehot = cases[K][0]
    for pair in ((0, 1), (K - 1, K // 2 - 1), (3, K - 4)):
        if pair[0] != pair[1]:
            assert ratio(onehot, swap_k=pair) > 4.0, (K, pair)


def test_why_the_one_hot_family_exists(cases):
    """At K = 200 a removed third-order product stays UNDER (K + 16) u S on same-signed dense inputs (measured 0.75 .. 0.89):
    the bound is a worst case over K roundings.  The one-hot rows of the same width put it tens of bounds out."""
    samesign = cases[200][3]
    assert samesign.name == "samesign"
    for name in D.THIRD_ORDER:
        r = ratio(samesign, drop=name)
        print("RATIO emulate[K=200] samesign without %s %.3f" % (name, r))
        assert r < 1.0, (name, r)
        assert ratio(cases[200][0], drop=name) > 4.0
