"""CPU: the instrument of tests/test_wgrad_products_gpu.py, proven before it is pointed at the device.

wgrad_product_ref.model restates the bf16-piece weight-gradient batch in numpy: every segment cut into the slabs of the launch
plan, a slab = dense_product_ref.emulate on the transposed operands with a 32-row k-step (truncating cut, six products, float32
accumulation per chunk), the slabs and the column sums' slabs added in float32.  Against the float64 reference and the bound
(n + 16) u S the full model must pass every family on every launch list the GPU file uses -- which is also where "the reference
alone stays within the bound on these inputs" is shown --, and a model with ONE fault must fail:
  a piece product removed (each of the six), two rows of B exchanged, the shift off by one (both ways), one slab of a stacked sum
  left out (each slab in turn), the column sums taken over the shifted row range.
A fault counts as shown when the worst ratio exceeds 4 (four bounds); measured on the CPU with these seeds: the full model 0.43 at
worst (one-hot), the weakest fault 8.4 (a third-order product on a one-row segment; 22 and more from 97 rows on)."""
import numpy as np
import pytest

import wgrad_product_ref as W

LISTS = [("piece_" + k, v[0], v[1]) for k, v in W.PIECE_LAUNCHES.items()] + [("piece_forty", W.FORTY, W.QUICK)] + \
        [("tiled_" + k, v[0], v[1]) for k, v in W.TILED_LAUNCHES.items()] + [("grouped", W.GROUPED, W.QUICK)] + \
        [("single", [W.S(M, N, [(R, 0)]) for R, M, N in W.SINGLE_SHAPES], W.QUICK)]


def ratios(out, **fault):
    """(worst ratio of C, worst ratio of the column sums) of the model with ``fault`` against the float64 reference."""
    want, bound, wc, bc = W.reference(out)
    C, cs = W.model(out, **fault)
    return W.worst_ratio(C, want, bound), W.worst_ratio(cs, wc, bc)


def steps(name, specs):
    K = W.sweep_length(name, specs)
    return sorted({0, K // 2, K - 1})                    # (the first, a middle and the last step of a one-hot sweep)


@pytest.mark.parametrize("tag,specs,fams", LISTS, ids=[t for t, _, _ in LISTS])
def test_the_full_model_passes_every_family_on_every_launch_list(tag, specs, fams):
    for name in fams:
        worst = 0.0
        for k in steps(name, specs):
            for out in W.build(specs, name, seed=len(specs) + 7 * k, k=k):
                worst = max(worst, *ratios(out))
        print("RATIO model %s %s %.3f" % (tag, name, worst))
        assert worst <= 1.0, (tag, name, worst)


@pytest.mark.parametrize("tag", list(W.TALL_LAUNCHES))
def test_the_full_model_passes_the_tall_launches(tag):
    specs, _, r0s = W.TALL_LAUNCHES[tag]
    for name, r0 in [("rowhot", r0s[1]), ("samesign", None), ("graded", None)]:
        worst = max(max(ratios(out)) for out in W.build(specs, name, seed=5, r0=r0, share=True))
        print("RATIO model tall_%s %s %.3f" % (tag, name, worst))
        assert worst <= 1.0, (tag, name, worst)


# one tile and one row; one row / column block more than a tile with a shift; two segments on a wide output; 8 full splits
MUTANT_SPECS = [W.S(4, 4, [(1, 0)]), W.S(132, 116, [(97, -33)]), W.S(128, 224, [(513, 1), (97, 0)], 1), W.S(260, 112, [(1024, 0)])]


@pytest.fixture(scope="module")
def rowhot():
    return W.build(MUTANT_SPECS, "rowhot", seed=3, r0=40)      # (live rows 40 .. of every segment: inside B's shifted range)


@pytest.mark.parametrize("name", list(W.PRODUCTS))
def test_every_removed_product_fails_rowhot(rowhot, name):
    for out in rowhot:
        r = ratios(out, drop=name)[0]
        print("RATIO model rowhot[%d,%d] without %s %.1f" % (out.M, out.N, name, r))
        assert ratios(out)[0] <= 1.0 and r > 4.0, (out.M, out.N, name, r)


def test_the_mirrored_and_bf16_cases_see_the_products_they_can():
    for out in W.build(MUTANT_SPECS[1:], "rowhot_b", seed=4, r0=40):
        for name in W.PRODUCTS:
            assert ratios(out, drop=name)[0] > 4.0, name
    for out in W.build(MUTANT_SPECS[1:], "bf16a", seed=4, r0=40):
        for name in ("a1b1", "a1b2", "a1b3"):
            assert ratios(out, drop=name)[0] > 4.0, name
        for name in ("a2b1", "a2b2", "a3b1"):
            assert ratios(out, drop=name) == ratios(out), name


def test_two_exchanged_rows_of_b_fail_rowhot(rowhot):
    for out in rowhot[1:]:
        r = ratios(out, swap_rows=(40, 41))[0]
        print("RATIO model rowhot[%d,%d] rows 40 <-> 41 of B %.1f" % (out.M, out.N, r))
        assert r > 4.0, (out.M, out.N, r)


@pytest.mark.parametrize("error", [1, -1])
def test_a_shift_off_by_one_fails_rowhot(rowhot, error):
    for out in rowhot:
        r = ratios(out, shift_error=error)[0]
        print("RATIO model rowhot[%d,%d] shift %+d %.1f" % (out.M, out.N, error, r))
        assert r > 4.0, (out.M, out.N, error, r)


def test_every_slab_left_out_fails_the_rowhot_sweep():
    """Two segments, 2 + 6 slabs: each slab left out in turn fails at the sweep steps whose live rows it holds (C and column sums),
    and ONLY there -- at the other steps the slab is all zeros and leaving it out changes nothing."""
    specs = [W.S(132, 116, [(97, 0), (513, 1)], 1)]
    K = W.sweep_length("rowhot", specs)
    outs = [W.build(specs, "rowhot", seed=9, k=k)[0] for k in range(K)]
    nslabs = sum(W.tns_plan(R)[1] for R, _ in specs[0].segs)
    assert (K, nslabs) == (4, 8)
    for i in range(nslabs):
        per_step = [ratios(out, skip_slab=i) for out in outs]
        print("RATIO model rowhot[132,116] without slab %d " % i + " ".join("%.3g/%.3g" % r for r in per_step))
        assert max(r[0] for r in per_step) > 4.0 and max(r[1] for r in per_step) > 4.0, (i, per_step)
        if i >= 2:                                       # (the 97-row segment has live rows in both slabs at every step: 132 columns)
            assert min(r[0] for r in per_step) <= 1.0, (i, per_step)


def test_column_sums_over_the_shifted_range_fail():
    specs = [W.S(132, 116, [(97, -33)]), W.S(128, 224, [(513, 1), (97, 0)], 1), W.S(260, 112, [(1024, -1)])]
    for name in ("rowhot", "samesign"):
        K = W.sweep_length(name, specs)
        worst = [0.0] * len(specs)
        for k in range(K):
            for i, out in enumerate(W.build(specs, name, seed=11, k=k)):
                assert ratios(out)[1] <= 1.0
                worst[i] = max(worst[i], ratios(out, colsum_shifted=True)[1])
        print("RATIO model %s column sums over the shifted range " % name + " ".join("%.3g" % r for r in worst))
        assert min(worst) > 4.0, (name, worst)


def test_why_the_rowhot_family_exists():
    """On same-signed dense operands of 1024 rows a removed third-order product stays UNDER (n + 16) u S: the bound is a worst case
    over n roundings.  One live row per element puts it tens of bounds out."""
    dense = W.build(MUTANT_SPECS[3:], "samesign", seed=3)[0]
    hot = W.build(MUTANT_SPECS[3:], "rowhot", seed=3)[0]
    for name in ("a1b3", "a2b2", "a3b1"):
        r = ratios(dense, drop=name)[0]
        print("RATIO model samesign[260,112,1024] without %s %.3f" % (name, r))
        assert r < 1.0 and ratios(hot, drop=name)[0] > 4.0, (name, r)


def test_the_families_are_what_they_claim():
    rs = np.random.RandomState(1)
    A, B = W.draw("rowhot", 97, 132, 116, rs, r0=90)
    assert ((A != 0).sum(0) == 1).all() and (np.nonzero(A[:, 0])[0] == [90]).all() and (np.nonzero(A[:, 10])[0] == [3]).all()
    A, B = W.draw("rowhot_b", 97, 132, 116, rs, r0=5)
    assert ((B != 0).sum(0) == 1).all() and (A != 0).all()
    A, B = W.draw("bf16a", 97, 132, 116, rs)
    assert (W.cut(A)[1] == 0).all() and (W.cut(B)[1] != 0).any()
    out = W.build([W.S(132, 116, [(96, 2)])], "cancel", seed=2)[0]
    want, bound, _, _ = W.reference(out)
    assert (want[:, 0::2] == 0).all() and (want[:, 1::2] != 0).all() and (bound > 50 * W.U).all()
    A, B = W.draw("dropout", 513, 132, 116, rs)
    rps, eff = W.tns_plan(513)
    assert (rps, eff) == (96, 6) and not A[3 * rps:4 * rps].any() and not B[3 * rps:4 * rps].any() and not A[:, 66].any()
    # every row of every segment is the live row of some sweep step
    specs = W.PIECE_LAUNCHES["splits"][0]
    for name in ("rowhot", "rowhot_b"):
        hit = [[np.zeros(R, bool) for R, _ in o.segs] for o in specs]
        for k in range(W.sweep_length(name, specs)):
            for o, out in zip(hit, W.build(specs, name, seed=1, k=k)):
                for h, seg in zip(o, out.segs):
                    h |= ((seg.A if name == "rowhot" else seg.B) != 0).any(1)
        assert all(h.all() for o in hit for h in o), name
    assert [W.tns_plan(R) for R in (1, 64, 65, 97, 512, 513, 1024, 3072)] == \
        [(32, 1), (64, 1), (64, 2), (64, 2), (64, 8), (96, 6), (128, 8), (192, 16)]
