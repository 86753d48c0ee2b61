"""Host side of the angular-graph tests (no device): what lets tests/test_angular_graph_gpu.py hold the kernels to a fixed margin.

  * anchor: the restatement of angular_graph_ref.py, evaluated in float32, is the CPU oracle's adjacency_tiles / create_big_adj
    (which test_oracle_vs_reference.py ties to the reference) on two ragged shapes;
  * yardstick stability: on EVERY case the device tests use, four further float32 evaluations of the restatement in other
    summation orders -- the stand-ins for a correct kernel -- stay within 2.5 x the pooled yardstick on every compared quantity,
    and the float64 / float32 references are finite throughout.  The device tests allow 4 x.
  * the new comparison bites: a float32 evaluation whose off-diagonal similarities are scaled by 1 + 3e-5 (ten times their rounding
    level) fails it while the 2e-5 absolute bound of the older tests does not notice.
"""
import numpy as np
import pytest
import torch

import angular_graph_ref as R
import mmdfn_oracle as O
from mm_dfn_amd.layout import DialogueLayout

# a Gram entry next to 1 that is k ulps (2^-24 each) off moves sim by k * 2^-24 * a / (pi sqrt(1 - a^2)) = k * 4.2e-6, and through the
# degrees every entry of its row and column by up to that much relatively (a degree is at least its diagonal entry, 0.9986).  The two
# evaluations run the same operations in the same order; only the matrix products may be summed differently (batched or not): k = 8.
ANCHOR_TOL = 8 * 2.0 ** -24 * R.SHRINK / (np.pi * np.sqrt(1 - R.SHRINK ** 2))


@pytest.mark.parametrize("lengths,M,D", [([5, 1, 3], 3, 200), ([33, 1, 7, 20], 2, 36)])
@pytest.mark.parametrize("modal_weight", [0.7, 1.0])
def test_float32_restatement_is_the_oracle(lengths, M, D, modal_weight):
    N = sum(lengths)
    feats = R.make_feats("randn", M, N, D, 3)
    g = R.angular_graph_ref(feats, lengths, modal_weight)
    tiles, cross, rdeg = O.adjacency_tiles([feats[m] for m in range(M)], lengths, modal_weight)
    mine = torch.cat([g["tiles"][i][m].reshape(-1) for i in range(len(lengths)) for m in range(M)])
    for name, a, b in (("tiles", mine, tiles), ("cross", g["cross"], cross), ("rdeg", g["rdeg"], rdeg)):
        e = R.err(a, b)
        print("%-6s restatement against the oracle: %.3e (bound %.3e)" % (name, e, ANCHOR_TOL))
        assert e <= ANCHOR_TOL, name
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    dense = O.create_big_adj([feats[m] for m in range(M)], lengths, modal_weight)
    e = R.err(R.dense_from(g, lengths, M, N), dense)
    print("dense  restatement against the oracle: %.3e" % e)
    assert e <= ANCHOR_TOL
    # the packed array holds the same entries, zeros in the padding columns
    flat = R.pack_tiles(lay, g["tiles"], M)
    diag, off, pad = R.entry_masks(lay, M)
    assert int(diag.sum()) == M * N and int(off.sum()) == M * sum(L * L - L for L in lengths)
    assert bool((diag | off | pad).eq(R.written_mask(lay, M)).all()) and float(flat[pad].abs().sum()) == 0.0
    assert R.err(flat[diag | off].sort().values, tiles.sort().values) <= ANCHOR_TOL


def test_input_families_reach_what_they_are_for():
    """The cosines each family is there to produce (float64, [33, 1, 32] x 3 x 200)."""
    lengths, M, D = R.STRIP_PLUS_ONE
    N = sum(lengths)
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    _, off, _ = R.entry_masks(lay, M)

    def cosines(family):
        g = R.angular_graph_ref(R.make_feats(family, M, N, D, 1).double(), lengths, 0.7)
        return R.pack_tiles(lay, g["cosg"], M)[off], g["cdot"], g["norm"]
    c, _, _ = cosines("randn")
    assert float(c.abs().max()) < 0.35
    for eps, lo in ((0.3, 0.85), (0.03, 0.998), (0.003, 0.99998)):
        c, _, _ = cosines("corr%g" % eps)
        assert float(c.min()) > lo and float(c.max()) < 1
    assert float(cosines("corr0.003")[0].max()) > 1 - 1.2e-5         # the steep end of acos
    c, _, _ = cosines("relu")
    assert 0.4 < float(c.min()) and float(c.max()) < 0.8
    c, cd, _ = cosines("dup")
    assert int((c > 1 - 1e-12).sum()) >= M * (N - 4) and float(cd[0].min()) > 1 - 1e-12
    c, cd, _ = cosines("anti")
    assert int((c < -1 + 1e-12).sum()) >= M * (N - 4) and float(cd[0].max()) < -1 + 1e-12
    _, _, n = cosines("scale")
    assert float(n.max() / n.min()) > 1e23


@pytest.mark.parametrize("case", R.all_cases(), ids=R.case_id)
def test_correct_float32_arithmetic_stays_within_the_yardstick(case):
    (lengths, M, D), family, mw = case
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    inp, r64, yard = R.reference(lengths, M, D, family, mw)            # (asserts that both references are finite)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    worst = {}
    for n, r32 in enumerate(R.stand_ins(inp, lengths, mw)):
        assert all(bool(torch.isfinite(v).all()) for v in r32.values())
        ratios = R.report("%s stand-in %d" % (R.case_id(case), n), R.errors(r32, r64, lay, M), yard)
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in worst.items() if not v <= R.STAND_IN_MARGIN}
    assert not bad, bad


@pytest.mark.parametrize("family", ["randn", "corr0.03"])
@pytest.mark.parametrize("shape", [R.STRIP_PLUS_ONE, R.LONG], ids=["33_1_32", "129_4"])
def test_errors_the_older_bounds_hide_fail_this_comparison(shape, family):
    """Three deliberate errors in a float32 evaluation (angular_graph_ref's ``fault``).  Off-diagonal similarities 3e-5 too large,
    in what is stored only or in the degrees too: inside the 2e-5 absolute bound of test_adjacency_build_forward and
    test_strip_form_against_the_oracle, outside 4 x the yardstick here -- the second one only through sim_off, a normalised entry
    does not move when every similarity is scaled alike.  The dd_q term of the backward pass dropped: the forward quantities do
    not move at all, d(features) leaves the margin."""
    lengths, M, D = shape
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    inp, r64, yard = R.reference(lengths, M, D, family, 0.7)
    clean = R.report("clean", R.errors(R.graph_eval(inp, lengths, 0.7, torch.float32), r64, lay, M), yard)
    assert max(clean.values()) <= R.STAND_IN_MARGIN
    for fault, caught_by in (("stored", ("sim_off", "tiles_off")), ("sim", ("sim_off",)), ("ddq", ("dfeats",))):
        r32 = R.graph_eval(inp, lengths, 0.7, torch.float32, fault=fault)
        ratios = R.report("fault " + fault, R.errors(r32, r64, lay, M), yard)
        assert float((r32["tiles"] - r64["tiles"]).abs().max()) < 2e-5 and float((r32["cross"] - r64["cross"]).abs().max()) < 2e-5
        for k in caught_by:
            assert ratios[k] > R.MARGIN, (fault, k, ratios[k])


@pytest.mark.parametrize("family", R.KIND1_FAMILIES)
@pytest.mark.parametrize("shape", [R.STRIP_PLUS_ONE, R.LONG], ids=["33_1_32", "129_4"])
def test_kind1_yardstick_on_structured_features(shape, family):
    """The kind-1 device tests (test_arccos_graph_gpu.py) measure against ONE float32 CPU evaluation whose diagonal is the rounded
    u.u, where the kernels take the constant 1.  On the structured families that is no stable measure: float32 evaluations in
    four other column orders reach 450 x its error (printed).  test_kind1_kernels_against_float64_on_structured_features
    therefore uses the pooled yardstick of evaluations with the constant diagonal; those other orders stay within 2.5 x of it."""
    from test_arccos_graph_gpu import graph_eval, graph_eval_pooled
    lengths, M, D = shape
    N, c = sum(lengths), 0.99999
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    g = torch.Generator().manual_seed(11 + N + M)
    feats = R.make_feats(family, M, N, D, R.KIND1_SEED)
    dtiles, dcross, addend = torch.randn(lay.tile_elems, generator=g), torch.randn(lay.npairs, N, generator=g), torch.randn(M, N, D, generator=g)
    r64 = graph_eval(feats, lengths, c, dtiles, dcross, addend, torch.float64, True)
    r32 = graph_eval(feats.clone(), lengths, c, dtiles, dcross, addend, torch.float32)    # (it marks a float32 argument as a leaf)
    keys = ("tiles", "cross", "rdeg", "dfeats", "dfeats_add")
    assert all(bool(torch.isfinite(r[k]).all()) for r in (r64, r32) for k in keys)
    shift = max(R.err(r64[k], graph_eval(feats, lengths, c, dtiles, dcross, addend, torch.float64)[k]) for k in keys)
    assert shift < 1e-10, shift                                  # (in float64 the two diagonals are the same graph)
    yard = graph_eval_pooled(feats, lengths, c, dtiles, dcross, addend, r64, R.pool_perms(D))
    worst, single = {}, {}
    for n, perm in enumerate([torch.arange(D - 1, -1, -1)] + R.pool_perms(D, 3, seed=41)):
        alt = graph_eval_pooled(feats, lengths, c, dtiles, dcross, addend, r64, [perm])
        old = graph_eval_pooled(feats, lengths, c, dtiles, dcross, addend, r64, [perm], unit_diagonal=False)
        for k in keys:
            one = max(R.err(r32[k], r64[k]), R.EPS_HALF)
            print("kind 1 %s %s order %d %-10s rounded diagonal: error %.3e, one evaluation %.3e (ratio %.2f)   constant diagonal: "
                  "error %.3e, pooled %.3e (ratio %.2f)" % (lengths, family, n, k, old[k], one, old[k] / one, alt[k], yard[k], alt[k] / yard[k]))
            worst[k] = max(worst.get(k, 0.0), alt[k] / yard[k])
            single[k] = max(single.get(k, 0.0), old[k] / one)
    print("worst against one evaluation", single)
    bad = {k: v for k, v in worst.items() if not v <= R.STAND_IN_MARGIN}
    assert not bad, bad
