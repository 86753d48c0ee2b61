"""The angular dialogue graph on the device: adjacency kind 0 of K5 (csrc/adjacency.hip, adjacency_small.hip, gram epilogue 1 of
tile_dot.hip) -- the graph of the default model -- through both launch forms and both strip heights, against float64, on
structured features.

Reference, yardstick and inputs are tests/angular_graph_ref.py's: the restatement evaluated in float64 is the reference value; per
quantity the largest error of eight float32 CPU evaluations in permuted column orders is the yardstick (floor 2^-24); a device
result passes at error <= 4 x yardstick (the margin of the GRU recurrence and kind-1 tests for another summation order;
test_angular_graph_host.py holds correct float32 arithmetic in the kernels' summation orders to 2.5 x on every case used here).
Errors are max |x - x64| / max |x64| over

  sim_off     T[p,q] / (r_p r_q) off the diagonal, from the result's own tiles and rdeg (raw entry points only)
  tiles_off   off-diagonal tile entries -- apart from the diagonal, whose rounded u.u goes through the steepest part of acos
  tiles_diag  diagonal tile entries
  cross, rdeg, unit, norm, cosg, cdot     what the forward entry point writes and the backward one reads
  dfeats, dfeats_add                      d(features) without and with the addend, from NaN-filled outputs

and the padding columns of every tile row are exactly 0 and written.  The input families (randn, corr(eps), relu, dup, anti,
scale) put off-diagonal cosines at 0, 0.6, 0.9 .. 1 - 1e-5, exactly +-1, and row norms over 24 decades.  Every case prints kernel
error, yardstick and ratio per quantity before it asserts; which form ran is asserted from the profiler's kernel names.

Worst measured ratio error / yardstick per quantity over all cases (MI355X; nothing is above 4, nothing was changed to get there):

                 strip form (both heights)   many-launch form   through ops.build_adjacency
  sim_off        3.72                        2.77               -
  tiles_off      2.47                        3.17               2.25
  tiles_diag     1.29                        2.25               1.72
  cross          1.02                        2.21               1.37
  rdeg           1.03                        2.38               -
  unit           1.04                        1.11               -
  norm           1.04                        0.83               -
  cosg           1.67                        1.67               -
  cdot           0.89                        1.00               -
  dfeats         2.47                        2.59               2.49
  dfeats_add     1.92                        2.46               -

(sim_off 3.72: [2, 1, 3] corr(0.03), 3.5e-6 against 9.4e-7; tiles_off 3.17: [129, 4] corr(0.003), 2.5e-5 against 7.8e-6; dfeats 2.59:
[129, 4] corr(0.03) at modal weight 1, 1.5e-4 against 5.9e-5.)  Strip against many-launch where acos is steep, d(features) of the
adjacency path alone relative to its largest value: corr(0.003) 1.5e-3 ([33, 1, 32]) and 2.9e-3 ([64, 65]) -- float32 itself is
1e-2 from float64 there --, dup 2.7e-5 and 1.4e-5; tiles 7e-7 .. 2.4e-5.
"""
import pytest
import torch

import angular_graph_ref as R
from mm_dfn_amd import _hip, ops
from mm_dfn_amd.layout import DialogueLayout
from test_arccos_graph_gpu import buffers, kernel_names, run_entry

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def run_case(case, monkeypatch=None, small=None, sr=None):
    """Both entry points on the case's inputs, every output NaN-filled first.  Returns (result dict, kernel names)."""
    (lengths, M, D), family, mw = case
    N = sum(lengths)
    if monkeypatch is not None:
        monkeypatch.setenv("MMDFN_ADJ_SMALL", str(small))
        if sr is not None:
            monkeypatch.setenv("MMDFN_ADJ_SR", str(sr))
    lay = DialogueLayout.get(lengths, M, torch.device(DEV))
    inp, _, _ = R.reference(lengths, M, D, family, mw)
    b = buffers(lay, M, N, D, 1)
    b.update({k: v.to(DEV) for k, v in inp.items()})
    names = kernel_names(lambda: run_entry(b, lay, M, N, D, mw, 0, True))
    res = {k: b[k].cpu() for k in ("tiles", "cosg", "cross", "cdot", "rdeg", "unit", "norm")}
    res["dfeats_add"] = b["dfeats"].cpu()
    b["dfeats"].fill_(NAN)
    run_entry(b, lay, M, N, D, mw, 0, False)
    res["dfeats"] = b["dfeats"].cpu()
    return res, names


def hold(tag, case, res, lines=None):
    """Print every figure, then: nothing the entry point is to write is NaN, padding columns are 0, every quantity is within 4 x."""
    (lengths, M, D), family, mw = case
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    _, r64, yard = R.reference(lengths, M, D, family, mw)
    ratios = R.report(tag + " " + R.case_id(case), R.errors(res, r64, lay, M), yard, lines)
    w = R.written_mask(lay, M)
    for k, v in res.items():
        assert not torch.isnan(v[w] if k in ("tiles", "cosg") else v).any(), k
    pad = R.entry_masks(lay, M)[2]
    if bool(pad.any()):
        assert float(res["tiles"][pad].abs().max()) == 0.0
        if "cosg" in res:
            assert float(res["cosg"][pad].abs().max()) == 0.0
    bad = {k: v for k, v in ratios.items() if not v <= R.MARGIN}
    assert not bad, (tag, R.case_id(case), bad)
    return ratios


def assert_form(names, form):
    strip = any("adj_strip_fwd_kernel" in n for n in names)
    if form == "strip":
        assert strip and any("adj_strip_bwd_kernel" in n for n in names) and not any("tile_dot" in n for n in names), names
    else:
        assert not strip and not any("adj_strip_bwd_kernel" in n for n in names), names
        assert any("tile_dot" in n for n in names) and any("bwd_etile_kernel" in n for n in names), names


@pytest.mark.parametrize("sr", [32, 64])
@pytest.mark.parametrize("case", R.STRIP_CASES, ids=R.case_id)
def test_strip_form_against_float64(case, sr, kernel_variants):
    res, names = run_case(case, kernel_variants, small=1, sr=sr)
    assert_form(names, "strip")
    assert any("adj_strip_fwd_kernel<%d" % sr in n.replace(" ", "") for n in names), names
    hold("strip %d" % sr, case, res)


@pytest.mark.parametrize("case", R.GENERAL_CASES, ids=R.case_id)
def test_many_launch_form_against_float64(case, request):
    if case[0] in R.FORCED_GENERAL:          # a shape the strip form would take: the tuning build's switch
        res, names = run_case(case, request.getfixturevalue("kernel_variants"), small=0)
    else:
        res, names = run_case(case)
    assert_form(names, "general")
    hold("many-launch", case, res)


@pytest.mark.parametrize("case", R.BOTH_FORMS, ids=R.case_id)
def test_distance_between_the_two_forms_where_acos_is_steep(case, kernel_variants):
    """Each form is held to float64 by the yardstick; how far they are from each other is printed, not bounded (the 6e-5 of
    test_strip_form_matches_the_many_launch_form was measured on randn features)."""
    general, names = run_case(case, kernel_variants, small=0)
    assert_form(names, "general")
    strip, names = run_case(case, kernel_variants, small=1)
    assert_form(names, "strip")
    hold("many-launch", case, general)
    hold("strip", case, strip)
    (lengths, M, D), _, _ = case
    w = R.written_mask(DialogueLayout.get(lengths, M, torch.device("cpu")), M)
    for k in ("tiles", "cross", "rdeg", "dfeats", "dfeats_add"):
        a, b = (strip[k][w], general[k][w]) if k == "tiles" else (strip[k], general[k])
        print("%-40s %-10s strip against many-launch %.3e (relative to the largest value)" % (R.case_id(case), k, R.err(a, b)))


@pytest.mark.parametrize("case", R.OPERATOR_CASES, ids=R.case_id)
def test_through_the_operator_against_float64(case):
    """ops.build_adjacency with the production library and no switches, backward through to_dense(): the autograd node's handling
    of the saved intermediates where they matter."""
    (lengths, M, D), family, mw = case
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    inp, _, _ = R.reference(lengths, M, D, family, mw)
    fg = inp["feats"].to(DEV).requires_grad_(True)
    cot = R.dense_cotangent(lay, M, inp["dtiles"], inp["dcross"]).to(DEV)
    box = {}

    def step():
        box["adj"] = adj = ops.build_adjacency(fg, lengths, mw)
        box["dense"] = adj.to_dense()
        (box["dense"] * cot).sum().backward()
    prev = _hip.set_tuning(False)                                       # the production library
    try:
        names = kernel_names(step)
    finally:
        _hip.set_tuning(prev)
    assert_form(names, "strip" if max(lengths) <= 128 else "general")
    adj = box["adj"]
    res = dict(tiles=adj.tiles.detach().cpu(), cross=adj.cross.detach().cpu(), dfeats=fg.grad.cpu())
    hold("operator", case, res)
    # the dense matrix holds those entries and nothing else
    back = R.dense_from(dict(tiles=list(_unpack(lay, M, res["tiles"])), cross=res["cross"]), lengths, M, sum(lengths))
    assert torch.equal(box["dense"].detach().cpu(), back)


def _unpack(lay, M, flat):
    for i, L in enumerate(lay.lengths):
        ld, base = int(lay.ld_host[i]), int(lay.tile_base_host[i])
        yield flat[base:base + M * L * ld].view(M, L, ld)[:, :, :L]
