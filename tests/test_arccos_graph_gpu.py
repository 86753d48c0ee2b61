"""The arccos (MMGCN) dialogue graph on the device: adjacency kind 1 of K5 (csrc/adjacency.hip, adjacency_small.hip, tile_dot.hip)
through both launch forms, MM_GCN2 and GCNII_lyc(adj=None) on top of it.

What is compared against what.  Every restatement below (the graph, MM_GCN2, GCNII_lyc) is written once, generic in the dtype, and
evaluated on the CPU in float64 (the reference value) and in float32 (the yardstick).  Errors are max |x - x64| / max |x64|.
A device result passes when its error is at most 4 x the float32 CPU evaluation's error on the same inputs (the margin the GRU
recurrence tests use for a different summation order); for the module goldens the float32 CPU run is the reference's own
(tests/golden/mmgcn2.npz, the reference modules run by tests/golden/make_golden_mmgcn2.py).  Two floors, both from the number
format, not from what the kernels give:

  * a float32 result is defined to half an ulp of its largest value only, so the float32 error counts as at least 2^-24;
  * d(features) of a batch whose dialogues all have ONE utterance is zero in exact arithmetic (every tile is the 1 x 1 matrix
    r S r = S / S, or S / (S + 2 c): the Gram entry is u.u = 1 whatever the features).  Its float64 value is rounding noise, the
    relative error is 0 / 0.  What a float32 evaluation leaves there is the rounding of the projection (du - u (u.du)) / ||x|| of a
    du that is parallel to u, so such a result is held to 4 x max(float32 CPU value, 2^-23 max |du64| / ||x||) in absolute terms.

Every case prints its figures (kernel error, float32 CPU error, ratio) before it asserts.
"""
import math
import os

import numpy as np
import pytest
import torch

from angular_graph_ref import (EPS_HALF, KIND1_FAMILIES, KIND1_SEED, SHRINK, dense_from, err, make_feats, pack_tiles, pool_perms,
                               written_mask)
from mm_dfn_amd import GCNII_lyc, MM_GCN2, _hip, ops, ops_flags
from mm_dfn_amd.layout import DialogueLayout, pair_list
from mm_dfn_amd.ops_pad import _lay_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- restatements (dtype-generic, CPU) ---------------------------------------------------------------------------------------------
def graph_ref(feats, lengths, c, unit_diagonal=False):
    """Arccos graph of (M, N, D) features: per-dialogue normalised tiles [(M, L, L)], cross (npairs, N), rdeg (M, N), unit.
    unit_diagonal: cos(x, x) is the constant 1, as the kernels define it (mmdfn_internal.h), not the rounded sum u.u -- the
    same value in float64 to 1e-12, in float32 an evaluation without the diagonal's 3e-5 of acos noise."""
    M, N, D = feats.shape
    c = float(np.float32(c))
    norm = (feats * feats).sum(-1).sqrt()
    unit = feats / norm[..., None]
    if unit.requires_grad:
        unit.retain_grad()
    S, deg, s = [], [], 0
    for L in lengths:
        u = unit[:, s:s + L]
        G = u @ u.transpose(1, 2)
        if unit_diagonal:
            G = torch.where(torch.eye(L, dtype=torch.bool), torch.ones_like(G), G)
        Si = torch.acos(SHRINK * G)
        S.append(Si)
        deg.append(Si.sum(-1) + (M - 1) * c)
        s += L
    rdeg = torch.cat(deg, 1).pow(-0.5)
    tiles, s = [], 0
    for L, Si in zip(lengths, S):
        r = rdeg[:, s:s + L]
        tiles.append(r[:, :, None] * Si * r[:, None, :])
        s += L
    pairs = pair_list(M)
    cross = torch.stack([rdeg[m] * c * rdeg[n] for m, n in pairs]) if pairs else feats.new_zeros(0, N)
    return dict(tiles=tiles, cross=cross, rdeg=rdeg, unit=unit, norm=norm)


def graph_eval(feats, lengths, c, dtiles, dcross, addend, dtype, unit_diagonal=False):
    """tiles / cross / rdeg / dfeats (without and with the addend) of the restatement in ``dtype`` on the CPU."""
    M, N, D = feats.shape
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    x = feats.to(dtype).requires_grad_(True)
    g = graph_ref(x, lengths, c, unit_diagonal)
    flat = pack_tiles(lay, g["tiles"], M)
    ((flat * dtiles.to(dtype)).sum() + (g["cross"] * dcross.to(dtype)).sum()).backward()
    du = (g["unit"].grad / g["norm"][..., None]).detach()
    return dict(tiles=flat.detach(), cross=g["cross"].detach(), rdeg=g["rdeg"].detach(), dfeats=x.grad,
                dfeats_add=x.grad + addend.to(dtype), du=du)


def graph_eval_pooled(feats, lengths, c, dtiles, dcross, addend, r64, perms, unit_diagonal=True):
    """{quantity: the largest error against ``r64`` of float32 evaluations with the feature columns in each order of ``perms``}
    -- the pooled yardstick of angular_graph_ref.py, for inputs on which one float32 evaluation is not a stable measure."""
    yard = {}
    for perm in perms:
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(len(perm))
        r = graph_eval(feats.detach()[..., perm].contiguous(), lengths, c, dtiles, dcross, addend[..., perm].contiguous(), torch.float32,
                       unit_diagonal)
        for k in ("tiles", "cross", "rdeg", "dfeats", "dfeats_add"):
            v = r[k][..., inv] if k.startswith("dfeats") else r[k]
            if v.numel():
                yard[k] = max(yard.get(k, EPS_HALF), err(v, r64[k]))
    return yard


def check(name, got, want64, want32, lines=None):
    """want32: the float32 CPU evaluation, or its error against ``want64`` already (a pooled yardstick)."""
    e, e32 = err(got, want64), want32 if isinstance(want32, float) else err(want32, want64)
    ratio = e / max(e32, EPS_HALF)
    msg = "%-28s kernel %.3e  float32 CPU %.3e  ratio %.2f" % (name, e, e32, ratio)
    print(msg)
    if lines is not None:
        lines.append(msg)
    assert e <= 4 * max(e32, EPS_HALF), msg
    return ratio


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


def no_library_kernels(names):
    bad = [n for n in names if n.startswith("Cijk_") or "rocblas" in n.lower() or "miopen" in n.lower()
           or "hipblaslt" in n.lower() or ("gemm" in n.lower() and "gemm_tn" not in n)]
    assert not bad, bad


# ---- the raw entry points -----------------------------------------------------------------------------------------------------------
def buffers(lay, M, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    nan = float("nan")
    full = lambda *shape: torch.full(shape, nan, dtype=torch.float32, device=DEV)
    b = dict(feats=torch.randn(M, N, D, generator=g), dtiles=torch.randn(lay.tile_elems, generator=g),
             dcross=torch.randn(lay.npairs, N, generator=g), addend=torch.randn(M, N, D, generator=g))
    b = {k: v.to(DEV) for k, v in b.items()}
    b.update(unit=full(M, N, D), norm=full(M, N), cosg=full(lay.tile_elems), cdot=full(lay.npairs, N), rdeg=full(M, N),
             tiles=full(lay.tile_elems), cross=full(lay.npairs, N), wsym=full(lay.tile_elems), etile=full(lay.tile_elems),
             ecross=full(lay.npairs, N), ddeg=full(M, N), dunit=full(M, N, D), dfeats=full(M, N, D))
    return b


def run_entry(b, lay, M, N, D, c, kind, addend, bwd=True):
    """kind None: the entry points without a kind argument."""
    P, lib = _hip.ptr, _hip.lib()
    tail = (c,) if kind is None else (c, kind)
    fwd = lib.mmdfn_adj_build if kind is None else lib.mmdfn_adj_build_kind
    rc = fwd(P(b["feats"]), P(b["unit"]), P(b["norm"]), P(b["cosg"]), P(b["cdot"]), P(b["rdeg"]), P(b["tiles"]), P(b["cross"]),
             *_lay_args(lay), lay.B, M, N, D, lay.max_len, *tail, _hip.stream())
    _hip.check(rc, "mmdfn_adj_build_kind")
    if bwd:
        bw = lib.mmdfn_adj_build_bwd if kind is None else lib.mmdfn_adj_build_bwd_kind
        rc = bw(P(b["dtiles"]), P(b["dcross"]), P(b["unit"]), P(b["norm"]), P(b["cosg"]), P(b["cdot"]), P(b["rdeg"]), P(b["tiles"]),
                P(b["cross"]), P(b["wsym"]), P(b["etile"]), P(b["ecross"]), P(b["ddeg"]), P(b["dunit"]), P(b["dfeats"]),
                P(b["addend"] if addend else None), *_lay_args(lay), lay.B, M, N, D, lay.max_len, *tail, _hip.stream())
        _hip.check(rc, "mmdfn_adj_build_bwd_kind")
    torch.cuda.synchronize()


STRIP = [(lengths, M, 200) for lengths in ([1], [1, 2, 3], [127, 128, 5]) for M in (1, 3)]
GENERAL = [([129, 4], 3, 200), ([5, 1, 3], 3, 260), ([9, 2], 6, 64)]


@pytest.mark.parametrize("lengths,M,D,form", [s + ("strip",) for s in STRIP] + [s + ("general",) for s in GENERAL])
def test_kind1_kernels_against_float64(lengths, M, D, form):
    kind1_against_float64(lengths, M, D, form)


# Structured features (angular_graph_ref.make_feats): kind 1 takes its diagonal as a constant, so its only ill-conditioned entries
# are off-diagonal cosines of +-1 -- correlated rows, exact duplicates, exact opposites -- and rows whose norms span 24 decades.
STRUCTURED = [(([33, 1, 32], 3, 200), "strip"), (([129, 4], 3, 200), "general")]


@pytest.mark.parametrize("family", KIND1_FAMILIES)
@pytest.mark.parametrize("shape,form", STRUCTURED, ids=["strip", "general"])
def test_kind1_kernels_against_float64_on_structured_features(shape, form, family):
    """Measured against the pooled yardstick of float32 evaluations that take the diagonal as the constant the kernels take.  One
    float32 evaluation with the rounded u.u on its diagonal, the yardstick of the test above, is no stable measure here: other
    column orders sit up to 450 x its error, and where the off-diagonal entries are well conditioned (scale) it is 100 x what
    float32 arithmetic gives on the entries the kernels do compute (test_angular_graph_host.py prints both).
    Worst measured kernel / yardstick (MI355X): strip form tiles 1.20, cross 1.30, rdeg 1.12, dfeats 1.10; many-launch form tiles
    2.61, cross 2.10, rdeg 1.43, dfeats 1.09."""
    lengths, M, D = shape
    kind1_against_float64(lengths, M, D, form, make_feats(family, M, sum(lengths), D, KIND1_SEED), family + " ", pooled=True)


def kind1_against_float64(lengths, M, D, form, feats=None, note="", pooled=False):
    N, c = sum(lengths), 0.99999
    lay = DialogueLayout.get(lengths, M, torch.device(DEV))
    b = buffers(lay, M, N, D, 11 + N + M)
    if feats is not None:
        b["feats"] = feats.to(DEV)
    names = kernel_names(lambda: run_entry(b, lay, M, N, D, c, 1, True))
    strip = any("adj_strip_fwd_kernel" in n for n in names)
    print("kernels:", sorted(n.replace("void (anonymous namespace)::", "").split("(")[0] for n in names if "kernel" in n))
    if form == "strip":
        assert strip and any("adj_strip_bwd_kernel" in n for n in names) and not any("tile_dot" in n for n in names), names
    else:
        assert not strip and not any("adj_strip_bwd_kernel" in n for n in names), names
        assert any("tile_dot" in n for n in names) and any("bwd_etile_kernel" in n for n in names), names
    cpu = {k: b[k].cpu() for k in ("feats", "dtiles", "dcross", "addend")}
    r64 = graph_eval(cpu["feats"], lengths, c, cpu["dtiles"], cpu["dcross"], cpu["addend"], torch.float64, pooled)
    r32 = graph_eval(cpu["feats"], lengths, c, cpu["dtiles"], cpu["dcross"], cpu["addend"], torch.float32, pooled)
    if pooled:
        r32 = dict(r32, **graph_eval_pooled(cpu["feats"], lengths, c, cpu["dtiles"], cpu["dcross"], cpu["addend"], r64, pool_perms(D)))
    w = written_mask(lay, M)
    tiles = b["tiles"].cpu()
    assert not torch.isnan(tiles[w]).any()             # every stored entry and every pad column is written
    tag = "%s%s M=%d D=%d " % (note, lengths, M, D)
    check(tag + "tiles", tiles[w], r64["tiles"][w], r32["tiles"] if pooled else r32["tiles"][w])
    pad = r64["tiles"][w] == 0                          # (a stored entry is an acos of less than 1: never 0)
    if bool(pad.any()):
        assert float(tiles[w][pad].abs().max()) == 0.0
    if M > 1:
        check(tag + "cross", b["cross"], r64["cross"], r32["cross"])
        assert float(b["cdot"].abs().max()) == 0.0     # no cross cosine is formed
        if form == "general":
            assert float(b["ecross"].abs().max()) == 0.0   # (scratch of the many-launch form only)
    check(tag + "rdeg", b["rdeg"], r64["rdeg"], r32["rdeg"])
    check(tag + "dfeats+addend", b["dfeats"], r64["dfeats_add"], r32["dfeats_add"])
    b["dfeats"].fill_(float("nan"))
    run_entry(b, lay, M, N, D, c, 1, False)
    got = b["dfeats"].cpu()
    assert not torch.isnan(got).any()
    if max(lengths) == 1:
        # zero in exact arithmetic (module docstring): absolute, against the float32 CPU value and the projection's rounding
        floor = 2.0 ** -23 * float(r64["du"].abs().max())
        bound = 4 * max(float(r32["dfeats"].abs().max()), floor)
        print("%-28s kernel max|.| %.3e  float32 CPU max|.| %.3e  float64 max|.| %.3e  rounding floor %.3e"
              % (tag + "dfeats (== 0)", float(got.abs().max()), float(r32["dfeats"].abs().max()), float(r64["dfeats"].abs().max()), floor))
        assert float(r64["dfeats"].abs().max()) <= 1e-9 * float(r64["du"].abs().max())
        assert float(got.abs().max()) <= bound
    else:
        check(tag + "dfeats", got, r64["dfeats"], r32["dfeats"])


@pytest.mark.parametrize("lengths,M,D", [([127, 128, 5], 3, 200), ([1, 2, 3], 1, 200), ([129, 4], 3, 200), ([9, 2], 6, 64)])
def test_kind0_through_the_new_entry_points_is_bit_identical(lengths, M, D):
    N = sum(lengths)
    lay = DialogueLayout.get(lengths, M, torch.device(DEV))
    for addend in (True, False):
        old, new = buffers(lay, M, N, D, 3), buffers(lay, M, N, D, 3)
        run_entry(old, lay, M, N, D, 0.7, None, addend)
        run_entry(new, lay, M, N, D, 0.7, 0, addend)
        w = written_mask(lay, M).to(DEV)
        for k in ("tiles", "cosg"):
            assert torch.equal(old[k][w], new[k][w]), k
        for k in ("cross", "cdot", "rdeg", "unit", "norm", "dfeats"):
            assert not torch.isnan(new[k]).any() and torch.equal(old[k], new[k]), k


def test_operator_layer_kinds():
    """build_adjacency(kind=...): the default is the angular graph, 'arccos' differs and is differentiable end to end."""
    g = torch.Generator().manual_seed(2)
    feats = torch.randn(3, 9, 200, generator=g).to(DEV)
    a0, a1 = ops.build_adjacency(feats, [5, 1, 3], 0.7), ops.build_adjacency(feats, [5, 1, 3], 0.7, kind="angular")
    assert torch.equal(a0.tiles, a1.tiles) and torch.equal(a0.cross, a1.cross)
    f = feats.clone().requires_grad_(True)
    a2 = ops.build_adjacency(f, [5, 1, 3], 0.99999, kind="arccos")
    assert a2.stacked_feats.shape == f.shape and not torch.equal(a2.tiles, a0.tiles)
    R = torch.randn(27, 27, generator=g).to(DEV)
    (a2.to_dense() * R).sum().backward()
    x = feats.cpu().double().requires_grad_(True)
    (dense_from(graph_ref(x, [5, 1, 3], 0.99999), [5, 1, 3], 3, 9) * R.cpu().double()).sum().backward()
    x32 = feats.cpu().requires_grad_(True)
    (dense_from(graph_ref(x32, [5, 1, 3], 0.99999), [5, 1, 3], 3, 9) * R.cpu()).sum().backward()
    check("build_adjacency dfeats", f.grad, x.grad, x32.grad)


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def gconv(cur, A, h0, W, lamda, alpha, l):
    theta = math.log(lamda / l + 1)
    hi = A @ cur
    return theta * (torch.cat([hi, h0], 1) @ W) + (1 - theta) * ((1 - alpha) * hi + alpha * h0)


def mmgcn2_ref(sd, a, v, l, lengths, lamda, alpha, use_residue, masks=None, scale=1.0):
    """MM_GCN2.forward (model_mm.py:219-258) in the dtype of its arguments; returns (out, dense adjacency, pre-activations).
    masks: {'a', 'l', 'v': (N, nfeat); 'layer': [nl + 1 x (3N, H)]} of 0 / 1 keep flags, or None."""
    N = a.shape[0]
    nl = len([k for k in sd if k.startswith("convs.")])
    drop = (lambda x, m: x) if masks is None else (lambda x, m: x * m * scale)
    mk = masks or dict(a=None, l=None, v=None, layer=[None] * (nl + 1))
    pres = []

    def fc(x, i):
        pres.append(x @ sd["fcs.%d.weight" % i].t() + sd["fcs.%d.bias" % i])
        return torch.relu(pres[-1])
    a_, l_, v_ = fc(drop(a, mk["a"]), 0), fc(drop(l, mk["l"]), 1), fc(drop(v, mk["v"]), 2)
    h0 = torch.cat([a_, v_, l_], 0)
    A = dense_from(graph_ref(torch.stack([a, v, l], 0), lengths, 0.99999), lengths, 3, N)
    cur = h0
    for i in range(nl):
        cur = drop(cur, mk["layer"][i])
        pres.append(gconv(cur, A, h0, sd["convs.%d.weight" % i], lamda, alpha, i + 1))
        cur = torch.relu(pres[-1])
    cur = drop(cur, mk["layer"][nl])
    out = torch.cat([cur[:N], cur[N:2 * N], cur[2 * N:]], -1)
    if use_residue:
        out = torch.cat([l, out], -1)
    return out, A, pres


def lyc_ref(sd, x, lengths, lamda, alpha):
    """GCNII_lyc.forward(adj=None, reason_flag=True, use_residue=True) without dropout (model_GCN.py:444-511)."""
    nl = len([k for k in sd if k.startswith("convs.")])
    A = dense_from(graph_ref(x[None], lengths, 0.0), lengths, 1, x.shape[0])
    pres = [x @ sd["fcs.0.weight"].t() + sd["fcs.0.bias"]]
    h0 = torch.relu(pres[0])
    cur, h, c = h0, torch.zeros_like(h0), torch.zeros_like(h0)
    for i in range(nl):
        q = cur
        g = q @ sd["rnn.weight_ih_l0"].t() + sd["rnn.bias_ih_l0"] + h @ sd["rnn.weight_hh_l0"].t() + sd["rnn.bias_hh_l0"]
        gi, gf, gg, go = g.chunk(4, 1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
        pres.append(gconv(h, A, h0, sd["convs.%d.weight" % i], lamda, alpha, i + 1))
        cur = torch.relu(pres[-1]) + q
    return torch.cat([x, cur], -1), A, pres


def run_ref(fn, sd, xs, G, dtype):
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xs = [x.detach().cpu().to(dtype).requires_grad_(True) for x in xs]
    out, A, pres = fn(sd, xs)
    (out * G.cpu().to(dtype)).sum().backward()
    res = {"out": out.detach(), "adj": A.detach()}
    res.update({"dx%d" % i: x.grad for i, x in enumerate(xs)})
    res.update({"grad/" + k: v.grad for k, v in sd.items()})
    return res, pres


def near_kink(pres, band=1e-5):
    """Share of ReLU pre-activations within ``band`` of the row maximum of zero."""
    n = sum(int((p.abs() < band * p.abs().amax(1, keepdim=True)).sum()) for p in pres)
    return n / sum(p.numel() for p in pres)


def run_module(m, xs, call, G):
    m.zero_grad(set_to_none=True)
    xs = [x.detach().to(DEV).requires_grad_(True) for x in xs]
    out = call(m, xs)
    (out * G.to(DEV)).sum().backward()
    res = {"out": out.detach()}
    res.update({"dx%d" % i: x.grad for i, x in enumerate(xs)})
    res.update({"grad/" + k: p.grad for k, p in m.named_parameters()})
    return res


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLD, "mmgcn2.npz"), allow_pickle=False)
    return {k: torch.from_numpy(g[k]) for k in g.files}


def test_mm_gcn2_against_the_reference_golden(gold):
    lengths = [int(n) for n in gold["dia_len"]]
    sd = {k[len("mm/sd/"):]: v for k, v in gold.items() if k.startswith("mm/sd/")}
    xs, G = [gold["mm/x_" + n] for n in "avl"], gold["mm/G"]
    # (the golden's dropout of 1e-12 keeps every element and its scale is 1 in float32: p = 0 here)
    m = MM_GCN2(200, 2, 100, 6, 0.0, 0.5, 0.2, True, True, True).to(DEV).train()
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    got = run_module(m, xs, lambda m, x: m(x[0], x[1], x[2], lengths, None), G)
    r64, pres = run_ref(lambda s, x: mmgcn2_ref(s, x[0], x[1], x[2], lengths, 0.5, 0.2, True), sd, xs, G, torch.float64)
    assert near_kink(pres) == 0.0
    want = {"out": gold["mm/out"], "adj": gold["mm/adj"]}
    want.update({"dx%d" % i: gold["mm/dx_" + n] for i, n in enumerate("avl")})
    want.update({"grad/" + k: gold["mm/grad/" + k] for k in sd})
    assert tuple(got["out"].shape) == (9, 500) and len(want) == 2 + 3 + 8
    got["adj"] = m.create_big_adj(*[x.to(DEV) for x in xs], lengths).to_dense()
    for k in want:
        check("MM_GCN2 " + k, got[k], r64[k], want[k])


def test_gcnii_lyc_without_adjacency_against_the_reference_golden(gold):
    lengths = [int(n) for n in gold["dia_len"]]
    sd = {k[len("lyc/sd/"):]: v for k, v in gold.items() if k.startswith("lyc/sd/")}
    xs, G = [gold["lyc/x_x"]], gold["lyc/G"]
    m = GCNII_lyc(200, 2, 20, 6, 0.0, 0.5, 0.2, True, True, True, reason_flag=True).to(DEV).train()
    m.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    got = run_module(m, xs, lambda m, x: m(x[0], lengths, None, adj=None), G)
    r64, pres = run_ref(lambda s, x: lyc_ref(s, x[0], lengths, 0.5, 0.2), sd, xs, G, torch.float64)
    assert near_kink(pres) == 0.0
    want = {"out": gold["lyc/out"], "adj": gold["lyc/adj"], "dx0": gold["lyc/dx_x"]}
    want.update({"grad/" + k: gold["lyc/grad/" + k] for k in sd})
    assert tuple(got["out"].shape) == (9, 220) and len(want) == 3 + 8
    got["adj"] = ops.build_adjacency(xs[0].to(DEV)[None], lengths, kind="arccos").to_dense()
    for k in want:
        check("GCNII_lyc " + k, got[k], r64[k], want[k])


def _mm_case(lengths, seed, nfeat=200, H=100, nl=2, p=0.0):
    torch.manual_seed(seed)
    m = MM_GCN2(nfeat, nl, H, 6, p, 0.5, 0.1, True, True, True)
    g = torch.Generator().manual_seed(seed + 1)
    N = sum(lengths)
    xs = [torch.randn(N, nfeat, generator=g) for _ in range(3)]
    G = torch.randn(N, nfeat + 3 * H, generator=g)
    return m, xs, G


def test_mm_gcn2_longer_dialogues_against_float64():
    """[33, 1, 64]: more than one strip, a one-utterance dialogue in the middle.  The seed is the first whose float64
    pre-activations all stay out of the ReLU band (chosen on the CPU restatement, before anything runs on the device)."""
    lengths = [33, 1, 64]
    for seed in range(200):
        m, xs, G = _mm_case(lengths, seed)
        fn = lambda s, x: mmgcn2_ref(s, x[0], x[1], x[2], lengths, 0.5, 0.1, True)
        with torch.no_grad():
            _, _, pres = fn({k: v.double() for k, v in m.state_dict().items()}, [x.double() for x in xs])
        if near_kink(pres) == 0.0:
            break
    else:
        raise AssertionError("no seed keeps the pre-activations out of the ReLU band")
    sd = m.state_dict()
    r64, _ = run_ref(fn, sd, xs, G, torch.float64)
    r32, _ = run_ref(fn, sd, xs, G, torch.float32)
    got = run_module(m.to(DEV).train(), xs, lambda m, x: m(x[0], x[1], x[2], lengths, None), G)
    print("seed", seed)
    for k in got:
        check("MM_GCN2 [33,1,64] " + k, got[k], r64[k], r32[k])


def test_mm_gcn2_dropout_against_float64_on_its_own_flags():
    """Train mode, p = 0.5: the flags the module drew (ops_flags.TAP) go into the float64 restatement.  A draw whose float64
    pre-activations come within 1e-5 of the row maximum of zero could flip a ReLU on a rounding; such a draw is not compared,
    the next seed is taken -- the share of such elements stays under 1 % in every draw and a clean draw must come within 8."""
    lengths, p = [7, 1, 4], 0.5
    N, nfeat, H, nl = sum(lengths), 200, 100, 2
    m, xs, G = _mm_case(lengths, 5, p=p)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    for draw in range(8):
        torch.manual_seed(100 + draw)
        ops_flags.TAP = tap = []
        try:
            got = run_module(m, xs, lambda m, x: m(x[0], x[1], x[2], lengths, None), G)
        finally:
            ops_flags.TAP = None
        assert len(tap) == 1 and tap[0][0] == 3 * N * nfeat + (nl + 1) * 3 * N * H and tap[0][1] == p and tap[0][3] == "mm_gcn2"
        flags = tap[0][2].cpu()
        assert bool(((flags == 0) | (flags == 1)).all()) and abs(float(flags.mean()) - 0.5) < 5 * (0.25 / flags.numel()) ** 0.5
        n_in = N * nfeat
        masks = dict(a=flags[:n_in].view(N, nfeat), l=flags[n_in:2 * n_in].view(N, nfeat), v=flags[2 * n_in:3 * n_in].view(N, nfeat),
                     layer=list(flags[3 * n_in:].view(nl + 1, 3 * N, H)))

        def fn(s, x, dt=None):
            mk = {k: ([t.to(x[0].dtype) for t in v] if k == "layer" else v.to(x[0].dtype)) for k, v in masks.items()}
            return mmgcn2_ref(s, x[0], x[1], x[2], lengths, 0.5, 0.1, True, masks=mk, scale=2.0)
        r64, pres = run_ref(fn, sd, xs, G, torch.float64)
        share = near_kink(pres)
        print("draw", draw, "share of pre-activations in the ReLU band", share)
        assert share < 0.01
        if share == 0.0:
            break
    else:
        raise AssertionError("no draw keeps the pre-activations out of the ReLU band")
    r32, _ = run_ref(fn, sd, xs, G, torch.float32)
    assert float((got["out"][:, nfeat:] == 0).float().mean()) > 0.5          # dropout and ReLU do cut
    for k in got:
        check("MM_GCN2 p=0.5 " + k, got[k], r64[k], r32[k])


def test_mm_gcn2_captured_equals_eager_and_runs_no_library_kernels():
    lengths = [33, 1, 64]
    m, xs, G = _mm_case(lengths, 3)
    m = m.to(DEV).train()
    xs = [x.to(DEV).requires_grad_(True) for x in xs]
    G = G.to(DEV)

    def step():
        m.zero_grad(set_to_none=True)
        for x in xs:
            x.grad = None
        out = m(xs[0], xs[1], xs[2], lengths, None)
        (out * G).sum().backward()
        return out

    def result(out):
        return [out.detach().clone()] + [x.grad.clone() for x in xs] + [p.grad.clone() for p in m.parameters()]
    want = result(step())
    torch.cuda.synchronize()
    names = kernel_names(step)
    no_library_kernels(names)
    for k in ("adj_strip_fwd_kernel", "adj_strip_bwd_kernel", "linear_", "gcnii_combine_fwd_kernel", "gcnii_combine_bwd_kernel"):
        assert any(k in n for n in names), (k, names)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for x in xs:
        x.grad.zero_()
    names = kernel_names(graph.replay)
    no_library_kernels(names)
    assert any("adj_strip_fwd_kernel" in n for n in names), names
    got = result(out)
    assert len(got) == 1 + 3 + 8
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
