"""Restatement of the angular dialogue graph (adjacency kind 0 of K5: MM_GCN.create_big_adj, model_mm.py:122-180), shared by
test_angular_graph_host.py and test_angular_graph_gpu.py; the helpers the arccos (kind 1) tests share with them live here too.

The graph is written once, generic in the dtype, after oracle/mmdfn_oracle.py (unit_rows, angular_sim, adjacency_tiles) and
evaluated on the CPU:

  * in float64: the reference value;
  * in float32, eight times, the feature columns permuted differently each time (an identity in exact arithmetic, another
    summation order in float32): per compared quantity the LARGEST of the eight errors against float64 is the yardstick.  A
    single float32 evaluation is not a stable measure where acos is steep (a Gram entry one ulp to either side moves an entry
    by 4e-6); the pooled one is: test_angular_graph_host.py holds four further float32 evaluations (other summation orders, the
    stand-ins for a correct kernel) to 2.5 x the yardstick on every case the device tests use, and the device tests allow 4 x.

Errors are max |x - x64| / max |x64|; a float32 result is defined to half an ulp of its largest value only, so a yardstick
counts as at least 2^-24.  Nothing here touches the device or the package's kernels.
"""
import math

import numpy as np
import torch

from mm_dfn_amd.layout import DialogueLayout, pair_list

SHRINK = float(np.float32(0.99999))          # the float32 constant the kernels and the reference's float32 tensors multiply by
EPS_HALF = 2.0 ** -24
MARGIN = 4.0                                  # a device result against the yardstick (the GRU recurrence and kind-1 margin)
STAND_IN_MARGIN = 2.5                         # a correct float32 evaluation against the yardstick (host test)
N_POOL = 8


# ---- shared with the kind-1 tests ---------------------------------------------------------------------------------------------------
def pack_tiles(lay, tiles, M):
    """[(M, L, L)] -> the flat block-tile array (pad columns 0)."""
    flat = tiles[0].new_zeros(lay.tile_elems)
    for i, L in enumerate(lay.lengths):
        ld, base = int(lay.ld_host[i]), int(lay.tile_base_host[i])
        blk = tiles[i].new_zeros(M, L, ld)
        blk[:, :, :L] = tiles[i]
        flat[base:base + M * L * ld] = blk.reshape(-1)
    return flat


def dense_from(g, lengths, M, N):
    """The dense (MN x MN) matrix of a restatement's tiles and cross diagonals."""
    A = g["cross"].new_zeros(M * N, M * N)
    s = 0
    for L, T in zip(lengths, g["tiles"]):
        for m in range(M):
            A[m * N + s:m * N + s + L, m * N + s:m * N + s + L] = T[m]
        s += L
    ar = torch.arange(N)
    for k, (m, n) in enumerate(pair_list(M)):
        A[m * N + ar, n * N + ar] = g["cross"][k]
        A[n * N + ar, m * N + ar] = g["cross"][k]
    return A


def dense_cotangent(lay, M, dtiles, dcross):
    """The (MN x MN) cotangent of to_dense() that is (dtiles, dcross) on the packed storage: a cross diagonal sits in the dense
    matrix twice, each copy takes half (exact)."""
    N = lay.N
    R = dtiles.new_zeros(M * N, M * N)
    for i, L in enumerate(lay.lengths):
        ld, base, rs = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        blk = dtiles[base:base + M * L * ld].view(M, L, ld)
        for m in range(M):
            R[m * N + rs:m * N + rs + L, m * N + rs:m * N + rs + L] = blk[m, :, :L]
    ar = torch.arange(N)
    for k, (m, n) in enumerate(pair_list(M)):
        R[m * N + ar, n * N + ar] = 0.5 * dcross[k]
        R[n * N + ar, m * N + ar] = 0.5 * dcross[k]
    return R


def written_mask(lay, M):
    mask = torch.zeros(lay.tile_elems, dtype=torch.bool)
    for i, L in enumerate(lay.lengths):
        ld, base = int(lay.ld_host[i]), int(lay.tile_base_host[i])
        mask[base:base + M * L * ld] = True
    return mask


def entry_masks(lay, M):
    """(diagonal, off-diagonal, padding) masks over the flat tile array."""
    diag = torch.zeros(lay.tile_elems, dtype=torch.bool)
    off = torch.zeros(lay.tile_elems, dtype=torch.bool)
    pad = torch.zeros(lay.tile_elems, dtype=torch.bool)
    for i, L in enumerate(lay.lengths):
        ld, base = int(lay.ld_host[i]), int(lay.tile_base_host[i])
        d = torch.zeros(M, L, ld, dtype=torch.bool)
        d[:, torch.arange(L), torch.arange(L)] = True
        o = torch.zeros(M, L, ld, dtype=torch.bool)
        o[:, :, :L] = True
        o &= ~d
        diag[base:base + M * L * ld] = d.reshape(-1)
        off[base:base + M * L * ld] = o.reshape(-1)
        pad[base:base + M * L * ld] = ~(d | o).reshape(-1)
    return diag, off, pad


def rdeg_outer(lay, M, rdeg):
    """r_p r_q in float64 at every stored entry of the flat tile array (1 in the padding columns)."""
    out = torch.ones(lay.tile_elems, dtype=torch.float64)
    r = rdeg.detach().double().cpu()
    for i, L in enumerate(lay.lengths):
        ld, base, rs = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        blk = torch.ones(M, L, ld, dtype=torch.float64)
        blk[:, :, :L] = r[:, rs:rs + L, None] * r[:, None, rs:rs + L]
        out[base:base + M * L * ld] = blk.reshape(-1)
    return out


def err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
FAMILIES = ("randn", "corr0.3", "corr0.03", "corr0.003", "relu", "dup", "anti", "scale")


# (lengths, M, D, family) -> seed where 0 gives a draw on which a stand-in of test_angular_graph_host.py leaves 2.5 x the yardstick
SEEDS = {((5, 1, 7, 3, 2, 9, 4, 1, 6), 3, 200, "corr0.03"): 1}


def make_feats(family, M, N, D, seed):
    """(M, N, D) float32 features of one input family, from a fixed seed on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, D, generator=g)
    if family == "randn":
        pass
    elif family.startswith("corr"):           # one base row per modality + eps * noise: off-diagonal cosines 0.9 .. 1 - 1e-5
        x = torch.randn(M, 1, D, generator=g) + float(family[4:]) * x
    elif family == "relu":                    # all-positive features, cosines around 0.6
        x = torch.relu(x + 1)
    elif family in ("dup", "anti"):           # odd rows +-(even neighbour), modality 1 a multiple of modality 0: cosines of +-1
        sign, factor = (1.0, 3.0) if family == "dup" else (-1.0, -2.0)
        x[:, 1::2] = sign * x[:, 0:N - 1:2]
        if M > 1:
            x[1] = factor * x[0]
    elif family == "scale":                   # norms over 24 decades inside one dialogue
        x = x * (10.0 ** torch.linspace(-12, 12, N, dtype=torch.float64))[None, :, None].float()
    else:
        raise ValueError(family)
    return x.contiguous()


def case_inputs(lengths, M, D, family):
    """feats, dtiles (the padding columns' values do not matter: nothing reads them), dcross, addend -- float32, CPU."""
    N = sum(lengths)
    seed = SEEDS.get((tuple(lengths), M, D, family), 0)
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    g = torch.Generator().manual_seed(1000 + seed + 7 * N + M)
    return dict(feats=make_feats(family, M, N, D, 17 + seed + N + M), dtiles=torch.randn(lay.tile_elems, generator=g),
                dcross=torch.randn(lay.npairs, N, generator=g), addend=torch.randn(M, N, D, generator=g))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _dot(a, b, chunk):
    """sum_k a[..., k] b[..., k]; ``chunk``: the way a row of lanes sums it -- lane j of ``chunk`` takes the columns j, j + chunk, ...
    one after the other, the lanes' partial sums are added last."""
    p = a * b
    if chunk is None:
        return p.sum(-1)
    p = torch.nn.functional.pad(p, (0, -p.shape[-1] % chunk))
    return p.reshape(*p.shape[:-1], -1, chunk).sum(-2).sum(-1)


def _gram(u, chunk):
    """u u^T; ``chunk``: the way a chain of matrix instructions sums it -- ``chunk`` columns at a time, one product after the other."""
    if chunk is None:
        return u @ u.transpose(1, 2)
    acc = 0
    for k in range(0, u.shape[-1], chunk):
        acc = acc + u[..., k:k + chunk] @ u[..., k:k + chunk].transpose(1, 2)
    return acc


def angular_sim(c):
    return 1.0 - torch.acos(c * SHRINK) / math.pi


def angular_graph_ref(feats, lengths, modal_weight, chunk=None, fault=None):
    """Angular graph of (M, N, D) features in their dtype.  Per dialogue the normalised tiles [(M, L, L)]; cross (npairs, N);
    rdeg (M, N); and what the entry point saves for its backward pass: unit = x / ||x|| (no epsilon), norm = ||x||, cosg [(M, L, L)]
    the raw cosine Gram tiles u u^T (diagonal included), cdot (npairs, N) the raw cross-modal cosines u_m . u_n.
    ``fault`` (deliberate errors, for the host test that shows the comparison notices them): 'sim' scales every off-diagonal similarity by 1 + 3e-5, 'stored' does so after the degrees are summed, 'ddq' drops
    the degrees' dependence on the second row of each pair (the dd_q term of the backward pass)."""
    M, N, D = feats.shape
    mw = float(np.float32(modal_weight))
    norm = _dot(feats, feats, chunk).sqrt()
    unit = feats / norm[..., None]
    pairs = pair_list(M)
    cdot = torch.stack([_dot(unit[m], unit[n], chunk) for m, n in pairs]) if pairs else feats.new_zeros(0, N)
    craw = angular_sim(cdot) * mw                                       # cross-modal entries before normalisation
    cosg, S, deg, s = [], [], [], 0
    for L in lengths:
        G = _gram(unit[:, s:s + L], chunk)
        Si = angular_sim(G)
        bend = torch.where(torch.eye(L, dtype=torch.bool), 1.0, 1.0 + 3e-5).to(G.dtype)
        if fault == "sim":
            Si = Si * bend
        Sd = Si if fault != "ddq" else angular_sim(unit[:, s:s + L] @ unit[:, s:s + L].detach().transpose(1, 2))
        if fault == "stored":
            Si = Si * bend
        d = torch.stack([sum((craw[pairs.index((min(m, n), max(m, n))), s:s + L] for n in range(M) if n != m), Sd[m].sum(-1))
                         for m in range(M)])                            # (the cross-modal entries enter the degrees)
        cosg.append(G)
        S.append(Si)
        deg.append(d)
        s += L
    rdeg = torch.cat(deg, 1).pow(-0.5)
    tiles, s = [], 0
    for L, Si in zip(lengths, S):
        r = rdeg[:, s:s + L]
        tiles.append((r[:, :, None] * Si) * r[:, None, :])
        s += L
    cross = torch.stack([craw[k] * rdeg[m] * rdeg[n] for k, (m, n) in enumerate(pairs)]) if pairs else feats.new_zeros(0, N)
    return dict(tiles=tiles, cross=cross, rdeg=rdeg, unit=unit, norm=norm, cosg=cosg, cdot=cdot)


# sim_off: the un-normalised off-diagonal similarities a result implies, T[p,q] / (r_p r_q) from ITS OWN tiles and rdeg.  A normalised
# entry of a short dialogue carries the rounding of its diagonal (through the degrees) and does not move when every similarity is
# scaled alike; sim_off carries the rounding of acos and two products only, so it is the sharpest of the quantities.
QUANTITIES = ("sim_off", "tiles_off", "tiles_diag", "cross", "rdeg", "unit", "norm", "cosg", "cdot", "dfeats", "dfeats_add")


def graph_eval(inp, lengths, modal_weight, dtype, perm=None, chunk=None, fault=None):
    """Every compared quantity of the restatement in ``dtype`` on the CPU, the feature columns taken in the order ``perm``
    (results come back in the original order).  dfeats: d/d feats of sum(tiles * dtiles) + sum(cross * dcross)."""
    feats = inp["feats"]
    M, N, D = feats.shape
    lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
    perm = torch.arange(D) if perm is None else perm
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(D)
    x = feats.to(dtype)[..., perm].contiguous().requires_grad_(True)
    g = angular_graph_ref(x, lengths, modal_weight, chunk, fault)
    flat = pack_tiles(lay, g["tiles"], M)
    ((flat * inp["dtiles"].to(dtype)).sum() + (g["cross"] * inp["dcross"].to(dtype)).sum()).backward()
    dfeats = x.grad[..., inv]
    return dict(tiles=flat.detach(), cosg=pack_tiles(lay, [c.detach() for c in g["cosg"]], M), cross=g["cross"].detach(),
                cdot=g["cdot"].detach(), rdeg=g["rdeg"].detach(), unit=g["unit"].detach()[..., inv], norm=g["norm"].detach(),
                dfeats=dfeats, dfeats_add=dfeats + inp["addend"].to(dtype))


def split(res, lay, M):
    """{quantity: tensor} of one evaluation, or of a device result given as a dict of the same names (those it holds); empty
    quantities (the cross diagonals of one modality) are left out."""
    diag, off, _ = entry_masks(lay, M)
    w = written_mask(lay, M)
    pick = dict(tiles_off=("tiles", off), tiles_diag=("tiles", diag), cosg=("cosg", w))
    out = {}
    if "tiles" in res and "rdeg" in res and bool(off.any()):
        out["sim_off"] = res["tiles"].detach().double().cpu()[off] / rdeg_outer(lay, M, res["rdeg"])[off]
    for k in QUANTITIES[1:]:
        src, mask = pick.get(k, (k, None))
        if src in res:
            v = res[src].detach().cpu()
            v = v if mask is None else v[mask]
            if v.numel():
                out[k] = v
    return out


def errors(res, ref64, lay, M):
    """{quantity: max |x - x64| / max |x64|}.  A quantity that is zero throughout in float64 (the cross diagonals at modal weight
    0) has no relative error: it is reported as 0.0 when the result is exactly zero too, inf otherwise."""
    a, b = split(res, lay, M), split(ref64, lay, M)
    out = {}
    for k in a:
        if float(b[k].abs().max()) == 0.0:
            out[k] = 0.0 if float(a[k].abs().max()) == 0.0 else float("inf")
        else:
            out[k] = err(a[k], b[k])
    return out


def pool_perms(D, n=N_POOL, seed=5):
    g = torch.Generator().manual_seed(seed + D)
    return [torch.randperm(D, generator=g) for _ in range(n)]


_CACHE = {}


def reference(lengths, M, D, family, modal_weight):
    """(inputs, float64 evaluation, yardstick {quantity: error}) of one case, computed once per process."""
    key = (tuple(lengths), M, D, family, float(modal_weight))
    if key not in _CACHE:
        lay = DialogueLayout.get(lengths, M, torch.device("cpu"))
        inp = case_inputs(lengths, M, D, family)
        r64 = graph_eval(inp, lengths, modal_weight, torch.float64)
        yard = {}
        for perm in pool_perms(D):
            r32 = graph_eval(inp, lengths, modal_weight, torch.float32, perm)
            assert all(bool(torch.isfinite(v).all()) for v in list(r32.values()) + list(r64.values())), key
            for k, e in errors(r32, r64, lay, M).items():
                yard[k] = max(yard.get(k, EPS_HALF), e)
        _CACHE[key] = (inp, r64, yard)
    return _CACHE[key]


def stand_ins(inp, lengths, modal_weight):
    """Four further float32 evaluations in other summation orders (what a correct kernel may do): the columns reversed, another
    permutation, and two in the orders the kernels use (_dot, _gram) -- 16 lanes per row with 16-column Gram steps, and 4 lanes
    with 4-column steps (the depth of one f32 MFMA) on permuted columns."""
    D = inp["feats"].shape[-1]
    g = torch.Generator().manual_seed(99 + D)
    p1, p2 = torch.randperm(D, generator=g), torch.randperm(D, generator=g)
    return [graph_eval(inp, lengths, modal_weight, torch.float32, torch.arange(D - 1, -1, -1)),
            graph_eval(inp, lengths, modal_weight, torch.float32, p1),
            graph_eval(inp, lengths, modal_weight, torch.float32, None, 16),
            graph_eval(inp, lengths, modal_weight, torch.float32, p2, 4)]


def report(tag, got_err, yard, lines=None):
    """Print kernel error, yardstick and ratio per quantity; return {quantity: ratio} (nothing is asserted here)."""
    ratios = {}
    for k in QUANTITIES:
        if k not in got_err:
            continue
        ratios[k] = got_err[k] / yard[k]
        msg = "%-58s %-10s error %.3e  yardstick %.3e  ratio %.2f" % (tag, k, got_err[k], yard[k], ratios[k])
        print(msg)
        if lines is not None:
            lines.append(msg)
    return ratios


# ---- the cases of the device tests (lengths, M, D) ----------------------------------------------------------------------------------
ONE = ([1], 3, 200)
TINY = ([2, 1, 3], 3, 200)
STRIP_PLUS_ONE = ([33, 1, 32], 3, 200)        # one strip of 32 plus one row, a one-utterance dialogue in the middle
TWO_STRIPS = ([64, 65], 3, 200)
LONGEST = ([127, 128], 2, 64)
NARROW = ([40, 41, 42], 3, 36)                # a width that is no multiple of 16
NINE = ([5, 1, 7, 3, 2, 9, 4, 1, 6], 3, 200)  # the block decode past eight dialogues
LONG = ([129, 4], 3, 200)                     # the many-launch form only: longer than a strip tile,
SIX = ([9, 2], 6, 64)                         # more than three modalities,
WIDE = ([5, 1, 3], 3, 260)                    # wider than 256
BASE = ("randn", "corr0.03")


def _cases(full, base, extra):
    out = [(s, f, 0.7) for s in full for f in FAMILIES] + [(s, f, 0.7) for s in base for f in BASE]
    return out + [c for c in extra if c not in out]


# strip form: every family on three shapes, the baseline pair on the rest, the form-against-form families on TWO_STRIPS,
# a duplicate-heavy case on the longest tile, modal weights 1 and 0 on STRIP_PLUS_ONE
STRIP_CASES = _cases([STRIP_PLUS_ONE, NARROW, NINE], [ONE, TINY, TWO_STRIPS, LONGEST],
                     [(TWO_STRIPS, "corr0.003", 0.7), (TWO_STRIPS, "dup", 0.7), (LONGEST, "dup", 0.7)]
                     + [(STRIP_PLUS_ONE, f, mw) for mw in (1.0, 0.0) for f in BASE])
# many-launch form: STRIP_PLUS_ONE and TWO_STRIPS are forced into it, the others take it by their shape
GENERAL_CASES = _cases([STRIP_PLUS_ONE, LONG, SIX], [TWO_STRIPS, WIDE],
                       [(TWO_STRIPS, "corr0.003", 0.7), (TWO_STRIPS, "dup", 0.7)]
                       + [(LONG, f, mw) for mw in (1.0, 0.0) for f in BASE])
FORCED_GENERAL = (STRIP_PLUS_ONE, TWO_STRIPS)
BOTH_FORMS = [(s, f, 0.7) for s in FORCED_GENERAL for f in ("corr0.003", "dup")]
OPERATOR_CASES = [(s, f, 0.7) for s in (STRIP_PLUS_ONE, LONG) for f in ("corr0.03", "dup", "anti")]
# kind 1 on structured inputs: one strip shape, one many-launch shape
KIND1_FAMILIES = ("corr0.03", "dup", "anti", "scale")
KIND1_SEED = 23


def all_cases():
    out = []
    for c in STRIP_CASES + GENERAL_CASES + OPERATOR_CASES:
        if c not in out:
            out.append(c)
    return out


def case_id(case):
    (lengths, M, D), family, mw = case
    return "%s-M%d-D%d-%s-mw%g" % ("_".join(str(n) for n in lengths), M, D, family, mw)
