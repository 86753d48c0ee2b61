"""The graph propagation kernels against float64 at every tiling edge: K6 and its transpose (csrc/propagate.hip,
propagate_split.hip), K6' (csrc/tile_dot.hip, the bf16-piece form in linear_split.hip) and the fused K6 + K7 strip launch
(csrc/gcn_small.hip).  References, bounds and input families: tests/graph_product_ref.py (proved on the CPU by
tests/test_graph_product_ref_host.py).  Every comparison is elementwise, (n + 16) u S, no element left out; every operand and
result is a column slice of a NaN-filled wider buffer, tile padding columns are NaN, and results are pre-filled with NaN.

Which kernel a case reaches is read off the dispatchers (mmdfn_launch_propagate, launch_tile_dot, mmdfn_tile_outer,
mmdfn_prop_layer_fwd); the tuning build's MMDFN_PROP_CFG / MMDFN_SPLIT_TAIL / MMDFN_TILEDOT_* switches force the others."""
import numpy as np
import pytest
import torch

import graph_product_ref as G
from mm_dfn_amd import _hip, ops
from mm_dfn_amd.layout import DialogueLayout
from mm_dfn_amd.ops_pad import _lay_args
from test_graph_product_ref_host import FUSED_CASES, FUSED_TWO_LAUNCH_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"

# 13 dialogues (more than the 8 of one XCD round): every block-row height (32, 64, 128) at L - 1, L, L + 1, chunk counts 1 .. 9
EDGE = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)

# (lengths, M, family): together M in {1, 2, 3, 6, 9}, single dialogues of 1 / 4 / 49 rows, 8 / 9 / 17 dialogues, 48 | 49 rows
SCENES = [(EDGE, 3, "dense"), (EDGE, 1, "perm"), (EDGE, 2, "samesign"), (EDGE, 2, "graded"), ((1,), 9, "dense"), ((4,), 6, "cross"),
          ((49,), 3, "perm"), ((5,) * 8, 2, "dense"), ((5,) * 9, 3, "cross"), ((3,) * 17, 9, "dense"), ((48, 5), 6, "dense"),
          ((49, 5), 2, "perm")]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                  # (a copy: the cached cases are read-only)


def _lay(lengths, M):
    return DialogueLayout.get(list(lengths), M, torch.device(DEV))


def _scene_name(lengths, M, family):
    ls = "x".join(str(L) for L in lengths) if len(lengths) <= 3 else "%dx%d.." % (len(lengths), lengths[0])
    return "%s.M%d.%s" % (ls, M, family)


def _propagate(name, lengths, M, family, d, transpose=False, shift=0):
    """One launch of mmdfn_propagate on a cached case: strided H and out inside NaN buffers, NaN tile padding."""
    case = G.propagate_case(tuple(lengths), M, family, d, transpose, True, shift)
    hbuf, hcols = G.wide(case.H, 4, 8)
    obuf, ocols = G.wide(np.full(case.H.shape, np.nan, np.float32), 8, 4)
    Hd, Od = _dev(hbuf), _dev(obuf)
    ops.propagate_raw(_dev(case.adj.tiles), _dev(case.adj.cross), Hd[:, hcols], _lay(lengths, M), transpose=transpose,
                      out=Od[:, ocols])
    got = G.check_wide(Od.cpu().numpy(), ocols)
    assert torch.equal(Hd.cpu().view(torch.int32), torch.from_numpy(hbuf).view(torch.int32))       # (the operand is read only)
    return G.check("%s.%s" % (name, _scene_name(lengths, M, family)), got, case.want, case.bound)


# ---- K6 forward, every tiling of the tuning build -------------------------------------------------------------------------------
PRODUCTION_TILINGS = {2: (4, 36, 100, 112), 1: (4, 100, 112), 7: (116, 200, 224), 5: (228, 256, 260, 512),
                      8: (4, 96, 100, 104, 112, 116, 128, 132, 260)}
# the tilings no production path takes: the widths at which the production ones change over
OTHER_TILINGS = {t: (4, 100, 112, 116, 224, 260) for t in (0, 3, 4, 6)}
FORWARD = sorted(((d, t, tail) for t, ds in list(PRODUCTION_TILINGS.items()) + list(OTHER_TILINGS.items()) for d in ds
                  for tail in ((None, "0") if t == 8 and 96 < d <= 112 else (None,))), key=lambda c: c[:2])


@pytest.mark.parametrize("d,tiling,tail", FORWARD)
def test_propagate_forward_tilings(d, tiling, tail, kernel_variants):
    """MMDFN_PROP_CFG 0 .. 7: the f32-MFMA tilings V2(NWR, NWC, NCTW, BKT, RPW) (1, 2, 5, 7 are production paths); 8: the bf16-piece
    kernel, with its 16-column tail tile (96 < d <= 112) and, MMDFN_SPLIT_TAIL=0, with four full tiles instead."""
    kernel_variants.setenv("MMDFN_PROP_CFG", str(tiling))
    if tail is None:
        kernel_variants.delenv("MMDFN_SPLIT_TAIL", raising=False)
    else:
        kernel_variants.setenv("MMDFN_SPLIT_TAIL", tail)
    name = "k6.cfg%d%s.d%d" % (tiling, "" if tail is None else ".tail" + tail, d)
    for lengths, M, family in SCENES:
        _propagate(name, lengths, M, family, d)
    if d == 100:
        for shift in (1, 7):                               # (the perm family's non-zero at two more columns of every row)
            _propagate(name + ".s%d" % shift, EDGE, 1, "perm", d, shift=shift)


# ---- K6 forward, the production library's own choice ----------------------------------------------------------------------------
# mmdfn_launch_propagate: bf16-piece kernel when max_len >= 128 and B M ceil(max_len / 128) ceil(d / 128) >= 48; else by width
# V2(2,4,2,16,1) | V2(8,1,7,16,1) (d <= 112, B M max_len <= | > 32768), V2(4,2,7,16,1) (d <= 224), V2(4,2,4,16,1)
DISPATCH = [
    ("piece", (128,) + (1,) * 85, 3, 100),          # B M max_len = 33 024 with max_len = 128: 258 piece workgroups >= 48
    ("v2_8_1_7", (127,) + (1,) * 86, 3, 100),       # B M max_len = 33 147 > 32 768 and max_len < 128: V2(8,1,7,16,1)
    ("piece", (128,) + (2,) * 15, 3, 100),          # 48 piece workgroups
    ("piece", (128,) + (2,) * 15, 3, 260),
    ("v2_2_4_2", (128,) + (2,) * 14, 3, 100),       # 45 piece workgroups: below the threshold, V2(2,4,2,16,1)
    ("v2_2_4_2", (5, 17, 33), 3, 100), ("v2_2_4_2", (5, 17, 33), 3, 112),
    ("v2_4_2_7", (5, 17, 33), 3, 116), ("v2_4_2_7", (5, 17, 33), 3, 224),
    ("v2_4_2_4", (5, 17, 33), 3, 228), ("v2_4_2_4", (5, 17, 33), 3, 260),
]


@pytest.mark.parametrize("path,lengths,M,d", DISPATCH)
def test_propagate_forward_production_dispatch(path, lengths, M, d):
    for family in ("dense", "perm", "samesign"):
        _propagate("k6.prod.%s.d%d" % (path, d), lengths, M, family, d)


# ---- K6 transposed: launch<2 | 4, 7 | 13 | 8> ----------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [112, 116, 208, 212, 512])
@pytest.mark.parametrize("rows", [48, 49])
def test_propagate_transposed_instantiations(rows, d):
    """max_len <= 48 picks two waves per workgroup, d <= 112 | <= 208 | wider picks 7 | 13 | 8 column tiles: all six, on the
    non-symmetric families (a product with A instead of A^T fails them); M = 9 has all 8 cross terms of a row."""
    nw, nct = (2 if rows <= 48 else 4), (7 if d <= 112 else 13 if d <= 208 else 8)
    name = "k6t.%d_%d.d%d" % (nw, nct, d)
    _propagate(name, (rows, 5), 9, "dense", d, transpose=True)
    _propagate(name, (rows, 5), 2, "perm", d, transpose=True)
    _propagate(name, (rows, 5), 3, "graded", d, transpose=True)
    _propagate(name, (rows,) + (1,) * 8, 6, "dense", d, transpose=True)   # 9 dialogues


@pytest.mark.parametrize("d", [4, 100, 116])
def test_propagate_transposed_edge_lengths(d):
    name = "k6t.4_%d.d%d" % (7 if d <= 112 else 13, d)
    for M, family in ((3, "dense"), (1, "perm"), (2, "samesign")):
        _propagate(name, EDGE, M, family, d, transpose=True)


# ---- K6' -----------------------------------------------------------------------------------------------------------------------
# M in {1, 2, 3, 4, 6, 7, 9}: cross diagonals inside the tile launch (M <= 3, K <= 208), CROSS_DOT(3 | 6, 7 | 13), the generic kernel
OUTER_SCENES = [(EDGE, 3, "dense"), ((5,) * 9, 2, "samesign"), ((3,) * 17, 9, "onehot"), ((49,), 7, "graded"), ((4,), 6, "dense"),
                ((1,), 4, "dense"), ((48, 5), 1, "onehot"), ((65, 17), 6, "samesign")]
OUTER_WIDTHS = [4, 100, 112, 116, 208, 212, 400, 408, 416, 512, 516, 800]
OUTER_MODES = {"default": {}, "v1": {"MMDFN_TILEDOT_V1": "1"}, "f32": {"MMDFN_TILEDOT_SPLIT": "0"},
               "piece": {"MMDFN_TILEDOT_SPLIT": "1"}}


def _tile_outer(name, lengths, M, family, d):
    """mmdfn_tile_outer fresh (into NaN-filled results: the padding columns come back as exact zeros) and in accumulate mode,
    X and Y strided inside NaN buffers."""
    lay = _lay(lengths, M)
    rows = M * lay.N
    X, Y = G.outer_operands(family, rows, d, rows + d)
    xbuf, xcols = G.wide(X, 4, 8)
    ybuf, ycols = G.wide(Y, 8, 4)
    Xd, Yd = _dev(xbuf)[:, xcols], _dev(ybuf)[:, ycols]
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)
    # fresh: the entry point overwrites (accumulate = 0), so NaN pre-fill must vanish everywhere, padding included
    dt, dc = nan(lay.tile_elems), nan(lay.npairs, lay.N)
    _hip.call("mmdfn_tile_outer", _hip.ptr(Xd), _hip.ptr(Yd), _hip.ptr(dt), _hip.ptr(dc), *_lay_args(lay), lay.B, M, lay.N, d,
              Xd.stride(0), Yd.stride(0), lay.max_len, 0, _hip.stream())
    scene = "%s.%s" % (name, _scene_name(lengths, M, family))
    worst = G.check_outer(scene + ".fresh", dt.cpu().numpy(), dc.cpu().numpy(), G.outer_reference(lengths, M, X, Y))
    rs = np.random.RandomState(rows)
    old_t = (rs.randn(lay.tile_elems) * 4).astype(np.float32)
    old_c = (rs.randn(lay.npairs, lay.N) * 4).astype(np.float32)
    acc_t, acc_c = ops.tile_outer_raw(Xd, Yd, lay, _dev(old_t), _dev(old_c))
    worst2 = G.check_outer(scene + ".acc", acc_t.cpu().numpy(), acc_c.cpu().numpy(),
                           G.outer_reference(lengths, M, X, Y, old_t, old_c), padding_zero=False)
    return max(worst + worst2)                                       # (both are (tiles, cross) pairs)


@pytest.mark.parametrize("mode", list(OUTER_MODES))
@pytest.mark.parametrize("d", OUTER_WIDTHS)
def test_tile_outer_widths_and_modalities(d, mode, kernel_variants):
    """d <= 208 one piece; 208 < d <= 512 cut at 200 columns with the tail rule d - c0 <= 208 (212 = 200 + 12, 400 = 200 + 200,
    408 = 200 + 208, 416 = 200 + 200 + 16, 512 = 200 + 200 + 112); d > 512 the bf16-piece kernel.  'v1': the first-generation
    kernels launch<4, 7 | 13>; 'f32' / 'piece': never / always the bf16-piece kernel."""
    for var in ("MMDFN_TILEDOT_V1", "MMDFN_TILEDOT_SPLIT", "MMDFN_TILEDOT_QSPLIT"):
        kernel_variants.delenv(var, raising=False)
    for var, value in OUTER_MODES[mode].items():
        kernel_variants.setenv(var, value)
    for lengths, M, family in OUTER_SCENES:
        _tile_outer("k6p.%s.d%d" % (mode, d), lengths, M, family, d)


@pytest.mark.parametrize("d", [100, 208, 400])
def test_tile_outer_production_piece_kernel_choice(d):
    """16 dialogues of 128 rows, M = 3: 48 blocks of 128 x 128, the production library's threshold for the bf16-piece kernel."""
    _tile_outer("k6p.prod_piece.d%d" % d, (128,) * 16, 3, "dense", d)
    _tile_outer("k6p.prod_piece.d%d" % d, (128,) * 16, 3, "onehot", d)


def test_tile_outer_first_generation_wide_kernel(kernel_variants):
    """launch<4, 32> (208 < K <= 512 in one piece): what a piece-kernel-sized launch runs when the bf16-piece kernel is switched off."""
    kernel_variants.setenv("MMDFN_TILEDOT_SPLIT", "0")
    kernel_variants.delenv("MMDFN_TILEDOT_V1", raising=False)
    for d in (212, 400, 512):
        _tile_outer("k6p.v1_4_32.d%d" % d, (128,) * 16, 3, "dense", d)


# ---- the fused K6 + K7 layer ---------------------------------------------------------------------------------------------------
def _fused_operands(lengths, M, H, variant):
    case = G.fused_case(tuple(lengths), M, H, "plain" if variant == "plain" else "q+mask")
    ref = G.fused_reference(case)
    lay = _lay(lengths, M)
    R = M * lay.N
    ldz = 2 * H if variant == "strided" else H
    ldo = H + 8 if variant == "strided" else H
    zbuf = np.full((R, ldz), np.nan, np.float32)
    zbuf[:, ldz - H:] = case.z
    zin = _dev(zbuf)[:, ldz - H:]
    opt = lambda a: None if a is None else _dev(a)
    return case, ref, lay, R, zin, ldo, _dev(case.h0), _dev(case.W), opt(case.q), opt(case.mk)


def _check_fused(name, ref, H, hi, out, gm):
    out = out.cpu().numpy()
    if out.shape[1] > H:
        assert np.isnan(out[:, H:]).all()                            # nothing written beyond the H columns
    return G.check_fused(name, ref, hi.cpu().numpy(), out[:, :H], gm.cpu().numpy())


@pytest.mark.parametrize("lengths,M,H", FUSED_CASES)
@pytest.mark.parametrize("variant", ["plain", "q+mask", "strided"])
def test_fused_layer_forward(lengths, M, H, variant):
    case, ref, lay, R, zin, ldo, h0, W, q, mk = _fused_operands(lengths, M, H, variant)
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)
    hi, out, gm = nan(R, H), nan(R, ldo), nan(R, H)
    P = _hip.ptr
    tiles, cross = _dev(case.adj.tiles), _dev(case.adj.cross)
    rc = _hip.call("mmdfn_prop_layer_fwd", P(tiles), P(cross), P(zin), zin.stride(0), *_lay_args(lay),
                   lay.B, M, lay.N, lay.max_len, P(h0), P(W), P(q), P(mk), P(hi), P(out), P(gm), case.theta, case.alpha, H, ldo,
                   case.ms, _hip.stream())
    assert rc == 0
    _check_fused("fused.%s.%s" % (variant, _scene_name(lengths, M, "H%d" % H)), ref, H, hi, out, gm)


@pytest.mark.parametrize("lengths,M,H", FUSED_TWO_LAUNCH_CASES)
@pytest.mark.parametrize("variant", ["plain", "strided"])
def test_fused_layer_declines_and_the_two_launches_meet_the_reference(lengths, M, H, variant):
    """M = 4, max_len = 129 and a grid of 4 128 strips: the dispatcher answers -2 and writes nothing; mmdfn_propagate +
    mmdfn_gcnii_layer_fwd, what the caller then runs, meet the same float64 reference."""
    case, ref, lay, R, zin, ldo, h0, W, q, mk = _fused_operands(lengths, M, H, variant)
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)
    hi, out, gm = nan(R, H), nan(R, ldo), nan(R, H)
    P = _hip.ptr
    tiles, cross = _dev(case.adj.tiles), _dev(case.adj.cross)
    rc = _hip.call("mmdfn_prop_layer_fwd", P(tiles), P(cross), P(zin), zin.stride(0), *_lay_args(lay), lay.B, M, lay.N, lay.max_len,
                   P(h0), P(W), P(q), P(mk), P(hi), P(out), P(gm), case.theta, case.alpha, H, ldo, case.ms, _hip.stream(),
                   allow=(-2,))
    assert rc == -2
    torch.cuda.synchronize()
    assert torch.isnan(hi).all() and torch.isnan(out).all() and torch.isnan(gm).all()
    ops.propagate_raw(tiles, cross, zin, lay, out=hi)
    _hip.call("mmdfn_gcnii_layer_fwd", P(hi), P(h0), P(W), P(q), P(mk), P(out), P(gm), case.theta, case.alpha, R, H, ldo, case.ms,
              _hip.stream())
    _check_fused("two_launch.%s.%s" % (variant, _scene_name(lengths, M, "H%d" % H)), ref, H, hi, out, gm)


# ---- argument checks -----------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing():
    lengths, d = (5, 3), 8
    nan = lambda *sh: torch.full(sh, float("nan"), device=DEV)
    P = _hip.ptr

    def propagate(M, d, ldh, ldo):
        lay = _lay(lengths, M)
        R = M * lay.N
        tiles, cross = torch.ones(lay.tile_elems, device=DEV), torch.ones(lay.npairs, lay.N, device=DEV)
        H, out = torch.ones(R, 16, device=DEV), nan(R, 16)
        with pytest.raises(_hip.HipLibraryError):
            _hip.call("mmdfn_propagate", P(tiles), P(cross), P(H), P(out), *_lay_args(lay), lay.B, M, lay.N, d, ldh, ldo,
                      lay.max_len, 0, _hip.stream())
        torch.cuda.synchronize()
        assert torch.isnan(out).all()

    propagate(10, d, 16, 16)            # more than 9 modalities
    propagate(3, 6, 16, 16)             # d % 4 != 0
    propagate(3, d, 4, 16)              # ldh < d
    propagate(3, d, 16, 4)              # ldo < d
    lay = _lay(lengths, 3)
    X, dt, dc = torch.ones(3 * lay.N, 16, device=DEV), nan(lay.tile_elems), nan(lay.npairs, lay.N)
    for dd, ldx in ((6, 16), (d, 4)):
        with pytest.raises(_hip.HipLibraryError):
            _hip.call("mmdfn_tile_outer", P(X), P(X), P(dt), P(dc), *_lay_args(lay), lay.B, 3, lay.N, dd, ldx, 16, lay.max_len, 0,
                      _hip.stream())
    torch.cuda.synchronize()
    assert torch.isnan(dt).all() and torch.isnan(dc).all()
