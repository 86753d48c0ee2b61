"""Float64 reference, derived elementwise bound, structured input families, launch lists and a numpy model for the weight-gradient
kernels (csrc/gemm_tn.hip, gemm_tn_split.hip, gemm_tn_split_body.h, the slab reduction and the foreign slab stacks).

Everything here runs on the CPU.  tests/test_wgrad_product_ref_host.py proves the instrument (the model passes; a model with one
piece product removed, two rows of B exchanged, the shift off by one, a slab left out or the column sums taken over the shifted
range does not); tests/test_wgrad_products_gpu.py points it at the kernels.

One output of a batch (include/mmdfn_hip.h, "Batch form"):

    C      = base   [accumulate] + sum_segments sum_r A_s[r, :]^T B_s[r + sh_s, :]       rows of B outside [0, R_s) count as zero
    colsum = base_c [accumulate] + sum_segments sum_r A_s[r, :]                          over ALL rows of A whatever the shift

The bound, with u = 2^-24, for every element, none excluded (the convention of dense_product_ref.py):

    |got - want| <= (n + 16) u S + 2^-126,        S = sum |A|^T |B_shifted| + |base|

n = that element's count of non-zero terms, (A != 0)^T (B_shifted != 0) summed over the segments (for a column sum: the non-zero
entries of the column).  It holds for any summation order, hence for any split of the rows into slabs.  Of the 16, two are the
piece products the bf16 form leaves out (<= 2^-23 |a||b| per product), the rest covers the epilogue (the slab sum, the addend).

The contraction index is the ROW here, so the one-hot families have one live row per output element: column m of A is non-zero
at row (r0 + m) mod R only (``rowhot``), or column n of B (``rowhot_b``).  n is 1, the bound 17 u |a b|, a missing third-order
piece product (2^-16 per product) tens of bounds away; sweeping r0 in steps of M makes every row the live row once, and every
slab in turn the only one that holds non-zero values: a slab skipped, read twice or taken from a neighbour's stack, or a row of A
paired with the wrong row of a shifted B, is a mismatch of the size of the value itself."""
import collections

import numpy as np

from dense_product_ref import TINY, U, _full, check, cut, emulate, to_bf16, worst_ratio, PRODUCTS  # noqa: F401  (re-exported)

Seg = collections.namedtuple("Seg", "A B sh")                    # A (R, M), B (R, N) float32; row r of A meets row r + sh of B
Output = collections.namedtuple("Output", "M N acc segs base base_c")   # segs: list of Seg; base (M, N), base_c (M,) float32
Spec = collections.namedtuple("Spec", "M N acc segs")            # segs: list of (R, sh)

ONEHOT = ("rowhot", "rowhot_b", "bf16a")
DENSE = ("samesign", "cancel", "graded", "dropout")
FAMILIES = ONEHOT + DENSE
QUICK = ONEHOT + ("samesign",)


def tns_plan(R, rows_target=256):
    """(rows per split, effective splits) of a segment in the bf16-piece form (tns_eff_splits, csrc/gemm_tn.hip): a multiple of 8
    splits, at least two 32-row chunks per split."""
    splits = max(8, 8 * ((R + 4 * rows_target) // (8 * rows_target)))
    splits = max(1, min(splits, (R + 63) // 64))
    rps = -(-(-(-R // splits)) // 32) * 32
    return rps, -(-R // rps)


def draw(name, R, M, N, rs, r0=0):
    """One segment's operands (A, B) of family ``name``; r0: the live row of column 0 in the one-hot families."""
    if name in ("rowhot", "bf16a"):
        A = np.zeros((R, M), np.float32)
        v = _full(rs, M)
        A[(r0 + np.arange(M)) % R, np.arange(M)] = to_bf16(v) if name == "bf16a" else v
        return A, _full(rs, R, N)
    if name == "rowhot_b":
        B = np.zeros((R, N), np.float32)
        B[(r0 + np.arange(N)) % R, np.arange(N)] = _full(rs, N)
        return _full(rs, R, M), B
    A, B = _full(rs, R, M), _full(rs, R, N)
    if name == "samesign":
        return np.abs(A), np.abs(B)
    if name == "cancel":
        # rows equal in pairs in A, +- pairs in B on the even output columns: want is exactly 0 there (even shifts) while S is full
        h = R // 2
        A[1:2 * h:2] = A[0:2 * h:2]
        B[1:2 * h:2, 0::2] = -B[0:2 * h:2, 0::2]
        if R % 2:
            A[-1] = 0.0
        return A, B
    if name == "graded":
        sa = (2.0 ** rs.randint(-20, 21, size=(1, M))).astype(np.float32)
        sb = (2.0 ** rs.randint(-20, 21, size=(1, N))).astype(np.float32)
        return A * sa, B * sb
    if name == "dropout":
        A = A * (rs.rand(R, M) < 0.5).astype(np.float32) * np.float32(2.0)
        A[::5] = 0.0                                    # zero rows
        B[3::7] = 0.0
        A[:, M // 2] = 0.0                              # one all-zero column
        rps, eff = tns_plan(R)
        lo = rps * (eff // 2)                           # one whole split's rows
        A[lo:lo + rps] = 0.0
        B[lo:lo + rps] = 0.0
        return A, B
    raise ValueError(name)


def sweep_length(name, specs):
    """Launches the one-hot sweep of ``name`` takes on these outputs: every row of every segment is the live row at least once."""
    if name in ("rowhot", "bf16a"):
        return max(-(-R // o.M) for o in specs for R, _ in o.segs)
    if name == "rowhot_b":
        return max(-(-R // o.N) for o in specs for R, _ in o.segs)
    return 1


def build(specs, name, seed, k=0, r0=None, share=False):
    """The outputs of one launch in family ``name``: step k of the one-hot sweep (r0 = k M, or k N for rowhot_b), or ``r0``.
    ``share``: the segments of an output (all of one length) use ONE operand pair."""
    rs = np.random.RandomState(seed)
    outs = []
    for o in specs:
        step = o.N if name == "rowhot_b" else o.M
        live = k * step if r0 is None else r0
        if share:
            assert len(set(o.segs)) == 1
            pair = draw(name, o.segs[0][0], o.M, o.N, rs, live)
            segs = [Seg(pair[0], pair[1], sh) for _, sh in o.segs]
        else:
            segs = [Seg(*draw(name, R, o.M, o.N, rs, live), sh) for R, sh in o.segs]
        outs.append(Output(o.M, o.N, o.acc, segs, _full(rs, o.M, o.N), _full(rs, o.M)))
    return outs


def shifted(B, sh):
    """Row r of the result is row r + sh of B, zero where that row does not exist."""
    R = B.shape[0]
    out = np.zeros_like(B)
    lo, hi = max(0, -sh), min(R, R - sh)
    if hi > lo:
        out[lo:hi] = B[lo + sh:hi + sh]
    return out


def reference(out):
    """(want, bound, want_c, bound_c) in float64 for one Output.  Segments that share their arrays are computed once."""
    M, N = out.M, out.N
    want, S, n = (np.zeros((M, N)) for _ in range(3))
    wc, Sc, nc = (np.zeros(M) for _ in range(3))
    seen = {}
    for seg in out.segs:
        key = (id(seg.A), id(seg.B), seg.sh)
        if key not in seen:
            A, Bs = np.asarray(seg.A, np.float64), np.asarray(shifted(seg.B, seg.sh), np.float64)
            assert A.shape[1] == M and Bs.shape[1] == N and A.shape[0] == Bs.shape[0]
            live = (A != 0).any(1) & (Bs != 0).any(1)       # (the other rows add exact zeros to all three products)
            Al, Bl = A[live], Bs[live]
            seen[key] = (Al.T @ Bl, np.abs(Al).T @ np.abs(Bl), (Al != 0).astype(np.float64).T @ (Bl != 0).astype(np.float64),
                         A.sum(0), np.abs(A).sum(0), (A != 0).sum(0).astype(np.float64))
        t = seen[key]
        want += t[0]; S += t[1]; n += t[2]; wc += t[3]; Sc += t[4]; nc += t[5]
    if out.acc:
        want += np.asarray(out.base, np.float64)
        S += np.abs(np.asarray(out.base, np.float64))
        wc += np.asarray(out.base_c, np.float64)
        Sc += np.abs(np.asarray(out.base_c, np.float64))
    return want, (n + 16) * U * S + TINY, wc, (nc + 16) * U * Sc + TINY


def stack_reference(slabs, base=None):
    """(want, bound) of a slab stack [splits][...] summed over its first axis (+ base): n counts the non-zero slabs per element."""
    s64 = np.asarray(slabs, np.float64)
    want, S, n = s64.sum(0), np.abs(s64).sum(0), (s64 != 0).sum(0).astype(np.float64)
    if base is not None:
        want = want + np.asarray(base, np.float64)
        S = S + np.abs(np.asarray(base, np.float64))
    return want, (n + 16) * U * S + TINY


def slab_hot(splits, shape, rs, k0=0):
    """A stack whose element e (row-major) is non-zero in slab (k0 + e) mod splits only."""
    count = int(np.prod(shape))
    flat = np.zeros((splits, count), np.float32)
    flat[(k0 + np.arange(count)) % splits, np.arange(count)] = _full(rs, count)
    return flat.reshape((splits,) + tuple(shape))


def slab_graded(splits, shape, rs):
    """A dense stack with one magnitude 2^(-20 .. 20) per element and another factor 2^(-6 .. 6) per slab."""
    e = (2.0 ** rs.randint(-20, 21, size=shape)).astype(np.float32)
    k = (2.0 ** rs.randint(-6, 7, size=(splits,) + (1,) * len(shape))).astype(np.float32)
    return _full(rs, splits, *shape) * e * k


# ---- the numpy model of the bf16-piece batch form ------------------------------------------------------------------------------
def model(out, drop=None, swap_rows=None, shift_error=0, skip_slab=None, colsum_shifted=False):
    """One Output as gemm_tn_split.hip forms it: every segment cut into the slabs of tns_plan, a slab = dense_product_ref.emulate
    on the transposed operands with 32-row steps, the slabs (and the column sums' slabs) added in float32 in stack order, the
    addend last.  The faults: ``drop`` a piece product; ``swap_rows`` = (r1, r2) of every B; the shift off by ``shift_error``;
    ``skip_slab`` = index in the output's stack left out of the sum; ``colsum_shifted``: column sums over the rows whose shifted
    row of B exists.  Returns (C, colsum) float32."""
    slabs, cslabs, seen = [], [], {}
    for seg in out.segs:
        key = (id(seg.A), id(seg.B), seg.sh)
        if key in seen:                                 # (segments that share their arrays: the same slabs again)
            slabs += seen[key][0]
            cslabs += seen[key][1]
            continue
        first = len(slabs)
        R = seg.A.shape[0]
        sh = seg.sh + shift_error
        Bs = shifted(seg.B, sh)
        rps, eff = tns_plan(R)
        live = np.ones(R, bool)
        if colsum_shifted:
            r = np.arange(R) + sh
            live = (r >= 0) & (r < R)
        for s in range(eff):
            lo, hi = s * rps, min(R, (s + 1) * rps)
            swap = None
            if swap_rows is not None and all(lo <= r < hi for r in swap_rows):
                swap = (swap_rows[0] - lo, swap_rows[1] - lo)
            elif swap_rows is not None and any(lo <= r < hi for r in swap_rows):
                raise ValueError("rows to exchange must lie in one slab")
            slabs.append(emulate(seg.A[lo:hi].T, Bs[lo:hi].T, drop=drop, swap_k=swap, step=32))
            col = np.zeros(out.M, np.float32)
            for r in range(lo, hi):
                if live[r]:
                    col = col + seg.A[r]
            cslabs.append(col)
        seen[key] = (slabs[first:], cslabs[first:])
    C, cs = np.zeros((out.M, out.N), np.float32), np.zeros(out.M, np.float32)
    for i, (p, c) in enumerate(zip(slabs, cslabs)):
        if i != skip_slab:
            C, cs = C + p, cs + c
    if out.acc:
        C, cs = out.base + C, out.base_c + cs
    assert C.dtype == np.float32 and cs.dtype == np.float32
    return C, cs


# ---- launch lists shared by the host and the GPU tests -------------------------------------------------------------------------
def S(M, N, segs, acc=0):
    return Spec(M, N, acc, [(R, sh) for R, sh in segs])


def all_shifts(R):
    rps, _ = tns_plan(R)
    return [0, 1, -1, 31, -31, 32, -32, 33, -33, rps, -rps, R - 1, 1 - R, R, -R, R + 1, -R - 1]


# bf16-piece batch form: tile 128 x 112 or 128 x 224 (N = 116, 224, 340), 32-row chunks, splits a multiple of 8 with at least two
# chunks each.  (launch name) -> (outputs, families)
PIECE_LAUNCHES = collections.OrderedDict([
    # every M and N class once, R on both sides of one and of two chunks, the short shifts
    ("edges", ([S(4, 4, [(1, 0)]), S(4, 112, [(31, -1)], 1), S(124, 4, [(32, 1)]), S(128, 116, [(33, -31)]),
                S(132, 224, [(63, 31)], 1), S(260, 228, [(64, -32)]), S(4, 340, [(65, 32)]), S(124, 112, [(97, -33)]),
                S(128, 224, [(65, 33)]), S(132, 4, [(1, 1)]), S(260, 116, [(1, -1)], 1)], FAMILIES)),
    # every shift class on one two-split segment (rows per split 64), one row and one column block more than a tile
    ("shifts", ([S(132, 116, [(97, sh)], i % 2) for i, sh in enumerate(all_shifts(97))], QUICK)),
    # 8 splits at 511 .. 1024 rows; 513 rows: 6 effective splits under 8 started workgroups per tile, a second segment behind
    ("splits", ([S(128, 224, [(511, 33)]), S(132, 116, [(512, 64)]), S(132, 112, [(512, -64)], 1),
                 S(260, 340, [(513, -512), (97, 0)]), S(124, 228, [(1023, 1022)]), S(128, 112, [(1024, -1024)], 1),
                 S(260, 112, [(1024, 1025)]), S(128, 116, [(513, 0), (513, 1)], 1)], QUICK)),
    # 16 splits of 192 rows
    ("long", ([S(260, 224, [(3072, 0)]), S(128, 340, [(3072, -1)], 1), S(132, 228, [(3072, 3071)])], QUICK)),
    # several segments per output, different lengths, wide and narrow outputs: the longest-first sort reorders them
    ("stacked", ([S(132, 116, [(97, 0), (1023, 1), (33, 0)], 1), S(128, 224, [(512, -32), (64, 0)]),
                  S(4, 4, [(65, 0), (33, 2), (1, 0)]), S(124, 112, [(511, 0), (31, -1)], 1)], FAMILIES)),
])
# 40 one-chunk segments on 40 outputs
FORTY = [S(4 * (1 + i % 5), 4 * (1 + i % 7), [(1 + (7 * i) % 32, (i % 3) - 1)], i % 2) for i in range(40)]

# exact-f32 tiled batch form: tiles 64 x 64 or 64 x 112 (N = 100, 112, 200), 32-row chunks
TILED_LAUNCHES = collections.OrderedDict([
    ("edges", ([S(4, 4, [(1, 0)]), S(60, 64, [(31, -1)], 1), S(64, 100, [(32, 1)]), S(68, 112, [(33, -31)]),
                S(4, 116, [(63, 31)], 1), S(60, 200, [(64, -32)]), S(64, 4, [(65, 32)]), S(68, 64, [(97, -33)]),
                S(60, 116, [(65, 33)], 1), S(68, 200, [(1, -1)])], FAMILIES)),
    ("shifts", ([S(68, 100, [(97, sh)], i % 2) for i, sh in enumerate(all_shifts(97))], QUICK)),
    ("splits", ([S(64, 112, [(511, 33)]), S(68, 116, [(512, -64)], 1), S(68, 200, [(513, -512), (97, 0)]),
                 S(60, 100, [(1023, 1022)]), S(64, 64, [(1024, 1025)], 1)], QUICK)),
    ("stacked", ([S(68, 116, [(97, 0), (1023, 1), (33, 0)], 1), S(64, 200, [(512, -32), (64, 0)]),
                  S(4, 4, [(65, 0), (33, 2), (1, 0)])], FAMILIES)),
])

# tall form: (name) -> (outputs, environment, live rows r0 of the rowhot cases).  Segments of one output share one operand pair.
# Kind 7: 8208 rows, target 768 -> 11 splits of 752 rows (the last: 688); with MMDFN_TN_TALL_ROWS7=2000: 5 splits of 1648 (1616).
# Kind 2: 32 x 16384 rows, target 2048 -> 8 splits of 2048; with MMDFN_TN_TALL_ROWS2=3000: 6 splits of 2736 (2704).  r0 values: the
# first 16-row chunk, a split boundary inside the live rows, a row range inside the last (shorter) split, and the last chunk (with
# the wrap to the first).
TALL_LAUNCHES = collections.OrderedDict([
    ("kind7", ([S(400, 100, [(8208, 0)] * 18)], {}, [0, 752 - 200, 8208 - 600, 8208 - 400, 8208 - 8])),
    ("kind7_rows2000", ([S(400, 100, [(8208, 0)] * 18, 1)], {"MMDFN_TN_TALL_ROWS7": "2000"}, [0, 1648 - 200, 8208 - 400])),
    ("kind2", ([S(100, 100, [(16384, 0)] * 32)], {}, [0, 2048 - 50, 16384 - 100, 16384 - 8])),
    ("kind2_rows3000", ([S(100, 100, [(16384, 0)] * 32, 1)], {"MMDFN_TN_TALL_ROWS2": "3000"}, [0, 2736 - 50, 16384 - 100])),
    ("kind7_336x80", ([S(336, 80, [(8208, 0)] * 18)], {}, [0, 752 - 100, 8208 - 336])),
])
TALL_DENSE = ("samesign", "graded")

# mmdfn_gemm_tn (one problem, explicit splits, no shift) and mmdfn_gemm_tn_grouped (<= 8 problems, shifts): 64 x 64 tiles
SINGLE_SHAPES = [(97, 68, 100), (513, 60, 64), (65, 4, 4), (1024, 64, 112), (33, 60, 116)]            # R, M, N
GROUPED = [S(68, 100, [(97, -33)]), S(4, 4, [(1, 0)]), S(64, 64, [(512, 64)]), S(60, 116, [(513, -513)]),
           S(68, 64, [(65, 64)]), S(64, 200, [(1023, 1)]), S(4, 112, [(31, 32)]), S(60, 4, [(97, -96)])]

# slab reduction alone: 8 lanes per element above 40 slabs, whose unrolled loop turns over at 64-slab strides
REDUCE_SPLITS = [1, 7, 8, 9, 40, 41, 48, 64, 65, 120, 121, 256]
REDUCE_SHAPES = [(4, 4), (12, 20), (100, 36)]
