"""GPU: the weight-gradient kernels (csrc/gemm_tn.hip, gemm_tn_split.hip, gemm_tn_split_body.h, the slab reduction, the foreign slab
stacks, the rider entry points) form by form against float64, slab by slab.

Reference, bound, input families and launch lists: tests/wgrad_product_ref.py (its instrument is proven on the CPU by
tests/test_wgrad_product_ref_host.py).  Every element of every result -- weights and column sums -- obeys
|got - want| <= (n + 16) u S + 2^-126.  The one-hot families (one live row per output element, swept so that every row of every
segment is the live one once) are what makes a missing piece product, a row of A paired with the wrong row of a shifted B or a
slab skipped, read twice or taken from a neighbour's stack visible; the dense families bring same-signed, cancelling, graded and
dropped-out operands.

Every launch is a direct C-ABI call:
  * A and B are column blocks of wider NaN-filled buffers (row stride M + 12 / N + 8) with one NaN guard row in front and one
    behind: nothing outside R x M / R x N may reach a result;
  * C and the column sums are blocks inside canary-filled buffers, 16-byte aligned ('vec') or at an odd offset with an odd row
    stride ('odd'); they hold NaN before a launch that does not accumulate and ``base`` before one that does; the canaries must be
    intact afterwards;
  * the workspace is exactly what the ..._workspace query returns, plus a canary tail, and NaN-filled before every launch: a
    reduction that reads a slab no workgroup wrote fails, a write past the query fails;
  * every launch runs twice and must give the same bits.

The tall form (one workgroup per whole-output slab, LDS-DMA operand rows) is a FALLBACK: production reaches it only for operands of
>= 2^30 elements or >= 2^24 rows -- never through a misaligned operand, which it refuses --, so it is driven here through
MMDFN_TN_SPLIT=0 of the tuning build, like most of the exact-f32 tiled form (which production also reaches with an operand 4
bytes off a 16-byte boundary: tested once that way).

The worst ratio of every form and family is recorded in profiles/r19_wgrad_products_parity.md."""
import numpy as np
import pytest
import torch

import wgrad_product_ref as W
from mm_dfn_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 1234.5
NAN = float("nan")
LAYOUTS = ("vec", "odd")
TAIL = 64                               # canary floats behind the workspace


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def guarded(Mx, pad, off=0):
    """Mx (numpy, R x C) as columns 4 .. 4 + C of a NaN-filled device buffer with row stride C + pad, one NaN row in front and one
    behind, the block's first element ``off`` floats past a 16-byte boundary.  Returns (view, row stride)."""
    R, C = Mx.shape
    ld = C + pad
    flat = torch.full(((R + 2) * ld + off,), NAN, device=DEV)
    view = flat[off:].view(R + 2, ld)[1:R + 1, 4:4 + C]
    view.copy_(dev(Mx))
    assert view.data_ptr() % 16 == 4 * off
    return view, ld


class Block:
    """A rows x cols block inside a canary-filled buffer with one canary row behind it (rows = 1: a column-sum vector);
    NaN-filled, or holding ``base`` for an accumulating launch."""

    def __init__(self, rows, cols, layout, base=None, extra_ld=0):
        self.c0, self.ld = (4, (cols + 3) // 4 * 4 + 8 + extra_ld) if layout == "vec" else (3, cols + 7 + extra_ld)
        self.rows, self.cols = rows, cols
        self.buf = torch.full((rows + 1, self.ld), CANARY, device=DEV)
        self.blk = self.buf[:rows, self.c0:self.c0 + cols]
        if base is None:
            self.blk.fill_(NAN)
        else:
            self.blk.copy_(dev(np.reshape(base, (rows, cols))))
        self.before = self.blk.clone()

    def result(self, tag):
        got = self.blk.clone()
        rest = self.buf.clone()
        rest[:self.rows, self.c0:self.c0 + self.cols] = CANARY
        assert bool((rest == CANARY).all()), "%s: wrote outside its block" % tag
        return got

    def untouched(self):
        return torch.equal(self.blk.view(torch.int32), self.before.view(torch.int32))


def workspace(floats):
    assert floats >= 0
    ws = torch.full((int(floats) + TAIL,), NAN, device=DEV)
    ws[int(floats):] = CANARY
    return ws


def tail_intact(ws):
    return bool((ws[-TAIL:] == CANARY).all())


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Batch:
    """One launch of mmdfn_gemm_tn_batch (or _ext / the rider entry points) staged on the device: the operands once (only read),
    the destinations and the workspace anew for every run.  Output i: layout LAYOUTS[(i + flip) % 2]; column sums to one
    destination (i % 3 == 0), to two (1) or not asked for (2).  The segments are given round-robin over the outputs, so that the
    slab order inside an output's stack is neither the argument order nor the launch's longest-first order."""

    def __init__(self, outs, flip=0, a_off=0):
        self.outs, self.flip = outs, flip
        staged = {}

        def operand(arr, pad, off=0):
            if id(arr) not in staged:
                staged[id(arr)] = guarded(arr, pad, off)
            return staged[id(arr)]

        self.segs = []                                  # (A view, lda, B view, ldb, R, shift, output)
        depth = max(len(o.segs) for o in outs)
        for j in range(depth):
            for i, o in enumerate(outs):
                if j < len(o.segs):
                    s = o.segs[j]
                    a, lda = operand(s.A, 12, a_off if (i == 0 and j == 0) else 0)
                    b, ldb = operand(s.B, 8)
                    self.segs.append((a, lda, b, ldb, s.A.shape[0], s.sh, i))
        ia = _hip.int_array
        self.shape_args = (len(self.segs), ia([s[4] for s in self.segs]), ia([s[6] for s in self.segs]), len(outs),
                           ia([o.M for o in outs]), ia([o.N for o in outs]))
        self.ws_floats = int(_hip.query("mmdfn_gemm_tn_batch_workspace", *self.shape_args))
        assert self.ws_floats > 0

    def stage_outputs(self):
        self.C, self.cs, self.cs2 = [], [], []
        for i, o in enumerate(self.outs):
            layout = LAYOUTS[(i + self.flip) % 2]
            self.C.append(Block(o.M, o.N, layout, o.base if o.acc else None))
            self.cs.append(Block(1, o.M, layout, o.base_c if o.acc else None) if i % 3 != 2 else None)
            self.cs2.append(Block(1, o.M, LAYOUTS[(i + self.flip + 1) % 2], o.base_c if o.acc else None) if i % 3 == 1 else None)
        self.ws = workspace(self.ws_floats)

    def args(self):
        pa, ia = _hip.ptr_array, _hip.int_array
        sg = self.segs
        blk = lambda col: [None if b is None else b.blk for b in col]
        return [len(sg), pa([s[0] for s in sg]), pa([s[2] for s in sg]), ia([s[4] for s in sg]), ia([s[1] for s in sg]),
                ia([s[3] for s in sg]), ia([s[5] for s in sg]), ia([s[6] for s in sg]), len(self.outs), pa(blk(self.C)),
                pa(blk(self.cs)), pa(blk(self.cs2)), ia([o.M for o in self.outs]), ia([o.N for o in self.outs]),
                ia([c.ld for c in self.C]), ia([o.acc for o in self.outs]), _hip.ptr(self.ws)]

    def launch(self, mode):
        lib = _hip.lib()
        if mode == "batch":
            return lib.mmdfn_gemm_tn_batch(*self.args(), None, _hip.stream())
        assert mode == "riders"                          # stage (nothing is launched), flush (the tiles), drain (the reduction)
        ctx = _hip.riders_context()
        rc = lib.mmdfn_wgrad_riders_stage(*self.args(), ctx, _hip.stream())
        assert rc == 0 and lib.mmdfn_wgrad_riders_staged(ctx) == 1, rc
        assert all(c.untouched() for c in self.C)
        assert lib.mmdfn_wgrad_riders_flush(ctx, _hip.stream()) == 0 and lib.mmdfn_wgrad_riders_staged(ctx) == 0
        return lib.mmdfn_wgrad_riders_drain(ctx, _hip.stream(), 0)

    def run(self, tag, mode="batch"):
        """Stage, launch, and return [(C, colsum or None)] per output after the canary checks."""
        self.stage_outputs()
        rc = self.launch(mode)
        assert rc == 0, (tag, rc)
        torch.cuda.synchronize()
        assert tail_intact(self.ws), "%s: wrote past the workspace query" % tag
        res = []
        for i in range(len(self.outs)):
            C = self.C[i].result("%s C%d" % (tag, i))
            cs = self.cs[i].result("%s colsum%d" % (tag, i)) if self.cs[i] is not None else None
            if self.cs2[i] is not None:
                assert bits_equal(cs, self.cs2[i].result("%s colsum2 %d" % (tag, i))), "%s: two bias destinations differ" % tag
            res.append((C, cs))
        return res


def check_outputs(tag, outs, first, second):
    for i, (o, (C, cs), (C2, cs2)) in enumerate(zip(outs, first, second)):
        t = "%s out%d[%dx%d]" % (tag, i, o.M, o.N)
        assert bits_equal(C, C2) and (cs is None or bits_equal(cs, cs2)), "%s: two identical launches differ" % t
        want, bound, wc, bc = W.reference(o)
        W.check(t, C.cpu().numpy(), want, bound)
        if cs is not None:
            W.check(t + " colsum", cs.cpu().numpy()[0], wc, bc)


def run_families(form, launch, specs, fams, mode="batch", a_off=0, share=False, r0s=None):
    """Every family of ``fams`` on one launch list: the one-hot families swept (or at the live rows ``r0s``), alternating the
    layouts from step to step; the dense families once in either layout assignment."""
    for name in fams:
        if name in W.ONEHOT and r0s is not None:
            variants = [dict(r0=r0) for r0 in r0s]
        elif name in W.ONEHOT:
            variants = [dict(k=k) for k in range(W.sweep_length(name, specs))]
        else:
            variants = [dict(), dict()]
        for v, kw in enumerate(variants):
            outs = W.build(specs, name, seed=1000 * len(specs) + 31 * v + len(name), share=share, **kw)
            b = Batch(outs, flip=v % 2, a_off=a_off)
            tag = "%s %s %s#%d" % (form, launch, name, v)
            check_outputs(tag, outs, b.run(tag, mode), b.run(tag, mode))


# ---- bf16-piece batch form (production default) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", list(W.PIECE_LAUNCHES))
def test_bf16_piece_batch_form(launch):
    """csrc/gemm_tn_split.hip through the production library: every operand here is 16-byte aligned, which is what selects it."""
    specs, fams = W.PIECE_LAUNCHES[launch]
    run_families("piece", launch, specs, fams)


def test_bf16_piece_batch_form_is_not_the_exact_f32_form(kernel_variants):
    """The production dispatch ran the piece kernels above: same bits as the tuning build's default, other bits than the exact-f32
    form forced by MMDFN_TN_SPLIT=0 (and both inside the bound)."""
    outs = W.build(W.PIECE_LAUNCHES["splits"][0], "samesign", seed=2)
    b = Batch(outs)
    _hip.set_tuning(False)
    prod = b.run("production")
    _hip.set_tuning(True)
    assert all(bits_equal(p[0], t[0]) for p, t in zip(prod, b.run("tuning")))
    kernel_variants.setenv("MMDFN_TN_SPLIT", "0")
    b = Batch(outs)                                      # (the workspace query of the other form)
    exact = b.run("exact")
    check_outputs("tiled splits samesign#dispatch", outs, exact, b.run("exact"))
    assert not all(bits_equal(p[0], e[0]) for p, e in zip(prod, exact))


def test_bf16_piece_batch_of_forty_segments():
    run_families("piece", "forty", W.FORTY, W.QUICK)


def test_batch_refuses_41_segments_and_an_output_nobody_feeds():
    """-1, and neither a destination nor the workspace is touched."""
    outs = W.build(W.FORTY, "samesign", seed=3)
    b = Batch(outs)
    b.stage_outputs()
    args = b.args()
    pa, ia = _hip.ptr_array, _hip.int_array
    sg = b.segs + b.segs[:1]
    args41 = [41, pa([s[0] for s in sg]), pa([s[2] for s in sg]), ia([s[4] for s in sg]), ia([s[1] for s in sg]),
              ia([s[3] for s in sg]), ia([s[5] for s in sg]), ia([s[6] for s in sg])] + args[8:]
    assert _hip.lib().mmdfn_gemm_tn_batch(*args41, None, _hip.stream()) == -1
    three = W.build([W.S(132, 116, [(97, 0)]), W.S(4, 4, [(1, 0)]), W.S(132, 116, [(33, 1)])], "samesign", seed=4)
    c = Batch(three)
    c.stage_outputs()
    cargs = c.args()
    cargs[7] = ia([0, 1, 0])                            # the third segment feeds output 0 as well: nobody feeds output 2
    assert _hip.lib().mmdfn_gemm_tn_batch(*cargs, None, _hip.stream()) == -1
    assert int(_hip.query("mmdfn_gemm_tn_batch_workspace", 1, ia([5]), ia([1]), 1, ia([4]), ia([4]))) == -1
    torch.cuda.synchronize()
    for q in (b, c):
        assert all(x.untouched() for col in (q.C, q.cs, q.cs2) for x in col if x is not None)
        assert bool(torch.isnan(q.ws[:-TAIL]).all()) and tail_intact(q.ws)


# ---- riders: stage -> flush -> drain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", ["stacked", "splits"])
def test_staged_batch_flushed_and_drained(launch):
    """mmdfn_wgrad_riders_stage plans the batch with the riders' rows target and launches nothing; mmdfn_wgrad_riders_flush runs
    its tiles, mmdfn_wgrad_riders_drain its slab reduction.  (tests/test_wgrad_riders_gpu.py pins the tiles that ride in a GRU
    launch to the batch bit for bit.)"""
    run_families("riders", launch, W.PIECE_LAUNCHES[launch][0], W.QUICK, mode="riders")


# ---- exact-f32 tiled batch form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", list(W.TILED_LAUNCHES))
def test_exact_f32_tiled_batch_form(launch, kernel_variants):
    kernel_variants.setenv("MMDFN_TN_SPLIT", "0")
    specs, fams = W.TILED_LAUNCHES[launch]
    run_families("tiled", launch, specs, fams)


def test_exact_f32_tiled_batch_form_through_a_misaligned_operand():
    """The production library with ONE operand of the batch 4 bytes off a 16-byte boundary: the whole batch leaves the piece form."""
    run_families("tiled_misaligned", "edges", W.TILED_LAUNCHES["edges"][0], W.QUICK, a_off=1)
    outs = W.build(W.TILED_LAUNCHES["edges"][0], "samesign", seed=6)
    off, aligned = Batch(outs, a_off=1).run("off"), Batch(outs).run("aligned")
    assert not all(bits_equal(a[0], b[0]) for a, b in zip(off, aligned))           # (another kernel ran)


# ---- tall form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("launch", list(W.TALL_LAUNCHES))
def test_tall_form(launch, kernel_variants):
    """gemm_tn_tall_kernel (a fallback, see the module docstring): the segments of the output share one operand pair and hold
    TALL_MIN_COST of work between them; rowhot at the live rows listed with the launch, samesign and graded.  That the tall
    kernel ran shows in the bits: MMDFN_TN_NO_TALL=1 gives others."""
    specs, env, r0s = W.TALL_LAUNCHES[launch]
    kernel_variants.setenv("MMDFN_TN_SPLIT", "0")
    for k, v in env.items():
        kernel_variants.setenv(k, v)
    run_families("tall", launch, specs, ("rowhot",), share=True, r0s=r0s)
    for v, name in enumerate(W.TALL_DENSE):
        outs = W.build(specs, name, seed=40 + v, share=True)
        b = Batch(outs, flip=v)
        tag = "tall %s %s#0" % (launch, name)
        tall = b.run(tag)
        check_outputs(tag, outs, tall, b.run(tag))
        if name == "samesign":
            kernel_variants.setenv("MMDFN_TN_NO_TALL", "1")
            tiled = Batch(outs, flip=v).run("no_tall")
            kernel_variants.delenv("MMDFN_TN_NO_TALL")
            assert not bits_equal(tall[0][0], tiled[0][0])


# ---- mmdfn_gemm_tn: one problem, explicit splits --------------------------------------------------------------------------------
def single_once(A, lda, B, ldb, R, M, N, splits, layout, want_colsum):
    C = Block(M, N, layout)
    cs = Block(1, M, layout) if want_colsum else None
    ws = workspace(splits * (M * N + M))
    rc = _hip.lib().mmdfn_gemm_tn(_hip.ptr(A), _hip.ptr(B), _hip.ptr(C.blk), _hip.ptr(cs.blk if cs else None), _hip.ptr(ws),
                                  R, M, N, lda, ldb, C.ld, splits, _hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert tail_intact(ws), "wrote past splits * (M N + M)"
    return C.result("gemm_tn C"), cs.result("gemm_tn colsum") if cs else None


@pytest.mark.parametrize("R,M,N", W.SINGLE_SHAPES)
def test_gemm_tn_with_explicit_splits(R, M, N):
    """splits = 1, 2, the library's own choice, and a count whose effective number of splits (after rounding the rows per split up
    to whole 32-row chunks) is smaller: the reduction must sum the effective ones only -- the rest of the workspace holds NaN."""
    own = int(_hip.query("mmdfn_gemm_tn_splits", R, M, N))
    effective = lambda s: -(-R // (-(-(-(-R // s)) // 32) * 32))
    more = next(s for s in range(own + 1, own + 64) if effective(s) < s)
    specs = [W.S(M, N, [(R, 0)])]
    for name in W.QUICK:
        for k in range(W.sweep_length(name, specs)):
            out = W.build(specs, name, seed=R + k, k=k)[0]
            (A, lda), (B, ldb) = guarded(out.segs[0].A, 12), guarded(out.segs[0].B, 8)
            want, bound, wc, bc = W.reference(out)
            for v, splits in enumerate(sorted({1, 2, own, more})):
                args = (A, lda, B, ldb, R, M, N, splits, LAYOUTS[(k + v) % 2], v % 2 == 0)
                (C, cs), (C2, cs2) = single_once(*args), single_once(*args)
                tag = "single [%d,%d,%d] splits=%d %s#%d" % (R, M, N, splits, name, k)
                assert bits_equal(C, C2) and (cs is None or bits_equal(cs, cs2)), tag
                W.check(tag, C.cpu().numpy(), want, bound)
                if cs is not None:
                    W.check(tag + " colsum", cs.cpu().numpy()[0], wc, bc)


# ---- mmdfn_gemm_tn_grouped ------------------------------------------------------------------------------------------------------
def grouped_once(outs, staged, flip, null_colsum):
    pa, ia = _hip.ptr_array, _hip.int_array
    n = len(outs)
    C = [Block(o.M, o.N, LAYOUTS[(i + flip) % 2]) for i, o in enumerate(outs)]
    cs = [None if i in null_colsum else Block(1, o.M, LAYOUTS[(i + flip) % 2]) for i, o in enumerate(outs)]
    R, M, N = ia([o.segs[0].A.shape[0] for o in outs]), ia([o.M for o in outs]), ia([o.N for o in outs])
    ws = workspace(int(_hip.query("mmdfn_gemm_tn_grouped_workspace", n, R, M, N)))
    rc = _hip.lib().mmdfn_gemm_tn_grouped(n, pa([s[0][0] for s in staged]), pa([s[1][0] for s in staged]), pa([c.blk for c in C]),
                                          pa([None if c is None else c.blk for c in cs]), R, M, N, ia([s[0][1] for s in staged]),
                                          ia([s[1][1] for s in staged]), ia([c.ld for c in C]), ia([o.segs[0].sh for o in outs]),
                                          _hip.ptr(ws), _hip.stream())
    if rc != 0:
        torch.cuda.synchronize()
        assert all(c.untouched() for c in C) and bool(torch.isnan(ws[:-TAIL]).all())
        return rc, None
    torch.cuda.synchronize()
    assert tail_intact(ws)
    return 0, [(c.result("grouped C"), None if s is None else s.result("grouped colsum")) for c, s in zip(C, cs)]


@pytest.mark.parametrize("count", [1, 8])
def test_gemm_tn_grouped(count):
    """1 and 8 problems in one launch pair, shifts up to and past the row count, a NULL column-sum entry next to a non-NULL one."""
    specs = W.GROUPED[:count]
    for name in W.QUICK:
        for k in range(W.sweep_length(name, specs)):
            outs = W.build(specs, name, seed=17 * count + k, k=k)
            staged = [(guarded(o.segs[0].A, 12), guarded(o.segs[0].B, 8)) for o in outs]
            null = {1, 4} if count == 8 else set()
            (rc, first), (_, second) = grouped_once(outs, staged, k, null), grouped_once(outs, staged, k, null)
            assert rc == 0
            check_outputs("grouped n=%d %s#%d" % (count, name, k), outs, first, second)


def test_gemm_tn_grouped_refuses_nine_problems():
    outs = W.build(W.GROUPED + W.GROUPED[:1], "samesign", seed=5)
    staged = [(guarded(o.segs[0].A, 12), guarded(o.segs[0].B, 8)) for o in outs]
    assert grouped_once(outs, staged, 0, set())[0] == -1


# ---- the slab reduction alone: mmdfn_gemm_tn_batch_ext with nseg = nout = 0 -----------------------------------------------------
def reduce_once(stacks, batch=None):
    """stacks: dicts(part (splits, M, N) or None, col (splits, M) or None, want_colsum, acc, layout, extra_ld, base, base_c); one
    reduction launch over all of them (behind the tiles of ``batch``, a staged Batch, when given).  Returns [(C, colsum)]."""
    pa, ia = _hip.ptr_array, _hip.int_array
    C, cs, part, col = [], [], [], []
    for s in stacks:
        M = s["M"]
        N = 0 if s["part"] is None else s["part"].shape[2]
        C.append(Block(M, N, s["layout"], s["base"] if s["acc"] else None, s["extra_ld"]) if N else None)
        cs.append(Block(1, M, s["layout"], s["base_c"] if s["acc"] else None) if s["want_colsum"] else None)
        part.append(None if s["part"] is None else dev(s["part"]))
        col.append(None if s["col"] is None else dev(s["col"]))
    blk = lambda c: [None if b is None else b.blk for b in c]
    ext = [len(stacks), pa(part), pa(col), pa(blk(C)), pa(blk(cs)), ia([s["M"] for s in stacks]),
           ia([0 if s["part"] is None else s["part"].shape[2] for s in stacks]), ia([0 if c is None else c.ld for c in C]),
           ia([s["splits"] for s in stacks]), ia([s["acc"] for s in stacks])]
    if batch is None:
        head = [0] + [None] * 7 + [0] + [None] * 8
    else:
        batch.stage_outputs()
        head = batch.args()
    rc = _hip.lib().mmdfn_gemm_tn_batch_ext(*head, *ext, None, _hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [(None if c is None else c.result("stack C"), None if s is None else s.result("stack colsum")) for c, s in zip(C, cs)]


def make_stacks(M, N, kind, seed, j=0):
    """One stack per slab count of REDUCE_SPLITS for an M x N output (N = 0: column sums only); options vary from stack to stack:
    accumulate (i % 2), a row stride past the layout's own (i % 3 == 0), column slabs present but no destination (i % 4 == 3)."""
    rs = np.random.RandomState(seed)
    stacks = []
    for i, splits in enumerate(W.REDUCE_SPLITS):
        shape, cshape = (M, N), (M,)
        if kind == "slabhot":
            part = W.slab_hot(splits, shape, rs, j * M * N) if N else None
            col = W.slab_hot(splits, cshape, rs, j * M)
        else:
            part = W.slab_graded(splits, shape, rs) if N else None
            col = W.slab_graded(splits, cshape, rs)
        stacks.append(dict(M=M, splits=splits, part=part, col=col, want_colsum=(N == 0 or i % 4 != 3), acc=i % 2,
                           layout=LAYOUTS[i % 2], extra_ld=5 if i % 3 == 0 else 0, base=W._full(rs, M, max(N, 1)),
                           base_c=W._full(rs, M)))
    return stacks


def check_stacks(tag, stacks, first, second):
    for s, (C, cs), (C2, cs2) in zip(stacks, first, second):
        t = "%s splits=%d" % (tag, s["splits"])
        if C is not None:
            assert bits_equal(C, C2), t
            W.check(t, C.cpu().numpy(), *W.stack_reference(s["part"], s["base"] if s["acc"] else None))
        if cs is not None:
            assert bits_equal(cs, cs2), t
            W.check(t + " colsum", cs.cpu().numpy()[0], *W.stack_reference(s["col"], s["base_c"] if s["acc"] else None))


@pytest.mark.parametrize("M,N", W.REDUCE_SHAPES + [(100, 0)])
def test_slab_reduction_alone(M, N):
    """Twelve foreign stacks of 1 .. 256 slabs in one reduction launch.  slab-hot: element e of the output is non-zero in slab
    (j M N + e) mod splits only, element m of the column sums in slab (j M + m) mod splits, j swept until every slab of the tallest
    stack has been the live one of both -- a slab skipped or read twice is a mismatch of the value itself; graded: dense, one
    magnitude per element and slab."""
    for j in range(-(-max(W.REDUCE_SPLITS) // M)):
        stacks = make_stacks(M, N, "slabhot", seed=M + N, j=j)
        check_stacks("reduce [%d,%d] slabhot#%d" % (M, N, j), stacks, reduce_once(stacks), reduce_once(stacks))
    stacks = make_stacks(M, N, "graded", seed=M + N + 1)
    check_stacks("reduce [%d,%d] graded" % (M, N), stacks, reduce_once(stacks), reduce_once(stacks))


def test_slab_reduction_behind_a_real_batch():
    """next > 0 in the call of a real batch: the batch's outputs and the foreign stacks leave one reduction launch."""
    outs = W.build(W.PIECE_LAUNCHES["stacked"][0], "samesign", seed=8)
    b = Batch(outs)
    stacks = make_stacks(12, 20, "graded", seed=9)[:8] + make_stacks(100, 0, "slabhot", seed=10, j=1)[8:]
    runs = []
    for _ in range(2):
        res = reduce_once(stacks, batch=b)
        assert tail_intact(b.ws)
        runs.append((res, [(b.C[i].result("C"), b.cs[i].result("cs") if b.cs[i] is not None else None) for i in range(len(outs))]))
    check_stacks("reduce_with_batch stacks", stacks, runs[0][0], runs[1][0])
    check_outputs("reduce_with_batch piece stacked samesign", outs, runs[0][1], runs[1][1])
    alone = b.run("alone")
    assert all(bits_equal(x[0], y[0]) for x, y in zip(alone, runs[0][1]))
