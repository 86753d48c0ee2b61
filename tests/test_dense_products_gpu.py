"""GPU: the dense projection kernels (csrc/linear.hip, linear_split.hip, linear_small.hip, linear_planes.hip) form by form against
float64, product by product.

Reference, bound and input families: tests/dense_product_ref.py (its instrument is proven on the CPU by
tests/test_dense_product_ref_host.py).  Every element of every result obeys |got - want| <= (n + 16) u S + 2^-126; the one-hot
families (n = 1, the non-zero swept over every k) are what makes a missing piece product or a misplaced k of a fragment layout
visible, the dense families bring same-signed, cancelling, graded and dropped-out operands.

Every launch is a direct C-ABI call on operands the operator layer would otherwise copy or re-dispatch:
  * X is a column block of a wider NaN-filled buffer (row stride K + 12): nothing past K may reach a result;
  * Y is a column block of a wider canary-filled buffer with one canary row behind it, once 16-byte aligned ('vec': the float4
    epilogues) and once 12 bytes off with an odd row stride ('odd': the scalar epilogues); it holds NaN before a launch that
    does not accumulate, so a kernel that reads it, or writes outside R x N, fails;
  * every launch runs twice and must give the same bits.

Where both are asked for, the activation comes AFTER the addend in linear.hip / linear_split.hip / linear_small.hip
(Y = act(X W^T + b + Y), what ops._Linear builds its backward mask on) and BEFORE it in linear_planes.hip
(Y = act(X B^T + b) * mask + Y); the bound is the same for both (ReLU is 1-Lipschitz).

The worst ratio of every form and family is recorded in profiles/r17_dense_products_parity.md."""
import functools

import numpy as np
import pytest
import torch

import dense_product_ref as D
from mm_dfn_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 1234.5
LAYOUTS = ("vec", "odd")
QUICK = ("onehot", "samesign")          # the families of the option / dispatch tests (onehot: its three cases)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def rows_in_nan(M, pad=12, off=0):
    """M (numpy, rows x cols) as a column block of a NaN-filled device buffer with row stride cols + pad, the first element
    ``off`` floats past the (256-byte aligned) allocation.  Returns (view, row stride)."""
    R, C = M.shape
    ld = C + pad
    flat = torch.full((R * ld + off,), float("nan"), device=DEV)
    view = flat[off:].view(R, ld)[:, :C]
    view.copy_(dev(M))
    return view, ld


class Out:
    """An R x N output block inside a canary-filled (R + 1) x ld buffer; NaN-filled, or holding ``base`` for an accumulating launch."""

    def __init__(self, R, N, layout, base=None):
        self.c0, self.ld = (4, (N + 3) // 4 * 4 + 8) if layout == "vec" else (3, N + 7)
        self.R, self.N = R, N
        self.buf = torch.full((R + 1, self.ld), CANARY, device=DEV)
        self.blk = self.buf[:R, self.c0:self.c0 + N]
        if base is None:
            self.blk.fill_(float("nan"))
        else:
            self.blk.copy_(base)

    def result(self, tag):
        got = self.blk.clone()
        rest = self.buf.clone()
        rest[:self.R, self.c0:self.c0 + self.N] = CANARY
        assert bool((rest == CANARY).all()), "%s: wrote outside R x N" % tag
        return got


class Prepared:
    """One input case on the device (staged once, only read) with its float64 references (computed once per option set)."""

    def __init__(self, case):
        self.case, self.name, self.n = case, case.name, case.n
        (self.R, self.K), self.N = case.X.shape, case.W.shape[0]
        self.base = D._full(np.random.RandomState(self.R + 3 * self.N), self.R, self.N)
        self._ref, self._dev = {}, {}

    def ref(self, bias=True, base=False, act=0, act_first=False):
        """(want, bound): act_first: act(X W^T + b) + base (the plane kernels), otherwise act(X W^T + b + base)."""
        key = (bias, base, act, act_first)
        if key not in self._ref:
            c = self.case
            if act and base and act_first:
                inner, _ = D.want_and_bound(c.X, c.W, c.bias if bias else None, None, c.n)
                _, bound = D.want_and_bound(c.X, c.W, c.bias if bias else None, self.base, c.n)
                want = np.maximum(inner, 0.0) + self.base.astype(np.float64)
            else:
                want, bound = D.want_and_bound(c.X, c.W, c.bias if bias else None, self.base if base else None, c.n)
                if act:
                    want = np.maximum(want, 0.0)
            self._ref[key] = (want, bound)
        return self._ref[key]

    def cached(self, key, make):
        if key not in self._dev:
            self._dev[key] = make()
        return self._dev[key]

    def x(self, off=0):
        return self.cached(("x", off), lambda: rows_in_nan(self.case.X, off=off))

    def w_blocks(self, N1):
        """The (N, K) weight as two contiguous row blocks split at N1 and the bias likewise (second block None for N1 == N)."""
        c = self.case
        return self.cached(("w", N1), lambda: (dev(c.W[:N1]), dev(c.W[N1:]) if N1 < self.N else None,
                                               dev(c.bias[:N1]), dev(c.bias[N1:]) if N1 < self.N else None))

    def w_kmajor(self):
        return self.cached("wk", lambda: dev(self.case.W.T))

    def base_dev(self):
        return self.cached("base", lambda: dev(self.base))


@functools.lru_cache(maxsize=None)
def prepared(R, K, N, only=None, expand=True):
    return [Prepared(c) for c in D.families(R, K, N, seed=10007 * R + 101 * K + N, expand=expand, only=only)]


def twice(tag, launch, want, bound):
    """Run ``launch() -> result`` twice: same bits, and the float64 check on the first."""
    got = launch()
    again = launch()
    assert torch.equal(got, again), "%s: two identical launches differ" % tag
    D.check(tag, got.cpu().numpy(), want, bound)
    return got


# ---- csrc/linear.hip and linear_split.hip: mmdfn_linear2 ---------------------------------------------------------------------
def linear2(prep, N1, layout, act=0, bias=True, base=False):
    x, ldx = prep.x()
    w1, w2, b1, b2 = prep.w_blocks(N1)
    out = Out(prep.R, prep.N, layout, prep.base_dev() if base else None)
    rc = _hip.lib().mmdfn_linear2(_hip.ptr(x), _hip.ptr(w1), _hip.ptr(w2), N1, _hip.ptr(b1 if bias else None),
                                  _hip.ptr(b2 if bias else None), _hip.ptr(out.blk), prep.R, prep.K, prep.N, ldx, out.ld, act,
                                  1 if base else 0, _hip.stream())
    assert rc == 0, rc
    return out.result("linear2")


def linear2_families(form, R, K, N, N1, only=None):
    for prep in prepared(R, K, N, only):
        for layout in LAYOUTS:
            tag = "%s[%d,%d,%d,%d,%s] %s" % (form, R, K, N, N1, layout, prep.name)
            twice(tag, lambda: linear2(prep, N1, layout), *prep.ref())


def linear2_options(form, R, K, N, N1):
    """act 0 / 1, bias / no bias, accumulate, and the activation behind the addend: each once, on the quick families."""
    for prep in prepared(R, K, N, QUICK):
        for opts in (dict(act=1), dict(bias=False), dict(base=True), dict(act=1, base=True), dict(act=1, bias=False)):
            layout = "odd" if opts.get("base") else "vec"
            tag = "%s[%d,%d,%d,%d,%s] %s %s" % (form, R, K, N, N1, layout, "+".join(sorted(opts)), prep.name)
            twice(tag, lambda: linear2(prep, N1, layout, **opts), *prep.ref(**opts))


# R and N on both sides of the 64 x 64 workgroup tile and of a 16-wide MFMA tile, an N1 split inside a tile, 1 / 2 / 3 / 7 / 13
# 16-wide k-chunks (odd and even counts: the two register sets of the pipeline) with a 4-wide remainder, R < 16, two bias blocks
LINEAR_SHAPES = [(1, 4, 1, 1), (17, 20, 15, 7), (64, 16, 64, 64), (65, 36, 65, 33), (63, 100, 130, 100), (130, 200, 67, 67)]


@pytest.mark.parametrize("R,K,N,N1", LINEAR_SHAPES)
def test_exact_f32_form_every_family(R, K, N, N1):
    """csrc/linear.hip, the production 64 x 64 workgroup tile <2, 2, 2, 2> (every shape here has fewer than 256 tiles of 128 x 128)."""
    linear2_families("linear", R, K, N, N1)


def test_exact_f32_form_options():
    linear2_options("linear", 65, 36, 65, 33)


SPLIT_SHAPES = [(1, 8, 1, 1), (128, 32, 128, 128), (129, 36, 130, 65), (300, 200, 67, 67), (257, 44, 256, 256)]


@pytest.mark.parametrize("R,K,N,N1", SPLIT_SHAPES)
def test_bf16_piece_form_every_family(R, K, N, N1, kernel_variants):
    """csrc/linear_split.hip forced by MMDFN_LIN_CFG=7: 128 x 128 blocks, 32-wide k chunks, the float4 and the scalar epilogue."""
    kernel_variants.setenv("MMDFN_LIN_CFG", "7")
    linear2_families("linear_split", R, K, N, N1)


def test_bf16_piece_form_options(kernel_variants):
    kernel_variants.setenv("MMDFN_LIN_CFG", "7")
    linear2_options("linear_split", 129, 36, 130, 65)


def test_bf16_piece_form_refuses_a_four_wide_contraction_and_falls_back(kernel_variants):
    """K = 4 < 8: the piece launcher answers -2 and mmdfn_linear2 runs the exact-f32 kernel; same bits as the production dispatch."""
    kernel_variants.setenv("MMDFN_LIN_CFG", "7")
    linear2_families("linear_split_fallback", 9, 4, 5, 5)
    prep = prepared(9, 4, 5)[3]
    forced = linear2(prep, 5, "vec")
    kernel_variants.setenv("MMDFN_LIN_CFG", "5")
    assert torch.equal(forced, linear2(prep, 5, "vec"))


def test_bf16_piece_form_is_the_dispatch_from_256_tiles_on(kernel_variants):
    """(32768, 32, 100): 256 tiles of 128 x 128, the threshold in mmdfn_linear2 -- the production library, no switch; its bits are
    those of the forced piece form and not those of the forced exact-f32 form."""
    R, K, N = 32768, 32, 100
    _hip.set_tuning(False)
    got = {}
    for prep in prepared(R, K, N, QUICK, False):
        tag = "linear_split_dispatch[%d,%d,%d,vec] %s" % (R, K, N, prep.name)
        got[prep.name] = twice(tag, lambda: linear2(prep, N, "vec"), *prep.ref())
    _hip.set_tuning(True)
    prep = prepared(R, K, N, QUICK, False)[3]
    assert prep.name == "samesign"
    kernel_variants.setenv("MMDFN_LIN_CFG", "7")
    assert torch.equal(got["samesign"], linear2(prep, N, "vec"))
    kernel_variants.setenv("MMDFN_LIN_CFG", "8")
    assert not torch.equal(got["samesign"], linear2(prep, N, "vec"))


# ---- csrc/linear_small.hip: mmdfn_linear_group_seg2 --------------------------------------------------------------------------
class Small:
    """One problem of a few-row group launch, staged.  kmajor: the weight is passed (K, N), n-contiguous; x_off: X starts that
    many floats off a 16-byte boundary; addend: None | 'acc' (accumulate onto Y) | 'aligned' | 'strided' | 'off4' (an out-of-place
    Z); K2: the last K2 columns of the case are a second segment (X2, Wk2)."""

    def __init__(self, prep, N1=None, kmajor=False, layout="vec", x_off=0, bias=True, addend=None, K2=0, ldw_pad=0):
        self.prep, self.layout, self.kmajor, self.addend, self.K2 = prep, layout, kmajor, addend, K2
        self.R, self.N, self.K = prep.R, prep.N, prep.K - K2
        self.N1 = self.N if (N1 is None or kmajor) else N1
        self.bias = bias and not kmajor
        c = prep.case
        if K2:
            self.x, self.ldx = prep.cached(("x1", K2), lambda: rows_in_nan(c.X[:, :self.K]))
            self.x2, self.ldx2 = prep.cached(("x2", K2), lambda: rows_in_nan(c.X[:, self.K:]))
            self.w = prep.cached(("wk1", K2), lambda: dev(c.W[:, :self.K].T))
            self.wk2 = prep.cached(("wk2", K2), lambda: dev(c.W[:, self.K:].T))
            self.w2 = self.b1 = self.b2 = None
            self.ldw = self.ldw2 = self.N
        else:
            self.x, self.ldx = prep.x(x_off)
            self.x2 = self.wk2 = None
            self.ldx2 = self.ldw2 = 0
            if kmajor:
                self.w, self.w2, self.b1, self.b2, self.ldw = prep.w_kmajor(), None, None, None, self.N
            elif ldw_pad:
                self.ldw = self.K + ldw_pad
                self.w = prep.cached(("wpad", ldw_pad, self.N1), lambda: rows_in_nan(c.W[:self.N1], pad=ldw_pad)[0])
                self.w2 = prep.cached(("w2pad", ldw_pad, self.N1), lambda: rows_in_nan(c.W[self.N1:], pad=ldw_pad)[0]) \
                    if self.N1 < self.N else None
                _, _, self.b1, self.b2 = prep.w_blocks(self.N1)
            else:
                self.w, self.w2, self.b1, self.b2 = prep.w_blocks(self.N1)
                self.ldw = self.K
        if not self.bias:
            self.b1 = self.b2 = None
        self.z, self.ldz = None, 0
        if addend == "aligned":
            self.z, self.ldz = prep.base_dev(), self.N
        elif addend == "strided":
            self.z, self.ldz = prep.cached("zs", lambda: rows_in_nan(prep.base, pad=8 + (-self.N) % 4, off=4))
        elif addend == "off4":
            self.z, self.ldz = prep.cached("zo", lambda: rows_in_nan(prep.base, pad=3, off=1))
        self.out = None

    def stage(self):
        self.out = Out(self.R, self.N, self.layout, self.prep.base_dev() if self.addend == "acc" else None)

    def ref(self, act=0):
        return self.prep.ref(bias=self.bias, base=self.addend is not None, act=act)


def small_launch(probs, act=0, entry="mmdfn_linear_group_seg2"):
    """Stage the outputs and launch the group once; returns the entry point's code."""
    for q in probs:
        q.stage()
    pa, ia = _hip.ptr_array, _hip.int_array
    col = lambda name: [getattr(q, name) for q in probs]
    head = [len(probs), pa(col("x")), pa(col("w")), pa(col("w2")), ia(col("N1")), pa(col("b1")), pa(col("b2")),
            pa([q.out.blk for q in probs])]
    tail = [ia(col("R")), ia(col("K")), ia(col("N")), ia(col("ldx")), ia(col("ldw")), ia([q.out.ld for q in probs]),
            ia([1 if q.kmajor else 0 for q in probs]), ia([1 if q.addend == "acc" else 0 for q in probs])]
    lib = _hip.lib()
    zs = [pa(col("z")), ia(col("ldz"))]
    if entry == "mmdfn_linear_group_addend":
        assert all(q.x2 is None for q in probs)
        return lib.mmdfn_linear_group_addend(*head, *zs, *tail, act, _hip.stream())
    return lib.mmdfn_linear_group_seg2(*head, *zs, *tail, pa(col("x2")), pa(col("wk2")), ia(col("K2")), ia(col("ldx2")),
                                       ia(col("ldw2")), act, _hip.stream())


def small_twice(tags, probs, act=0, entry="mmdfn_linear_group_seg2"):
    """The group launched twice: code 0, the same bits, every problem inside its bound.  Returns the results."""
    runs = []
    for _ in range(2):
        rc = small_launch(probs, act, entry)
        assert rc == 0, (tags, rc)
        runs.append([q.out.result(t) for q, t in zip(probs, tags)])
    for q, tag, a, b in zip(probs, tags, *runs):
        assert torch.equal(a, b), "%s: two identical launches differ" % tag
        D.check(tag, a.cpu().numpy(), *q.ref(act))
    return runs[0]


# a covering set of R in {1, 31, 33, 65} x K in {4, 60, 64, 68, 132, 768} x N: both sides of the 32- / 64-row tiles, of the 64-wide
# staged chunk (and of the four-wave k split of the register form), of the 64-column tile
SMALL_NK = [(1, 4, 1, 1), (31, 60, 63, 1), (33, 64, 64, 64), (65, 68, 65, 37), (1, 132, 130, 37), (31, 768, 1, 1), (33, 4, 130, 130),
            (65, 60, 64, 37), (1, 64, 65, 1), (31, 68, 130, 1), (33, 132, 63, 37), (65, 768, 65, 65), (31, 132, 64, 1)]   # R, K, N, N1
SMALL_KN = [(1, 4, 4), (31, 60, 64), (33, 64, 68), (65, 68, 132), (1, 132, 64), (31, 768, 4), (33, 4, 132), (65, 60, 68)]   # R, K, N
SMALL_FORMS = {"lds_default": {}, "lds_nst2": {"MMDFN_LSM_NST": "2"}, "lds_tm64": {"MMDFN_LSM_TM": "64"},
               "register_ring": {"MMDFN_LSM_V1": "1"}, "register_ring_unaligned_x": None}


def small_form(form, request):
    """Select the library and the switches of a few-row form; returns the X offset (floats) its problems use."""
    env = SMALL_FORMS[form]
    if env:
        mp = request.getfixturevalue("kernel_variants")
        for k, v in env.items():
            mp.setenv(k, v)
    return 1 if env is None else 0      # (production library, X 4 bytes off a 16-byte boundary: the register ring without a switch)


@pytest.mark.parametrize("R,K,N,N1", SMALL_NK)
@pytest.mark.parametrize("form", list(SMALL_FORMS))
def test_few_row_forms_n_major_every_family(form, R, K, N, N1, request):
    x_off = small_form(form, request)
    for prep in prepared(R, K, N):
        for layout in LAYOUTS:
            tag = "small_%s[%d,%d,%d,%d,%s] %s" % (form, R, K, N, N1, layout, prep.name)
            small_twice([tag], [Small(prep, N1=N1, layout=layout, x_off=x_off)])


@pytest.mark.parametrize("R,K,N", SMALL_KN)
@pytest.mark.parametrize("form", list(SMALL_FORMS))
def test_few_row_forms_k_major_every_family(form, R, K, N, request):
    x_off = small_form(form, request)
    for prep in prepared(R, K, N):
        for layout in LAYOUTS:
            tag = "small_%s_kmajor[%d,%d,%d,%s] %s" % (form, R, K, N, layout, prep.name)
            small_twice([tag], [Small(prep, kmajor=True, layout=layout, x_off=x_off)])


@pytest.mark.parametrize("form", list(SMALL_FORMS))
def test_few_row_forms_options(form, request):
    x_off = small_form(form, request)
    for prep in prepared(33, 68, 65, QUICK):
        for act, kw in ((1, {}), (0, dict(bias=False)), (0, dict(addend="acc")), (1, dict(addend="acc")), (0, dict(addend="off4"))):
            tag = "small_%s[33,68,65,37,odd] act%d+%s %s" % (form, act, "+".join("%s=%s" % i for i in sorted(kw.items())), prep.name)
            small_twice([tag], [Small(prep, N1=37, layout="odd", x_off=x_off, **kw)], act=act)


@pytest.mark.parametrize("form", ["lds_default", "lds_nst2", "lds_tm64"])
def test_few_row_lds_forms_past_768(form, request):
    small_form(form, request)
    for prep in prepared(33, 772, 65):
        small_twice(["small_%s[33,772,65,37,vec] %s" % (form, prep.name)], [Small(prep, N1=37)])
    for prep in prepared(31, 772, 68, QUICK):
        small_twice(["small_%s_kmajor[31,772,68,odd] %s" % (form, prep.name)], [Small(prep, kmajor=True, layout="odd")])


@pytest.mark.parametrize("form", ["register_ring", "register_ring_unaligned_x"])
def test_few_row_register_form_refuses_past_768(form, request):
    x_off = small_form(form, request)
    prep = prepared(33, 772, 65)[3]
    q = Small(prep, N1=37, x_off=x_off)
    assert small_launch([q]) == -1
    assert bool(torch.isnan(q.out.result("refused")).all())           # nothing was launched


def test_few_row_k_major_odd_width_takes_the_register_form():
    """A K-major weight with N % 4 != 0 cannot be staged by 16-byte DMA: production library, register ring, and right; that it IS
    the register form shows in the refusal of K = 772, which the LDS forms take."""
    for prep in prepared(33, 68, 5):
        for layout in LAYOUTS:
            small_twice(["small_register_ring_kmajor_n5[33,68,5,%s] %s" % (layout, prep.name)],
                        [Small(prep, kmajor=True, layout=layout)])
    assert small_launch([Small(prepared(33, 772, 5, QUICK)[3], kmajor=True)]) == -1
    assert small_launch([Small(prepared(31, 772, 68, QUICK)[3], kmajor=True)]) == 0


def test_few_row_64_row_tiles_by_dispatch(kernel_variants):
    """(6400, 400, 256): 400 tiles of 64 x 64 and K >= 400 -- the production library picks the 64-row tile; its bits are those of
    the forced 64-row form and not those of the 32-row form (which splits every chunk's k between two waves)."""
    R, K, N = 6400, 400, 256
    _hip.set_tuning(False)
    got = {}
    for prep in prepared(R, K, N, QUICK, False):
        got[prep.name] = small_twice(["small_lds_tm64_dispatch[%d,%d,%d,vec] %s" % (R, K, N, prep.name)], [Small(prep)])[0]
    _hip.set_tuning(True)
    q = Small(prepared(R, K, N, QUICK, False)[3])
    for tm, same in (("64", True), ("32", False)):
        kernel_variants.setenv("MMDFN_LSM_TM", tm)
        assert small_launch([q]) == 0
        assert torch.equal(got["samesign"], q.out.result("tm" + tm)) == same, tm


def test_few_row_group_of_eight():
    """One launch of eight problems: N-major with one and with two blocks (one with padded weight rows), K-major, the three kinds of
    out-of-place addend, accumulate; every problem has the bits of its own launch."""
    P = prepared
    for fam in range(7):
        probs = [Small(P(65, 68, 65)[fam], N1=37, layout="odd"),
                 Small(P(33, 64, 64)[fam], layout="vec", addend="aligned"),
                 Small(P(65, 68, 132)[fam], kmajor=True, layout="vec", addend="strided"),
                 Small(P(31, 60, 63)[fam], N1=1, layout="odd", addend="off4"),
                 Small(P(33, 132, 63)[fam], N1=37, layout="vec", addend="acc", ldw_pad=4),
                 Small(P(1, 132, 64)[fam], kmajor=True, layout="odd", addend="acc"),
                 Small(P(31, 768, 4)[fam], kmajor=True, layout="vec"),
                 Small(P(1, 4, 1)[fam], layout="odd", bias=False)]
        name = probs[0].prep.name
        tags = ["small_group8[%d:%d,%d,%d] %s" % (i, q.R, q.K, q.N, name) for i, q in enumerate(probs)]
        together = small_twice(tags, probs)
        for q, tag, got in zip(probs, tags, together):
            assert small_launch([q]) == 0
            assert torch.equal(got, q.out.result(tag)), tag


@pytest.mark.parametrize("K,K2", [(64, 4), (68, 132), (4, 64)])
def test_few_row_second_segment(K, K2):
    """Y = X . W + X2 . Wk2 (+ Z): the families are drawn at width K + K2 and cut at K, so the one-hot sweep walks through both
    segments and n = K + K2 on the dense ones.  The problem next to it, without a second segment, is mmdfn_linear_group_addend's
    bit for bit."""
    R, N = 33, 68
    plain = prepared(65, 68, 132)
    for i, prep in enumerate(prepared(R, K + K2, N)):
        for layout, addend in (("vec", None), ("odd", "strided")):
            two = Small(prep, kmajor=True, layout=layout, addend=addend, K2=K2)
            one = Small(plain[i], kmajor=True, layout=layout, addend=addend)
            tags = ["small_seg2[%d,%d+%d,%d,%s] %s" % (R, K, K2, N, layout, prep.name),
                    "small_seg2_neighbour[65,68,132,%s] %s" % (layout, prep.name)]
            got = small_twice(tags, [two, one])
            assert small_launch([one], entry="mmdfn_linear_group_addend") == 0
            assert torch.equal(got[1], one.out.result("addend"))


def test_few_row_second_segment_is_refused_by_the_register_form():
    prep = prepared(33, 68, 68, QUICK)[3]
    q = Small(prep, kmajor=True, K2=4)
    q.x, q.ldx = rows_in_nan(prep.case.X[:, :64], off=1)               # X 4 bytes off: no LDS staging, two launches for the caller
    assert small_launch([q]) == -2
    assert bool(torch.isnan(q.out.result("refused")).all())


# ---- csrc/linear_planes.hip ---------------------------------------------------------------------------------------------------
def planes_buffer(N, K):
    nbytes = int(_hip.query("mmdfn_weight_planes_workspace", N, K))
    assert nbytes > 0 and nbytes % 16 == 0
    return torch.full((nbytes // 4,), float("nan"), device=DEV)        # (the cut must write all of it, zeros outside N x K)


def stored_forms(B, mode, n1, ld_pad):
    """The stored matrices (w1, w2, ld) from which mmdfn_cut_weight_planes reads B[n][k] in ``mode`` (include/mmdfn_hip.h):
      0  B[n][k] = stored[n][k], stored rows split at n1        1  B[n][k] = stored[k][n], stored rows (= k) split at n1
      2  B[n][k] = w1[k][n] (n < n1), w2[k][n - n1] beyond      3  as 2 with k = 4 u + g  <->  stored row g (K / 4) + u
    Both blocks share the row stride; NaN fills what lies past a stored row."""
    N, K = B.shape
    if mode in (0, 1):
        stored = B if mode == 0 else B.T
        blocks = (stored[:n1], stored[n1:])
    else:
        S = B.T                                                         # [k][n]
        if mode == 3:
            H = K // 4
            S = np.concatenate([S[g::4] for g in range(4)])             # row g H + u  <-  k = 4 u + g
            assert all((S[g * H + u] == B[:, 4 * u + g]).all() for g in range(4) for u in range(H))
        blocks = (S[:, :n1], S[:, n1:])
    ld = max(b.shape[1] for b in blocks) + ld_pad
    out = [rows_in_nan(b, pad=ld - b.shape[1])[0] if b.size else None for b in blocks]
    return out[0], out[1], ld


def cut_planes(specs):
    """specs: list of (B numpy (N, K), mode, n1, ld_pad); ONE grouped cut launch; returns the plane buffers."""
    keep, w1s, w2s, n1s, lds, Ns, Ks, modes, planes = [], [], [], [], [], [], [], [], []
    for B, mode, n1, ld_pad in specs:
        w1, w2, ld = stored_forms(B, mode, n1, ld_pad)
        keep.append((w1, w2))
        w1s.append(w1); w2s.append(w2); n1s.append(n1); lds.append(ld); Ns.append(B.shape[0]); Ks.append(B.shape[1])
        modes.append(mode)
        planes.append(planes_buffer(*B.shape))
    pa, ia = _hip.ptr_array, _hip.int_array
    rc = _hip.lib().mmdfn_cut_weight_planes(len(specs), pa(w1s), pa(w2s), ia(n1s), ia(lds), ia(Ns), ia(Ks), ia(modes), pa(planes),
                                            _hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return planes


def planes_of(prep, mode=0, n1=None, ld_pad=0):
    n1 = prep.N if n1 is None else n1
    return prep.cached(("planes", mode, n1, ld_pad), lambda: cut_planes([(prep.case.W, mode, n1, ld_pad)])[0])


def linear_planes(prep, planes, layout, nb1=None, act=0, bias=True, base=False):
    x, ldx = prep.x()
    nb1 = prep.N if nb1 is None else nb1
    _, _, b1, b2 = prep.w_blocks(nb1)
    out = Out(prep.R, prep.N, layout, prep.base_dev() if base else None)
    rc = _hip.lib().mmdfn_linear_planes(_hip.ptr(x), _hip.ptr(planes), _hip.ptr(b1 if bias else None),
                                        _hip.ptr(b2 if bias else None), nb1, _hip.ptr(out.blk), prep.R, prep.K, prep.N, ldx,
                                        out.ld, act, 1 if base else 0, _hip.stream())
    assert rc == 0, rc
    return out.result("linear_planes")


PLANES_SHAPES = [(1, 4, 1), (63, 12, 31), (64, 16, 32), (65, 20, 33), (130, 36, 65), (200, 200, 130)]


@pytest.mark.parametrize("R,K,N", PLANES_SHAPES)
def test_planes_narrow_form_every_family(R, K, N):
    """64 x 64 workgroups (fewer than 400 workgroups of the wide form), the weight cut in mode 0, biases split inside a tile."""
    nb1 = max(1, N // 3)
    for prep in prepared(R, K, N):
        for layout in LAYOUTS:
            tag = "planes_narrow[%d,%d,%d,%s] %s" % (R, K, N, layout, prep.name)
            twice(tag, lambda: linear_planes(prep, planes_of(prep), layout, nb1), *prep.ref())


def test_planes_wide_form_by_dispatch():
    """(5120, 36, 600): 80 row blocks x 5 blocks of four column tiles = 400 workgroups, from where pl_form picks the 64 x 128 form."""
    for prep in prepared(5120, 36, 600, QUICK, False):
        tag = "planes_wide[5120,36,600,vec] %s" % prep.name
        twice(tag, lambda: linear_planes(prep, planes_of(prep, n1=300), "vec", 300), *prep.ref())


def test_planes_options():
    for prep in prepared(130, 36, 65, QUICK):
        for opts in (dict(act=1), dict(bias=False), dict(base=True), dict(act=1, base=True)):
            tag = "planes_narrow[130,36,65,odd] %s %s" % ("+".join(sorted(opts)), prep.name)
            twice(tag, lambda: linear_planes(prep, planes_of(prep), "odd", 33, **opts), *prep.ref(act_first=True, **opts))


CUT_SHAPES = PLANES_SHAPES + [(33, 100, 40)]          # (mode 3: K = 4 H with H = 1, 9, 25 among them)


@pytest.mark.parametrize("R,K,N", CUT_SHAPES)
def test_cut_weight_planes_every_mode(R, K, N):
    """mmdfn_cut_weight_planes modes 0 - 3 against the header's definition of B[n][k], all variants of a shape in ONE grouped cut
    launch: mode 0 from 16-byte rows (two float4 loads per lane) and with ld = K + 1 (the scalar path, which also serves the last
    partial group of eight k), two blocks split at n1 in {1, 33, full}.  The one-hot sweep through mmdfn_linear_planes is the
    check: row r of Y is x . B[:, r % K], so one misplaced element of any plane fails; and every variant must give the bits of
    the plain mode-0 cut, the planes being a function of B alone."""
    preps = prepared(R, K, N, ("onehot",))
    for prep in preps:
        B = prep.case.W
        specs, names = [], []
        for mode, ld_pad, label in ((0, 0, "m0"), (0, 1, "m0_scalar"), (1, 0, "m1"), (2, 3, "m2"), (3, 0, "m3")):
            if mode == 3 and K % 4:
                continue
            extent = K if mode == 1 else N
            for n1 in sorted({min(1, extent), min(33, extent), extent}):
                if mode in (2, 3) and ld_pad == 0:
                    pad = (-max(n1, N - n1)) % 4                       # (ld % 4 == 0 wants 16-byte aligned blocks: they are)
                else:
                    pad = ld_pad
                specs.append((B, mode, n1, pad))
                names.append("%s_n1=%d" % (label, n1))
        assert len(specs) <= 16
        planes = cut_planes(specs)
        for name, pl in zip(names, planes):
            assert bool(torch.isfinite(pl).all()), name
            assert torch.equal(pl.view(torch.int32), planes[0].view(torch.int32)), name
            tag = "planes_cut_%s[%d,%d,%d,vec] %s" % (name.split("_n1")[0], R, K, N, prep.name)
            twice(tag, lambda: linear_planes(prep, pl, "vec", bias=False), *prep.ref(bias=False))


def planes_group(probs, act=0, mask_scale=1.0, xscale=1.0, entry="in"):
    """probs: dicts(prep, planes, nb1, layout, mask, xmask, want_xdrop, x); returns (outs, xdrops); an R = 0 problem has prep None."""
    pa, ia = _hip.ptr_array, _hip.int_array
    X, PL, B1, B2, NB1, Y, R, K, N, LDX, LDY, MASK, XMASK, XDROP, outs = ([] for _ in range(15))
    for q in probs:
        prep = q["prep"]
        x, ldx = q.get("x") or prep.x()
        _, _, b1, b2 = prep.w_blocks(q["nb1"])
        out = Out(prep.R, prep.N, q["layout"])
        empty = q.get("empty", False)
        xd = torch.full((prep.R, prep.K), float("nan"), device=DEV) if q.get("xmask") is not None else None
        X.append(x); PL.append(q["planes"]); B1.append(b1); B2.append(b2); NB1.append(q["nb1"]); Y.append(out.blk)
        R.append(0 if empty else prep.R); K.append(prep.K); N.append(prep.N); LDX.append(ldx); LDY.append(out.ld)
        MASK.append(q.get("mask")); XMASK.append(q.get("xmask")); XDROP.append(xd); outs.append(out)
    args = [len(probs), pa(X), pa(PL), pa(B1), pa(B2), ia(NB1), pa(Y), ia(R), ia(K), ia(N), ia(LDX), ia(LDY), act, 0,
            pa(MASK), mask_scale]
    lib = _hip.lib()
    if entry == "group":
        assert all(m is None for m in XMASK)
        rc = lib.mmdfn_linear_planes_group(*args, _hip.stream())
    else:
        rc = lib.mmdfn_linear_planes_group_in(*args, pa(XMASK), pa(XDROP), xscale, _hip.stream())
    assert rc == 0, rc
    return [o.result("planes_group") for o in outs], XDROP


def test_planes_group_with_an_empty_problem_and_the_mask_epilogue():
    """mmdfn_linear_planes_group: four problems of which one has R = 0 (its Y stays untouched), each with the bits of its own
    launch; then Y = act(X B^T + b) * mask * mask_scale with the bound scaled by mask_scale."""
    shapes = [(130, 36, 65), (63, 12, 31), (65, 20, 33), (200, 200, 130)]
    for fam in range(7):
        probs = [dict(prep=prepared(*s)[fam], nb1=max(1, s[2] // 3), layout=LAYOUTS[i % 2], empty=(i == 1)) for i, s in enumerate(shapes)]
        for q in probs:
            q["planes"] = planes_of(q["prep"])
        runs = [planes_group(probs, entry="group")[0] for _ in range(2)]
        for i, (q, a, b) in enumerate(zip(probs, *runs)):
            prep = q["prep"]
            if q["empty"]:
                assert bool(torch.isnan(a).all())
                continue
            assert torch.equal(a, b)
            D.check("planes_group[%d:%d,%d,%d] %s" % (i, prep.R, prep.K, prep.N, prep.name), a.cpu().numpy(), *prep.ref())
            assert torch.equal(a, linear_planes(prep, q["planes"], q["layout"], q["nb1"]))
    scale = 1.0 / 0.6
    for fam, prep in enumerate(prepared(130, 36, 65, QUICK)):
        keep = (np.random.RandomState(fam).rand(prep.R, prep.N) < 0.6).astype(np.float32)
        q = dict(prep=prep, planes=planes_of(prep), nb1=33, layout="odd", mask=dev(keep))
        for act in (0, 1):
            want, bound = prep.ref(act=act)
            runs = [planes_group([q], act=act, mask_scale=scale, entry="group")[0][0] for _ in range(2)]
            assert torch.equal(*runs)
            got = runs[0].cpu().numpy()
            D.check("planes_group_mask[130,36,65,odd] act%d %s" % (act, prep.name), got, want * keep * np.float32(scale), bound * scale)
            assert (got[keep == 0] == 0).all()


def test_planes_group_input_dropout():
    """mmdfn_linear_planes_group_in: problem 0 contracts (x * keep) * xscale -- formed in float32 first, as the kernel's staging
    step does -- and writes exactly those rows to xdrop; problem 1 has no xmask and the bits of its own launch."""
    xscale = np.float32(1.0 / 0.7)
    for fam, prep in enumerate(prepared(130, 36, 65, QUICK)):
        other = prepared(65, 20, 33, QUICK)[fam]
        keep = (np.random.RandomState(10 + fam).rand(prep.R, prep.K) < 0.7).astype(np.float32)
        xd = (prep.case.X * keep) * xscale                                   # float32, the expression of the kernel
        assert xd.dtype == np.float32
        want, bound = D.want_and_bound(xd, prep.case.W, prep.case.bias, None, prep.n)
        probs = [dict(prep=prep, planes=planes_of(prep), nb1=33, layout="vec", xmask=dev(keep)),
                 dict(prep=other, planes=planes_of(other), nb1=11, layout="odd")]
        runs = [planes_group(probs, xscale=float(xscale)) for _ in range(2)]
        (y0, y1), (drop0, _) = runs[0]
        assert torch.equal(y0, runs[1][0][0]) and torch.equal(y1, runs[1][0][1])
        D.check("planes_group_in_xmask[130,36,65,vec] %s" % prep.name, y0.cpu().numpy(), want, bound)
        assert np.array_equal(drop0.cpu().numpy().view(np.uint32), xd.view(np.uint32))
        D.check("planes_group_in_plain[65,20,33,odd] %s" % other.name, y1.cpu().numpy(), *other.ref())
        assert torch.equal(y1, linear_planes(other, probs[1]["planes"], "odd", 11))
