"""GPU: launches of the encoder that a neighbouring projection launch absorbed, each against the form it replaces.

* the party-ordered store of the first party-GRU layer's input projection (csrc/linear_planes.hip, PARTY) against the
  projection in utterance order followed by mmdfn_party_gather: S and rank bit for bit;
* the inter-layer dropout formed in the second GRU layer's input projection (csrc/linear_planes.hip, INMASK) against
  ops.mask_scale followed by the same projection: outputs and the saved dropped activations bit for bit;
* the second K segment of the few-row LDS kernel (csrc/linear_small.hip): y = x wk + x2 wk2 + z in one launch against float64,
  within the bound of this kernel family (TOL_PROJ of tests/test_party_glue_gpu.py) and within twice the error of the two
  accumulating launches it replaces; a problem without a second segment keeps the bits of its own launch;
* ops.project_gather with a context rider: every gradient against float64 with the rider's input gradient as second segment
  and as a launch of its own.
"""
import numpy as np
import pytest
import torch

from mm_dfn_amd import _hip, ops, ops_linear, ops_party
from util import party_qmask, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL_PROJ = 2e-5      # x max|ref|: tests/test_party_glue_gpu.py's bound for the few-row projection kernels


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _flags(shape, kind, g):
    if kind == "zero":
        return torch.zeros(*shape, device=DEV)
    if kind == "one":
        return torch.ones(*shape, device=DEV)
    return (torch.rand(*shape, device=DEV, generator=g) < 0.6).float()


@pytest.mark.parametrize("kind", ["random", "zero", "one"])
@pytest.mark.parametrize("R,K,N", [(8800, 200, 600), (7040, 600, 600), (4100, 200, 600), (130, 600, 200), (64, 200, 68), (1, 8, 40)])
def test_input_dropout_in_the_projection_is_mask_scale_then_projection(R, K, N, kind):
    """(x * keep) * scale formed in the staging step: Y and the dropped rows equal, bit for bit, ops.mask_scale + the plain
    launch.  Buffers are NaN-poisoned first (every element of the dropped copy must be written, rows of a last partial row
    block included); a second problem WITHOUT flags rides in the same launch and keeps the bits of its own launch.  Shapes:
    R a multiple of 64 and not, both tile forms (64 x 128 and 64 x 64 workgroups), K = 200 and 600."""
    g = _gen(R + K + N)
    scale = 1.0 / 0.6
    n1 = N // 2
    x = torch.randn(R, K, device=DEV, generator=g)
    keep = _flags((R, K), kind, g)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.1
    b = torch.randn(N, device=DEV, generator=g)
    w1, w2, b1, b2 = w[:n1].contiguous(), w[n1:].contiguous(), b[:n1].contiguous(), b[n1:].contiguous()
    x_other = torch.randn(333, K, device=DEV, generator=g)
    (xs,) = ops.mask_scale([x], [keep], scale)
    want = ops_linear.linear_planes_group_raw([dict(x=xs, w1=w1, w2=w2, b1=b1, b2=b2)])[0]
    want_other = ops_linear.linear_planes_group_raw([dict(x=x_other, w1=w1, w2=w2, b1=b1, b2=b2)])[0]
    nan = float("nan")
    y = torch.full((R, N), nan, device=DEV)
    y_other = torch.full((333, N), nan, device=DEV)
    xd = torch.full((R, K), nan, device=DEV)
    ops_linear.linear_planes_group_raw([dict(x=x, w1=w1, w2=w2, b1=b1, b2=b2, out=y, xmask=keep, xdrop=xd),
                                        dict(x=x_other, w1=w1, w2=w2, b1=b1, b2=b2, out=y_other)], xscale=scale)
    assert torch.equal(xd, xs)
    assert torch.equal(y, want)
    assert torch.equal(y_other, want_other)
    # without a copy of the dropped rows
    y2 = torch.full((R, N), nan, device=DEV)
    ops_linear.linear_planes_group_raw([dict(x=x, w1=w1, w2=w2, b1=b1, b2=b2, out=y2, xmask=keep)], xscale=scale)
    assert torch.equal(y2, want)


@pytest.mark.parametrize("rows", [(7040, 1760), (4100, 130)])
def test_linear2_group_node_with_fused_dropout_is_the_two_launch_node(rows):
    """The autograd node (what gru.bigru2 calls for its second layer): outputs and every gradient with the dropout inside the
    projection launch equal those of the node with ops.mask_scale in front, bit for bit (the weight gradients contract the
    dropped rows the launch wrote out)."""
    K, H3 = 200, 300
    res = {}
    for fused in (False, True):
        g = _gen(17)
        groups, masks, leaves = [], [], []
        for R in rows:
            x = torch.randn(R, K, device=DEV, generator=g).requires_grad_(True)
            prm = [(torch.randn(H3, K, device=DEV, generator=g) * 0.1).requires_grad_(True) for _ in range(2)]
            bs = [torch.randn(H3, device=DEV, generator=g).requires_grad_(True) for _ in range(2)]
            groups.append((x, prm[0], prm[1], bs[0], bs[1]))
            masks.append((torch.rand(R, K, device=DEV, generator=g) < 0.6).float())
            leaves += [x] + prm + bs
        wy = [torch.randn(R, 2 * H3, device=DEV, generator=g) for R in rows]
        prev, ops_linear.FUSE_INPUT_DROPOUT = ops_linear.FUSE_INPUT_DROPOUT, fused
        try:
            ys = ops_linear.linear2_group(groups, masks=masks, scale=1.0 / 0.6)
        finally:
            ops_linear.FUSE_INPUT_DROPOUT = prev
        assert ys is not None
        sum((y * w_).sum() for y, w_ in zip(ys, wy)).backward()
        res[fused] = [y.detach() for y in ys] + [t.grad for t in leaves]
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def _seg2_case(R, K, K2, N, seed, with_addend=True):
    g = _gen(seed)
    x = torch.randn(R, K, device=DEV, generator=g)
    x2 = torch.randn(R, K2, device=DEV, generator=g)
    wk = torch.randn(K, N, device=DEV, generator=g) * 0.1
    wk2 = torch.randn(K2, N, device=DEV, generator=g) * 0.1
    z = torch.randn(R, N, device=DEV, generator=g) if with_addend else None
    want = x.double() @ wk.double() + x2.double() @ wk2.double()
    if z is not None:
        want = want + z.double()
    return x, x2, wk, wk2, z, want


@pytest.mark.parametrize("R,K,K2,N", [(1760, 600, 600, 200), (1750, 600, 600, 200), (1000, 600, 200, 200), (77, 68, 100, 200),
                                      (33, 8, 4, 68), (1760, 200, 600, 600), (7040, 600, 600, 200)])
def test_two_k_segments_against_float64(R, K, K2, N):
    """y = x wk + x2 wk2 + z in ONE launch against float64: within TOL_PROJ x max, and within 2 x the error of the two-launch
    form it replaces (y = x wk + z, then y += x2 wk2) on the same inputs -- a reordering of one fp32 sum (exact-f32 MFMA in
    both), not a change of arithmetic.  K, K2 multiples of 64 and not; R a multiple of 32 and not; 32- and 64-row tiles.
    Measured on an MI355X (max |err| / max |ref|, one launch | two launches): see profiles/r07_absorbed_launches.md."""
    x, x2, wk, wk2, z, want = _seg2_case(R, K, K2, N, R + K + K2)
    scale = float(want.abs().max())
    out = torch.full((R, N), float("nan"), device=DEV)
    got = ops.linear_group_raw([dict(x=x, wk=wk, x2=x2, wk2=wk2, addend=z, out=out)])
    assert got is not None
    two = ops.linear_group_raw([dict(x=x, wk=wk, addend=z)])[0]
    ops.linear_group_raw([dict(x=x2, wk=wk2, out=two, accumulate=True)])
    e_one = float((out.double() - want).abs().max()) / scale
    e_two = float((two.double() - want).abs().max()) / scale
    print("seg2 R=%d K=%d K2=%d N=%d: one launch %.3e, two launches %.3e (x max|ref|)" % (R, K, K2, N, e_one, e_two))
    assert e_one < TOL_PROJ
    assert e_one <= 2.0 * e_two
    # no addend
    got = ops.linear_group_raw([dict(x=x, wk=wk, x2=x2, wk2=wk2)])[0]
    want0 = want - z.double()
    assert float((got.double() - want0).abs().max()) < TOL_PROJ * float(want0.abs().max())


def test_problem_without_second_segment_keeps_its_bits_in_a_mixed_launch():
    """One launch with a two-segment problem and a plain K-major problem (and a plain (N, K) one): the plain problems equal their
    own launches bit for bit (same chunk order, same partial-tile reduction; all three launches take the 32-row tile form)."""
    x, x2, wk, wk2, z, want = _seg2_case(500, 600, 600, 200, 5)
    g = _gen(6)
    xp = torch.randn(301, 600, device=DEV, generator=g)
    wp = torch.randn(600, 200, device=DEV, generator=g) * 0.1
    zp = torch.randn(301, 200, device=DEV, generator=g)
    xn = torch.randn(130, 200, device=DEV, generator=g)
    wn = torch.randn(68, 200, device=DEV, generator=g) * 0.1
    bn = torch.randn(68, device=DEV, generator=g)
    plain = ops.linear_group_raw([dict(x=xp, wk=wp, addend=zp)])[0]
    plain_n = ops.linear_group_raw([dict(x=xn, w=wn, b=bn)])[0]
    seg_alone = ops.linear_group_raw([dict(x=x, wk=wk, x2=x2, wk2=wk2, addend=z)])[0]
    outs = ops.linear_group_raw([dict(x=x, wk=wk, x2=x2, wk2=wk2, addend=z), dict(x=xp, wk=wp, addend=zp), dict(x=xn, w=wn, b=bn)])
    assert torch.equal(outs[1], plain)
    assert torch.equal(outs[2], plain_n)
    assert torch.equal(outs[0], seg_alone)
    assert float((outs[0].double() - want).abs().max()) < TOL_PROJ * float(want.abs().max())


def test_second_segment_is_refused_for_unaligned_operands():
    """The register form (operands that are not 16-byte aligned) has no second segment: the operator reports it (None) and the
    caller runs two launches."""
    x, x2, wk, wk2, z, _ = _seg2_case(64, 64, 64, 64, 9)
    xu = torch.empty(64 * 68 + 1, device=DEV)[1:].view(64, 68)[:, :64]     # 4-byte aligned rows
    xu.copy_(x)
    assert xu.data_ptr() % 16 != 0
    import ctypes
    from mm_dfn_amd import _hip
    lib = _hip.lib()
    out = torch.empty(64, 64, device=DEV)
    ia, pa = _hip.int_array, _hip.ptr_array
    rc = lib.mmdfn_linear_group_seg2(1, pa([xu]), pa([wk]), pa([None]), ia([64]), pa([None]), pa([None]), pa([out]), None, None,
                                     ia([64]), ia([64]), ia([64]), ia([68]), ia([64]), ia([64]), ia([1]), ia([0]), pa([x2]), pa([wk2]),
                                     ia([64]), ia([64]), ia([64]), 0, _hip.stream())
    assert rc == -2


def _party_case_qmask(L, lengths, P, seed, kind):
    q = party_qmask(lengths, L, P, seed, pad_flag=True)
    if kind == "solo":            # dialogue 0 has one speaker only (count = L: no padding row), the others never speak in it
        q[:, 0, :] = 0.0
        q[:, 0, 0] = 1.0
    return q


PARTY_CASES = [
    # (L, lengths, P, qmask kind)
    (110, [110] * 16, 2, "mixed"),                           # cfg2's own shape
    (110, [110] * 16, 2, "solo"),
    (37, [37, 20, 9, 30, 1], 3, "mixed"),                    # L % 4 = 1, L B = 185: a partial row block, ragged
    (37, [37, 20, 9, 30, 1], 3, "solo"),
    (33, [33, 5, 17, 33, 8, 2, 29], 9, "mixed"),             # P = 9, L B = 231
    (70, [70, 3], 2, "mixed"),                               # B = 2: a row block spans 32 utterances
    (5, [5] * 70, 3, "mixed"),                               # B = 70 > 64: a row block inside one utterance step
]


@pytest.mark.parametrize("Mn,rider", [(1, False), (1, True), (2, False), (2, True)])
@pytest.mark.parametrize("case", PARTY_CASES, ids=lambda c: "L%d-B%d-P%d-%s" % (c[0], len(c[1]), c[2], c[3]))
def test_party_ordered_store_is_projection_then_gather(case, Mn, rider):
    """S and rank of the one-launch form equal, bit for bit, the plane projection in utterance order followed by
    mmdfn_party_gather (+ bias); S, rank and the rider's output are NaN- / garbage-poisoned first, so a row nobody wrote fails.
    The qmasks hold one-hot, zero-hot and multi-hot rows, a flag on a padding row, a speaker that never speaks in a dialogue
    (its whole column is bias rows) and ("solo") a dialogue with one speaker only (no padding row in its column)."""
    L, lengths, P, kind = case
    B, H, N, n1 = len(lengths), 200, 600, 300
    q = _party_case_qmask(L, lengths, P, 5 + L, kind).to(DEV)
    flags = q.sum(2)
    assert bool((flags >= 2).any()) and bool((flags == 0).any())
    assert bool((q.sum(0) == 0).any())                         # a (dialogue, speaker) that never speaks
    if kind == "solo":
        assert float(q[:, 0, 0].sum()) == L
    g = _gen(L + B + P)
    Xs = [torch.randn(L, B, H, device=DEV, generator=g) for _ in range(Mn)]
    w = torch.randn(N, H, device=DEV, generator=g) * 0.1
    b = torch.randn(N, device=DEV, generator=g)
    w1, w2, b1, b2 = w[:n1].contiguous(), w[n1:].contiguous(), b[:n1].contiguous(), b[n1:].contiguous()
    rw = torch.randn(N, H, device=DEV, generator=g) * 0.1
    rb = torch.randn(N, device=DEV, generator=g)
    rw1, rw2, rb1, rb2 = rw[:n1].contiguous(), rw[n1:].contiguous(), rb[:n1].contiguous(), rb[n1:].contiguous()
    # two launches
    G = [torch.empty(L * B, N, device=DEV) for _ in range(Mn)]
    probs = [dict(x=x.view(L * B, H), w1=w1, w2=w2, out=o) for x, o in zip(Xs, G)]
    if rider:
        probs.append(dict(x=Xs[Mn - 1].view(L * B, H), w1=rw1, w2=rw2, b1=rb1, b2=rb2))
    ref = ops_linear.linear_planes_group_raw(probs)
    S_ref = torch.full((L, Mn * B * P, N), float("nan"), device=DEV)
    rank_ref = torch.full((L, B, P), -7, dtype=torch.int32, device=DEV)
    rc = _hip.lib().mmdfn_party_gather(Mn, _hip.ptr_array(G), _hip.ptr(q), _hip.ptr(b), _hip.ptr(S_ref), _hip.ptr(rank_ref),
                                       L, B, P, N, _hip.stream())
    assert rc == 0
    # one launch
    S = torch.full((L, Mn * B * P, N), float("nan"), device=DEV)
    rank = torch.full((L, B, P), -7, dtype=torch.int32, device=DEV)
    probs = [dict(x=x.view(L * B, H), w1=w1, w2=w2, b1=b1, b2=b2, party_m=i) for i, x in enumerate(Xs)]
    r_out = torch.full((L * B, N), float("nan"), device=DEV)
    if rider:
        probs.append(dict(x=Xs[Mn - 1].view(L * B, H), w1=rw1, w2=rw2, b1=rb1, b2=rb2, out=r_out))
    got = ops_linear.linear_planes_group_raw(probs, party=dict(qmask=q, S=S, rank=rank))
    assert got is not None
    assert not bool(torch.isnan(S_ref).any())
    assert torch.equal(rank, rank_ref)
    assert torch.equal(S, S_ref)
    if rider:
        assert torch.equal(r_out, ref[Mn])


def test_party_ordered_store_refuses_shapes_it_does_not_cover():
    """P > 16: the entry point answers -2 before any launch (the operator returns None) and the node keeps its two launches."""
    L, B, P, H, N = 4, 2, 17, 8, 8
    q = torch.zeros(L, B, P, device=DEV)
    q[:, :, 0] = 1.0
    x = torch.randn(L * B, H, device=DEV)
    w1, w2 = torch.randn(4, H, device=DEV), torch.randn(4, H, device=DEV)
    S = torch.zeros(L, B * P, N, device=DEV)
    rank = torch.zeros(L, B, P, dtype=torch.int32, device=DEV)
    assert ops_linear.linear_planes_group_raw([dict(x=x, w1=w1, w2=w2, party_m=0)], party=dict(qmask=q, S=S, rank=rank)) is None


@pytest.mark.parametrize("segment", [True, False], ids=["absorbed", "launches"])
@pytest.mark.parametrize("lengths,P", [([110] * 16, 2), ([37, 20, 9, 30], 3), ([110, 64, 97, 110, 13, 110, 80, 41, 110, 7, 55, 110, 101, 29, 110, 3], 3)])
def test_project_gather_with_context_rider_gradients(lengths, P, segment):
    """ops.project_gather with the context GRU's contraction of the text rows as rider: party pre-activations, the rider's
    output and every gradient against float64 (gather, then project: tests/test_party_glue_gpu.py) within TOL_PROJ x max, with
    the absorbed forms (party-ordered store; the rider's input gradient as second K segment of the source modality's problem:
    what the model runs) and with the launches they replace.  The 16-dialogue shapes take the plane form."""
    import mmdfn_vectorised as V
    L, B = max(lengths), len(lengths)
    H, N, n1 = 200, 600, 300
    q = party_qmask(lengths, L, P, 77)
    rs = np.random.RandomState(78 + L)
    t = lambda *sh: torch.from_numpy(rs.randn(*sh).astype(np.float32))
    Xs = [t(L, B, H) for _ in range(2)]
    wbuf, bbuf, rwbuf, rbbuf = t(N, H) * 0.1, t(N), t(N, H) * 0.1, t(N)
    Wg, Wp, Wr = t(L, 2 * B * P, N), [t(L, B, H) for _ in range(2)], t(L, B, N)
    X64 = [x.double().requires_grad_(True) for x in Xs]
    p64 = [v.double().requires_grad_(True) for v in (wbuf[:n1], wbuf[n1:], bbuf[:n1], bbuf[n1:], rwbuf[:n1], rwbuf[n1:], rbbuf[:n1], rbbuf[n1:])]
    S64 = V.party_gather(torch.stack(X64, 0), V.party_plan(q))
    g64 = torch.nn.functional.linear(S64, torch.cat(p64[0:2]), torch.cat(p64[2:4]))
    r64 = torch.nn.functional.linear(X64[1], torch.cat(p64[4:6]), torch.cat(p64[6:8]))
    ((g64 * Wg.double()).sum() + (r64 * Wr.double()).sum() + sum((x * p_.double()).sum() for x, p_ in zip(X64, Wp))).backward()
    Xk = [x.to(DEV, copy=True).requires_grad_(True) for x in Xs]
    wk, bk, rwk, rbk = wbuf.to(DEV), bbuf.to(DEV), rwbuf.to(DEV), rbbuf.to(DEV)
    prm = [wk[:n1].requires_grad_(True), wk[n1:].requires_grad_(True), bk[:n1].requires_grad_(True), bk[n1:].requires_grad_(True)]
    rprm = [rwk[:n1].requires_grad_(True), rwk[n1:].requires_grad_(True), rbk[:n1].requires_grad_(True), rbk[n1:].requires_grad_(True)]
    prev, ops_party.RIDER_DX_SEGMENT = ops_party.RIDER_DX_SEGMENT, segment
    prev_s, ops_party.PARTY_ORDERED_STORE = ops_party.PARTY_ORDERED_STORE, segment
    try:
        gk, rank, *rest = ops.project_gather(Xk, q.to(DEV), *prm, wk, bk, riders=[(1, *rprm, rwk)])
        passed, rk = rest[:2], rest[2]
        ((gk * Wg.to(DEV)).sum() + (rk * Wr.to(DEV)).sum() + sum((x * p_.to(DEV)).sum() for x, p_ in zip(passed, Wp))).backward()
    finally:
        ops_party.RIDER_DX_SEGMENT = prev
        ops_party.PARTY_ORDERED_STORE = prev_s
    assert torch.equal(rank.cpu(), torch.where(q != 0, torch.cumsum((q != 0).long(), 0) - 1, torch.full_like(q, -1, dtype=torch.long)).int())
    assert rel_err(gk, g64) < TOL_PROJ
    assert rel_err(rk, r64) < TOL_PROJ
    for a, ref in zip(prm + rprm, p64):
        assert rel_err(a.grad, ref.grad) < TOL_PROJ
    for a, ref in zip(Xk, X64):
        assert rel_err(a.grad, ref.grad) < TOL_PROJ
