"""GPU: the speaker-party glue kernels (K3 / K4, csrc/encoder_glue.hip) against the index-op composition of
oracle/mmdfn_vectorised.py (party_plan / party_gather / party_scatter, checked against the oracle on the CPU in
tests/test_host_logic.py) run in float64 on the CPU, gradients by autograd, at the edges of their launch geometry:
row slices of at least 8 and (destination-driven backward) at most 256 rows, L up to MAXL = 2048, B*P around 1024 (where
the slicing collapses to one slice), P = 16, four modalities with a zero speaker weight (E holds one block per non-zero
weight), widths that are not multiples of 64, and qmask rows that are one-hot, zero-hot, multi-hot (the last flagged
speaker wins) or flagged on padding."""
import numpy as np
import pytest
import torch

import mmdfn_vectorised as V
from mm_dfn_amd import _hip, ops
from mm_dfn_amd.dialogue_model import _flat_index, _flat_inverse
from util import party_qmask, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-6           # x max|ref|: the kernels copy, scale by w or add P terms in fp32 (tests/test_gru_gpu.py's K3/K4 bound)
TOL_PROJ = 2e-5      # x max|ref|: a K = 200 fp32 contraction in front of the gather (tests/test_gru_gpu.py's project_gather bound)

# (L, B, P, Mn, H, speaker weights, flag on a padding row, multi-hot rows claimed)
CASES = [
    (1, 1, 1, 1, 4, [1.5], False, False),                     # minimal
    (7, 3, 2, 3, 4, [3.0, 0.0, 1.0], True, True),             # B*P = 6: one 7-row slice
    (8, 2, 3, 3, 68, [1.0, 2.0, 0.5], False, True),           # one 8-row slice
    (9, 3, 2, 3, 200, [3.0, 0.0, 1.0], True, True),           # two slices of 5 and 4 rows
    (255, 2, 3, 3, 4, [1.0, 2.0, 0.5], True, True),
    (256, 3, 2, 3, 68, [3.0, 0.0, 1.0], False, True),
    (257, 2, 3, 3, 4, [0.0, 0.0, 2.0], True, True),           # last slice holds one row
    (2047, 1, 2, 3, 4, [3.0, 0.0, 1.0], False, True),         # B*P = 2: 256 slices of 8 rows
    (2048, 1, 2, 3, 4, [1.0, 2.0, 0.5], False, True),
    (2047, 32, 4, 3, 4, [3.0, 0.0, 1.0], True, True),         # B*P = 128: 8 slices of 256 (and 255) rows
    (2048, 32, 4, 3, 4, [1.0, 2.0, 0.5], True, True),
    (17, 341, 3, 3, 4, [3.0, 0.0, 1.0], True, True),          # B*P = 1023
    (17, 512, 2, 3, 4, [1.0, 2.0, 0.5], True, True),          # B*P = 1024
    (17, 205, 5, 3, 4, [3.0, 0.0, 1.0], True, True),          # B*P = 1025
    (17, 128, 9, 3, 4, [1.0, 2.0, 0.5], True, True),          # B*P = 1152
    (12, 3, 16, 3, 68, [3.0, 0.0, 1.0], True, True),          # P = 16
    (20, 3, 3, 4, 4, [1.0, 0.0, 2.0, 0.5], True, True),       # Mn = 4, a zero weight between non-zero ones
    (33, 2, 3, 4, 200, [0.5, 1.0, 2.0, 3.0], True, True),     # Mn = 4, every modality gathered
]


def _ids(c):
    return "L%d-B%d-P%d-M%d-H%d-w%s" % (c[0], c[1], c[2], c[3], c[4], "_".join("%g" % x for x in c[5]))


def _setup(case, seed):
    L, B, P, Mn, H, w, pad_flag, multi = case
    rs = np.random.RandomState(seed)
    lengths = [L] + [int(x) for x in rs.randint(1, L + 1, size=B - 1)]
    if B > 1 and L > 1:
        lengths[-1] = int(rs.randint(1, L))           # at least one dialogue with padding
    q = party_qmask(lengths, L, P, seed + 1, pad_flag=pad_flag)
    valid = torch.arange(L).view(L, 1) < torch.tensor(lengths).view(1, B)
    flags = q.sum(2)
    if multi:
        # the check is not empty: a valid multi-hot utterance, and a modality whose party term it reaches
        assert bool(((flags >= 2) & valid).any()) and any(x != 0.0 for x in w)
        assert bool(((flags == 0) & valid).any())
    if P >= 3 or (P == 2 and B >= 2):
        assert float(q[:, B - 1, P - 1].sum()) == 0.0       # a speaker silent in one dialogue
    if pad_flag:
        assert bool(((flags > 0) & ~valid).any())
    assert bool(((flags == 1) & valid).any())
    return lengths, q, valid, rs


def _rank_of(q):
    """The kernels' rank layout (L, B, P) int32: position of utterance t among speaker p's utterances, -1 if not flagged."""
    mask = q != 0
    return torch.where(mask, torch.cumsum(mask.to(torch.int64), 0) - 1, torch.full_like(mask, -1, dtype=torch.int64)).to(torch.int32)


def _stripped_rows(lengths, B):
    return torch.from_numpy(np.concatenate([np.arange(n, dtype=np.int64) * B + j for j, n in enumerate(lengths)]))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_party_gather_matches_plan(case):
    """S and rank bit-equal to the fp32 CPU composition (S is a copy plus one bias add); the scatter-add backward dX within
    1e-6 x max of float64."""
    L, B, P, Mn, H, w = case[:6]
    lengths, q, valid, rs = _setup(case, 100 + L + B)
    act = [m for m in range(Mn) if w[m] != 0.0]
    Mg = len(act)
    X = torch.from_numpy(rs.randn(Mg, L, B, H).astype(np.float32))
    bias = torch.from_numpy(rs.randn(H).astype(np.float32))
    WS = torch.from_numpy(rs.randn(L, Mg * B * P, H).astype(np.float32))
    plan = V.party_plan(q)
    for with_bias in (False, True):
        Xk = [X[i].to(DEV, copy=True).requires_grad_(True) for i in range(Mg)]
        Sk, rank = ops.party_gather(Xk, q.to(DEV), bias.to(DEV) if with_bias else None)
        (Sk * WS.to(DEV)).sum().backward()
        S32 = V.party_gather(X, plan)
        if with_bias:
            S32 = S32 + bias
        assert torch.equal(rank.cpu(), _rank_of(q))
        assert float((Sk.detach().cpu() - S32).abs().max()) == 0.0
        X64 = X.double().requires_grad_(True)
        (V.party_gather(X64, plan) * WS.double()).sum().backward()
        for i in range(Mg):
            assert rel_err(Xk[i].grad, X64.grad[i]) < TOL, i


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_party_combine_matches_scatter(case):
    """out = strip_pad(base_m + w_m scatter(E)) and its gradients dbase, dE (E a leaf input) against float64, for both
    backward forms: destination-driven (with inv, what the model runs) and pre-zeroed (without).  dE must be exactly 0
    wherever no gradient goes (a later speaker flagged on the utterance, k at or past the party's count, a flagged padding
    row), and the two forms write w*g and g from the same operands, so they must agree bit for bit."""
    L, B, P, Mn, H, w = case[:6]
    lengths, q, valid, rs = _setup(case, 200 + L + B)
    act = [m for m in range(Mn) if w[m] != 0.0]
    nact, N = len(act), sum(lengths)
    base = torch.from_numpy(rs.randn(Mn, L, B, H).astype(np.float32))
    E = torch.from_numpy(rs.randn(L, nact * B * P, H).astype(np.float32))
    Wg = torch.from_numpy(rs.randn(Mn, N, H).astype(np.float32))
    # float64 reference
    plan = V.party_plan(q)
    b64, E64 = base.double().requires_grad_(True), E.double().requires_grad_(True)
    U = V.party_scatter(E64, plan, nact)
    outs = [b64[m] + w[m] * U[act.index(m)] if m in act else b64[m] for m in range(Mn)]
    out64 = torch.stack(outs, 0).reshape(Mn, L * B, H).index_select(1, _stripped_rows(lengths, B))
    (out64 * Wg.double()).sum().backward()
    # where dE must be exactly zero: (k, b, p) is live iff k < count, p is the last speaker flagged on utterance src[k]
    # and that utterance is not padding
    src, _, sel = plan
    has = src < L
    t = src.clamp(max=L - 1)
    bidx = torch.arange(B).view(1, B, 1).expand(L, B, P)
    pidx = torch.arange(P).view(1, 1, P).expand(L, B, P)
    live3 = has & sel[t, bidx, pidx] & valid[t, bidx]
    live = live3.view(L, 1, B * P, 1).expand(L, nact, B * P, H).reshape(L, nact * B * P, H)
    assert not bool(E64.grad[~live].any())
    if case[7]:
        # some party does NOT take the gradient of a valid multi-hot utterance it was gathered for
        assert bool((has & valid[t, bidx] & ~live3).any())
    rank = _rank_of(q).to(DEV)
    idx = _flat_index(lengths, L, B, DEV)
    inv = _flat_inverse(lengths, L, B, DEV)
    res = {}
    for form in ("dst", "zeroed"):
        bk = [base[m].to(DEV, copy=True).requires_grad_(True) for m in range(Mn)]
        Ek = E.to(DEV, copy=True).requires_grad_(True)
        outk = ops.party_combine(bk, Ek, rank, idx, w, inv=inv if form == "dst" else None)
        (outk * Wg.to(DEV)).sum().backward()
        dbase = torch.stack([x.grad for x in bk], 0).cpu()
        dE = Ek.grad.cpu()
        assert rel_err(outk, out64) < TOL, form
        assert rel_err(dbase, b64.grad) < TOL, form
        assert rel_err(dE, E64.grad) < TOL, form
        assert not bool(dE[~live].any()), form
        res[form] = (dbase, dE)
    assert torch.equal(res["dst"][0], res["zeroed"][0])
    assert torch.equal(res["dst"][1], res["zeroed"][1])


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("P,lengths,nact,N", [(2, [7, 3, 5], 2, 600), (3, [9, 4], 3, 68), (2, [200, 37, 120, 9], 2, 68)])
def test_project_gather_small_and_odd_widths(P, lengths, nact, N, batched):
    """ops.project_gather (projection of the utterances, then the gather, bias on every party row) against the gather in
    float64 followed by the projection: gate pre-activations, both weight blocks, both bias blocks and the input gradients
    within 2e-5 x max.  The first two shapes have fewer than 64 * 48 party rows (fewer column-sum slabs than the kernel's
    48); N = 68 is a width the 64-column blocks do not divide.  ``batched``: under ops.wgrad_batch(), where the bias
    gradient comes out of party_gather_bwd_colsum's slabs, else out of the colsum kernel."""
    L, B = max(lengths), len(lengths)
    H, n1 = 200, N // 2
    q = party_qmask(lengths, L, P, 31 + N)
    rs = np.random.RandomState(32 + L)
    t = lambda *sh: torch.from_numpy(rs.randn(*sh).astype(np.float32))
    Xs = [t(L, B, H) for _ in range(nact)]
    wbuf, bbuf = t(N, H) * 0.1, t(N)
    Wg, Wp = t(L, nact * B * P, N), [t(L, B, H) for _ in range(nact)]
    # float64: gather, then the projection of every party row (padding rows included)
    X64 = [x.double().requires_grad_(True) for x in Xs]
    w64 = [wbuf[:n1].double().requires_grad_(True), wbuf[n1:].double().requires_grad_(True)]
    b64 = [bbuf[:n1].double().requires_grad_(True), bbuf[n1:].double().requires_grad_(True)]
    S64 = V.party_gather(torch.stack(X64, 0), V.party_plan(q))
    g64 = torch.nn.functional.linear(S64, torch.cat(w64), torch.cat(b64))
    ((g64 * Wg.double()).sum() + sum((x * p_.double()).sum() for x, p_ in zip(X64, Wp))).backward()
    # the node
    Xk = [x.to(DEV, copy=True).requires_grad_(True) for x in Xs]
    wk, bk = wbuf.to(DEV), bbuf.to(DEV)
    prm = [wk[:n1].requires_grad_(True), wk[n1:].requires_grad_(True), bk[:n1].requires_grad_(True), bk[n1:].requires_grad_(True)]
    gk, rank, *passed = ops.project_gather(Xk, q.to(DEV), *prm, wk, bk)
    loss = (gk * Wg.to(DEV)).sum() + sum((x * p_.to(DEV)).sum() for x, p_ in zip(passed, Wp))
    if batched:
        with ops.wgrad_batch():
            loss.backward()
    else:
        loss.backward()
    assert rel_err(gk, g64) < TOL_PROJ
    for a, ref in zip(prm, w64 + b64):
        assert rel_err(a.grad, ref.grad) < TOL_PROJ
    for a, ref in zip(Xk, X64):
        assert rel_err(a.grad, ref.grad) < TOL_PROJ


def test_party_gather_rejects_more_than_maxl_rows():
    """L = 2049 exceeds the kernels' MAXL = 2048 (the row lists live in LDS): the gather entry point refuses it before any
    launch and the operator raises."""
    L, B, P, H = 2049, 1, 2, 4
    q = torch.zeros(L, B, P, device=DEV)
    q[:, 0, 0] = 1.0
    with pytest.raises(_hip.HipLibraryError, match="mmdfn_party_gather failed with code -1"):
        ops.party_gather([torch.zeros(L, B, H, device=DEV)], q)
