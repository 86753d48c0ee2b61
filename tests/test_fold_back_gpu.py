"""GPU: the fold-back of the encoder input projections (csrc/fold_back.hip, ops_party.FOLD_BACK).

* the kernel against float64 numpy: one term pair and the model's three (GRU, modality) pairs sharing outputs, with and without
  b_m, fresh outputs and accumulation into non-zero gradients, the -2 answers, two runs bit-equal.  Bound per element:
  (K + 1) 2^-24 sum |terms| (K products in the chain; an existing gradient counts as a term);
* ops.project_gather with named sources: every parameter gradient against float64 within the bound of
  test_project_gather_with_context_rider_gradients (TOL_PROJ x max) AND within twice the error of the switched-off path on the
  same inputs; forward outputs bit-equal with the switch on and off; D = 512 > H keeps today's launches;
* a small DialogueGNNModel: eager train.backward against a CapturedStep with a FlatAdam bucket (bit-equal), accumulation into
  existing gradients, a plain loss.backward() (old path), and the kernel names of one step.
Every test prints its figures before it asserts.
"""
import numpy as np
import pytest
import torch

from mm_dfn_amd import FocalLoss, _hip, ops, ops_party, ops_wgrad, synthetic
from mm_dfn_amd import train as T
from util import party_qmask, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL_PROJ = 2e-5      # x max|ref|: the bound of tests/test_encoder_absorbed_launches_gpu.py's node test
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the kernel
def _terms(rs, pairs, H, bias):
    """pairs: [(gru id, modality id, n1, n2, D)] -> one term per (direction half, pair), in the model's registration order."""
    t = lambda *sh: torch.from_numpy(rs.randn(*sh).astype(np.float32)).to(DEV)
    wih, wm, bm, terms = {}, {}, {}, []
    for g, m, n1, n2, D in pairs:
        if m not in wm:
            wm[m], bm[m] = t(H, D) * 0.1, (t(H) if bias else None)
        for h, n in enumerate((n1, n2)):
            if (g, h) not in wih:
                wih[(g, h)] = t(n, H) * 0.1
            terms.append(dict(M=t(n, D), c=t(n), wih=wih[(g, h)], wm=wm[m], bm=bm[m], ko=("ih", g, h), km=("m", m)))
    return terms


def _call(terms, H, outs, acc, tickets=None):
    pa, ia = _hip.ptr_array, _hip.int_array
    n, D = ia([t["M"].shape[0] for t in terms]), ia([t["M"].shape[1] for t in terms])
    dwm = pa([outs[t["km"]] for t in terms])
    nws = _hip.query("mmdfn_fold_back_workspace", len(terms), dwm, n, D, H)
    assert nws >= 0
    ws = torch.empty(max(int(nws), 2), device=DEV)
    if tickets is None:
        tickets = torch.zeros(int(_hip.query("mmdfn_fold_back_tickets")), dtype=torch.int32, device=DEV)
    rc = _hip.lib().mmdfn_fold_back(len(terms), pa([t["M"] for t in terms]), pa([t["c"] for t in terms]),
                                    pa([t["wih"] for t in terms]), pa([t["wm"] for t in terms]), pa([t["bm"] for t in terms]),
                                    pa([outs[t["ko"]] for t in terms]), dwm,
                                    pa([outs.get(("b",) + t["km"][1:]) for t in terms]), n, D, H,
                                    ia([acc] * len(terms)), ia([acc] * len(terms)), _hip.ptr(ws), _hip.ptr(tickets), _hip.stream())
    torch.cuda.synchronize()
    return rc, tickets


def _reference(terms, H, start):
    """float64 results and the per-element bounds (K + 1) 2^-24 sum |terms|, keyed like the outputs."""
    f = lambda x: x.double().cpu().numpy()
    val, mag, K = {}, {}, {}
    for k, g in start.items():
        val[k], mag[k], K[k] = f(g).copy(), np.abs(f(g)), (1 if float(g.abs().max()) > 0 else 0)
    for t in terms:
        M, c, wih, wm = f(t["M"]), f(t["c"]), f(t["wih"]), f(t["wm"])
        ko, km, kb = t["ko"], t["km"], ("b",) + t["km"][1:]
        val[ko] += M @ wm.T
        mag[ko] += np.abs(M) @ np.abs(wm).T
        K[ko] += M.shape[1]
        val[km] += wih.T @ M
        mag[km] += np.abs(wih).T @ np.abs(M)
        K[km] += M.shape[0]
        if t["bm"] is not None:
            bm = f(t["bm"])
            val[ko] += np.outer(c, bm)
            mag[ko] += np.outer(np.abs(c), np.abs(bm))
            K[ko] += 1
            val[kb] += wih.T @ c
            mag[kb] += np.abs(wih).T @ np.abs(c)
            K[kb] += M.shape[0]
    return val, {k: (K[k] + 1) * EPS * mag[k] for k in val}


def _outputs(terms, H, acc, rs):
    outs = {}
    for t in terms:
        n, D = t["M"].shape
        for k, shape in ((t["ko"], (n, H)), (t["km"], (H, D)), (("b",) + t["km"][1:], (H,))):
            if k in outs or (k[0] == "b" and t["bm"] is None):
                continue
            outs[k] = (torch.from_numpy(rs.randn(*shape).astype(np.float32)).to(DEV) if acc
                       else torch.full(shape, float("nan"), device=DEV))
    return outs


SHAPES = [(12, 8, 4), (600, 200, 100), (600, 200, 68), (600, 8, 100)]


@pytest.mark.parametrize("acc", [0, 1], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("pairs", ["one", "three"])
@pytest.mark.parametrize("N,H,D", SHAPES)
def test_fold_back_kernel_against_float64(N, H, D, pairs, bias, acc):
    """One (GRU, modality) pair, and the model's three -- (party, a), (party, l), (context, l): dW_ih of the party GRU collects
    a and l, dW_l / db_l collect party and context -- against float64.  Fresh outputs are NaN-poisoned first; accumulated ones
    start from random gradients.  A second run from the same start is bit-equal, and the ticket words are zero again."""
    rs = np.random.RandomState(N + H + D + 7 * acc + (3 if bias else 0))
    n1 = N // 2
    spec = [(0, 0, n1, N - n1, D)] if pairs == "one" else [(1, 1, n1, N - n1, D), (0, 0, n1, N - n1, D), (0, 1, n1, N - n1, D)]
    terms = _terms(rs, spec, H, bias)
    outs = _outputs(terms, H, acc, rs)
    start = {k: (v.clone() if acc else torch.zeros_like(v)) for k, v in outs.items()}
    want, bound = _reference(terms, H, start)
    rc, tickets = _call(terms, H, outs, acc)
    assert rc == 0
    assert int(tickets.abs().sum()) == 0
    for k in sorted(outs, key=str):
        got = outs[k].double().cpu().numpy()
        err = np.abs(got - want[k])
        ratio = float((err / np.maximum(bound[k], 1e-300)).max())
        print("fold_back N=%d H=%d D=%d %s bias=%d acc=%d %s: max err %.3g, max err/bound %.3g" % (
            N, H, D, pairs, bias, acc, k, float(err.max()), ratio))
        assert np.isfinite(got).all(), k
        assert (err <= bound[k]).all(), (k, ratio)
    again = {k: (start[k].clone() if acc else torch.full_like(v, float("nan"))) for k, v in outs.items()}
    rc, tickets = _call(terms, H, again, acc, tickets)
    assert rc == 0 and int(tickets.abs().sum()) == 0
    for k in outs:
        assert torch.equal(outs[k], again[k]), k


@pytest.mark.parametrize("acc", [0, 1], ids=["fresh", "accumulate"])
def test_fold_back_single_term_writes_dwm_without_slabs(acc):
    """One term alone: dW_m / db_m have one contribution, which the workgroup writes itself (no slab, no ticket)."""
    rs = np.random.RandomState(11 + acc)
    terms = _terms(rs, [(0, 0, 40, 40, 68)], 72, True)[:1]
    outs = _outputs(terms, 72, acc, rs)
    start = {k: (v.clone() if acc else torch.zeros_like(v)) for k, v in outs.items()}
    want, bound = _reference(terms, 72, start)
    rc, tickets = _call(terms, 72, outs, acc)
    assert rc == 0 and int(tickets.abs().sum()) == 0
    for k in outs:
        err = np.abs(outs[k].double().cpu().numpy() - want[k])
        assert (err <= bound[k]).all(), k


def test_fold_back_answers_minus_two_for_shapes_it_does_not_cover():
    rs = np.random.RandomState(3)
    ok = _terms(rs, [(0, 0, 6, 6, 4)], 8, True)
    outs = _outputs(ok, 8, 0, rs)
    assert _call(ok, 8, outs, 0)[0] == 0
    pa, ia = _hip.ptr_array, _hip.int_array

    def rc_of(terms, H, n=None, D=None):
        n = ia(n or [t["M"].shape[0] for t in terms])
        D = ia(D or [t["M"].shape[1] for t in terms])
        o = [outs[("ih", 0, 0)]] * len(terms)
        tick = torch.zeros(int(_hip.query("mmdfn_fold_back_tickets")), dtype=torch.int32, device=DEV)
        ws = torch.empty(1 << 16, device=DEV)
        return _hip.lib().mmdfn_fold_back(len(terms), pa([t["M"] for t in terms]), pa([t["c"] for t in terms]),
                                          pa([t["wih"] for t in terms]), pa([t["wm"] for t in terms]), pa([t["bm"] for t in terms]),
                                          pa(o), pa([outs[("m", 0)]] * len(terms)), pa([outs[("b", 0)]] * len(terms)), n, D, H,
                                          ia([0] * len(terms)), ia([0] * len(terms)), _hip.ptr(ws), _hip.ptr(tick), _hip.stream())

    assert rc_of(ok, 6) == -2                                # H no multiple of 4
    assert rc_of(ok, 8, D=[6, 6]) == -2                      # D no multiple of 4
    assert rc_of(ok, 8, n=[6, 10]) == -2                     # two terms of one dW_ih disagree on its rows
    assert rc_of(ok * 9, 8) == -2                            # more than 16 terms
    assert _hip.query("mmdfn_fold_back_workspace", 2, pa([outs[("m", 0)]] * 2), ia([6, 6]), ia([6, 4]), 8) == -2
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the node
NODE_CASES = [([5, 3], 2), ([7, 4, 1], 3), ([110] * 16, 2)]


def _node_inputs(lengths, P, D, bias):
    L, B = max(lengths), len(lengths)
    H, N, n1 = 200, 600, 300
    q = party_qmask(lengths, L, P, 77)
    if lengths == [7, 4, 1]:
        q[:, :, P - 1] = 0.0                                   # a speaker that never speaks
    rs = np.random.RandomState(78 + L + D)
    t = lambda *sh: torch.from_numpy(rs.randn(*sh).astype(np.float32))
    v = dict(q=q, u=[t(L, B, D) for _ in range(2)], Wm=[t(H, D) * 0.1 for _ in range(2)],
             bm=[t(H) if bias else None for _ in range(2)], w=t(N, H) * 0.1, b=t(N) if bias else None, rw=t(N, H) * 0.1,
             rb=t(N) if bias else None, Wg=t(L, 2 * B * P, N), Wp=t(L, B, H), Wr=t(L, B, N))
    v.update(L=L, B=B, H=H, N=N, n1=n1, P=P)
    return v


def _node_float64(v, rider):
    import mmdfn_vectorised as V
    n1 = v["n1"]
    d = lambda x: None if x is None else x.double().requires_grad_(True)
    Wm, bm = [d(x) for x in v["Wm"]], [d(x) for x in v["bm"]]
    w, b, rw, rb = d(v["w"]), d(v["b"]), d(v["rw"]), d(v["rb"])
    X = [torch.nn.functional.linear(u.double(), W, bb) for u, W, bb in zip(v["u"], Wm, bm)]
    S = V.party_gather(torch.stack(X, 0), V.party_plan(v["q"]))
    loss = (torch.nn.functional.linear(S, w, b) * v["Wg"].double()).sum() + (X[0] * v["Wp"].double()).sum()
    if rider:
        loss = loss + (torch.nn.functional.linear(X[1], rw, rb) * v["Wr"].double()).sum()
    loss.backward()
    g = lambda x, sl=slice(None): None if x is None else x.grad[sl]
    ref = {"W_a": g(Wm[0]), "W_l": g(Wm[1]), "b_a": g(bm[0]), "b_l": g(bm[1]), "w1": g(w, slice(0, n1)), "w2": g(w, slice(n1, None)),
           "b1": g(b, slice(0, n1)), "b2": g(b, slice(n1, None))}
    if rider:
        ref.update({"rw1": g(rw, slice(0, n1)), "rw2": g(rw, slice(n1, None)), "rb1": g(rb, slice(0, n1)), "rb2": g(rb, slice(n1, None))})
    return {k: x for k, x in ref.items() if x is not None}


def _node_run(v, rider, fold, names=None):
    """One forward + backward of linear_group -> project_gather (sources named) inside a wgrad_batch scope."""
    n1 = v["n1"]
    leaf = lambda x: None if x is None else x.to(DEV, copy=True).requires_grad_(True)
    Wm, bm = [leaf(x) for x in v["Wm"]], [leaf(x) for x in v["bm"]]
    wk, bk, rwk, rbk = v["w"].to(DEV), (None if v["b"] is None else v["b"].to(DEV)), v["rw"].to(DEV), (None if v["rb"] is None else v["rb"].to(DEV))
    half = lambda x: (None, None) if x is None else (x[:n1].requires_grad_(True), x[n1:].requires_grad_(True))
    (w1, w2), (b1, b2), (rw1, rw2), (rb1, rb2) = half(wk), half(bk), half(rwk), half(rbk)
    u = [x.to(DEV) for x in v["u"]]
    prev, ops_party.FOLD_BACK = ops_party.FOLD_BACK, fold
    try:
        def step():
            Xs = ops.linear_group(u, Wm, bm)
            gk, rank, *rest = ops.project_gather(Xs, v["q"].to(DEV), w1, w2, b1, b2, wk, bk,
                                                 riders=[(1, rw1, rw2, rb1, rb2, rwk)] if rider else [],
                                                 sources=[(u[0], Wm[0], bm[0]), (u[1], Wm[1], bm[1])])
            loss = (gk * v["Wg"].to(DEV)).sum() + (rest[0] * v["Wp"].to(DEV)).sum()
            if rider:
                loss = loss + (rest[2] * v["Wr"].to(DEV)).sum()
            with ops.wgrad_batch():
                loss.backward()
            return gk, (rest[2] if rider else None)
        if names is not None:
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                gk, rk = step()
                torch.cuda.synchronize()
            names.extend(e.key for e in prof.key_averages())
        else:
            gk, rk = step()
    finally:
        ops_party.FOLD_BACK = prev
    got = {"W_a": Wm[0], "W_l": Wm[1], "b_a": bm[0], "b_l": bm[1], "w1": w1, "w2": w2, "b1": b1, "b2": b2}
    if rider:
        got.update({"rw1": rw1, "rw2": rw2, "rb1": rb1, "rb2": rb2})
    return gk, rk, {k: p.grad for k, p in got.items() if p is not None}


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("rider", [True, False], ids=["rider", "norider"])
@pytest.mark.parametrize("D", [4, 100, 512])
@pytest.mark.parametrize("lengths,P", NODE_CASES, ids=["L5-B2-P2", "L7-B3-P3-silent", "L110-B16-P2"])
def test_project_gather_with_sources_gradients(lengths, P, D, rider, bias):
    """Modality a reaches the combine stage through its passthrough alias (an addend), modality l does not (its X receives no
    gradient at all): the model's situation.  D = 4 and 100 fold back, D = 512 > H = 200 keeps today's launches."""
    v = _node_inputs(lengths, P, D, bias)
    ref = _node_float64(v, rider)
    names = []
    gk1, rk1, on = _node_run(v, rider, True, names)
    gk0, rk0, off = _node_run(v, rider, False)
    assert torch.equal(gk1, gk0) and (not rider or torch.equal(rk1, rk0))       # the forward pass is not touched
    folded = any("fold_back_kernel" in n for n in names)
    assert folded == (D <= 200), names
    assert sorted(on) == sorted(ref) == sorted(off)
    for k in sorted(ref):
        e_on, e_off = rel_err(on[k], ref[k]), rel_err(off[k], ref[k])
        print("node %s P=%d D=%d rider=%d bias=%d %s: err on %.3g, off %.3g" % (
            "x".join(map(str, (max(lengths), len(lengths)))), P, D, rider, bias, k, e_on, e_off))
    for k in sorted(ref):
        e_on, e_off = rel_err(on[k], ref[k]), rel_err(off[k], ref[k])
        assert e_on < TOL_PROJ, (k, e_on)
        assert e_on <= 2.0 * e_off, (k, e_on, e_off)
    if not folded:
        for k in ref:
            assert torch.equal(on[k], off[k]), k


# ------------------------------------------------------------------------------------------------ the model
CFG = dict(P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)


def _model(seed=5):
    m = synthetic.build_model(dropout=0.0, **CFG)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), seed))
    return m.cuda().train()


def _batch():
    cfg = dict(B=3, L=9, **CFG)
    b = synthetic.make_batch(31, lengths=[9, 4, 7], device="cuda", **cfg)
    return b, T.flatten_labels(b["label"], b["lengths"])


def _loss(m, b, label):
    lp = m(b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"])[0]
    return FocalLoss(gamma=0.5)(lp, label), lp


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_model_step_eager_captured_accumulated_and_plain():
    from mm_dfn_amd import distributed
    from mm_dfn_amd.graphs import CapturedStep
    from mm_dfn_amd.optim import FlatAdam
    b, label = _batch()
    # eager, inside the scope (train.backward); kernel names of this one step
    m0 = _model()
    from torch.profiler import ProfilerActivity, profile
    loss0, lp0 = _loss(m0, b, label)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        T.backward(loss0)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    counts = {e.key: e.count for e in prof.key_averages()}
    assert any("fold_back_kernel" in n for n in names), names
    g0 = _grads(m0)
    # the switched-off step: one more few-row launch (the dX product) and no fold-back kernel
    prev, ops_party.FOLD_BACK = ops_party.FOLD_BACK, False
    try:
        m_off = _model()
        loss_off, lp_off = _loss(m_off, b, label)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            T.backward(loss_off)
            torch.cuda.synchronize()
        counts_off = {e.key: e.count for e in prof.key_averages()}
    finally:
        ops_party.FOLD_BACK = prev
    assert not any("fold_back_kernel" in n for n in counts_off)
    lds = lambda c: sum(v for k, v in c.items() if "linear_lds_kernel" in k or "linear_small" in k or "linear_group" in k)
    print("few-row launches in backward: on %d, off %d" % (lds(counts), lds(counts_off)))
    assert lds(counts) == lds(counts_off) - 1
    assert torch.equal(loss0, loss_off) and torch.equal(lp0, lp_off)
    g_off = _grads(m_off)
    # plain loss.backward() outside the scope: the old path, same bound
    m1 = _model()
    loss1, _ = _loss(m1, b, label)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss1.backward()
        torch.cuda.synchronize()
    counts_plain = {e.key: e.count for e in prof.key_averages()}
    assert not any("fold_back_kernel" in n for n in counts_plain)          # outside the scope: the input-gradient launch
    assert lds(counts_plain) == lds(counts_off)
    g1 = _grads(m1)
    assert sorted(g0) == sorted(g1) == sorted(g_off)
    for k in sorted(g0):
        e, e_off = rel_err(g0[k], g1[k]), rel_err(g_off[k], g1[k])
        if e > 0:
            print("model %s: scope vs plain %.3g (switched off: %.3g)" % (k, e, e_off))
        assert e < TOL_PROJ, (k, e)
    # a second backward accumulates into the existing .grad
    loss0b, _ = _loss(m0, b, label)
    T.backward(loss0b)
    torch.cuda.synchronize()
    for k, p in m0.named_parameters():
        if p.grad is not None:
            assert rel_err(p.grad, 2.0 * g0[k]) < 4 * EPS * 4, k
    # three forward passes ahead of ONE backward pass: 18 fold-back terms, more than one launch takes
    m3 = _model()
    T.backward(sum(_loss(m3, b, label)[0] for _ in range(3)))
    torch.cuda.synchronize()
    g3 = _grads(m3)
    folded = [k for k in g3 if k.startswith(("linear_a.", "linear_l.", "lstm_l.weight_ih_l0", "lstm_l.bias_ih_l0",
                                             "rnn_parties.weight_ih_l0"))]
    assert len(folded) == 10
    for k in folded:                            # every gradient the fold-back launches write
        assert rel_err(g3[k], 3.0 * g1[k]) < TOL_PROJ, k
    # captured with a FlatAdam bucket: the gradients land in the flat buffer, bit-equal to the eager ones
    m2 = _model()
    opt = FlatAdam(m2, lr=1e-3, capturable=True)

    def fwd_bwd():
        loss, _ = _loss(m2, b, label)
        T.backward(loss)
        return loss

    cap = CapturedStep(m2, fwd_bwd, warmup=1, optimizer=opt)
    try:
        loss2 = cap.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss2.detach(), loss0.detach())
        name_of = {id(p): k for k, p in m2.named_parameters()}
        off, seen = 0, 0
        for p in opt.bucket.params:
            got = distributed.slot_view(opt.bucket.flat, off, p)
            off += distributed.slot_size(p)
            assert torch.equal(got, g0[name_of[id(p)]]), name_of[id(p)]
            seen += 1
        assert seen == len(g0)
    finally:
        cap.close()
