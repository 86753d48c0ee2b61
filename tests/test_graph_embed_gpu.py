"""Speaker / modality embeddings of the graph input on the device (csrc/graph_embed.hip, ops.graph_embeddings,
MM_GCN.forward_stacked with use_speaker / use_modal).

Kernel level.  The forward is plain float32 adds: the device result must EQUAL a float32 numpy evaluation.  The backward sums
rows: against a float64 evaluation every table entry is held to (n + 1) 2^-24 sum |terms|, n the number of rows in its sum --
the bound of any summation order of n float32 terms -- a speaker without an utterance and an absent modality must get exactly
0.0, and two runs on the same input must agree bit for bit.

Module level.  MM_GCN.forward_stacked against the reference's own float32 run (tests/golden/mm_gcn_embeddings.npz, written by
tests/golden/make_golden_embeddings.py) with the pass rule of tests/test_arccos_graph_gpu.py: the error against a float64
restatement is at most 4 x the error of the reference's float32 run against that restatement, floor 2^-24; the three figures
are printed before the assertion.
"""
import os

import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from angular_graph_ref import EPS_HALF, err
from mm_dfn_amd import MM_GCN, _hip, ops, ops_embed
from mm_dfn_amd.layout import flat_index

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW = {'a': 0, 'v': 1, 'l': 2}


# ---- inputs and CPU references ---------------------------------------------------------------------------------------------------
def split_lengths(N):
    """Up to three dialogues of N utterances in all, the first one the longest."""
    if N < 3:
        return [N]
    a = N - 2 * (N // 3)
    return [a, N // 3, N // 3]


def make_case(present, N, D, S, seed, with_speaker=True, with_modal=True):
    """X (M, N, D), qmask (L, B, S) with one-hot rows except an all-zero row (utterance 0) and a tie (utterance 1, when there
    are two parties), flat_idx, the two tables and a cotangent -- float32 numpy, and the speaker of every row."""
    rs = np.random.RandomState(seed)
    M = len(present)
    lengths = split_lengths(N)
    L, B, P = max(lengths), len(lengths), S
    q = np.zeros((L, B, P), np.float32)
    for b, n in enumerate(lengths):
        q[np.arange(n), b, rs.randint(0, P, size=n)] = 1
    q[0, 0, :] = 0                                        # all-zero row: speaker 0
    lo = P // 2 if P > 2 else 0
    if lengths[0] > 1 and P > 1:
        q[1, 0, :] = 0
        q[1, 0, lo] = q[1, 0, P - 1] = 0.5                # a tie: the first maximum counts
        if P > 2:
            q[1, 0, 0] = 0.25
    idx = flat_index(lengths, L, B, torch.device("cpu")).numpy()
    spk = np.argmax(q.reshape(L * B, P)[idx], axis=-1)    # numpy: the first maximum, as torch.argmax
    assert spk[0] == 0 and (lengths[0] < 2 or P < 2 or spk[1] == lo)
    return dict(present=present, M=M, N=N, D=D, S=S, P=P, lengths=lengths, q=q, idx=idx, spk=spk,
                X=rs.randn(M, N, D).astype(np.float32), dY=rs.randn(M, N, D).astype(np.float32),
                speaker=rs.randn(S, D).astype(np.float32) if with_speaker and 'l' in present else None,
                modal=rs.randn(3, D).astype(np.float32) if with_modal else None)


def forward_ref(c):
    """float32 numpy, the reference's order: (x + speaker[s]) + modal[2]."""
    Y = c["X"].copy()
    for i, m in enumerate(c["present"]):
        if m == 'l' and c["speaker"] is not None:
            Y[i] = Y[i] + c["speaker"][c["spk"]]
        if c["modal"] is not None:
            Y[i] = Y[i] + c["modal"][ROW[m]][None, :]
    return Y


def backward_ref(c):
    """float64 sums, their sums of magnitudes and row counts: (dspeaker, |.|, n), (dmodal, |.|, n)."""
    dY = c["dY"].astype(np.float64)
    S, D, N = c["S"], c["D"], c["N"]
    sp = mo = None
    if c["speaker"] is not None:
        l = c["present"].index('l')
        ds, mag, cnt = np.zeros((S, D)), np.zeros((S, D)), np.zeros(S)
        for s in range(S):
            sel = c["spk"] == s
            ds[s], mag[s], cnt[s] = dY[l][sel].sum(0), np.abs(dY[l][sel]).sum(0), sel.sum()
        sp = (ds, mag, cnt)
    if c["modal"] is not None:
        dm, mag, cnt = np.zeros((3, D)), np.zeros((3, D)), np.zeros(3)
        for i, m in enumerate(c["present"]):
            dm[ROW[m]], mag[ROW[m]], cnt[ROW[m]] = dY[i].sum(0), np.abs(dY[i]).sum(0), N
        mo = (dm, mag, cnt)
    return sp, mo


def dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_forward(c, X=None, Y=None):
    """The C entry point; returns (code, Y, spk)."""
    X = dev(c["X"]) if X is None else X
    Y = torch.full_like(X, float("nan")) if Y is None else Y
    spk = torch.full((c["N"],), -7, dtype=torch.int32, device=DEV)
    speaker, modal = dev(c["speaker"]), dev(c["modal"])
    q, idx = dev(c["q"]), dev(c["idx"])
    rows = [ROW[m] for m in c["present"]]
    l_slot = c["present"].index('l') if 'l' in c["present"] else -1
    rc = _hip.call("mmdfn_graph_embed_fwd", _hip.ptr(X), _hip.ptr(q), _hip.ptr(idx), _hip.ptr(speaker), _hip.ptr(modal),
                   _hip.int_array(rows), l_slot, _hip.ptr(Y), _hip.ptr(spk), c["M"], c["N"], c["D"], c["P"], c["S"],
                   c["q"].shape[0] * c["q"].shape[1], _hip.stream(), allow=(-1, -2))
    torch.cuda.synchronize()
    return rc, Y, spk


def raw_backward(c, spk, dY=None):
    dY = dev(c["dY"]) if dY is None else dY
    nan = float("nan")
    dspk = torch.full((c["S"], c["D"]), nan, device=DEV) if c["speaker"] is not None else None
    dmod = torch.full((3, c["D"]), nan, device=DEV) if c["modal"] is not None else None
    rows = [ROW[m] for m in c["present"]]
    l_slot = c["present"].index('l') if 'l' in c["present"] else -1
    rc = _hip.call("mmdfn_graph_embed_bwd", _hip.ptr(dY), _hip.ptr(spk), _hip.ptr(dspk), _hip.ptr(dmod), _hip.int_array(rows),
                   l_slot, c["M"], c["N"], c["D"], c["S"], _hip.stream(), allow=(-1, -2))
    torch.cuda.synchronize()
    return rc, dspk, dmod


def check_case(c):
    tag = "%s N=%d D=%d S=%d" % (c["present"], c["N"], c["D"], c["S"])
    rc, Y, spk = raw_forward(c)
    assert rc == 0, tag
    assert torch.equal(Y.cpu(), torch.from_numpy(forward_ref(c))), tag
    if c["speaker"] is not None:
        assert torch.equal(spk.cpu(), torch.from_numpy(c["spk"].astype(np.int32))), tag
    if c["speaker"] is None and c["modal"] is None:
        return
    rc, dspk, dmod = raw_backward(c, spk)
    assert rc == 0, tag
    sp, mo = backward_ref(c)
    for name, got, ref in (("dspeaker", dspk, sp), ("dmodal", dmod, mo)):
        if ref is None:
            continue
        want, mag, cnt = ref
        got64 = got.cpu().double().numpy()
        assert not np.isnan(got64).any(), (tag, name)
        bound = (cnt[:, None] + 1) * 2.0 ** -24 * mag
        worst = float((np.abs(got64 - want) / np.maximum(bound, 1e-300)).max()) if (cnt > 0).any() else 0.0
        print("%-32s %-8s worst |got - ref64| / bound %.3f" % (tag, name, worst))
        assert (np.abs(got64 - want) <= bound).all(), (tag, name, worst)
        assert (got64[cnt == 0] == 0.0).all(), (tag, name)       # no utterance / absent modality: exactly zero
    rc, dspk2, dmod2 = raw_backward(c, spk)
    for a, b in ((dspk, dspk2), (dmod, dmod2)):
        assert a is None or torch.equal(a, b), tag              # bit-reproducible


# ---- the raw entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("present", ["avl", "al", "av"])
@pytest.mark.parametrize("D", [200, 4, 12])
def test_kernels_against_cpu_references(present, D):
    """N = 1 and one below, at and one above the backward launch's row-group count; S = 1 and 9 (all-zero row and tie in every
    case that has room for them); 'al': l in slot 1; 'av': no speaker part, the speaker table is NULL."""
    R = ops_embed.backward_rows()
    for N in (1, R - 1, R, R + 1):
        for S in (1, 9):
            check_case(make_case(present, N, D, S, 100 + N + S))


def test_forward_workgroup_boundary_and_speaker_limits():
    """One below, at and one above a forward workgroup's 16-byte lanes (D = 4: one lane per row), more rows than three backward
    passes, and the largest speaker table of the LDS sums."""
    T = ops_embed.forward_threads()
    for N in (T // 2 - 1, T // 2, T // 2 + 1):
        check_case(make_case("al", N, 4, 2, 7 + N))
    check_case(make_case("avl", 3 * ops_embed.backward_rows() + 5, 200, ops_embed.max_speakers(), 9))


@pytest.mark.parametrize("with_speaker,with_modal", [(True, False), (False, True)])
def test_each_table_null_in_turn(with_speaker, with_modal):
    for present in ("avl", "al"):
        check_case(make_case(present, 70, 200, 3, 21, with_speaker, with_modal))


def test_uncovered_shapes_answer_minus_two_and_launch_nothing():
    c = make_case("avl", 9, 6, 2, 31)                     # D % 4 != 0
    rc, Y, spk = raw_forward(c)
    assert rc == -2 and bool(torch.isnan(Y).all()) and bool((spk == -7).all())
    rc, dspk, dmod = raw_backward(c, torch.zeros(9, dtype=torch.int32, device=DEV))
    assert rc == -2 and bool(torch.isnan(dspk).all()) and bool(torch.isnan(dmod).all())
    c = make_case("avl", 9, 8, 2, 32)                     # a view offset by one float
    buf = torch.zeros(c["M"] * 9 * 8 + 1, device=DEV)
    off = buf[1:].view(c["M"], 9, 8)
    off.copy_(dev(c["X"]))
    rc, Y, _ = raw_forward(c, X=off)
    assert rc == -2 and bool(torch.isnan(Y).all())
    rc, _, _ = raw_forward(c, Y=off)
    assert rc == -2
    rc, dspk, dmod = raw_backward(c, torch.zeros(9, dtype=torch.int32, device=DEV), dY=off)
    assert rc == -2 and bool(torch.isnan(dspk).all())
    c = make_case("avl", 9, 8, ops_embed.max_speakers() + 1, 33)
    assert raw_forward(c)[0] == -2
    # the operator takes its torch path for them: same values, gradients through autograd
    for c, X in ((make_case("avl", 9, 6, 2, 31), None), (make_case("avl", 9, 8, 2, 32), off)):
        X = (dev(c["X"]) if X is None else X).requires_grad_(True)
        sw, mw = dev(c["speaker"]).requires_grad_(True), dev(c["modal"]).requires_grad_(True)
        Y = ops.graph_embeddings(X, dev(c["q"]), dev(c["idx"]), sw, mw, c["present"])
        assert torch.equal(Y.detach().cpu(), torch.from_numpy(forward_ref(c)))
        (Y * dev(c["dY"])).sum().backward()
        sp, mo = backward_ref(c)
        assert np.abs(sw.grad.cpu().numpy() - sp[0]).max() < 1e-5 and np.abs(mw.grad.cpu().numpy() - mo[0]).max() < 1e-5
        assert torch.equal(X.grad, dev(c["dY"]))


def test_more_parties_than_speakers_is_refused():
    c = make_case("avl", 9, 8, 3, 41)
    c["speaker"], c["S"] = c["speaker"][:2], 2            # P = 3 > S = 2
    assert raw_forward(c)[0] == -1
    with pytest.raises(ValueError):
        ops.graph_embeddings(dev(c["X"]), dev(c["q"]), dev(c["idx"]), dev(c["speaker"]), dev(c["modal"]), "avl")


# ---- the operator -------------------------------------------------------------------------------------------------------------------
def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # (device activity only: the runtime's own calls, hipLaunchKernel / hipDeviceSynchronize, are listed next to the kernels)
    return [e.key for e in prof.key_averages() if not e.key.startswith("hip") for _ in range(e.count)]


def test_operator_gradients_and_launch_count():
    """ops.graph_embeddings: bit-equal to the torch adds of MM_GCN.forward, dX is dY, a table that is not used gets no gradient,
    and the site is ONE launch each way."""
    c = make_case("avl", 70, 200, 3, 51)
    X = dev(c["X"]).requires_grad_(True)
    sw, mw = dev(c["speaker"]).requires_grad_(True), dev(c["modal"]).requires_grad_(True)
    q, idx, G = dev(c["q"]), dev(c["idx"]), dev(c["dY"])
    out = {}

    def fwd():
        out["Y"] = ops.graph_embeddings(X, q, idx, sw, mw, "avl")

    def bwd():
        out["g"] = torch.autograd.grad(out["Y"], (X, sw, mw), G)
    names = kernel_names(fwd)
    assert len(names) == 1 and "graph_embed_fwd_kernel" in names[0], names
    names = kernel_names(bwd)
    assert len(names) == 1 and "graph_embed_bwd_kernel" in names[0], names
    # the torch path of MM_GCN.forward on separate tensors
    a, v, l = (dev(c["X"][i]) for i in range(3))
    s = torch.argmax(torch.cat([q[:n, b] for b, n in enumerate(c["lengths"])], 0), -1)
    l = l + sw.detach()[s]
    want = torch.stack([a + mw.detach()[0].reshape(1, -1), v + mw.detach()[1].reshape(1, -1), l + mw.detach()[2].reshape(1, -1)])
    assert torch.equal(out["Y"].detach(), want)
    assert out["g"][0].data_ptr() == G.data_ptr()                    # dX is dY itself
    sp, mo = backward_ref(c)
    assert np.abs(out["g"][1].cpu().numpy() - sp[0]).max() < 1e-4 and np.abs(out["g"][2].cpu().numpy() - mo[0]).max() < 1e-4
    # unused tables: no gradient at all (what the reference leaves: .grad is None)
    Xav = dev(c["X"][:2]).requires_grad_(True)
    Y = ops.graph_embeddings(Xav, q, idx, sw, None, "av")
    assert Y is Xav                                                  # nothing to add
    sw.grad = mw.grad = None
    Y = ops.graph_embeddings(Xav, q, idx, sw, mw, "av")
    (Y * G[:2]).sum().backward()
    assert sw.grad is None and mw.grad is not None and float(mw.grad[2].abs().max()) == 0.0
    sw.grad = mw.grad = None
    Y = ops.graph_embeddings(X, q, idx, sw, None, "avl")
    (Y * G).sum().backward()
    assert mw.grad is None and sw.grad is not None


# ---- the module against the reference ------------------------------------------------------------------------------------------------
def restatement(sd, xs, present, lengths, qmask, G, dtype):
    """model_mm.MM_GCN.forward with use_speaker / use_modal, reason_flag=True, no dropout, in ``dtype`` on the CPU: the
    embeddings in the reference's order in front of the oracle's restated graph + stack.  Returns (results, pre-activations)."""
    params = {"graph_model." + k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    spk_w = params["graph_model.speaker_embeddings.weight"].requires_grad_(True)
    mod_w = params["graph_model.modal_embeddings.weight"].requires_grad_(True)
    xs = {m: xs[m].detach().cpu().to(dtype).requires_grad_(True) for m in present}
    s = torch.argmax(torch.cat([qmask[:n, b] for b, n in enumerate(lengths)], 0), -1)
    feats = []
    for m in present:
        x = xs[m]
        if m == 'l':
            x = x + spk_w[s]
        feats.append(x + mod_w[ROW[m]].reshape(1, -1))
    probe = O.ReluProbe()
    prev = O.set_relu_probe(probe)
    try:
        out = O.mm_gcn(feats, lengths, params, O.default_cfg(2, lamda=0.5, alpha=0.2))
    finally:
        O.set_relu_probe(prev)
    (out * G.cpu().to(dtype)).sum().backward()
    res = {"out": out.detach(), "dmodal": mod_w.grad}
    if 'l' in present:
        res["dspeaker"] = spk_w.grad
    res.update({"dx_" + m: xs[m].grad for m in present})
    return res, list(probe.pre.values())


def near_kink(pres, band=1e-5):
    n = sum(int((p.abs() < band * p.abs().amax(1, keepdim=True)).sum()) for p in pres)
    return n / sum(p.numel() for p in pres)


def run_module(m, xs, present, lengths, qmask, G):
    m.zero_grad(set_to_none=True)
    feats = torch.stack([xs[k] for k in present], 0).to(DEV).requires_grad_(True)
    out = m.forward_stacked(feats, lengths, qmask.to(DEV))
    (out * G.to(DEV)).sum().backward()
    res = {"out": out.detach(), "dmodal": m.modal_embeddings.weight.grad, "dspeaker": m.speaker_embeddings.weight.grad}
    res.update({"dx_" + k: feats.grad[i] for i, k in enumerate(present)})
    return res


def check(name, got, want64, want32):
    e, e32 = err(got, want64), err(want32, want64)
    msg = "%-28s device %.3e  float32 CPU %.3e  ratio %.2f" % (name, e, e32, e / max(e32, EPS_HALF))
    print(msg)
    assert e <= 4 * max(e32, EPS_HALF), msg


def module(D, H, present, P=3):
    return MM_GCN(D, D, D, D, 2, H, 6, 0.0, 0.5, 0.2, True, True, True, n_speakers=P, modals=list(present), use_speaker=True,
                  use_modal=True, reason_flag=True)


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(GOLD, "mm_gcn_embeddings.npz"), allow_pickle=False)
    return {k: torch.from_numpy(g[k]) for k in g.files}


@pytest.mark.parametrize("present", ["avl", "al", "av"])
def test_forward_stacked_against_the_reference_golden(gold, present):
    lengths = [int(n) for n in gold["dia_len"]]
    sd = {k[len("sd/"):]: v for k, v in gold.items() if k.startswith("sd/")}
    case = {k[len(present) + 1:]: v for k, v in gold.items() if k.startswith(present + "/")}
    xs, G, qmask = {m: case["x_" + m] for m in present}, case["G"], gold["qmask"]
    D, H = xs[present[0]].shape[1], 8
    # (the golden's dropout of 1e-12 keeps every element and its scale is 1 in float32: p = 0 here)
    m = module(D, H, present)
    m.load_state_dict(sd)
    got = run_module(m.to(DEV).train(), xs, present, lengths, qmask, G)
    r64, pres = restatement(sd, xs, present, lengths, qmask, G, torch.float64)
    assert near_kink(pres) == 0.0
    want = {k: case[k] for k in ["out", "dmodal"] + ["dx_" + k for k in present]}
    assert tuple(got["out"].shape) == (sum(lengths), len(present) * (D + H))
    if 'l' in present:
        want["dspeaker"] = case["dspeaker"]
    else:
        assert "dspeaker" not in case and got["dspeaker"] is None          # the reference leaves .grad None, so does the device
    absent = [ROW[k] for k in "avl" if k not in present]
    for r in absent:
        assert float(case["dmodal"][r].abs().max()) == 0.0 and float(got["dmodal"][r].abs().max()) == 0.0
    for k in want:
        check("MM_GCN %s %s" % (present, k), got[k], r64[k], want[k])


def test_forward_stacked_at_model_size_against_float64():
    """(D, H) = (200, 100), lengths [33, 1, 64], nine parties: the float32 CPU restatement is the yardstick.  The seed is the
    first whose float64 pre-activations all stay out of the ReLU band (chosen on the CPU, before anything runs on the device)."""
    lengths, present, D, H, P = [33, 1, 64], "avl", 200, 100, 9
    N, L, B = sum(lengths), max(lengths), len(lengths)
    for seed in range(200):
        torch.manual_seed(seed)
        m = module(D, H, present, P)
        g = torch.Generator().manual_seed(seed + 1)
        xs = {k: torch.randn(N, D, generator=g) for k in present}
        G = torch.randn(N, 3 * (D + H), generator=g)
        qmask = torch.zeros(L, B, P)
        for b, n in enumerate(lengths):
            qmask[torch.arange(n), b, torch.randint(0, P, (n,), generator=g)] = 1
        sd = m.state_dict()
        r64, pres = restatement(sd, xs, present, lengths, qmask, G, torch.float64)
        if near_kink(pres) == 0.0:
            break
    else:
        raise AssertionError("no seed keeps the pre-activations out of the ReLU band")
    r32, _ = restatement(sd, xs, present, lengths, qmask, G, torch.float32)
    got = run_module(m.to(DEV).train(), xs, present, lengths, qmask, G)
    print("seed", seed)
    for k in r64:
        check("MM_GCN (200, 100) " + k, got[k], r64[k], r32[k])
