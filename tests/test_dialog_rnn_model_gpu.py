"""GPU: DialogRNNModel (recurrent_models.py: two DialogueRNN encoders on K17 + masked matching attention on K14) and
MaskedNLLLoss (K15) against goldens exported from the reference (tests/golden/make_golden_dialog_rnn_model.py) and against the
float64 restatement of the model (tests/dialogue_rnn_ref.py, which reproduces every golden array: test_dialog_rnn_model_host.py).

Tolerances.  Reference goldens: tests/test_lstm_model_gpu.py's figures (outputs 1e-4 absolute, losses 1e-5, digests and stored
gradient rows 2e-4 relative).  Float64: not a figure fixed in advance -- per quantity the error of a float32 CPU run of the
restatement against the float64 run on the same case (e_f32) is measured, and the device may err by 3 x that.  Both figures are
printed per quantity (pytest -s) and kept in profiles/dialog_rnn_model.md."""
import os

import numpy as np
import pytest
import torch

import dialogue_rnn_ref as DR
from mm_dfn_amd import DialogRNNModel, MaskedNLLLoss, ops, ops_flags, synthetic, train
from mm_dfn_amd.optim import FlatAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24
FACTOR = 3.0


def err_max(got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    return float((got - want).abs().max())


def build(name, seed, dropout=0.0, dropout_rec=0.0, rec_site=None):
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    m = DialogRNNModel(D_m, DR.D_G, DR.D_P, DR.D_E, DR.D_H, n_classes=C, context_attention=kind, dropout_rec=dropout_rec,
                       dropout=dropout, att2=att2)
    m.dropout_rec.p = 0.0 if rec_site is None else rec_site       # (the constructor gives this site dropout + 0.15)
    sd = synthetic.seeded_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    return m.to(DEV), sd, DR.case_inputs(name, seed + 1)


def flat_logp(log_prob):
    return log_prob.transpose(0, 1).contiguous().view(-1, log_prob.shape[2])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "dialog_rnn_model.npz"), allow_pickle=False)


def restatement(name, sd, inputs, dtype, **kw):
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    U, qmask, umask, label, weight = inputs
    prm = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    lp, alpha, emotions, af, ab = DR.forward_any(prm, U, qmask, umask, kind, att2, **kw)
    l1 = DR.masked_nll(flat_logp(lp), label, umask)
    l2 = DR.masked_nll(flat_logp(lp), label, umask, weight)
    l2.backward()
    out = dict(log_prob=lp.detach(), emotions=emotions.detach(), alpha_f=af, alpha_b=ab, loss_plain=torch.tensor(l1.item(), dtype=torch.float64),
               loss_weighted=torch.tensor(l2.item(), dtype=torch.float64))
    if alpha is not None:
        out["alpha"] = alpha.detach()
    out.update({"grad " + k: p.grad for k, p in prm.items() if p.grad is not None and float(p.grad.abs().max()) > 0})
    return out


@pytest.fixture(scope="module")
def cpu_results():
    """name -> (float64 run, float32 run) of the restatement on the golden cases, computed once."""
    seed = int(np.load(os.path.join(GOLD, "dialog_rnn_model.npz"))["seed"])
    out = {}
    for name, (kind, D_m, T, lengths, P, C, att2) in DR.CASES.items():
        sd = synthetic.seeded_state_dict(DialogRNNModel(D_m, 150, 150, 100, DR.D_H, n_classes=C, context_attention=kind,
                                                        att2=att2).state_dict(), seed)
        inputs = DR.case_inputs(name, seed + 1)
        out[name] = (restatement(name, sd, inputs, torch.float64), restatement(name, sd, inputs, torch.float32))
    return out


def against_float64(tag, got, r64, r32):
    """Every quantity of ``r64``: the device's max error must be <= FACTOR x the float32 run's.  Prints both."""
    bad = {}
    for k, want in r64.items():
        e_dev, e_f32 = err_max(got[k], want), err_max(r32[k], want)
        print("DRNN-MODEL %s %-58s err_device=%.3g err_f32cpu=%.3g ratio=%.2f" % (tag, k, e_dev, e_f32, e_dev / e_f32 if e_f32 else
                                                                                 float("inf") if e_dev else 0.0), flush=True)
        if not e_dev <= FACTOR * e_f32:
            bad[k] = (e_dev, e_f32)
    return bad


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_golden_cases_and_float64(name, golden, cpu_results):
    g = golden
    seed = int(g["seed"])
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    B = len(lengths)
    m, sd, (U, qmask, umask, label, weight) = build(name, seed)
    U, qmask, umask, label, weight = [t.to(DEV) for t in (U, qmask, umask, label, weight)]
    r64, r32 = cpu_results[name]
    # ---- eval: outputs
    m.eval()
    with torch.no_grad():
        log_prob, alpha, af, ab, emotions = m(U, qmask, umask)
    assert tuple(log_prob.shape) == (T, B, C) and len(af) == len(ab) == T - 1
    assert all(tuple(a.shape) == (B, t + 1) for t, a in enumerate(af)) and all(tuple(a.shape) == (B, t + 1) for t, a in enumerate(ab))
    got = dict(log_prob=log_prob, emotions=emotions, alpha_f=DR.pack_alpha(af, T, B), alpha_b=DR.pack_alpha(ab, T, B))
    assert np.abs(log_prob.cpu().numpy() - g[name + "/log_prob"]).max() < 1e-4
    assert np.abs(emotions.cpu().numpy() - g[("a" if name == "c" else name) + "/emotions"]).max() < 1e-4
    assert np.abs(got["alpha_f"].numpy() - g[name + "/alpha_f"]).max() < 1e-4
    assert np.abs(got["alpha_b"].numpy() - g[name + "/alpha_b"]).max() < 1e-4
    for b, n in enumerate(lengths):        # reverse rows beyond a length are exactly zero
        assert float(emotions[n:, b, DR.D_E:].abs().max()) == 0.0 if n < T else True
    if att2:
        assert len(alpha) == T and tuple(alpha[0].shape) == (B, T)
        got["alpha"] = torch.stack(alpha)
        assert np.abs(got["alpha"].cpu().numpy() - g[name + "/alpha"]).max() < 1e-4
    else:
        assert alpha == []
    # ---- train mode (dropout 0): losses and gradients
    m.train()
    log_prob = m(U, qmask, umask)[0]
    plain = MaskedNLLLoss()(flat_logp(log_prob), label.view(-1), umask)
    assert abs(plain.item() - float(g[name + "/loss_plain"])) < 1e-5
    loss = MaskedNLLLoss(weight)(flat_logp(log_prob), label.view(-1), umask)
    assert abs(loss.item() - float(g[name + "/loss_weighted"])) < 1e-5
    got["loss_plain"], got["loss_weighted"] = plain.detach(), loss.detach()
    train.backward(loss)
    ops.join_weight_grads()
    grads = {k: p.grad for k, p in m.named_parameters()}
    for k, gr in grads.items():
        key = name + "/digest/" + k
        if key in g.files:
            want = g[key]
            assert gr is not None, k
            assert abs(DR.digest(gr)[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
            got["grad " + k] = gr
        else:                                                       # (att2=False: the attention's transform is not on the path)
            assert k.startswith("matchatt.") and (gr is None or float(gr.abs().max()) == 0.0), k
    stored = [x[len(name) + 6:] for x in g.files if x.startswith(name + "/grad/")]
    assert len(stored) == 4
    for k in stored:
        want = g[name + "/grad/" + k]
        assert np.abs(grads[k][::DR.GRAD_ROWS[k][name]].cpu().numpy() - want).max() / np.abs(want).max() < 2e-4, k
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    bad = against_float64(name, got, r64, r32)
    assert not bad, bad


def test_dropout_step_against_float64_on_replayed_flags():
    """dropout 0.3, dropout_rec 0.2: the keep flags of every site are read from the tap and replayed in the restatement (float64
    and float32); log_prob and every gradient are compared under the 3 x rule, and every tapped draw is used exactly once."""
    name, p, p_rec = "a", 0.3, 0.2
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    B = len(lengths)
    m, sd, inputs = build(name, 21, dropout=p, dropout_rec=p_rec, rec_site=p + 0.15)
    U, qmask, umask, label, weight = inputs
    m.train()
    torch.manual_seed(5)
    ops_flags.TAP = []
    try:
        log_prob = m(U.to(DEV), qmask.to(DEV), umask.to(DEV))[0]
        draws, ops_flags.TAP = ops_flags.TAP, None
    finally:
        ops_flags.TAP = None
    loss = MaskedNLLLoss(weight.to(DEV))(flat_logp(log_prob), label.view(-1).to(DEV), umask.to(DEV))
    train.backward(loss)
    ops.join_weight_grads()
    sizes = {"drnn_g": T * B * DR.D_G, "drnn_q": T * B * DR.D_P, "drnn_e": T * B * DR.D_E, "drnn_rec": T * B * DR.D_E}
    assert sorted((site, n) for n, pp, t, site in draws) == sorted([(s, n) for s, n in sizes.items() for _ in range(2)] +
                                                                   [("head", T * B * DR.D_H)])
    flags = {}
    for n, pp, t, site in draws:
        assert pp == pytest.approx({"head": p, "drnn_rec": p + 0.15}.get(site, p_rec)), site
        f = t.detach().cpu()
        assert set(f.unique().tolist()) <= {0.0, 1.0} and abs(float(f.mean()) - (1 - pp)) < 0.1, site
        flags.setdefault(site, []).append(f)
    keeps = [{k: flags["drnn_" + k][d].view(T, B, -1) for k in ("g", "q", "e")} for d in range(2)]
    rec_keep = [f.view(T, B, DR.D_E) for f in flags["drnn_rec"]]
    kw = dict(keeps=keeps, p_rec=p_rec, rec_keep=rec_keep, p_out=p + 0.15, head_keep=flags["head"][0], p=p)
    r64 = restatement(name, sd, inputs, torch.float64, **kw)
    r32 = restatement(name, sd, inputs, torch.float32, **kw)
    got = {"log_prob": log_prob}
    got.update({"grad " + k: prm.grad for k, prm in m.named_parameters()})
    keys = ["log_prob"] + [k for k in r64 if k.startswith("grad ")]
    assert len(keys) == 1 + len(list(m.parameters()))
    bad = against_float64("dropout", got, {k: r64[k] for k in keys}, r32)
    assert not bad, bad


def test_training_step_runs_the_fused_recurrence_and_no_library_gemm():
    """Every dense product of a DialogRNNModel training step runs on this package's kernels: drnn_seq_fwd / drnn_seq_bwd in the
    device trace, no Tensile (`Cijk_*`) kernel, no ATen matmul and no MIOpen recurrence, for both attention kinds."""
    from torch.profiler import ProfilerActivity, profile
    for name in ("a", "b"):
        m, sd, (U, qmask, umask, label, weight) = build(name, 4, dropout=0.1, dropout_rec=0.1, rec_site=0.25)
        m.train()
        U, qmask, umask, label = [t.to(DEV) for t in (U, qmask, umask, label)]
        loss_f = MaskedNLLLoss()

        def step():
            m.zero_grad(set_to_none=True)
            train.backward(loss_f(flat_logp(m(U, qmask, umask)[0]), label.view(-1), umask))
            ops.join_weight_grads()
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.key for e in prof.key_averages()]
        assert sum("drnn_seq_fwd" in n for n in names) == 1 and sum("drnn_seq_bwd" in n for n in names) == 1, names
        assert any("match_att_" in n for n in names) and any("masked_nll" in n for n in names), names
        bad = [n for n in names if n.startswith("Cijk_") or ("gemm" in n.lower() and "gemm_tn" not in n)
               or "miopen" in n.lower() or "bmm" in n.lower()]
        assert not bad, names


class _Loader(list):
    pass


def test_three_steps_of_train_or_eval_model_with_flat_adam_against_float64_adam():
    """As tests/test_lstm_model_gpu.py's three-step comparison (the reference script's Adam, lr 3e-4, weight_decay 1e-4): the
    same three steps run in the restatement on the CPU in float64 and float32 with torch.optim.Adam, and per parameter the
    device's error against float64 must be <= 4 err_f32cpu + 8 u max|want| (that test's calibration rule).  Both errors are
    printed per tensor (profiles/dialog_rnn_model.md)."""
    name = "a"
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    m, sd, _ = build(name, 9)
    batches = [DR.case_inputs(name, 100 + i) for i in range(3)]
    loader = _Loader([(U, U[:, :, :4], U[:, :, :4], qmask, umask, label, ["v%d" % i]) for i, (U, qmask, umask, label, _) in
                      enumerate(batches)])
    weight = batches[0][4]
    opt = FlatAdam(m, lr=3e-4, weight_decay=1e-4)
    res = train.train_or_eval_model(m, MaskedNLLLoss(weight.to(DEV)), loader, 0, True, opt, cuda_flag=True,
                                    target_names=["c%d" % i for i in range(C)])
    assert len(res) == 9 and res[8] == [[], [], [], []]

    def cpu_steps(dtype):
        prm = {k: torch.nn.Parameter(v.to(dtype).clone()) for k, v in sd.items()}
        ref_opt = torch.optim.Adam(list(prm.values()), lr=3e-4, weight_decay=1e-4)
        losses, counts = [], []
        for U, qmask, umask, label, _ in batches:
            ref_opt.zero_grad()
            lp = DR.forward_any(prm, U, qmask, umask, kind, att2)[0]
            loss = DR.masked_nll(flat_logp(lp), label, umask, weight)
            loss.backward()
            ref_opt.step()
            losses.append(loss.item())
            counts.append(float(umask.sum()))
        return prm, losses, counts
    P64, losses, counts = cpu_steps(torch.float64)
    P32, _, _ = cpu_steps(torch.float32)
    got = m.state_dict()
    bad = {}
    for k in P64:
        want = P64[k].detach()
        top = float(want.abs().max())
        e_dev = float((got[k].detach().double().cpu() - want).abs().max())
        e_f32 = float((P32[k].detach().double() - want).abs().max())
        print("DRNN-ADAM3 %-58s err_device=%.3g err_f32cpu=%.3g max|want|=%.3g" % (k, e_dev, e_f32, top), flush=True)
        if not e_dev <= 4 * e_f32 + 8 * U32 * top:
            bad[k] = (e_dev, e_f32, top)
    assert not bad, bad
    want_loss = round(sum(l * c for l, c in zip(losses, counts)) / sum(counts), 4)
    assert abs(res[2] - want_loss) <= 1.0001e-4
    # an evaluation pass returns the attention weights of every batch, the encoders' included
    ev = train.train_or_eval_model(m, MaskedNLLLoss(weight.to(DEV)), loader, 0, False, None, cuda_flag=True)
    assert len(ev[8][0]) == 3 * T and len(ev[8][1]) == len(ev[8][2]) == 3 * (T - 1) and ev[8][3] == ["v0", "v1", "v2"]


def test_dialogue_model_bits_unchanged_around_a_dialog_rnn_model_forward():
    """The DialogueGNNModel cfg of test_variants_gpu.CASES['avl_lstm'] gives the same bits before and after a DialogRNNModel
    forward + backward in the same process (shared flag pool, weight-gradient queue, plane registry)."""
    import test_variants_gpu as V
    dm, b = V.build("avl_lstm")
    dm = dm.to(DEV).eval()
    run = lambda: dm(b["textf"].to(DEV), b["qmask"].to(DEV), b["umask"].to(DEV), b["lengths"], b["acouf"].to(DEV),
                     b["visuf"].to(DEV))[0]
    with torch.no_grad():
        before = run().clone()
    for name in ("a", "b"):
        m, sd, (U, qmask, umask, label, weight) = build(name, 2, dropout=0.3, dropout_rec=0.2, rec_site=0.45)
        m.train()
        lp = m(U.to(DEV), qmask.to(DEV), umask.to(DEV))[0]
        train.backward(MaskedNLLLoss()(flat_logp(lp), label.view(-1).to(DEV), umask.to(DEV)))
        ops.join_weight_grads()
    with torch.no_grad():
        after = run()
    assert torch.equal(before, after)


@pytest.mark.parametrize("kind", ["simple", "general"])
def test_dialogue_rnn_on_its_own_against_float64(kind):
    """``DialogueRNN.forward(U, qmask)`` alone (one direction in the launch, every dialogue at full length, a plain
    ``loss.backward()``): e, the alpha list, dU and every parameter's gradient against the restatement's encoder.  These shapes
    are not the issue's golden cases, so the rule is the kernel tests' calibration: per quantity the device's max error against
    float64 must be <= 4 x a float32 CPU run's + 8 u max|want|."""
    from mm_dfn_amd import DialogueRNN
    T, B, P, D_m = 5, 3, 3, 8
    torch.manual_seed(11)
    m = DialogueRNN(D_m, DR.D_G, DR.D_P, DR.D_E, context_attention=kind, dropout=0.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    U, qmask, _, _, _ = DR.make_inputs(D_m, T, [T] * B, P, 3, 12, zero_rows=[(2, 0)])
    w = torch.from_numpy(np.random.RandomState(13).standard_normal((T, B, DR.D_E)).astype(np.float32))
    Ud = U.to(DEV).requires_grad_(True)
    e, alist = m(Ud, qmask.to(DEV))
    assert tuple(e.shape) == (T, B, DR.D_E) and len(alist) == T - 1 and all(tuple(a.shape) == (B, t + 1) for t, a in enumerate(alist))
    (e * w.to(DEV)).sum().backward()
    got = {"e": e, "alpha": DR.pack_alpha(alist, T, B), "dU": Ud.grad}
    got.update({"grad " + k: p.grad for k, p in m.named_parameters()})

    def run(dtype):
        prm = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        Ur = U.to(dtype).requires_grad_(True)
        e_r, alpha_r = DR.encoder(prm, "", Ur, qmask, [T] * B, kind)
        (e_r * w.to(dtype)).sum().backward()
        res = {"e": e_r.detach(), "alpha": alpha_r, "dU": Ur.grad}
        res.update({"grad " + k: p.grad for k, p in prm.items()})
        return res
    r64, r32 = run(torch.float64), run(torch.float32)
    assert set(got) == set(r64)
    bad = {}
    for k, want in r64.items():
        top = float(want.abs().max())
        e_dev, e_f32 = err_max(got[k], want), err_max(r32[k], want)
        print("DRNN-ALONE %s %-44s err_device=%.3g err_f32cpu=%.3g max|want|=%.3g" % (kind, k, e_dev, e_f32, top), flush=True)
        if not (top > 0 and e_dev <= 4 * e_f32 + 8 * U32 * top):
            bad[k] = (e_dev, e_f32, top)
    assert not bad, bad
    # an in-place change of a cell parameter between forward and backward is refused, not silently mixed
    e2 = m(U.to(DEV), qmask.to(DEV))[0]
    with torch.no_grad():
        m.dialogue_cell.e_cell.weight_hh.mul_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        e2.sum().backward()
