"""GPU: LSTMModel (recurrent_models.py: BiLSTM on K16 + masked matching attention on K14) and MaskedNLLLoss (K15) against goldens
exported from the reference (tests/golden/make_golden_lstm_model.py) and against the float64 restatement of the model
(tests/lstm_model_ref.py: an explicit float64 loop, not torch's LSTM).

Tolerances: reference goldens use tests/test_variants_gpu.py's figures (|log_prob| < 1e-4, loss < 1e-5, gradients and digests
< 2e-4 relative); float64 comparisons use tests/test_fusion_kernels_gpu.py's rel_max < 1e-5.  A float32 torch.nn.LSTM
restatement on the CPU meets every one of them with a factor 4 to spare (tests/test_lstm_model_host.py)."""
import os

import numpy as np
import pytest
import torch

import lstm_model_ref as LR
from mm_dfn_amd import LSTMModel, MaskedNLLLoss, ops, ops_flags, synthetic, train
from mm_dfn_amd.optim import FlatAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24


def rel_max(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    den = float(want.abs().max())
    if den == 0.0:
        return float(got.abs().max())
    return float((got - want).abs().max()) / den


def build(name, seed, dropout=0.0):
    D_m, L, lengths, C, att2 = LR.CASES[name]
    m = LSTMModel(D_m, LR.D_E, LR.D_H, n_classes=C, dropout=dropout, att2=att2)
    sd = synthetic.seeded_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    return m.to(DEV), sd, LR.case_inputs(name, seed + 1)


def flat_logp(log_prob):
    return log_prob.transpose(0, 1).contiguous().view(-1, log_prob.shape[2])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "lstm_model.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def float64_results():
    """name -> (log_prob, alpha, emotions, loss_plain, loss_weighted, gradients of the weighted loss), computed once."""
    seed = int(np.load(os.path.join(GOLD, "lstm_model.npz"))["seed"])
    out = {}
    for name, (D_m, L, lengths, C, att2) in LR.CASES.items():
        sd = synthetic.seeded_state_dict(LSTMModel(D_m, LR.D_E, LR.D_H, C, 0.0, att2).state_dict(), seed)
        P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        U, _, umask, label, weight = LR.case_inputs(name, seed + 1)
        lp, alpha, emotions = LR.forward64(P, U, umask, att2)
        l1 = LR.masked_nll(flat_logp(lp), label, umask)
        l2 = LR.masked_nll(flat_logp(lp), label, umask, weight)
        l2.backward()
        out[name] = (lp.detach(), None if alpha is None else alpha.detach(), emotions.detach(), l1.item(), l2.item(),
                     {k: p.grad for k, p in P.items()})
    return out


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_golden_cases_and_float64(name, golden, float64_results):
    g = golden
    seed = int(g["seed"])
    D_m, L, lengths, C, att2 = LR.CASES[name]
    m, sd, (U, qmask, umask, label, weight) = build(name, seed)
    U, qmask, umask, label, weight = [t.to(DEV) for t in (U, qmask, umask, label, weight)]
    lp64, alpha64, em64, l1_64, l2_64, grads64 = float64_results[name]
    # ---- eval: outputs
    m.eval()
    with torch.no_grad():
        log_prob, alpha, af, ab, emotions = m(U, qmask, umask)
    assert tuple(log_prob.shape) == (L, len(lengths), C) and af == [] and ab == []
    assert np.abs(log_prob.cpu().numpy() - g[name + "/log_prob"]).max() < 1e-4
    assert rel_max(log_prob, lp64) < 1e-5
    em_name = "a" if name == "c" else name
    assert np.abs(emotions.cpu().numpy() - g[em_name + "/emotions"]).max() < 1e-4
    assert rel_max(emotions, em64) < 1e-5
    if att2:
        assert len(alpha) == L and tuple(alpha[0].shape) == (len(lengths), L)
        assert np.abs(torch.stack(alpha).cpu().numpy() - g[name + "/alpha"]).max() < 1e-4
        assert rel_max(torch.stack(alpha), alpha64) < 1e-5
    else:
        assert alpha == []
    # ---- train mode (dropout 0): losses and gradients
    m.train()
    log_prob = m(U, qmask, umask)[0]
    plain = MaskedNLLLoss()(flat_logp(log_prob), label.view(-1), umask)
    assert abs(plain.item() - float(g[name + "/loss_plain"])) < 1e-5
    assert abs(plain.item() - l1_64) < 1e-5 * abs(l1_64)
    loss = MaskedNLLLoss(weight)(flat_logp(log_prob), label.view(-1), umask)
    assert abs(loss.item() - float(g[name + "/loss_weighted"])) < 1e-5
    assert abs(loss.item() - l2_64) < 1e-5 * abs(l2_64)
    train.backward(loss)
    ops.join_weight_grads()
    grads = {k: p.grad for k, p in m.named_parameters()}
    worst = {}
    for k, gr in grads.items():
        key = name + "/digest/" + k
        if key in g.files:
            want = g[key]
            assert gr is not None, k
            assert abs(LR.digest(gr)[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
            worst[k] = rel_max(gr, grads64[k])
        else:                                                       # (att2=False: the attention's transform is not on the path)
            assert k.startswith("matchatt.") and (gr is None or float(gr.abs().max()) == 0.0), k
    print("LSTM-MODEL %s worst gradient rel_max vs float64: %.3g (%s)" % (name, max(worst.values()), max(worst, key=worst.get)),
          flush=True)
    assert all(v < 1e-5 for v in worst.values()), {k: v for k, v in worst.items() if not v < 1e-5}
    stored = [x[len(name) + 6:] for x in g.files if x.startswith(name + "/grad/")]
    assert "lstm.weight_ih_l0" in stored and "linear.weight" in stored and (not att2 or "matchatt.transform.weight" in stored)
    for k in stored:
        want = g[name + "/grad/" + k]
        got = grads[k][::LR.GRAD_ROWS[k][name]].cpu().numpy()
        assert np.abs(got - want).max() / np.abs(want).max() < 2e-4, k


def test_dropout_step_against_float64_on_replayed_flags():
    """p = 0.5: the keep flags of the two dropout sites (between the LSTM layers, in front of smax_fc) are read from the tap and
    replayed in the float64 restatement; log_prob and every gradient are compared, and every tapped draw is used exactly once."""
    name, p = "a", 0.5
    D_m, L, lengths, C, att2 = LR.CASES[name]
    B = len(lengths)
    m, sd, (U, qmask, umask, label, weight) = build(name, 21, dropout=p)
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
    assert sorted((site, n) for n, pp, t, site in draws) == [("head", L * B * LR.D_H), ("lstm", L * B * 2 * LR.D_E)]
    assert all(pp == p for _, pp, _, _ in draws)
    used = {site: 0 for _, _, _, site in draws}
    flags = {}
    for n, pp, t, site in draws:
        flags[site] = t.detach().cpu()
        used[site] += 1
        kept = float(flags[site].mean())
        assert set(flags[site].unique().tolist()) <= {0.0, 1.0} and 0.35 < kept < 0.65, (site, kept)
    assert used == {"lstm": 1, "head": 1}
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    lp64, _, _ = LR.forward64(P, U, umask, att2, lstm_keep=flags["lstm"], head_keep=flags["head"], p=p)
    LR.masked_nll(flat_logp(lp64), label, umask, weight).backward()
    assert rel_max(log_prob, lp64) < 1e-5
    for k, prm in m.named_parameters():
        assert rel_max(prm.grad, P[k].grad) < 1e-5, k


def test_training_step_launches_no_library_gemm():
    """Every dense product of an LSTMModel training step runs on this package's kernels: no Tensile (`Cijk_*`) kernel, no ATen
    matmul and no MIOpen recurrence in the device trace, at D_m = 100 and 600."""
    from torch.profiler import ProfilerActivity, profile
    for name in ("a", "b"):
        m, sd, (U, qmask, umask, label, weight) = build(name, 4, dropout=0.1)
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
        assert any("lstm_seq_fwd" in n for n in names) and any("lstm_seq_bwd" in n for n in names), names
        assert any("match_att_" in n for n in names) and any("masked_nll" in n for n in names), names
        bad = [n for n in names if n.startswith("Cijk_") or ("gemm" in n.lower() and "gemm_tn" not in n)
               or "miopen" in n.lower() or "bmm" in n.lower()]
        assert not bad, names


class _Loader(list):
    pass


def test_three_steps_of_train_or_eval_model_with_flat_adam_against_float64_adam():
    """Optimizer settings: the reference script's own (run_train_erc.py:300-302,512: Adam, lr 3e-4, weight_decay 1e-4).  Adam
    divides every gradient entry by its own running magnitude, so what reaches a parameter is lr times the entry's RELATIVE
    error, and entries far below a tensor's typical gradient carry large relative errors in any float32 evaluation.  Nobody has
    measured what that leaves after three steps of this model, so the bound is not a figure: the same three steps run in a
    float32 torch restatement on the CPU (torch.nn.LSTM's kernels, torch.optim.Adam), and per parameter the device's error
    against float64 must be <= 4 err_f32cpu + 8 u max|want| (the calibration rule of tests/test_gru_recurrence_kernels_gpu.py).
    Both errors are printed per tensor (profiles/lstm_model.md).

    MEASURED (MI355X): all 22 tensors meet it; the tightest is lstm.weight_hh_l1_reverse, err_device 2.05e-07 against
    err_f32cpu 4.81e-08, max|want| 0.101: allowed 2.4e-07.  The figure is lr times the relative error of gradient entries near
    Adam's eps (this tensor's gradient spans 7.5e-12 .. 4.3e-04): the tail of a distribution.  With the GRU kernels' gate
    non-linearities on the hardware exp / rcp units, 1 - 2 / (1 + e^2x), the same tensor was at 6.60e-07 and missed: that form
    is accurate absolutely, not relatively, and most of g and tanh(c) is small here.  K16 therefore evaluates the gates with
    libm's tanhf / expf (csrc/lstm_seq.hip); over 8 seeds the device's figure is then 0.87-1.42 times the float32 restatement's
    in the median per tensor (profiles/lstm_model.md)."""
    name = "a"
    D_m, L, lengths, C, att2 = LR.CASES[name]
    m, sd, _ = build(name, 9)
    batches = [LR.case_inputs(name, 100 + i) for i in range(3)]
    loader = _Loader([(U, U[:, :, :4], U[:, :, :4], qmask, umask, label, ["v%d" % i]) for i, (U, qmask, umask, label, _) in
                      enumerate(batches)])
    weight = batches[0][4]
    opt = FlatAdam(m, lr=3e-4, weight_decay=1e-4)
    res = train.train_or_eval_model(m, MaskedNLLLoss(weight.to(DEV)), loader, 0, True, opt, cuda_flag=True,
                                    target_names=["c%d" % i for i in range(C)])
    assert len(res) == 9 and res[8] == [[], [], [], []]
    assert res[4].shape == res[5].shape == res[6].shape == (3 * L * len(lengths),)

    def cpu_steps(dtype):
        P = {k: torch.nn.Parameter(v.to(dtype).clone()) for k, v in sd.items()}
        ref_opt = torch.optim.Adam(list(P.values()), lr=3e-4, weight_decay=1e-4)
        losses, counts = [], []
        for U, qmask, umask, label, _ in batches:
            ref_opt.zero_grad()
            enc = None if dtype == torch.float64 else LR.torch_lstm_encoder(P)
            lp, _, _ = LR.forward_any(P, U, umask, att2, encoder=enc)
            loss = LR.masked_nll(flat_logp(lp), label, umask, weight)
            loss.backward()
            ref_opt.step()
            losses.append(loss.item())
            counts.append(float(umask.sum()))
        return P, losses, counts
    P64, losses, counts = cpu_steps(torch.float64)
    P32, _, _ = cpu_steps(torch.float32)
    got = m.state_dict()
    bad = {}
    for k in P64:
        want = P64[k].detach()
        top = float(want.abs().max())
        e_dev = float((got[k].detach().double().cpu() - want).abs().max())
        e_f32 = float((P32[k].detach().double() - want).abs().max())
        print("LSTM-ADAM3 %-32s err_device=%.3g err_f32cpu=%.3g max|want|=%.3g" % (k, e_dev, e_f32, top), flush=True)
        if not e_dev <= 4 * e_f32 + 8 * U32 * top:
            bad[k] = (e_dev, e_f32, top)
    assert not bad, bad
    want_loss = round(sum(l * c for l, c in zip(losses, counts)) / sum(counts), 4)
    assert abs(res[2] - want_loss) <= 1.0001e-4
    # an evaluation pass returns the attention weights of every batch
    ev = train.train_or_eval_model(m, MaskedNLLLoss(weight.to(DEV)), loader, 0, False, None, cuda_flag=True)
    assert len(ev[8][0]) == 3 * L and tuple(ev[8][0][0].shape) == (len(lengths), L) and ev[8][3] == ["v0", "v1", "v2"]


def test_dialogue_model_bits_unchanged_around_an_lstm_model_forward():
    """The DialogueGNNModel cfg of test_variants_gpu.CASES['avl_lstm'] gives the same bits before and after an LSTMModel
    forward + backward in the same process (shared flag pool, weight-gradient queue, plane registry)."""
    import test_variants_gpu as V
    dm, b = V.build("avl_lstm")
    dm = dm.to(DEV).eval()
    run = lambda: dm(b["textf"].to(DEV), b["qmask"].to(DEV), b["umask"].to(DEV), b["lengths"], b["acouf"].to(DEV),
                     b["visuf"].to(DEV))[0]
    with torch.no_grad():
        before = run().clone()
    for name in ("a", "b"):
        m, sd, (U, qmask, umask, label, weight) = build(name, 2, dropout=0.3)
        m.train()
        lp = m(U.to(DEV), qmask.to(DEV), umask.to(DEV))[0]
        train.backward(MaskedNLLLoss()(flat_logp(lp), label.view(-1).to(DEV), umask.to(DEV)))
        ops.join_weight_grads()
    with torch.no_grad():
        after = run()
    assert torch.equal(before, after)


def test_stacked_copy_fallback_and_pairing():
    """Parameters that an owner has laid out non-adjacently (marked as FlatAdam marks its slots) take a copied stacked operand
    for the input-gradient launch; the result equals the adjacent-view path's.  ``pair_lstm_weights`` pairs such a module."""
    from mm_dfn_amd import gru as fused_gru
    from mm_dfn_amd import lstm as fused
    name = "b"
    outs = []
    for flagged in (False, True):
        m, sd, (U, qmask, umask, label, weight) = build(name, 3)
        m.train()
        if flagged:
            for prm in m.lstm.parameters():
                prm._mmdfn_flat = True
            assert fused._stacked_view(m.lstm.weight_ih_l1, m.lstm.weight_ih_l1_reverse) is None
        else:
            assert fused.pair_lstm_weights(m) == 4 and fused_gru.pair_gru_weights(m) == 0
            assert fused._adjacent(m.lstm.weight_ih_l0, m.lstm.weight_ih_l0_reverse)
        lp = m(U.to(DEV), qmask.to(DEV), umask.to(DEV))[0]
        train.backward(MaskedNLLLoss()(flat_logp(lp), label.view(-1).to(DEV), umask.to(DEV)))
        ops.join_weight_grads()
        outs.append((lp.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert rel_max(outs[1][1][k], outs[0][1][k]) < 1e-5, k
