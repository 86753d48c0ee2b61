"""GPU: CNNFeatureExtractor (cnn_features.py on K18, csrc/cnn_features.hip) against goldens exported from the reference
(tests/golden/make_golden_cnn_features.py) and against the float64 restatement of the module (tests/cnn_features_ref.py), alone
and in front of LSTMModel + MaskedNLLLoss (golden case c).

Tolerances are tests/test_lstm_model_gpu.py's: against the reference's goldens |outputs| < 1e-4, the NLL loss < 1e-5, digests
and stored gradient rows < 2e-4 relative; against float64 rel_max < 1e-5 (outputs, losses, every gradient).  The "loss" of cases
a / b is sum(features G) with G > 0 scaled by 1 / G.numel(), a mean of non-negative terms of order 1: it takes the same absolute
1e-5 against the golden and relative 1e-5 against float64 as the NLL losses."""
import os

import numpy as np
import pytest
import torch

import cnn_features_ref as CR
import lstm_model_ref as LR
from mm_dfn_amd import CNNFeatureExtractor, LSTMModel, MaskedNLLLoss, ops, ops_flags, synthetic, train
from mm_dfn_amd.optim import FlatAdam

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_max(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    den = float(want.abs().max())
    if den == 0.0:
        return float(got.abs().max())
    return float((got - want).abs().max()) / den


def flat_logp(log_prob):
    return log_prob.transpose(0, 1).contiguous().view(-1, log_prob.shape[2])


def state(name, seed):
    """(extractor state_dict, LSTMModel state_dict or None, inputs) of a golden case, as the golden maker builds them."""
    c = CR.MODEL_CASES[name]
    inputs = CR.model_inputs(name, seed + 1)
    sd = synthetic.seeded_state_dict(CNNFeatureExtractor(*c["args"]).state_dict(), seed)
    if c["frozen"]:
        sd["embedding.weight"] = torch.from_numpy(inputs[6])
    lsd = None
    if c["lstm"]:
        lsd = synthetic.seeded_state_dict(LSTMModel(*CR.LSTM_ARGS, n_classes=CR.N_CLASSES, dropout=0.0).state_dict(), seed + 7)
    return sd, lsd, inputs


def build(name, seed, dropout=0.0):
    c = CR.MODEL_CASES[name]
    sd, lsd, inputs = state(name, seed)
    args = c["args"][:5] + (dropout,)
    cnn = CNNFeatureExtractor(*args)
    if c["frozen"]:
        cnn.init_pretrained_embeddings_from_numpy(inputs[6])
    cnn.load_state_dict(sd)
    lstm = None
    if c["lstm"]:
        lstm = LSTMModel(*CR.LSTM_ARGS, n_classes=CR.N_CLASSES, dropout=0.0)
        lstm.load_state_dict(lsd)
        lstm = lstm.to(DEV)
    return cnn.to(DEV), lstm, sd, lsd, inputs


def float64_case(name, sd, lsd, inputs, keep=None, p=0.0):
    """(features, log_prob or None, loss, {parameter: gradient}) of the restatement in float64; LSTMModel keys carry 'lstm_model.'."""
    c = CR.MODEL_CASES[name]
    x, qmask, umask, label, weight, G, _ = inputs
    P = {k: v.double().requires_grad_(not (c["frozen"] and k == "embedding.weight")) for k, v in sd.items()}
    feats, _, _ = CR.module_forward(P, x, umask, keep=keep, p=p)
    lp = None
    if c["lstm"]:
        Q = {k: v.double().requires_grad_(True) for k, v in lsd.items()}
        lp, _, _ = LR.forward64(Q, feats, umask, True)
        loss = LR.masked_nll(flat_logp(lp), label, umask, weight)
        P.update({"lstm_model." + k: v for k, v in Q.items()})
    else:
        loss = (feats * G.double()).sum()
    loss.backward()
    return feats.detach(), None if lp is None else lp.detach(), loss.item(), {k: v.grad for k, v in P.items() if v.grad is not None}


def device_step(name, cnn, lstm, inputs):
    x, qmask, umask, label, weight, G, _ = [t.to(DEV) if torch.is_tensor(t) else t for t in inputs]
    feats = cnn(x, umask)
    lp = None
    if lstm is not None:
        lp = lstm(feats, qmask, umask)[0]
        loss = MaskedNLLLoss(weight)(flat_logp(lp), label.view(-1), umask)
    else:
        loss = (feats * G).sum()
    train.backward(loss)
    ops.join_weight_grads()
    grads = {k: p.grad for k, p in cnn.named_parameters()}
    if lstm is not None:
        grads.update({"lstm_model." + k: p.grad for k, p in lstm.named_parameters()})
    return feats, lp, loss, grads


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "cnn_features.npz"), allow_pickle=False)


@pytest.mark.parametrize("name", sorted(CR.MODEL_CASES))
def test_golden_cases_and_float64(name, golden):
    g = golden
    seed = int(g["seed"])
    c = CR.MODEL_CASES[name]
    L, B, W = c["x"]
    cnn, lstm, sd, lsd, inputs = build(name, seed)
    f64, lp64, loss64, grads64 = float64_case(name, sd, lsd, inputs)
    x, umask = inputs[0].to(DEV), inputs[2].to(DEV)
    # ---- eval: features, exact zeros under the mask, integer ids give the same bits as float ids
    cnn.eval()
    with torch.no_grad():
        feats_eval = cnn(x, umask)
        assert torch.equal(cnn(x.long(), umask), feats_eval)
    assert tuple(feats_eval.shape) == (L, B, c["args"][2])
    assert np.abs(feats_eval.cpu().numpy() - g[name + "/features"]).max() < 1e-4
    assert rel_max(feats_eval, f64) < 1e-5
    for b, n in enumerate(c["lengths"]):
        assert n == L or float(feats_eval[n:, b].abs().max()) == 0.0
    # ---- train mode (dropout 0) equals eval mode; losses and gradients
    cnn.train()
    if lstm is not None:
        lstm.train()
    feats, lp, loss, grads = device_step(name, cnn, lstm, inputs)
    assert torch.equal(feats.detach(), feats_eval)
    want_loss = float(g[name + "/loss"])
    if lstm is not None:
        assert np.abs(lp.detach().cpu().numpy() - g[name + "/log_prob"]).max() < 1e-4
        assert rel_max(lp, lp64) < 1e-5
        assert abs(loss.item() - want_loss) < 1e-5
    else:
        assert abs(loss.item() - want_loss) < 1e-5
    assert abs(loss.item() - loss64) < 1e-5 * abs(loss64)
    worst = {}
    for k, gr in grads.items():
        key = name + "/digest/" + k
        if key not in g.files:
            assert k == "embedding.weight" and c["frozen"] and gr is None, k
            continue
        assert gr is not None, k
        want = g[key]
        assert abs(CR.digest(gr)[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
        worst[k] = rel_max(gr, grads64[k])
    print("CNN-MODEL %s worst gradient rel_max vs float64: %.3g (%s)" % (name, max(worst.values()), max(worst, key=worst.get)),
          flush=True)
    assert all(v < 1e-5 for v in worst.values()), {k: v for k, v in worst.items() if not v < 1e-5}
    stored = [k[len(name) + 6:] for k in g.files if k.startswith(name + "/grad/")]
    assert "convs.0.weight" in stored and "fc.weight" in stored and (("embedding.weight" in stored) == (not c["frozen"]))
    for k in stored:
        want = g[name + "/grad/" + k]
        got = grads[k][::CR.MODEL_GRAD_ROWS[k]].cpu().numpy()
        assert np.abs(got - want).max() / np.abs(want).max() < 2e-4, k


def test_dropout_step_against_float64_on_replayed_flags():
    """p = 0.5 on the pooled block: the keep flags are read from the tap and replayed in the float64 restatement; features and
    every gradient are compared, and the one tapped draw covers the block (its element count rounded up to a multiple of 4)."""
    name, p = "a", 0.5
    c = CR.MODEL_CASES[name]
    L, B, W = c["x"]
    cnn, _, sd, _, inputs = build(name, 21, dropout=p)
    cnn.train()
    torch.manual_seed(5)
    ops_flags.TAP = []
    try:
        feats, _, loss, grads = device_step(name, cnn, None, inputs)
        draws, ops_flags.TAP = ops_flags.TAP, None
    finally:
        ops_flags.TAP = None
    n = L * B * len(c["args"][4]) * c["args"][3]
    assert [(site, cnt, pp) for cnt, pp, t, site in draws] == [("cnn", (n + 3) & ~3, p)]
    keep = draws[0][2].detach().cpu()
    assert set(keep.unique().tolist()) <= {0.0, 1.0} and 0.35 < float(keep.mean()) < 0.65
    f64, _, loss64, grads64 = float64_case(name, sd, None, inputs, keep=keep, p=p)
    assert rel_max(feats, f64) < 1e-5
    assert abs(loss.item() - loss64) < 1e-5 * abs(loss64)
    for k, gr in grads.items():
        assert rel_max(gr, grads64[k]) < 1e-5, k
    # eval mode ignores the dropout
    cnn.eval()
    with torch.no_grad():
        ev = cnn(inputs[0].to(DEV), inputs[2].to(DEV))
    assert rel_max(ev, float64_case(name, sd, None, inputs)[0]) < 1e-5


def test_training_step_launches_no_library_gemm_or_convolution():
    """The device trace of a training step of extractor + LSTMModel (dropout on) holds the K18 kernels and no Tensile (`Cijk_*`)
    kernel, no ATen matmul, no MIOpen kernel and no embedding-gather or im2col kernel of the library path."""
    from torch.profiler import ProfilerActivity, profile
    cnn, lstm, sd, lsd, inputs = build("c", 4, dropout=0.3)
    cnn.train()
    lstm.train()

    def step():
        cnn.zero_grad(set_to_none=True)
        lstm.zero_grad(set_to_none=True)
        device_step("c", cnn, lstm, inputs)
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    for kern in ("cnn_cut", "cnn_pool_fwd", "cnn_wgrad", "cnn_table_keys", "cnn_table_bounds", "cnn_table_bwd"):
        assert sum(kern in n for n in names) == 1, (kern, names)
    assert any("lstm_seq_fwd" in n for n in names) and any("masked_nll" in n for n in names), names
    bad = [n for n in names if n.startswith("Cijk_") or ("gemm" in n.lower() and "gemm_tn" not in n) or "miopen" in n.lower()
           or "bmm" in n.lower() or "convolution" in n.lower() or "conv1d" in n.lower() or "im2col" in n.lower()
           or "embedding" in n.lower()]
    assert not bad, names


def test_three_flat_adam_steps_change_the_weights_the_next_forward_reads():
    """FlatAdam writes the parameters behind autograd's back.  K18 cuts its weight planes inside every forward launch, so there
    is nothing to refresh: after three steps the forward equals the float64 restatement ON THE UPDATED parameters, and differs
    from the features before the steps."""
    name = "a"
    cnn, _, sd, _, inputs = build(name, 9)
    cnn.train()
    opt = FlatAdam(cnn, lr=1e-2, weight_decay=1e-4)
    before = {k: v.detach().clone() for k, v in cnn.state_dict().items()}
    feats0 = cnn(inputs[0].to(DEV), inputs[2].to(DEV)).detach().clone()
    for i in range(3):
        opt.zero_grad()
        device_step(name, cnn, None, CR.model_inputs(name, 100 + i))
        opt.step()
    after = {k: v.detach().cpu().clone() for k, v in cnn.state_dict().items()}
    for k in before:
        assert float((after[k] - before[k].cpu()).abs().max()) > 1e-3, k
    feats1 = cnn(inputs[0].to(DEV), inputs[2].to(DEV))
    assert float((feats1.detach() - feats0).abs().max()) > 1e-3
    want = float64_case(name, after, None, inputs)[0]
    assert rel_max(feats1, want) < 1e-5


def test_captured_step_replays_the_eager_bits():
    """graphs.CapturedStep around extractor forward + backward on static inputs: replays on new (valid) tokens give the eager
    step's bits, features and every gradient.  (The id check is skipped under capture and at replay; an invalid id raises in
    eager mode, on the host.)"""
    from mm_dfn_amd.graphs import CapturedStep
    name = "a"
    cnn, _, sd, _, inputs = build(name, 5)
    cnn.train()
    V = CR.MODEL_CASES[name]["args"][0]
    xa, xb = inputs[0], CR.model_inputs(name, 301)[0]
    xc = xb.clone()
    xc[0, 0, 3] = V - 1
    x, umask, G = inputs[0].to(DEV).clone(), inputs[2].to(DEV), inputs[5].to(DEV)
    held = {}

    def step():
        feats = cnn(x, umask)
        held["out"] = feats.detach()     # (only a detached alias outlives the pass)
        loss = (feats * G).sum()
        loss.backward()
        return loss

    def result():
        torch.cuda.synchronize()
        return [held["out"].clone()] + [p.grad.clone() for p in cnn.parameters()]
    want = []
    for xin in (xa, xb, xc):
        x.copy_(xin)
        cnn.zero_grad(set_to_none=True)
        step()
        want.append(result())
    assert not torch.equal(want[0][0], want[1][0])
    cap = CapturedStep(cnn, step, warmup=2)
    try:
        for xin, w in ((xb, want[1]), (xa, want[0]), (xc, want[2])):
            x.copy_(xin)
            cap.replay()
            got = result()
            assert len(got) == len(w) == 1 + 9
            for i, (a, b) in enumerate(zip(got, w)):
                assert torch.equal(a, b), i
    finally:
        cap.close()


@pytest.mark.parametrize("bad", ["V", "-1", "nan", "inf"])
def test_an_invalid_float_id_raises_on_the_host_before_any_kernel(bad):
    """The module's check runs on the ids the kernels would read and on the float tensor they come from."""
    from torch.profiler import ProfilerActivity, profile
    name = "a"
    cnn, _, sd, _, inputs = build(name, 5)
    V = CR.MODEL_CASES[name]["args"][0]
    x, umask = inputs[0].clone(), inputs[2].to(DEV)
    cnn(x.to(DEV), umask)
    x[0, 0, 3] = {"V": float(V), "-1": -1.0, "nan": float("nan"), "inf": float("inf")}[bad]
    x = x.to(DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        with pytest.raises(ValueError):
            cnn(x, umask)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert not any("cnn_" in n for n in names), names
