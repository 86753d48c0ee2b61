"""Graph-free fusion baselines on the device: end to end against the reference goldens (tests/golden/make_golden_fusion.py),
the LMF kernels and the ReLU-free head against float64 restatements (torch on the device, tests only)."""
import os

import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd import FocalLoss, ops, train
from mm_dfn_amd.fusion import LMF
from test_fusion_baselines import CASES, build
from test_oracle_golden import GOLD, _digest

DEV = "cuda"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fusion_baselines_against_reference_goldens(name):
    from test_fusion_baselines import CFG
    from mm_dfn_amd import synthetic
    g = np.load(os.path.join(GOLD, "fusion_baselines.npz"), allow_pickle=False)
    m = build(name).to(DEV)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    b = synthetic.make_batch(CASES[name][3] + 1, lengths=[14, 5, 9], **CFG)
    run = lambda: m(b["textf"].to(DEV), b["qmask"].to(DEV), b["umask"].to(DEV), b["lengths"], b["acouf"].to(DEV),
                    b["visuf"].to(DEV))[0]
    m.eval()
    with torch.no_grad():
        logp = run()
    assert np.abs(logp.cpu().numpy() - g[name + "/log_prob"]).max() < 1e-4
    m.train()
    logp = run()
    loss = FocalLoss(gamma=0.5)(logp, train.flatten_labels(b["label"].to(DEV), b["lengths"]))
    assert abs(loss.item() - float(g[name + "/loss"])) < 1e-5
    train.backward(loss)
    grads = {k: p.grad for k, p in m.named_parameters()}
    live = [str(x) for x in g[name + "/live_params"]]
    for k in live:
        want = g[name + "/gd/" + k]
        assert grads[k] is not None, k
        got = _digest(grads[k])
        # all three components: sum |g| and sum g^2 relative to themselves, the signed sum (which may cancel) relative to sum |g|
        assert abs(got[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
        assert abs(got[2] - want[2]) / (want[2] + 1e-30) < 4e-4, k
        assert abs(got[0] - want[0]) / (want[1] + 1e-12) < 2e-4, k
    for k, gr in grads.items():
        if k not in live:
            assert gr is None or float(gr.abs().max()) == 0.0, k


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 37, 300])
def test_lmf_kernels_against_float64(N):
    torch.manual_seed(N)
    mod = LMF().to(DEV)
    with torch.no_grad():
        mod.fusion_bias.normal_()
        for net in (mod.audio_subnet, mod.video_subnet, mod.text_subnet):
            net.weight.mul_(3.0)
    xs = [torch.randn(N, 300, device=DEV, requires_grad=True) for _ in range(3)]
    G = torch.randn(N, 300, device=DEV, dtype=torch.float64)
    out = mod(*xs)
    assert tuple(out.shape) == (N, 300)
    (out.double() * G).sum().backward()
    got = [x.grad.clone() for x in xs] + [p.grad.clone() for p in mod.parameters()]
    ref = LMF().to(DEV).double()
    ref.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    xd = [x.detach().double().requires_grad_(True) for x in xs]
    want_out = O.lmf(xd, dict(ref.named_parameters()))
    (want_out * G).sum().backward()
    want = [x.grad for x in xd] + [p.grad for p in ref.parameters()]
    assert (out.double() - want_out).abs().max() / want_out.abs().max() < 1e-5
    names = ["dx_a", "dx_v", "dx_t"] + [k for k, _ in mod.named_parameters()]
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape, n
        assert float((a.double() - b).abs().max() / b.abs().max()) < 1e-5, n


@pytest.mark.gpu
@pytest.mark.parametrize("stacked", [False, True])
def test_head_without_relu_against_float64(stacked):
    torch.manual_seed(3)
    N, M, Wm, C = 53, 3, 300, 6
    F = torch.randn(M, N, Wm, device=DEV) if stacked else torch.randn(N, 400, device=DEV)
    W = torch.randn(C, M * Wm if stacked else 400, device=DEV) * 0.05
    b = torch.randn(C, device=DEV)
    F.requires_grad_(True)
    W.requires_grad_(True)
    b.requires_grad_(True)
    Fw = F.shape[1] if stacked else N
    mask = (torch.rand(N, W.shape[1], device=DEV) > 0.4).float()
    ms = 1.0 / 0.6
    G = torch.randn(N, C, device=DEV, dtype=torch.float64)
    logp = ops._Head.apply(F, mask, ms, W, b, False)
    (logp.double() * G).sum().backward()
    Fd, Wd, bd = (t.detach().double().requires_grad_(True) for t in (F, W, b))
    flat = Fd.permute(1, 0, 2).reshape(Fw, -1) if stacked else Fd
    want = torch.log_softmax((flat * mask.double() * ms) @ Wd.t() + bd, 1)       # no ReLU (model.py:1403-1404)
    (want * G).sum().backward()
    assert (logp.double() - want).abs().max() < 1e-5
    for a, w in ((F.grad, Fd.grad), (W.grad, Wd.grad), (b.grad, bd.grad)):
        assert float((a.double() - w).abs().max() / w.abs().max()) < 1e-5
    # the ReLU form is unchanged and differs from this one where features are negative
    relu_logp = ops._Head.apply(F.detach(), mask, ms, W.detach(), b.detach())
    assert float((relu_logp - logp.detach()).abs().max()) > 1e-3


def _lmf_step_setup(seed):
    from test_fusion_baselines import CFG
    from mm_dfn_amd import synthetic
    m = build("lmf_only").to(DEV).train()          # every dropout p = 0 (dropout=0.0; LMF applies none)
    b = synthetic.make_batch(seed, lengths=[14, 5, 9], device=DEV, **CFG)
    label = train.flatten_labels(b["label"], b["lengths"])
    loss_f = FocalLoss(gamma=0.5)

    def fwd_bwd():
        logp = m(b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"])[0]
        loss = loss_f(logp, label)
        train.backward(loss)
        return loss
    return m, fwd_bwd


@pytest.mark.gpu
def test_lmf_only_captured_step_equals_eager_over_flat_adam_steps():
    """The lmf_only training step replayed from a captured graph (graphs.CapturedStep, the engine of train.StepGraphCache)
    between FlatAdam steps gives the losses of the same steps run eagerly: the per-call buffers of the LMF backward (the
    [dP | g | T] matrix, the column-sum and gemm_tn workspaces) are safe under capture, and the factors re-pointed into
    FlatAdam's slots are read where they live."""
    from mm_dfn_amd.graphs import CapturedStep
    from mm_dfn_amd.optim import FlatAdam

    def eager():
        m, fwd_bwd = _lmf_step_setup(931)
        opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4)
        losses = []
        for _ in range(4):
            m.zero_grad(set_to_none=True)
            losses.append(float(fwd_bwd()))
            opt.step()
        return losses

    def captured():
        m, fwd_bwd = _lmf_step_setup(931)
        m.zero_grad(set_to_none=True)
        fwd_bwd()
        opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4)
        opt.bucket.flatten()
        opt._materialise()
        cap = CapturedStep(m, fwd_bwd, warmup=2, bucket=opt.bucket)
        losses = []
        for _ in range(4):
            losses.append(float(cap.replay()))
            opt.step(grads_already_flat=True)
        return losses

    want, got = eager(), captured()
    assert want[0] != want[-1]                       # the steps do move the loss
    for a, b in zip(got, want):
        assert abs(a - b) <= 2e-5 * abs(b), (got, want)


@pytest.mark.gpu
def test_lmf_only_training_step_runs_no_library_kernels():
    """A whole lmf_only training step (encoder, residual products, LMF, head, loss, backward) launches only this package's
    kernels for its products: no Tensile (Cijk_), rocBLAS / hipBLASLt or MIOpen kernel in the device trace."""
    from torch.profiler import ProfilerActivity, profile
    m, fwd_bwd = _lmf_step_setup(932)
    fwd_bwd()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        m.zero_grad(set_to_none=True)
        fwd_bwd()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert any("lmf_fwd_kernel" in n for n in names) and any("lmf_bwd_kernel" in n for n in names), names
    assert any("head_fwd_kernel" in n for n in names), names
    bad = [n for n in names if n.startswith("Cijk_") or "rocblas" in n.lower() or "miopen" in n.lower()
           or "hipblaslt" in n.lower() or ("gemm" in n.lower() and "gemm_tn" not in n)]
    assert not bad, bad
