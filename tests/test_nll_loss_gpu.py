"""mm_dfn_amd.loss.NLLLoss on the device (csrc/nll_loss.hip) against torch.nn.functional.nll_loss in float64 on the CPU: loss
and d loss / d log_prob under an upstream gradient of 1 and of 0.37.

Bounds, from the number format: the loss within (N + 4) 2^-24 relative to sum w |logp| / sum w (the scale of the terms it is
made of), every non-zero gradient entry within (N + 4) 2^-24 relative to its own value."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mm_dfn_amd import FocalLoss, NLLLoss
from mm_dfn_amd import loss as loss_mod

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


def make(N, C, seed, weights, ignore_some=False, ignore_index=-100):
    g = torch.Generator().manual_seed(seed)
    logp = torch.log_softmax(torch.randn(N, C, generator=g) * 2.0, 1)
    target = torch.randint(0, C, (N,), generator=g)
    if ignore_some:
        target[torch.rand(N, generator=g) < 0.3] = ignore_index
        target[0] = ignore_index
    w = None
    if weights:
        w = torch.rand(C, generator=g) + 0.25
        if weights == "zero":
            w[1] = 0.0                                   # a class that does not count
            target[N // 2] = 1                           # ... and is met
    return logp, target, w


def reference(logp, target, w, reduction, ignore_index, up):
    x = logp.double().requires_grad_(True)
    loss = F.nll_loss(x, target, None if w is None else w.double(), ignore_index=ignore_index, reduction=reduction)
    loss.backward(torch.tensor(float(np.float32(up)), dtype=torch.float64))
    keep = target != ignore_index
    wt = torch.ones(int(keep.sum()), dtype=torch.float64) if w is None else w.double()[target[keep]]
    mag = float((wt * logp.double()[keep].gather(1, target[keep].view(-1, 1)).view(-1).abs()).sum())
    if reduction == "mean":
        mag /= float(wt.sum())
    return float(loss), x.grad, mag


def device(loss_f, logp, target, up):
    x = logp.to(DEV).requires_grad_(True)
    loss = loss_f(x, target.to(DEV))
    loss.backward(torch.tensor(up, dtype=torch.float32, device=DEV))
    return float(loss), x.grad.cpu()


def compare(N, C, weights, reduction, ignore_some=False, seed=0):
    logp, target, w = make(N, C, 10 * N + C + seed, weights, ignore_some)
    loss_f = NLLLoss(weight=w, reduction=reduction)
    for up in (1.0, 0.37):
        want, dwant, mag = reference(logp, target, w, reduction, -100, up)
        got, dgot = device(loss_f, logp, target, up)
        bound = (N + 4) * EPS
        rel = abs(got - want) / mag
        nz = dwant != 0
        grel = float(((dgot.double() - dwant).abs()[nz] / dwant.abs()[nz]).max()) if bool(nz.any()) else 0.0
        print("N=%d C=%d weights=%s %s ignore=%s up=%.2f  loss err / bound %.3f  gradient err / bound %.3f"
              % (N, C, weights, reduction, ignore_some, up, rel / bound, grel / bound))
        assert rel <= bound
        assert grel <= bound
        if bool((~nz).any()):
            assert float(dgot[~nz].abs().max()) == 0.0


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("weights", [None, "table", "zero"])
def test_against_float64(weights, reduction):
    """N = 1 and one below, at and one above the forward launch's workgroup; C = 6 and 7."""
    T = loss_mod.nll_block_rows()
    for N in (1, T - 1, T, T + 1):
        for C in (6, 7):
            if weights == "zero" and N == 1:
                continue                                 # (the only row has weight 0: 0 / 0, torch's NaN -- below)
            compare(N, C, weights, reduction)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_some_rows_ignored(reduction):
    for weights in (None, "table"):
        compare(70, 6, weights, reduction, ignore_some=True)
        compare(loss_mod.nll_block_rows() + 3, 7, weights, reduction, ignore_some=True)


def test_other_ignore_index_and_zero_weight_sum():
    logp, target, w = make(40, 6, 5, "table", ignore_some=True, ignore_index=4)
    want, dwant, mag = reference(logp, target, w, "mean", 4, 1.0)
    got, dgot = device(NLLLoss(weight=w, ignore_index=4), logp, target, 1.0)
    assert abs(got - want) <= 44 * EPS * mag and float((dgot.double() - dwant).abs().max()) <= 44 * EPS * float(dwant.abs().max())
    # every row that counts has weight 0: 0 / 0, NaN as in torch
    w0 = torch.tensor([0.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    got, _ = device(NLLLoss(weight=w0), logp, torch.zeros(40, dtype=torch.int64), 1.0)
    assert np.isnan(got) and bool(torch.isnan(F.nll_loss(logp, torch.zeros(40, dtype=torch.int64), w0)))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_every_row_ignored_gives_zero_with_zero_gradients(reduction):
    logp, _, w = make(33, 6, 1, "table")
    target = torch.full((33,), -100, dtype=torch.int64)
    got, dgot = device(NLLLoss(weight=w, reduction=reduction), logp, target, 1.0)
    assert got == 0.0 and float(dgot.abs().max()) == 0.0


def test_bad_label_poisons_the_loss():
    logp, target, w = make(33, 6, 2, "table")
    for bad in (6, -1, 1000):
        t = target.clone()
        t[7] = bad
        got, dgot = device(NLLLoss(weight=w), logp, t, 1.0)
        assert np.isnan(got) and bool(torch.isnan(dgot[7]).all())


def test_short_weight_table_raises():
    logp, target, _ = make(9, 7, 3, None)
    with pytest.raises(IndexError):
        NLLLoss(weight=torch.ones(6))(logp.to(DEV), target.to(DEV))


def test_reduction_none_is_not_implemented():
    with pytest.raises(NotImplementedError):
        NLLLoss(reduction="none")


def test_focal_loss_with_gamma_zero_is_another_loss():
    """FocalLoss(gamma=0, alpha=w) divides by the number of rows, NLLLoss(weight=w) by the sum of the target classes' weights."""
    logp, target, w = make(50, 6, 4, "table")
    nll, _ = device(NLLLoss(weight=w), logp, target, 1.0)
    focal, _ = device(FocalLoss(gamma=0, alpha=w.clone()), logp, target, 1.0)
    wsum = float(w.double()[target].sum())
    assert abs(nll - focal) > 1e-3 * abs(nll)
    assert abs(nll * wsum - focal * 50) <= 1e-5 * abs(focal * 50)        # the same numerator
    want, _, _ = reference(logp, target, w, "mean", -100, 1.0)
    assert abs(nll - want) <= 54 * EPS * abs(want)
