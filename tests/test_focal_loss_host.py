"""CPU: the host fallback of FocalLoss (mm_dfn_amd/loss.py, what the gloo data-parallel test runs) with ``ignore_index`` against
the oracle on the rows that count, and the float64 reference + derived bounds that the device tests of the three kernel forms
share (tests/test_loss_optimizer_kernels_gpu.py imports them from here)."""
import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd.loss import FocalLoss

U = 2.0 ** -24
IGNORE = -100


def focal_inputs(N, C, seed, pt1_row=None, alpha=False):
    """log-probabilities (N, C) (the first C columns of a (C + 1)-class log-softmax, so that C = 1 is not all zeros), labels and
    an optional class-weight table; ``pt1_row`` gets log-prob 0 at its label: pt = 1 exactly."""
    rs = np.random.RandomState(seed)
    logp = torch.log_softmax(torch.from_numpy(rs.randn(N, C + 1).astype(np.float32)) * 3, 1)[:, :C].contiguous()
    tgt = torch.from_numpy(rs.randint(0, C, size=N).astype(np.int64))
    if pt1_row is not None:
        logp[pt1_row] = torch.tensor([0.0] + [-100.0] * (C - 1))
        tgt[pt1_row] = 0
    al = torch.from_numpy(rs.uniform(0.5, 2.0, size=C).astype(np.float32)) if alpha else None
    return logp, tgt, al


def focal_reference(logp, tgt, gamma, alpha, size_average, keep=None, upstream=1.0, count=None):
    """(loss, loss bound, grad (N, C), grad bound (N, C)) in float64: ``O.focal_loss`` on the rows ``keep`` selects (all by
    default) and its autograd gradient times ``upstream``, scattered back to N rows (zero elsewhere); the mean divides by
    ``count`` (default: the number of kept rows).

    Bounds, u = 2^-24.  The weight (1 - pt)^gamma cancels at pt -> 1, so its bound is an interval evaluation: expf is good to 2 ulp
    (4 u pt absolute on pt), hence the weight lies between (1 - pt -+ 4 u pt)^gamma, plus 16 u relative for powf, the class
    weight and the scale.  A gradient entry is pointwise in the weight; the loss sums one term per kept row:
    (rows + 16) u sum |w lp| plus the weights' bounds times |lp|."""
    N, C = logp.shape
    keep = torch.ones(N, dtype=torch.bool) if keep is None else keep
    rows = int(keep.sum())
    lp = logp.detach().double()[keep].requires_grad_(True)
    t = tgt[keep]
    a = None if alpha is None else alpha.double()
    loss = O.focal_loss(lp, t, gamma, a, False)
    (g,) = torch.autograd.grad(loss, lp)
    scale = 1.0 / max(count if count is not None else rows, 1) if size_average else 1.0
    lpt = lp.detach().gather(1, t.view(-1, 1)).view(-1)
    pt = lpt.exp()
    at = torch.ones_like(pt) if a is None else a.gather(0, t)
    w = (1 - pt) ** gamma
    d = 4 * U * pt
    w_b = torch.maximum((1 - pt + d) ** gamma - w, w - (1 - pt - d).clamp_min(0.0) ** gamma) + 16 * U * w
    loss_b = scale * ((rows + 16) * U * (w * at * lpt).abs().sum() + (w_b * at * lpt.abs()).sum())
    grad = torch.zeros(N, C, dtype=torch.float64)
    grad[keep] = g * scale * upstream
    row_b = torch.zeros(N, dtype=torch.float64)
    row_b[keep] = w_b * at * scale * abs(upstream)
    grad_b = torch.zeros(N, C, dtype=torch.float64)
    grad_b[torch.arange(N)[keep], t] = row_b[keep]
    return float(loss.detach()) * scale, float(loss_b), grad, grad_b + 16 * U * grad.abs()


def ignore_mask(N, kind, seed):
    """Rows to leave out: 'none'; 'ends' = the first and the last row and about a tenth of the others; 'half'."""
    rs = np.random.RandomState(seed)
    ig = np.zeros(N, bool)
    if kind == "ends":
        ig[rs.rand(N) < 0.1] = True
        ig[0] = ig[N - 1] = True
    elif kind == "half":
        ig[rs.rand(N) < 0.5] = True
        ig[N // 2] = False                            # (the pt = 1 row counts)
    return torch.from_numpy(ig)


@pytest.mark.parametrize("kind", ["none", "ends", "half"])
@pytest.mark.parametrize("gamma,use_alpha,size_average", [(0.0, False, True), (0.5, True, True), (2.0, False, False),
                                                          (0.5, False, False), (2.0, True, True)])
def test_host_focal_loss_ignore_index_against_oracle(gamma, use_alpha, size_average, kind):
    N, C = 211, 7
    logp, tgt, alpha = focal_inputs(N, C, 60 + int(10 * gamma), pt1_row=N // 2, alpha=use_alpha)
    ig = ignore_mask(N, kind, 61)
    labels = torch.where(ig, torch.full_like(tgt, IGNORE), tgt)
    want, want_b, grad, grad_b = focal_reference(logp, tgt, gamma, alpha, size_average, keep=~ig, upstream=1.7)
    lg = logp.clone().requires_grad_(True)
    f = FocalLoss(gamma=gamma, alpha=None if alpha is None else alpha.tolist(), size_average=size_average, ignore_index=IGNORE)
    got = f(lg, labels)
    (got * 1.7).backward()
    assert abs(got.item() - want) <= want_b, (got.item(), want, want_b)
    assert bool(((lg.grad.double() - grad).abs() <= grad_b).all())
    assert bool((lg.grad[ig] == 0).all())
    if kind == "none":                                 # the same numbers as the form without ignore_index
        lp2 = logp.clone().requires_grad_(True)
        got2 = FocalLoss(gamma=gamma, alpha=None if alpha is None else alpha.tolist(), size_average=size_average)(lp2, tgt)
        (got2 * 1.7).backward()
        assert got2.item() == got.item() and torch.equal(lp2.grad, lg.grad)


@pytest.mark.parametrize("size_average", [True, False])
def test_host_focal_loss_with_every_row_ignored_is_zero(size_average):
    """As the device form (csrc/focal_loss.hip divides by max(count, 1)): loss 0 and zero gradients, not the NaN of an empty mean."""
    logp, tgt, _ = focal_inputs(9, 6, 62)
    lg = logp.clone().requires_grad_(True)
    loss = FocalLoss(gamma=0.5, size_average=size_average, ignore_index=IGNORE)(lg, torch.full_like(tgt, IGNORE))
    loss.backward()
    assert loss.item() == 0.0
    assert lg.grad.shape == logp.shape and bool((lg.grad == 0).all())
