"""GPU: the three forms of the fused focal loss (csrc/focal_loss.hip: plain backward kernel, unit-seed gradient written by the
forward launch, the ``*_ignore`` form of the bucketed captured steps) and the fused Adam step (csrc/optimizer.hip) called
directly, against float64 restatements with derived bounds (test_focal_loss_host.focal_reference; adam_reference below).
Every test prints its worst error-to-bound ratio (profiles/r08_fusion_loss_optimizer_parity.md records them)."""
import numpy as np
import pytest
import torch

from mm_dfn_amd import FocalLoss, _hip, train
from test_focal_loss_host import IGNORE, focal_inputs, focal_reference, ignore_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

# (N, C, gamma, alpha, mean): every N in {1, 63, 1024, 1025, 2500} (the forward kernel strides rows over 1024 threads), every C in
# {1, 2, 7}, every gamma in {0, 0.5, 2}, class weights on and off, both reductions
FOCAL_CASES = [(1, 1, 0.0, False, True), (1, 7, 2.0, True, False), (63, 2, 0.5, False, True), (63, 7, 0.0, True, False),
               (1024, 7, 0.5, True, True), (1024, 1, 2.0, False, False), (1025, 2, 2.0, True, True), (1025, 7, 0.5, False, False),
               (2500, 7, 0.5, False, True), (2500, 2, 0.0, True, False), (2500, 1, 0.5, True, True)]
IGNORE_CASES = [c for c in FOCAL_CASES if c[0] > 1]


def loss_module(gamma, alpha, mean, ignore=None):
    return FocalLoss(gamma=gamma, alpha=None if alpha is None else alpha.tolist(), size_average=mean, ignore_index=ignore)


def check_loss(tag, loss, grad, ref):
    want, want_b, g, g_b = ref
    r_loss = abs(loss.item() - want) / want_b if want_b > 0 else float(loss.item() != want)
    err = (grad.detach().double().cpu() - g).abs()
    r_grad = float(torch.where(g_b > 0, err / g_b.clamp_min(1e-300), (err != 0).double() * 2).max())
    print("RATIO %s loss %.3f grad %.3f" % (tag, r_loss, r_grad))
    assert r_loss <= 1.0, (tag, loss.item(), want, want_b)
    assert r_grad <= 1.0, (tag, r_grad)


def variants(N):
    """Every case carries a pt = 1 row; a single-row case is also run on an ordinary row."""
    return (0, None) if N == 1 else (N // 2,)


@pytest.mark.parametrize("N,C,gamma,alpha,mean", FOCAL_CASES)
def test_focal_loss_plain_form_against_float64(N, C, gamma, alpha, mean):
    for pt1 in variants(N):
        logp, tgt, al = focal_inputs(N, C, 7 * N + C, pt1, alpha)
        f = loss_module(gamma, al, mean)
        tag = "focal_plain[N=%d,C=%d,g=%g,a=%d,mean=%d,pt1=%s]" % (N, C, gamma, alpha, mean, pt1)
        # the backward kernel: an upstream gradient that is not 1
        lg = logp.to(DEV).requires_grad_(True)
        loss = f(lg, tgt.to(DEV))
        (loss * 1.7).backward()
        check_loss(tag + " bwd", loss, lg.grad, focal_reference(logp, tgt, gamma, al, mean, upstream=1.7))
        # the unit seed: the forward launch wrote the gradient; train.backward hands it out with no backward launch
        la = logp.to(DEV).requires_grad_(True)
        loss_a = f(la, tgt.to(DEV))
        train.backward(loss_a)
        check_loss(tag + " unit", loss_a, la.grad, focal_reference(logp, tgt, gamma, al, mean))
        lb = logp.to(DEV).requires_grad_(True)
        f(lb, tgt.to(DEV)).backward()                                     # a fresh graph through the backward kernel
        assert torch.equal(la.grad, lb.grad), tag
        assert loss_a.item() == loss.item()
        once = la.grad.clone()
        train.backward(loss_a)                                            # a second pass over the kept graph accumulates
        assert torch.equal(la.grad, once + once), tag


@pytest.mark.parametrize("kind", ["none", "ends", "half"])
@pytest.mark.parametrize("N,C,gamma,alpha,mean", IGNORE_CASES)
def test_focal_loss_ignore_form_against_float64(N, C, gamma, alpha, mean, kind):
    logp, tgt, al = focal_inputs(N, C, 7 * N + C, N // 2, alpha)
    ig = ignore_mask(N, kind, N + C)
    labels = torch.where(ig, torch.full_like(tgt, IGNORE), tgt)
    lg = logp.to(DEV).requires_grad_(True)
    loss = loss_module(gamma, al, mean, IGNORE)(lg, labels.to(DEV))
    (loss * 1.7).backward()
    tag = "focal_ignore[N=%d,C=%d,g=%g,a=%d,mean=%d,%s]" % (N, C, gamma, alpha, mean, kind)
    check_loss(tag, loss, lg.grad, focal_reference(logp, tgt, gamma, al, mean, keep=~ig, upstream=1.7))
    assert bool((lg.grad[ig.to(DEV)] == 0).all()), tag


@pytest.mark.parametrize("N,C,gamma,alpha,mean", FOCAL_CASES)
def test_focal_loss_ignore_form_equals_plain_form_bit_for_bit(N, C, gamma, alpha, mean):
    """With no row left out the two forms run the same arithmetic in the same order: same loss, same gradient, to the bit --
    for an upstream gradient of 1.7 (both backward kernels) and of 1 (the plain form's unit-seed gradient)."""
    logp, tgt, al = focal_inputs(N, C, 7 * N + C, N // 2, alpha)
    for up in (1.7, 1.0):
        grads, losses = [], []
        for ignore in (None, IGNORE):
            lg = logp.to(DEV).requires_grad_(True)
            loss = loss_module(gamma, al, mean, ignore)(lg, tgt.to(DEV))
            if up == 1.0:
                train.backward(loss)
            else:
                (loss * up).backward()
            grads.append(lg.grad)
            losses.append(loss.item())
        assert losses[0] == losses[1], (losses, up)
        assert torch.equal(grads[0], grads[1]), up


@pytest.mark.parametrize("k", [1, 1023])
@pytest.mark.parametrize("N,C,gamma,alpha,mean", IGNORE_CASES)
def test_focal_loss_ignored_padding_rows_change_nothing(N, C, gamma, alpha, mean, k):
    """The bucket-padding contract of train.StepGraphCache: k rows labelled IGNORE appended to a batch leave the loss and the
    real rows' gradient unchanged to the bit, and get a zero gradient themselves."""
    logp, tgt, al = focal_inputs(N, C, 7 * N + C, N // 2, alpha)
    pad, _, _ = focal_inputs(k, C, 5)
    f = loss_module(gamma, al, mean, IGNORE)
    lg = logp.to(DEV).requires_grad_(True)
    loss = f(lg, tgt.to(DEV))
    (loss * 1.7).backward()
    lp = torch.cat([logp, pad]).to(DEV).requires_grad_(True)
    loss_p = f(lp, torch.cat([tgt, torch.full((k,), IGNORE, dtype=torch.int64)]).to(DEV))
    (loss_p * 1.7).backward()
    assert loss_p.item() == loss.item()
    assert torch.equal(lp.grad[:N], lg.grad)
    assert bool((lp.grad[N:] == 0).all())


@pytest.mark.parametrize("bad", [-1, "C"])
@pytest.mark.parametrize("ignore", [None, IGNORE])
@pytest.mark.parametrize("mean", [False, True])
def test_focal_loss_bad_label_poisons_its_row_only(mean, ignore, bad):
    """A label outside [0, C) in a row that counts: NaN loss, that row's gradient all NaN, every other row's gradient finite and
    what it is without the bad row -- under mean reduction divided by a count that includes the bad row."""
    N, C, gamma = 1025, 7, 0.5
    logp, tgt, al = focal_inputs(N, C, 91, N // 2, True)
    ig = ignore_mask(N, "ends", 92) if ignore is not None else torch.zeros(N, dtype=torch.bool)
    row = 700
    assert not bool(ig[row])
    labels = torch.where(ig, torch.full_like(tgt, IGNORE), tgt)
    labels[row] = C if bad == "C" else bad
    lg = logp.to(DEV).requires_grad_(True)
    loss = loss_module(gamma, al, mean, ignore)(lg, labels.to(DEV))
    (loss * 1.7).backward()
    assert bool(torch.isnan(loss))
    grad = lg.grad.cpu()
    assert bool(torch.isnan(grad[row]).all())
    good = ~ig
    good[row] = False
    others = torch.ones(N, dtype=torch.bool)
    others[row] = False
    assert bool(torch.isfinite(grad[others]).all())
    _, _, g, g_b = focal_reference(logp, tgt, gamma, al, mean, keep=good, upstream=1.7, count=int(good.sum()) + 1)
    err = (grad.double() - g).abs()[others]
    assert bool((err <= g_b[others]).all()), float((err / g_b[others].clamp_min(1e-300)).max())
    assert bool((grad[ig] == 0).all())


@pytest.mark.parametrize("mean", [False, True])
def test_focal_loss_with_every_row_ignored_is_zero_on_the_device(mean):
    logp, tgt, _ = focal_inputs(1025, 7, 93)
    lg = logp.to(DEV).requires_grad_(True)
    loss = loss_module(0.5, None, mean, IGNORE)(lg, torch.full_like(tgt, IGNORE).to(DEV))
    (loss * 1.7).backward()
    assert loss.item() == 0.0
    assert bool((lg.grad == 0).all())


# ---- mmdfn_adam_step -----------------------------------------------------------------------------------------------------------
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
F32 = lambda x: float(np.float32(x))


def adam_reference(p, g, m, v, lr, wd, step):
    """torch.optim.Adam's step with L2 folded into the gradient, in float64, on the float32-rounded lr / betas / eps / wd that the
    ABI receives; the bias corrections in float64.  Returns (dp, m', v', mag of m', mag of v')."""
    lr, b1, b2, eps, wd = F32(lr), F32(BETA1), F32(BETA2), F32(EPS), F32(wd)
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gg = g + wd * p
    gg_mag = g.abs() + wd * p.abs()
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    dp = -(lr / bc1) * m2 / (v2.sqrt() / bc2 ** 0.5 + eps)
    return dp, m2, v2, b1 * m.abs() + (1 - b1) * gg_mag, b2 * v + (1 - b2) * gg_mag * gg_mag


def adam_inputs(n, step, seed):
    """Gradients of magnitude 0.1 .. 2 and parameters of magnitude 1e-6 .. 2, log-uniform (g + wd p does not cancel; where |p|
    is below the update, the bound is 16 u of the update itself and not the rounding of p), prior moments of a run in progress
    for step > 1 (m with the sign of g: an average of past gradients), and entries with g = m = v = 0 (with and without p = 0)."""
    gen = torch.Generator().manual_seed(seed)
    sign = lambda: 1.0 - 2.0 * (torch.rand(n, generator=gen) < 0.5).float()
    g = (0.1 + 1.9 * torch.rand(n, generator=gen)) * sign()
    p = 2.0 * 10.0 ** (-6.3 * torch.rand(n, generator=gen)) * sign()
    if step > 1:
        m = g * (0.5 + 1.5 * torch.rand(n, generator=gen))
        v = g * g * (0.5 + 1.5 * torch.rand(n, generator=gen))
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    zero = torch.zeros(n, dtype=torch.bool)
    if n >= 5:
        zero[[1, n - 1]] = True
        zero[n // 2] = True
        g[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
        p[n // 2] = 0.0
    return p, g, m, v, zero


def adam_call(p, g, m, v, n, lr, wd, step):
    return _hip.lib().mmdfn_adam_step(_hip.ptr(p), _hip.ptr(g), _hip.ptr(m), _hip.ptr(v), n, lr, BETA1, BETA2, EPS, wd, step,
                                      _hip.stream())


STEPS = [1, 2, 3, 5, 10, 100, 100000]                          # (at the last one beta^t underflows to 0)
ADAM_CASES = ([(n, STEPS[i % 7], (0.0, 1e-4)[i % 2], 1e-3) for i, n in enumerate([1, 3, 4, 5, 7, 1023, 1024, 1025])]
              + [(1025, s, wd, 1e-3) for s in STEPS for wd in (0.0, 1e-4)]
              + [(1023, 3, 1e-4, 0.0), (7, 1, 0.0, 0.0)]
              + [(2048 * 256 * 4 + 5, 2, 1e-4, 1e-3), (2048 * 256 * 4 + 5, 1, 0.0, 1e-3)])     # past the block cap, with a tail


@pytest.mark.parametrize("n,step,wd,lr", ADAM_CASES)
def test_adam_step_against_float64(n, step, wd, lr):
    """|dp_got - dp_want| <= 16 u |dp_want| + u (|p| + |p'|)  (the update, then the rounding of p - update);  m and v to 8 u of
    their magnitude.  Entries past n keep their values."""
    p, g, m, v, zero = adam_inputs(n, step, 17 * step + n % 1000)
    dp, m2, v2, m_mag, v_mag = adam_reference(p, g, m, v, lr, wd, step)
    pad = 8
    sentinel = (3.5, -1.25, 7.0, 9.0)
    dev = []
    for t, s in zip((p, g, m, v), sentinel):
        dev.append(torch.cat([t, torch.full((pad,), s)]).to(DEV))
    assert adam_call(*dev, n, lr, wd, step) == 0
    torch.cuda.synchronize()
    pg, gg, mg, vg = (t.cpu() for t in dev)
    for t, s in zip((pg, gg, mg, vg), sentinel):
        assert bool((t[n:] == s).all())
    assert torch.equal(gg[:n], g)
    pg, mg, vg = pg[:n].double(), mg[:n].double(), vg[:n].double()
    assert bool(torch.isfinite(pg).all() and torch.isfinite(mg).all() and torch.isfinite(vg).all())
    dp_got = pg - p.double()
    dp_b = 16 * U * dp.abs() + U * (p.double().abs() + (p.double() + dp).abs())
    tiny = 1e-300
    r_p = float(((dp_got - dp).abs() / dp_b.clamp_min(tiny)).max())
    r_m = float(((mg - m2).abs() / (8 * U * m_mag).clamp_min(tiny)).max())
    r_v = float(((vg - v2).abs() / (8 * U * v_mag).clamp_min(tiny)).max())
    print("RATIO adam[n=%d,step=%d,wd=%g,lr=%g] dp %.3f m %.3f v %.3f" % (n, step, wd, lr, r_p, r_m, r_v))
    assert r_p <= 1.0 and r_m <= 1.0 and r_v <= 1.0, (r_p, r_m, r_v)
    # g = m = v = 0: the moments stay 0 and the update is exactly 0 (0 / (0 + eps), no NaN) wherever wd p is 0 as well
    still = zero & ((p == 0) | torch.tensor(F32(wd) == 0.0))
    if bool(still.any()):
        assert bool((dp_got[still] == 0).all()) and bool((mg[still] == 0).all()) and bool((vg[still] == 0).all())
    if lr == 0.0:
        assert bool((dp_got == 0).all())


def test_adam_step_refuses_empty_buffers_and_step_zero():
    t = [torch.ones(8, device=DEV) for _ in range(4)]
    assert adam_call(*t, 0, 1e-3, 0.0, 1) == -1
    assert adam_call(*t, -4, 1e-3, 0.0, 1) == -1
    assert adam_call(*t, 8, 1e-3, 0.0, 0) == -1
    assert adam_call(*t, 8, 1e-3, 0.0, -1) == -1
    torch.cuda.synchronize()
    assert all(bool((x == 1).all()) for x in t)
