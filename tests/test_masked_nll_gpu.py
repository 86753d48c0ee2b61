"""GPU: MaskedNLLLoss on the fused launches (csrc/nll_loss.hip, K15) against the float64 formula
    loss = sum_i m_i w[t_i] (-pred[i, t_i]) / sum_i m_i w[t_i]
at the launch edges of its one-workgroup forward (rows below, at and past one pass of its threads, several passes).

Bounds: both sums are reduced in float64 on the device, so the loss is the rounded quotient of sums of exactly representable
products (m in {0, 1}; w[t] pred is one float32 product per row, rounded once when a weight table is given): |got - want| <=
4 u |want|-scale, taken as 4 u sum |terms| / den.  A gradient entry is three float32 factors: 4 u |want|."""
import pytest
import torch

from mm_dfn_amd import MaskedNLLLoss

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def inputs(N, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.log_softmax(2.0 * torch.randn(N, C, generator=g), 1)
    target = torch.randint(0, C, (N,), generator=g)
    if kind == "ones":
        mask = torch.ones(N)
    elif kind == "zeros":
        mask = torch.zeros(N)
    else:
        mask = (torch.rand(N, generator=g) < 0.6).float()
        mask[N - 1] = 1.0
    weight = 0.25 + torch.rand(C, generator=g)
    return pred, target, mask, weight


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["ones", "ragged", "zeros"])
@pytest.mark.parametrize("C", [2, 7])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
def test_masked_nll_against_float64(N, C, kind, weighted):
    pred, target, mask, weight = inputs(N, C, kind, 31 * N + C)
    w64 = weight.double() if weighted else torch.ones(C, dtype=torch.float64)
    p64 = pred.double().requires_grad_(True)
    coef = mask.double() * w64[target]
    terms = coef * (-p64[torch.arange(N), target])
    den = coef.sum()
    if kind == "zeros":
        want, dwant, mag = torch.zeros((), dtype=torch.float64), torch.zeros(N, C, dtype=torch.float64), 0.0
    else:
        want = terms.sum() / den
        dwant, = torch.autograd.grad(want, p64)
        mag = float(terms.detach().abs().sum() / den)
    pd = pred.to(DEV).requires_grad_(True)
    loss_f = MaskedNLLLoss(weight.to(DEV) if weighted else None)
    # the mask in the reference's (batch, seq_len) shape when N factors, flat otherwise
    m2 = mask.view(5, -1) if N % 5 == 0 else mask.view(1, -1)
    loss = loss_f(pd, target.to(DEV), m2.to(DEV))
    seed = torch.tensor(1.5, device=DEV)
    loss.backward(seed)
    err = abs(float(loss.double().cpu()) - float(want))
    bound = 4 * U * mag + 2.0 ** -126
    print("RATIO masked_nll[N=%d,C=%d,%s,w=%d] loss %.3f" % (N, C, kind, weighted, err / bound))
    assert torch.isfinite(loss).all() and err <= bound
    got = pd.grad.double().cpu()
    dwant = 1.5 * dwant
    assert bool(torch.isfinite(got).all())
    ratio = float(((got - dwant).abs() / (4 * U * dwant.abs() + 2.0 ** -126)).max())
    print("RATIO masked_nll[N=%d,C=%d,%s,w=%d] dpred %.3f" % (N, C, kind, weighted, ratio))
    assert ratio <= 1.0
    # rows of masked positions are exact zeros
    assert float(pd.grad[(mask == 0).to(DEV)].abs().max() if bool((mask == 0).any()) else 0.0) == 0.0


def test_short_weight_table_raises():
    pred, target, mask, weight = inputs(10, 7, "ones", 3)
    with pytest.raises(IndexError):
        MaskedNLLLoss(weight[:5].to(DEV))(pred.to(DEV), target.to(DEV), mask.view(2, 5).to(DEV))


def test_unit_seed_and_reproducible():
    """Through train.backward (the cached unit seed) and twice: the same bits."""
    from mm_dfn_amd import train
    pred, target, mask, weight = inputs(600, 6, "ragged", 11)
    out = []
    for _ in range(2):
        pd = pred.to(DEV).requires_grad_(True)
        loss = MaskedNLLLoss(weight.to(DEV))(pd, target.to(DEV), mask.view(20, 30).to(DEV))
        train.backward(loss)
        out.append((loss.detach().clone(), pd.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
