"""float64 restatements of the masked matching attention (MatchingAttention(att_type='general2'), reference model.py:66-76,84)
for the tests: the reference's per-query procedure, the closed form the kernel implements, and the elementwise error bounds of
the kernel tests (the convention at the top of tests/test_fusion_kernels_gpu.py).

Shapes: X (Tq, B, D) queries (the transform already applied), M (L, B, D) memory, mask (B, L) of 0 / 1.
"""
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126


def reference_loop(X, M, mask):
    """The reference's procedure, one query row at a time: mask the memory, batched product, mask the scores, tanh, softmax over
    ALL keys, mask the weights, renormalise, pool the UNMASKED memory.  Returns pool (Tq, B, D), alpha (Tq, B, L)."""
    X, M, mask = X.double(), M.double(), mask.double()
    pools, alphas = [], []
    mem = M.transpose(0, 1)                                        # (B, L, D)
    masked_mem = mem * mask.unsqueeze(2)
    for t in range(X.shape[0]):
        q = X[t].unsqueeze(1)                                      # (B, 1, D)
        score = torch.bmm(q, masked_mem.transpose(1, 2)) * mask.unsqueeze(1)
        w = torch.softmax(torch.tanh(score), dim=2) * mask.unsqueeze(1)
        alpha = w / w.sum(dim=2, keepdim=True)
        pools.append(torch.bmm(alpha, mem)[:, 0, :])
        alphas.append(alpha[:, 0, :])
    return torch.stack(pools), torch.stack(alphas)


def closed_form(X, M, mask, zero_rows=True):
    """z = <X, M>, e = mask exp(tanh z), alpha = e / sum e, pool = alpha M.  ``zero_rows``: a dialogue whose mask row is all zero
    gives zeros (the package's rule) instead of the reference's 0 / 0."""
    X, M, mask = X.double(), M.double(), mask.double()
    z = torch.einsum("tbd,sbd->tbs", X, M)
    e = (mask != 0).double().unsqueeze(0) * torch.exp(torch.tanh(z))
    S = e.sum(2, keepdim=True)
    if zero_rows:
        S = torch.where(S == 0, torch.ones_like(S), S)
    alpha = e / S
    return torch.einsum("tbs,sbd->tbd", alpha, M), alpha


def bounded_reference(X, M, mask, G):
    """{name: (want, bound)} for pool, alpha and the gradients dX, dM of sum(pool * G) (alpha is not differentiated through).
    Values: float64 autograd on the closed form.  Bounds: |got - want| <= (n + 16) u mag, n the number of summed terms, mag the
    formula with absolute terms; a quantity computed from an earlier rounded one adds that one's bound times the derivative's
    magnitude (z -> tanh -> exp -> row sum -> alpha -> pool; dP, alpha -> r -> dz -> dX, dM).  In dz the factor 1 - tanh^2 is
    formed in float32 from the stored tanh: its absolute error is 2 |tanh| times tanh's bound plus 2 u for the square and the
    difference (near saturation the factor is small and this is what matters); dP - r cancels, so its mag is |dP| + |r|."""
    X = X.detach().double().cpu().requires_grad_(True)
    M = M.detach().double().cpu().requires_grad_(True)
    mask, G = mask.detach().double().cpu(), G.detach().double().cpu()
    Tq, B, D = X.shape
    L = M.shape[0]
    pool, alpha = closed_form(X, M, mask)
    dX, dM = torch.autograd.grad(pool, (X, M), G)
    X, M, pool, alpha = X.detach(), M.detach(), pool.detach(), alpha.detach()
    keep = (mask != 0).double().unsqueeze(0)                       # (1, B, L)
    aX, aM, aG = X.abs(), M.abs(), G.abs()
    k16 = 16 * U
    kD, kL, kT = (D + 16) * U, (L + 16) * U, (2 * Tq + 16) * U
    # forward chain
    z = torch.einsum("tbd,sbd->tbs", X, M)
    b_z = kD * torch.einsum("tbd,sbd->tbs", aX, aM)
    th = torch.tanh(z)
    sech2 = 1 - th * th
    b_th = k16 * th.abs() + sech2 * b_z
    e = keep * torch.exp(th)
    b_e = keep * (k16 * e + e * b_th)
    S = e.sum(2, keepdim=True)
    b_S = kL * S + b_e.sum(2, keepdim=True)
    Ssafe = torch.where(S == 0, torch.ones_like(S), S)
    b_alpha = k16 * alpha + b_e / Ssafe + alpha * b_S / Ssafe
    b_pool = kL * torch.einsum("tbs,sbd->tbd", alpha, aM) + torch.einsum("tbs,sbd->tbd", b_alpha, aM) + TINY
    # backward chain
    dP = torch.einsum("tbd,sbd->tbs", G, M)
    b_dP = kD * torch.einsum("tbd,sbd->tbs", aG, aM)
    r = (alpha * dP).sum(2, keepdim=True)
    b_r = kL * (alpha * dP.abs()).sum(2, keepdim=True) + (b_alpha * dP.abs() + alpha * b_dP).sum(2, keepdim=True)
    dz = alpha * (dP - r) * sech2
    b_dz = (k16 * alpha * (dP.abs() + r.abs()) * sech2 + b_alpha * (dP - r).abs() * sech2 + alpha * (b_dP + b_r) * sech2
            + alpha * (dP - r).abs() * (2 * th.abs() * b_th + 2 * U))
    b_dX = kL * torch.einsum("tbs,sbd->tbd", dz.abs(), aM) + torch.einsum("tbs,sbd->tbd", b_dz, aM) + TINY
    b_dM = (kT * (torch.einsum("tbs,tbd->sbd", dz.abs(), aX) + torch.einsum("tbs,tbd->sbd", alpha, aG))
            + torch.einsum("tbs,tbd->sbd", b_dz, aX) + torch.einsum("tbs,tbd->sbd", b_alpha, aG) + TINY)
    return {"pool": (pool, b_pool), "alpha": (alpha, b_alpha + TINY), "dX": (dX, b_dX), "dM": (dM, b_dM)}, float(z.abs().max())
