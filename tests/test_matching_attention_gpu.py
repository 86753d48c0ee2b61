"""GPU: the matching-attention kernels (csrc/matching_attention.hip, K14) driven directly through ``ops.matching_attention`` at
their launch edges -- dialogue lengths around the 16-key / 16-query tile, one query against many keys, several workgroups per
dialogue, a width that fills a fraction of one column tile -- against float64 (tests/matching_attention_ref.py).

Bounds are the derived ones of tests/test_fusion_kernels_gpu.py: elementwise |got - want| <= (n + 16) u mag (+ 2^-126), chained
through the quantities each output is computed from (matching_attention_ref.bounded_reference).  Every case prints its worst
error-to-bound ratio per output.

Masks of a five-dialogue batch: full; a prefix of length 1; holes (the mask is read, not a length); all zero (zeros expected,
finite everywhere, the other dialogues unaffected: each is checked against its own float64 value); valid keys that end before
the last key tile begins.  One-dialogue batches run a full and a holed mask."""
import pytest
import torch

import matching_attention_ref as R
from mm_dfn_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (Tq, L): Tq = L around the tile edges, one query against 17 keys, the flagship length
SHAPES = [(1, 1), (3, 3), (15, 15), (16, 16), (17, 17), (33, 33), (130, 130), (1, 17), (110, 110)]


def masks_for(L, B, g):
    if B == 1:
        holes = (torch.rand(1, L, generator=g) < 0.6).float()
        holes[0, int(torch.randint(0, L, (1,), generator=g))] = 1.0
        return [torch.ones(1, L), holes]
    m = torch.zeros(B, L)
    m[0] = 1.0                                                      # full (a prefix of length L)
    m[1, :1] = 1.0                                                  # prefix of length 1
    m[2] = (torch.rand(L, generator=g) < 0.5).float()               # holes
    m[2, L - 1] = 1.0
    m[2, L // 2] = 0.0 if L > 2 else m[2, L // 2]
    # m[3]: all zero
    last_tile = 16 * ((L - 1) // 16)
    m[4, :max(1, last_tile - 1 if last_tile else L // 2)] = 1.0     # ends before the last key tile begins (when there are two)
    return [m]


def run_case(Tq, L, B, D, scale, mask, seed):
    g = torch.Generator().manual_seed(seed)
    # z is a sum of D products: standard deviation sc^2 sqrt(D).  "sat": sigma 1.3, |z| reaches ~4 (tanh saturating);
    # "small": |z| stays below 0.1
    sigma = 1.3 if scale == "sat" else 0.015
    sc = (sigma / D ** 0.5) ** 0.5
    X = sc * torch.randn(Tq, B, D, generator=g)
    M = sc * torch.randn(L, B, D, generator=g)
    G = torch.randn(Tq, B, D, generator=g)
    ref, zmax = R.bounded_reference(X, M, mask, G)
    Xd, Md = X.to(DEV).requires_grad_(True), M.to(DEV).requires_grad_(True)
    pool, alpha = ops.matching_attention(Xd, Md, mask.to(DEV))
    assert not alpha.requires_grad
    pool.backward(G.to(DEV))
    got = {"pool": pool, "alpha": alpha, "dX": Xd.grad, "dM": Md.grad}
    tag = "match_att[Tq=%d,L=%d,B=%d,D=%d,%s,|z|<=%.2f] " % (Tq, L, B, D, scale, zmax)
    for name in ("pool", "alpha", "dX", "dM"):
        want, bound = ref[name]
        gt = got[name].detach().double().cpu()
        assert tuple(gt.shape) == tuple(want.shape), (tag, name)
        assert bool(torch.isfinite(gt).all()), tag + name + ": not finite"
        ratio = float(((gt - want).abs() / bound).max())
        print("RATIO %s%s %.3f" % (tag, name, ratio))
        assert ratio <= 1.0, "%s%s: error / bound = %.3f" % (tag, name, ratio)
    rows = mask.sum(1) > 0
    asum = alpha.double().sum(2).cpu()
    assert float((asum[:, rows] - 1.0).abs().max()) <= (L + 16) * R.U
    if bool((~rows).any()):                                         # the all-zero dialogue: exact zeros
        for name in got:
            assert float(got[name].detach()[:, ~rows.to(DEV)].abs().max()) == 0.0, tag + name
    # a second identical call gives the same bits
    X2, M2 = X.to(DEV).requires_grad_(True), M.to(DEV).requires_grad_(True)
    pool2, alpha2 = ops.matching_attention(X2, M2, mask.to(DEV))
    pool2.backward(G.to(DEV))
    for a, b in ((pool, pool2), (alpha, alpha2), (Xd.grad, X2.grad), (Md.grad, M2.grad)):
        assert torch.equal(a, b), tag + "not bit-reproducible"
    return zmax


@pytest.mark.parametrize("D", [200, 12])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Tq,L", SHAPES)
def test_matching_attention_against_float64(Tq, L, B, D):
    if L == 110:
        B = 2 if B == 1 else B
    g = torch.Generator().manual_seed(7 * L + B)
    if B == 2:
        m = torch.ones(2, L)
        m[1, 70:] = 0.0
        m[1, 5] = 0.0
        masks = [m]
    else:
        masks = masks_for(L, B, g)
    for k, mask in enumerate(masks):
        for scale in ("sat", "small"):
            zmax = run_case(Tq, L, B, D, scale, mask, 1000 * L + 10 * B + D + k)
            if scale == "small":
                assert zmax < 0.1
            elif D == 200 and Tq * L * B >= 1000:
                assert zmax > 3.5


def test_unsupported_shapes_raise():
    mask = torch.ones(2, 5, device=DEV)
    for D in (6, 2, 260):
        X = torch.zeros(5, 2, D, device=DEV)
        with pytest.raises(ValueError):
            ops.matching_attention(X, X.clone(), mask)
    L = ops._hip.query("mmdfn_match_att_max_len") + 1
    assert L - 1 >= 512
    assert ops._hip.query("mmdfn_match_att_max_width") >= 256
    with pytest.raises(ValueError):
        ops.matching_attention(torch.zeros(1, 1, 8, device=DEV), torch.zeros(L, 1, 8, device=DEV), torch.ones(1, L, device=DEV))
    with pytest.raises(ValueError):                                  # shapes that do not belong together
        ops.matching_attention(torch.zeros(3, 2, 8, device=DEV), torch.zeros(5, 2, 8, device=DEV), torch.ones(2, 4, device=DEV))


def test_longest_served_dialogue_and_widest_row():
    """L at the cap (the 16 x L score tile fills the LDS allocation) and D at the widest served row, one launch each way."""
    L = int(ops._hip.query("mmdfn_match_att_max_len"))
    D = int(ops._hip.query("mmdfn_match_att_max_width"))
    mask = torch.ones(1, L)
    mask[0, 100:900] = 0.0
    run_case(3, L, 1, D, "sat", mask, 5)
