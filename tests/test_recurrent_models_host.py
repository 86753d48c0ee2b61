"""CPU: the host-side contract of the recurrent baseline (GRUModel, MatchingAttention, MaskedNLLLoss, K14 / K15 entry points):
state_dict keys against the reference's, constructor refusals, the loss on host tensors, the header's declarations, and the
float64 restatement of the attention (tests/matching_attention_ref.py) against the closed form the kernel implements."""
import os

import pytest
import torch

import matching_attention_ref as MA
from mm_dfn_amd import GRUModel, MaskedNLLLoss, MatchingAttention, _hip

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _keys(path):
    with open(path) as f:
        return [(ln.split()[0], tuple(int(d) for d in ln.split()[1:])) for ln in f if ln.strip()]


def test_state_dict_keys_and_shapes_match_the_reference():
    m = GRUModel(100, 100, 32, n_classes=6, dropout=0.5, att2=True)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _keys(os.path.join(GOLD, "state_dict_keys_gru_model.txt"))
    wide = GRUModel(600, 100, 100)                                   # (MELD text width; the reference's default 7 classes)
    assert tuple(wide.gru.weight_ih_l0.shape) == (300, 600) and wide.smax_fc.out_features == 7
    assert not GRUModel(100, 100, 32, att2=False).att2


def test_constructor_refusals():
    with pytest.raises(NotImplementedError):
        GRUModel(100, 150, 100)                                      # the recurrence kernels are built for H = 100
    for D_m in (342, 2, 772):
        with pytest.raises(NotImplementedError):
            GRUModel(D_m, 100, 100)
    for att_type, kw in (("dot", {}), ("general", {}), ("concat", dict(alpha_dim=8))):
        with pytest.raises(NotImplementedError, match="model.py:58-65,77-82"):
            MatchingAttention(200, 200, att_type=att_type, **kw)
    att = MatchingAttention(200, 40, att_type="general2")
    assert tuple(att.transform.weight.shape) == (200, 40) and att.transform.bias is not None


def test_masked_nll_on_host_tensors_is_the_reference_formula():
    g = torch.Generator().manual_seed(0)
    B, L, C = 3, 7, 6
    pred = torch.log_softmax(torch.randn(B * L, C, generator=g), 1).requires_grad_(True)
    target = torch.randint(0, C, (B * L,), generator=g)
    mask = (torch.rand(B, L, generator=g) < 0.7).float()
    weight = 0.5 + torch.rand(C, generator=g)
    for w in (None, weight):
        loss = MaskedNLLLoss(w)(pred, target, mask)
        got, = torch.autograd.grad(loss, pred)
        m = mask.view(-1)
        ww = torch.ones(B * L) if w is None else w[target]
        p2 = pred.detach().clone().requires_grad_(True)
        want = (m * ww * -p2[torch.arange(B * L), target]).sum() / (m * ww).sum()
        dwant, = torch.autograd.grad(want, p2)
        assert abs(loss.item() - want.item()) < 1e-6
        assert float((got - dwant).abs().max()) < 1e-7
        assert float(got[m == 0].abs().max()) == 0.0


def test_header_declares_the_new_entry_points_and_the_abi_stays_23():
    assert _hip.ABI_VERSION == 23
    for name, nargs in (("mmdfn_match_att_max_width", 0), ("mmdfn_match_att_max_len", 0), ("mmdfn_match_att_workspace", 4),
                        ("mmdfn_match_att_fwd", 11), ("mmdfn_match_att_bwd", 14), ("mmdfn_masked_nll_fwd", 10),
                        ("mmdfn_masked_nll_bwd", 9)):
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name]) == nargs, name
    import ctypes
    assert _hip.RESTYPES["mmdfn_match_att_workspace"] is ctypes.c_int64
    # the K12 signatures are untouched
    assert len(_hip.SIGNATURES["mmdfn_nll_loss_fwd"]) == 11 and len(_hip.SIGNATURES["mmdfn_nll_loss_bwd"]) == 9


def test_cpu_tensors_raise_on_the_device_operators():
    from mm_dfn_amd import ops
    with pytest.raises(_hip.HipLibraryError):
        ops.matching_attention(torch.zeros(2, 1, 8), torch.zeros(2, 1, 8), torch.ones(1, 2))
    with pytest.raises(_hip.HipLibraryError):
        GRUModel(100, 100, 32)(torch.zeros(3, 2, 100), torch.zeros(3, 2, 2), torch.ones(2, 3))


@pytest.mark.parametrize("Tq,L,B,D", [(1, 1, 1, 4), (5, 5, 3, 12), (1, 17, 2, 8), (9, 9, 4, 200)])
def test_reference_loop_restatement_agrees_with_the_closed_form(Tq, L, B, D):
    g = torch.Generator().manual_seed(L + D)
    X = torch.randn(Tq, B, D, dtype=torch.float64, generator=g) * 0.5
    M = torch.randn(L, B, D, dtype=torch.float64, generator=g) * 0.5
    mask = (torch.rand(B, L, generator=g) < 0.6).double()            # holes
    mask[:, 0] = 1.0
    if B > 1:
        mask[1] = 0.0
        mask[1, : max(1, L // 2)] = 1.0                              # a prefix
    pool, alpha = MA.reference_loop(X, M, mask)
    cpool, calpha = MA.closed_form(X, M, mask)
    assert float((pool - cpool).abs().max()) < 1e-14 and float((alpha - calpha).abs().max()) < 1e-14
    assert float((alpha.sum(2) - 1.0).abs().max()) < 1e-14 and float(alpha[:, mask == 0].abs().max() if bool((mask == 0).any()) else 0) == 0.0
    # an all-zero mask row: the reference divides 0 by 0, the package's rule is zeros
    mask[0] = 0.0
    assert bool(torch.isnan(MA.reference_loop(X, M, mask)[1][:, 0]).all())
    zp, za = MA.closed_form(X, M, mask)
    assert float(zp[:, 0].abs().max()) == 0.0 and float(za[:, 0].abs().max()) == 0.0
