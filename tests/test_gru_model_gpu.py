"""GPU: GRUModel (recurrent_models.py: BiGRU + masked matching attention on K14) and MaskedNLLLoss (K15) against goldens exported
from the reference (tests/golden/make_golden_gru_model.py) and against the float64 restatement of the model
(tests/gru_model_ref.py).

Tolerances: reference goldens use tests/test_variants_gpu.py's figures (|log_prob| < 1e-4, loss < 1e-5, gradients and digests
< 2e-4 relative); float64 comparisons use tests/test_fusion_kernels_gpu.py's rel_max < 1e-5."""
import os

import numpy as np
import pytest
import torch

import gru_model_ref as GR
from mm_dfn_amd import GRUModel, MaskedNLLLoss, MatchingAttention, ops, ops_flags, synthetic, train
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


def build(name, seed, dropout=0.0):
    D_m, L, lengths, C, att2 = GR.CASES[name]
    m = GRUModel(D_m, GR.D_E, GR.D_H, n_classes=C, dropout=dropout, att2=att2)
    sd = synthetic.seeded_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    return m.to(DEV), sd, GR.case_inputs(name, seed + 1)


def flat_logp(log_prob):
    return log_prob.transpose(0, 1).contiguous().view(-1, log_prob.shape[2])


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "gru_model.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def float64_results():
    """name -> (log_prob, alpha, emotions, loss_plain, loss_weighted, gradients of the weighted loss), computed once."""
    seed = int(np.load(os.path.join(GOLD, "gru_model.npz"))["seed"])
    out = {}
    for name, (D_m, L, lengths, C, att2) in GR.CASES.items():
        sd = synthetic.seeded_state_dict(GRUModel(D_m, GR.D_E, GR.D_H, C, 0.0, att2).state_dict(), seed)
        P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        U, _, umask, label, weight = GR.case_inputs(name, seed + 1)
        lp, alpha, emotions = GR.forward64(P, U, umask, att2)
        l1 = GR.masked_nll(flat_logp(lp), label, umask)
        l2 = GR.masked_nll(flat_logp(lp), label, umask, weight)
        l2.backward()
        out[name] = (lp.detach(), None if alpha is None else alpha.detach(), emotions.detach(), l1.item(), l2.item(),
                     {k: p.grad for k, p in P.items()})
    return out


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_golden_cases_and_float64(name, golden, float64_results):
    g = golden
    seed = int(g["seed"])
    D_m, L, lengths, C, att2 = GR.CASES[name]
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
    for k, gr in grads.items():
        key = name + "/digest/" + k
        if key in g.files:
            want = g[key]
            assert gr is not None, k
            assert abs(GR.digest(gr)[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
            assert rel_max(gr, grads64[k]) < 1e-5, k
        else:                                                       # (att2=False: the attention's transform is not on the path)
            assert k.startswith("matchatt.") and (gr is None or float(gr.abs().max()) == 0.0), k
    stored = [x[len(name) + 6:] for x in g.files if x.startswith(name + "/grad/")]
    assert "gru.weight_ih_l0" in stored and "linear.weight" in stored and (not att2 or "matchatt.transform.weight" in stored)
    for k in stored:
        want = g[name + "/grad/" + k]
        got = grads[k][::GR.GRAD_ROWS[k][name]].cpu().numpy()
        assert np.abs(got - want).max() / np.abs(want).max() < 2e-4, k


def test_one_query_forward_equals_row_of_forward_all():
    torch.manual_seed(3)
    att = MatchingAttention(200, 200, att_type='general2').to(DEV)
    L, B = 19, 3
    M = torch.randn(L, B, 200, device=DEV) * 0.3
    mask = torch.ones(B, L, device=DEV)
    mask[1, 11:] = 0.0
    mask[2, 4] = 0.0
    with torch.no_grad():
        pool_all, alpha_all = att.forward_all(M, mask)
        assert tuple(pool_all.shape) == (L, B, 200) and tuple(alpha_all.shape) == (L, B, L)
        for t in (0, 7, L - 1):
            pool, alpha = att(M, M[t], mask)
            assert tuple(pool.shape) == (B, 200) and tuple(alpha.shape) == (B, 1, L)
            # the same kernel on the same operands; only the query's transform runs with other rows beside it
            assert rel_max(pool, pool_all[t]) < 1e-5 and rel_max(alpha[:, 0], alpha_all[t]) < 1e-5
        pool, alpha = att(M, M[2])                                   # mask=None: every key counts
        ref_pool, ref_alpha = att.forward_all(M, None)
        assert rel_max(pool, ref_pool[2]) < 1e-5
    small = MatchingAttention(200, 40, att_type='general2').to(DEV)  # mem_dim != cand_dim: the transform maps to mem_dim
    with torch.no_grad():
        pool, alpha = small(M, torch.randn(B, 40, device=DEV), mask)
    assert tuple(pool.shape) == (B, 200) and bool(torch.isfinite(pool).all())
    with pytest.raises(ValueError):
        small.forward_all(M, mask)


def test_dropout_step_against_float64_on_replayed_flags():
    """p = 0.5: the keep flags of the two dropout sites (between the GRU layers, in front of smax_fc) are read from the tap and
    replayed in the float64 restatement; log_prob and every gradient are compared, and every tapped draw is used exactly once."""
    name, p = "a", 0.5
    D_m, L, lengths, C, att2 = GR.CASES[name]
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
    assert sorted((site, n) for n, pp, t, site in draws) == [("gru", L * B * 2 * GR.D_E), ("head", L * B * GR.D_H)]
    assert all(pp == p for _, pp, _, _ in draws)
    used = {site: 0 for _, _, _, site in draws}
    flags = {}
    for n, pp, t, site in draws:
        flags[site] = t.detach().cpu()
        used[site] += 1
        kept = float(flags[site].mean())
        assert set(flags[site].unique().tolist()) <= {0.0, 1.0} and 0.35 < kept < 0.65, (site, kept)
    assert used == {"gru": 1, "head": 1}
    P = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    lp64, _, _ = GR.forward64(P, U, umask, att2, gru_keep=flags["gru"], head_keep=flags["head"], p=p)
    GR.masked_nll(flat_logp(lp64), label, umask, weight).backward()
    assert rel_max(log_prob, lp64) < 1e-5
    for k, prm in m.named_parameters():
        assert rel_max(prm.grad, P[k].grad) < 1e-5, k


def test_training_step_launches_no_library_gemm():
    """Every dense product of a GRUModel training step runs on this package's kernels: no Tensile (`Cijk_*`) kernel, no ATen
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
        assert any("match_att_rows" in n for n in names) and any("match_att_keys" in n for n in names), names
        assert any("gru_seq" in n for n in names) and any("masked_nll" in n for n in names), names
        bad = [n for n in names if n.startswith("Cijk_") or ("gemm" in n.lower() and "gemm_tn" not in n)
               or "miopen" in n.lower() or "bmm" in n.lower()]
        assert not bad, names


class _Loader(list):
    pass


def test_three_steps_of_train_or_eval_model_with_flat_adam_against_float64_adam():
    """Optimizer settings: the reference script's own (run_train_erc.py:300-302,512: Adam, lr 3e-4, weight_decay 1e-4).  Adam
    divides every gradient entry by its own running magnitude, so what reaches a parameter is lr times the entry's RELATIVE
    error: entries far below a tensor's typical gradient carry float32 relative errors of ~1e-3, and at lr = 1e-3 without
    weight decay the recurrent weights of the reverse direction ended at 2.4e-5 of the tensor's largest entry after three steps
    (measured once, gru.weight_hh_l0_reverse) -- every gradient of these batches is within 1e-5 of float64
    (test_golden_cases_and_float64).  The bound is the issue's: < 1e-5 of the tensor's largest entry after step 3."""
    name = "a"
    D_m, L, lengths, C, att2 = GR.CASES[name]
    m, sd, _ = build(name, 9)
    batches = [GR.case_inputs(name, 100 + i) for i in range(3)]
    loader = _Loader([(U, U[:, :, :4], U[:, :, :4], qmask, umask, label, ["v%d" % i]) for i, (U, qmask, umask, label, _) in
                      enumerate(batches)])
    weight = batches[0][4]
    opt = FlatAdam(m, lr=3e-4, weight_decay=1e-4)
    res = train.train_or_eval_model(m, MaskedNLLLoss(weight.to(DEV)), loader, 0, True, opt, cuda_flag=True,
                                    target_names=["c%d" % i for i in range(C)])
    assert len(res) == 9 and res[8] == [[], [], [], []]
    assert res[4].shape == res[5].shape == res[6].shape == (3 * L * len(lengths),)
    # the same three steps in float64 torch
    P = {k: torch.nn.Parameter(v.double()) for k, v in sd.items()}
    ref_opt = torch.optim.Adam(list(P.values()), lr=3e-4, weight_decay=1e-4)
    losses, counts = [], []
    for U, qmask, umask, label, _ in batches:
        ref_opt.zero_grad()
        lp64, _, _ = GR.forward64(P, U, umask, att2)
        loss = GR.masked_nll(flat_logp(lp64), label, umask, weight)
        loss.backward()
        ref_opt.step()
        losses.append(float(loss))
        counts.append(float(umask.sum()))
    got = m.state_dict()
    for k in P:
        assert rel_max(got[k], P[k]) < 1e-5, k
    want_loss = round(sum(l * c for l, c in zip(losses, counts)) / sum(counts), 4)
    assert abs(res[2] - want_loss) <= 1.0001e-4
    # an evaluation pass returns the attention weights of every batch
    ev = train.train_or_eval_model(m, MaskedNLLLoss(weight.to(DEV)), loader, 0, False, None, cuda_flag=True)
    assert len(ev[8][0]) == 3 * L and tuple(ev[8][0][0].shape) == (len(lengths), L) and ev[8][3] == ["v0", "v1", "v2"]


def test_dialogue_model_bits_unchanged_around_a_gru_model_forward():
    """The shared bigru2: the DialogueGNNModel cfg of test_variants_gpu.CASES['avl_lstm'] gives the same bits before and after
    a GRUModel forward + backward in the same process."""
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


def test_wide_first_layer_on_the_stacked_copy_fallback_and_pairing():
    """gru.bigru2 with a first layer of another input width (D_m = 600): parameters that an owner has laid out non-adjacently
    (marked as FlatAdam marks its slots) take the copied stacked operand, which must leave the first layer's (300, 600) weights
    out; the result equals the adjacent-view path's.  ``pair_gru_weights`` pairs such a module."""
    from mm_dfn_amd import gru as fused
    name = "b"
    D_m, L, lengths, C, att2 = GR.CASES[name]
    outs = []
    for flagged in (False, True):
        m, sd, (U, qmask, umask, label, weight) = build(name, 3)
        m.train()
        if flagged:
            for prm in m.gru.parameters():
                prm._mmdfn_flat = True
            assert fused._stacked_view(m.gru.weight_ih_l1, m.gru.weight_ih_l1_reverse) is None
        else:
            assert fused.pair_gru_weights(m) == 4
            assert fused._adjacent(m.gru.weight_ih_l0, m.gru.weight_ih_l0_reverse)
        lp = m(U.to(DEV), qmask.to(DEV), umask.to(DEV))[0]
        train.backward(MaskedNLLLoss()(flat_logp(lp), label.view(-1).to(DEV), umask.to(DEV)))
        ops.join_weight_grads()
        outs.append((lp.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert rel_max(outs[1][1][k], outs[0][1][k]) < 1e-5, k
