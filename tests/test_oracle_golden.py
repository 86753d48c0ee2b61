"""CPU: the oracle restatement against the golden vectors exported from the real reference
(tests/golden/make_golden.py).  This is what pins the oracle on machines without /root/reference."""
import os

import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd import synthetic

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def test_focal_loss():
    g = load("focal.npz")
    rs = np.random.RandomState(400)
    logp = torch.log_softmax(torch.from_numpy(rs.randn(50, 6).astype(np.float32)), 1).requires_grad_(True)
    tgt = torch.from_numpy(rs.randint(0, 6, size=50))
    alpha = torch.from_numpy(rs.uniform(0.5, 2.0, size=6).astype(np.float32))
    for tag, a, gamma in (("plain", None, 0.0), ("g05", None, 0.5), ("alpha_g1", alpha, 1.0)):
        logp.grad = None
        l = O.focal_loss(logp, tgt, gamma, a)
        l.backward()
        assert abs(l.item() - float(g["loss_" + tag])) < 1e-6
        assert np.abs(logp.grad.numpy() - g["grad_" + tag]).max() < 1e-7


def test_adjacency_forward_backward():
    g = load("adjacency.npz")
    for ci in range(3):
        lengths = [int(x) for x in g["lengths%d" % ci]]
        rs = np.random.RandomState(200 + ci)
        N = sum(lengths)
        feats = [torch.from_numpy(rs.randn(N, 200).astype(np.float32)).requires_grad_(True) for _ in range(3)]
        R = torch.from_numpy(rs.randn(3 * N, 3 * N).astype(np.float32))
        A = O.create_big_adj(feats, lengths)
        assert np.abs(A.detach().numpy() - g["adj%d" % ci]).max() < 2e-5
        (A * R).sum().backward()
        got = np.stack([f.grad.numpy() for f in feats], 0)
        want = g["dfeats%d" % ci]
        assert np.abs(got - want).max() / np.abs(want).max() < 1e-4
        # packed block-tile form == dense form
        t, c, _ = O.adjacency_tiles([f.detach() for f in feats], lengths)
        assert (O.tiles_to_dense(t, c, lengths, 3) - A.detach()).abs().max() < 1e-6


def test_gcnii_stack():
    g = load("gcnii.npz")
    for ci in range(3):
        nl, reason = [int(x) for x in g["cfg%d" % ci]]
        rs = np.random.RandomState(300 + ci)
        lengths = [9, 4]
        N = sum(lengths)
        shapes = {"convs.%d.weight" % i: torch.empty(200, 100) for i in range(nl)}
        shapes.update({"fcs.0.weight": torch.empty(100, 200), "fcs.0.bias": torch.empty(100),
                       "rnn.weight_ih_l0": torch.empty(400, 100), "rnn.weight_hh_l0": torch.empty(400, 100),
                       "rnn.bias_ih_l0": torch.empty(400), "rnn.bias_hh_l0": torch.empty(400)})
        params = {k: v.requires_grad_(True) for k, v in synthetic.seeded_state_dict(shapes, 300 + ci).items()}
        x = torch.from_numpy(rs.randn(3 * N, 200).astype(np.float32)).requires_grad_(True)
        feats = [torch.from_numpy(rs.randn(N, 200).astype(np.float32)) for _ in range(3)]
        adj = O.create_big_adj(feats, lengths)
        R = torch.from_numpy(rs.randn(3 * N, 300).astype(np.float32))
        y = O.gcnii_stack(x, adj, params, "", nl, 0.5, 0.2, reason_flag=bool(reason))
        assert np.abs(y.detach().numpy() - g["y%d" % ci]).max() < 2e-5
        (y * R).sum().backward()
        assert np.abs(x.grad.numpy() - g["dx%d" % ci]).max() / np.abs(g["dx%d" % ci]).max() < 1e-4
        assert np.abs(params["convs.0.weight"].grad.numpy() - g["dW0_%d" % ci]).max() / np.abs(g["dW0_%d" % ci]).max() < 1e-4


E2E = {
    "iemocap_b1": (dict(B=1, L=110, P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512), 101, [110]),
    "iemocap_ragged_refdims": (dict(B=4, L=60, P=2, C=6, nlayers=2, D_t=100, D_a=1582, D_v=342), 102, [60, 27, 41, 33]),
    "meld_like": (dict(B=6, L=33, P=9, C=7, nlayers=4, D_t=600, D_a=300, D_v=342), 103, [33, 3, 17, 9, 24, 1]),
    "deep16": (dict(B=3, L=20, P=2, C=6, nlayers=16, D_t=100, D_a=100, D_v=512), 104, [20, 13, 7]),
}


def _digest(g):
    g = g.detach().double().reshape(-1)
    return np.array([g.sum().item(), g.abs().sum().item(), (g * g).sum().item()])


@pytest.mark.parametrize("name", ["iemocap_ragged_refdims", "meld_like", "deep16"])
def test_end_to_end_logits_and_grads(name):
    cfg, seed, lengths = E2E[name]
    g = load("e2e_%s.npz" % name)
    model = synthetic.build_model(**cfg)
    params = {k: v.clone().requires_grad_(True) for k, v in
              synthetic.seeded_state_dict(model.state_dict(), seed).items()}
    b = synthetic.make_batch(seed + 1, lengths=lengths, **cfg)
    ocfg = O.default_cfg(cfg["nlayers"])
    logp = O.forward(params, b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"], ocfg,
                     engine="aten")
    assert np.abs(logp.detach().numpy() - g["log_prob"]).max() < 1e-4
    label = O.flatten_labels(b["label"], b["lengths"])
    loss = O.focal_loss(logp, label, 0.5)
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    loss.backward()
    live = [str(x) for x in g["live_params"]]
    for k in live:
        want = g["gd/" + k]
        got = _digest(params[k].grad)
        assert abs(got[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
    for k in params:
        if k not in live:
            assert params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, k
    for k in [x[2:] for x in g.files if x.startswith("g/")]:
        want = g["g/" + k]
        assert np.abs(params[k].grad.numpy() - want).max() / np.abs(want).max() < 1e-4, k


def test_three_step_training_trace():
    g = load("train_trace.npz")
    cfg = dict(B=3, L=24, P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)
    model = synthetic.build_model(**cfg)
    params = {k: v.clone().requires_grad_(True) for k, v in
              synthetic.seeded_state_dict(model.state_dict(), 500).items()}
    opt = torch.optim.Adam(list(params.values()), lr=3e-4, weight_decay=1e-4)
    ocfg = O.default_cfg(2)
    losses, preds = [], []
    for s, lengths in enumerate([[24, 11, 17], [9, 24, 2], [13, 13, 20]]):
        b = synthetic.make_batch(600 + s, lengths=lengths, **cfg)
        opt.zero_grad()
        lens = O.lengths_from_umask(b["umask"])
        assert lens == lengths
        logp = O.forward(params, b["textf"], b["qmask"], b["umask"], lens, b["acouf"], b["visuf"], ocfg, engine="aten")
        loss = O.focal_loss(logp, O.flatten_labels(b["label"], lens), 0.5)
        loss.backward()
        opt.step()
        losses.append(round(loss.item(), 4))
        preds.append(logp.argmax(1).numpy())
    assert np.abs(np.array(losses) - g["losses"]).max() < 2e-4
    assert (np.concatenate(preds) == g["preds"]).mean() > 0.99
    assert np.abs(params["smax_fc.weight"].detach().numpy() - g["smax_fc.weight"]).max() < 1e-5
    assert np.abs(params["graph_model.graph_net.convs.1.weight"].detach().numpy() - g["convs1"]).max() < 1e-5


DEEP_CFG = dict(B=3, L=14, P=2, C=6, nlayers=3, D_t=100, D_a=100, D_v=512)
DEEP_LENGTHS = [14, 5, 9]


def deep_state(att_type="concat_subsequently", reason_flag=True):
    m = synthetic.build_model(graph_type="DeepGCN", att_type=att_type, reason_flag=reason_flag, **DEEP_CFG)
    return m, synthetic.seeded_state_dict(m.state_dict(), 800)


def test_deepgcn_state_dict_keys_match_reference():
    m, _ = deep_state()
    want = open(os.path.join(GOLD, "state_dict_keys_deepgcn.txt")).read().split("\n")[:-1]
    got = ["%s %s" % (k, "x".join(map(str, v.shape))) for k, v in m.state_dict().items()]
    assert sorted(got) == sorted(want)


def test_deepgcn_oracle_against_reference_golden():
    """graph_type='DeepGCN' (three unimodal GCNII graphs) -- eval log-probs for both fusions, and the
    gradients of the gate-less variant (the reference cannot back-propagate the gated one, see make_golden.py)."""
    g = load("deepgcn.npz")
    b = synthetic.make_batch(801, lengths=DEEP_LENGTHS, **DEEP_CFG)
    args = (b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"])
    cfg = O.default_cfg(DEEP_CFG["nlayers"])
    for att in ("concat_subsequently", "gated"):
        _, sd = deep_state(att)
        with torch.no_grad():
            logp = O.forward_deepgcn(sd, *args, cfg, att_type=att)
        assert np.abs(logp.numpy() - g["logp_" + att]).max() < 2e-5, att
    _, sd = deep_state()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logp = O.forward_deepgcn(params, *args, dict(cfg, reason_flag=False))
    assert np.abs(logp.detach().numpy() - g["logp_nogate"]).max() < 2e-5
    R = torch.from_numpy(np.random.RandomState(802).randn(*logp.shape).astype(np.float32))
    (logp * R).sum().backward()
    for k in [f[5:] for f in g.files if f.startswith("grad_")]:
        want = g["grad_" + k]
        assert np.abs(params[k].grad.numpy() - want).max() / np.abs(want).max() < 2e-4, k


ENC_CASES = {"l15_p3": (15, 3, [15, 6, 11]), "l33_p9": (33, 9, [33, 9, 1, 20]), "l110_p2": (110, 2, [110, 47])}


def enc_setup(name):
    L, P, lengths = ENC_CASES[name]
    cfg = dict(B=len(lengths), L=L, P=P, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)
    m = synthetic.build_model(**cfg)
    return cfg, synthetic.seeded_state_dict(m.state_dict(), 600), synthetic.make_batch(601, lengths=lengths, **cfg), m


@pytest.mark.parametrize("name", sorted(ENC_CASES))
def test_encoder_stack_against_reference_golden(name):
    """the features DialogueGNNModel hands to MM_GCN (projections, context BiGRU, speaker-party BiGRU,
    pad strip) for 3 / 9 / 2 speakers."""
    g = load("encoders_graphconv.npz")
    cfg, sd, b, _ = enc_setup(name)
    with torch.no_grad():
        feats = O.encoders(sd, b["textf"], b["qmask"], b["lengths"], b["acouf"], b["visuf"], O.default_cfg(2), engine="aten")
    got = torch.stack(list(feats), 0).numpy()
    assert got.shape == g["enc_" + name].shape
    assert np.abs(got - g["enc_" + name]).max() < 2e-5


def test_graph_convolution_against_reference_golden():
    """GraphConvolution.forward (variant) at layer indices 1, 2, 16."""
    g = load("encoders_graphconv.npz")
    rs = np.random.RandomState(610)
    n = 37
    w = synthetic.seeded_state_dict({"weight": torch.empty(200, 100)}, 611)["weight"]
    x = torch.from_numpy(rs.randn(n, 100).astype(np.float32))
    h0 = torch.from_numpy(rs.randn(n, 100).astype(np.float32))
    adj = torch.from_numpy(rs.uniform(0, 1, size=(n, n)).astype(np.float32))
    adj = adj / adj.sum(1, keepdim=True)
    for l in (1, 2, 16):
        assert np.abs(O.graph_convolution(x, adj, h0, 0.5, 0.2, l, w).numpy() - g["gconv_l%d" % l]).max() < 1e-5


def test_mfn_and_two_modality_gated_attention():
    """O.mfn and the two-modality form of O.gated_attention_general against the reference modules' fixtures
    (tests/golden/fusion_modules.npz, tests/golden/make_golden.py export_fusion_modules), in float64 on the seeds and inputs of
    test_model_gpu.test_mfn_and_gated_attention_modules_against_reference_golden.  The fixtures are float32 results, so the
    bounds are that test's (MFN) and its 2e-6 (gated)."""
    from mm_dfn_amd import MFN, MMGatedAttention
    g = load("fusion_modules.npz")
    rs = np.random.RandomState(700)
    params = {k: v.double().requires_grad_(True) for k, v in synthetic.seeded_state_dict(MFN().state_dict(), 700).items()}
    x = torch.from_numpy(rs.randn(9, 2, 900).astype(np.float32)).double().requires_grad_(True)
    R = torch.from_numpy(rs.randn(9, 2, 400).astype(np.float32)).double()
    y = O.mfn(x, params)
    (y * R).sum().backward()
    assert np.abs(y.detach().numpy() - g["mfn_y"]).max() < 1e-5
    assert np.abs(x.grad.numpy() - g["mfn_dx"]).max() / np.abs(g["mfn_dx"]).max() < 1e-4
    assert np.abs(params["gamma1_fc1.weight"].grad.numpy() - g["mfn_dW"]).max() / np.abs(g["mfn_dW"]).max() < 1e-4
    assert all(params[k].grad is None for k in params if k.startswith(("out_fc1.", "out_fc2.")))
    gp = {k: v.double() for k, v in synthetic.seeded_state_dict(MMGatedAttention(300, 100).state_dict(), 701).items()}
    a, v, l = (torch.from_numpy(rs.randn(11, 300).astype(np.float32)).double() for _ in range(3))
    assert np.abs(O.gated_attention_general(a, v, l, gp, prefix="").numpy() - g["gated_avl"]).max() < 2e-6
    al = O.gated_attention_general(a, v, l, gp, prefix="", modals="al")
    assert tuple(al.shape) == (11, 100) and np.abs(al.numpy() - g["gated_al"]).max() < 2e-6
    # the pair blocks of the three-modality output are the two-modality outputs, in the order av | al | vl
    avl = O.gated_attention_general(a, v, l, gp, prefix="")
    for i, pair in enumerate(("av", "al", "vl")):
        assert torch.equal(O.gated_attention_general(a, v, l, gp, prefix="", modals=pair), avl[:, 100 * i:100 * (i + 1)])
