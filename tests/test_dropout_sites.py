"""CPU: the oracle's dropout sites (mmdfn_oracle.DropoutTape / dropout_site), which tests/test_dropout_replay_gpu.py feeds
with the keep flags the device drew.

* the GRU site against two stacked single-layer torch.nn.GRU modules with the mask between them, float64;
* the graph and head sites against the REAL reference run in train() with seeded masks (tests/golden/dropout_sites.npz,
  exported by tests/golden/make_golden.py export_dropout_sites): values, gradients, and the number, order and shapes of
  the sites;
* the fixture itself is regenerated bit for bit where the reference tree is present."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd import synthetic
from test_oracle_golden import GOLD, _digest, load

sys.path.insert(0, GOLD)


@pytest.fixture
def tape_scope():
    """Installs tapes for the duration of a test and always removes them."""
    def install(tape):
        O.set_dropout_tape(tape)
        return tape
    yield install
    O.set_dropout_tape(None)


def _gru_params(seed, dtype):
    g = torch.nn.GRU(200, 100, num_layers=2, bidirectional=True)
    sd = synthetic.seeded_state_dict(g.state_dict(), seed, scale=1.5)
    return {k: v.to(dtype) for k, v in sd.items()}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", [(7, 3), (33, 40), (1, 5)])
def test_gru_site_against_two_stacked_single_layer_grus(shape, p, tape_scope):
    """O.bigru2 under a tape == layer 0 (nn.GRU) -> y1 * M / (1 - p) -> layer 1 (nn.GRU), forward and every gradient, in
    float64; both of the oracle's engines."""
    T, R = shape
    rs = np.random.RandomState(1000 + T)
    x = torch.from_numpy(rs.randn(T, R, 200))
    w = torch.from_numpy(rs.randn(T, R, 200))
    M = torch.from_numpy((rs.random_sample((T, R, 200)) >= p).astype(np.float64))
    assert 0 < float(M.mean()) < 1
    sd = _gru_params(40 + T, torch.float64)
    # the statement: two single-layer modules
    layers = []
    for layer in range(2):
        g = torch.nn.GRU(200, 100, num_layers=1, bidirectional=True).double()
        g.load_state_dict({k: sd[k.replace("_l0", "_l%d" % layer)] for k in g.state_dict()})
        layers.append(g)
    xr = x.clone().requires_grad_(True)
    y1 = layers[0](xr)[0]
    want = layers[1](y1 * M / (1 - p))[0]
    (want * w).sum().backward()
    want_grads = {k.replace("_l0", "_l%d" % layer): prm.grad for layer, g in enumerate(layers) for k, prm in g.named_parameters()}
    assert len(want_grads) == 16
    for engine in ("manual", "aten"):
        params = {"g." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
        xo = x.clone().requires_grad_(True)
        tape = tape_scope(O.DropoutTape({"site": M.float()}))       # (any dtype: the site casts the mask)
        got = O.bigru2(xo, params, "g.", p, True, engine, site="site")
        (got * w).sum().backward()
        assert tape.seen == [("site", (T, R, 200))]
        assert float((got - want).detach().abs().max()) < 1e-12, engine
        assert float((xo.grad - xr.grad).abs().max()) <= 1e-11 * float(xr.grad.abs().max()), engine
        for k, gw in want_grads.items():
            assert float((params["g." + k].grad - gw).abs().max()) <= 1e-11 * float(gw.abs().max()), (engine, k)
    # the mask matters (a tape of ones is another function) and a missing mask is the identity
    xo = x.clone()
    tape_scope(O.DropoutTape({}))
    ident = O.bigru2(xo, sd_prefixed(sd), "g.", p, True, "manual", site="site")
    tape_scope(None)
    plain = O.bigru2(xo, sd_prefixed(sd), "g.", 0.0, False, "manual")
    assert float((ident - plain).abs().max()) == 0.0
    assert float((ident - want.detach()).abs().max()) > 1e-3


def sd_prefixed(sd):
    return {"g." + k: v for k, v in sd.items()}


def test_without_a_tape_the_sites_are_torch_dropout():
    """No tape: dropout_site is F.dropout, call for call (same generator consumption), as before the hook existed."""
    x = torch.from_numpy(np.random.RandomState(5).randn(50, 40).astype(np.float32))
    assert O.set_dropout_tape(None) is None
    torch.manual_seed(11)
    got = O.dropout_site(x, 0.3, True, "anything")
    torch.manual_seed(11)
    want = torch.nn.functional.dropout(x, 0.3, True)
    assert torch.equal(got, want)
    assert O.dropout_site(x, 0.3, False, "anything") is x


def test_a_mask_of_the_wrong_shape_is_refused(tape_scope):
    x = torch.ones(4, 6)
    tape_scope(O.DropoutTape({"s": torch.ones(6, 4)}))
    with pytest.raises(ValueError):
        O.dropout_site(x, 0.5, True, "s")


class _SeededTape(O.DropoutTape):
    """Draws the mask of every graph / head site from one RandomState in call order, the way the exporter's stand-in for
    torch.nn.functional.dropout did in the reference run; the GRU sites stay off (identity), as they were there."""

    def __init__(self, seed, p):
        super().__init__()
        self.rs, self.p = np.random.RandomState(seed), p

    def mask(self, site, x):
        from make_golden import seeded_keep_mask
        self.seen.append((site, tuple(x.shape)))
        if site == "lstm_l" or site.startswith("party."):
            return None
        return seeded_keep_mask(self.rs, x.shape, self.p)


def _site_cases():
    # (imported lazily by name: make_golden imports the reference shim, which only patches anything when asked to)
    from make_golden import DROPOUT_SITE_CASES
    return DROPOUT_SITE_CASES


@pytest.mark.parametrize("name", ["p2_d50", "p2_d10", "p3_d50", "p3_d10"])
def test_graph_and_head_sites_against_the_reference(name, tape_scope):
    """The oracle in train mode with the reference run's seeded masks at its graph and head sites: log-probs, loss, the
    digest of every live gradient and the stored full gradients at the bounds of test_end_to_end_logits_and_grads; and
    the oracle's non-GRU sites are, in number, order and shape, the dropout calls the reference made -- which pins the
    position, order and scale of every one of them."""
    cfg, seed, lengths, p, mseed = _site_cases()[name]
    g = load("dropout_sites.npz")
    model = synthetic.build_model(**cfg)
    params = {k: v.clone().requires_grad_(True) for k, v in synthetic.seeded_state_dict(model.state_dict(), seed).items()}
    b = synthetic.make_batch(seed + 1, lengths=lengths, **cfg)
    ocfg = O.default_cfg(cfg["nlayers"], dropout=p)
    tape = tape_scope(_SeededTape(mseed, p))
    logp = O.forward(params, b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"], ocfg, training=True,
                     engine="aten")
    # the reference's dropout calls, in order
    ref_shapes = [tuple(int(d) for d in s) for s in g[name + "/site_shapes"]]
    ours = [(s, shape) for s, shape in tape.seen if s != "lstm_l" and not s.startswith("party.")]
    pre = "graph_model.graph_net."
    assert [s for s, _ in ours] == [pre + "x", pre + "h0"] + [pre + "conv%d" % i for i in range(cfg["nlayers"])] + ["head"]
    assert [shape for _, shape in ours] == ref_shapes
    # the GRU sites: the context GRU and one per (modality, speaker) pass -- the oracle encodes the zero-weight modality too
    gru_sites = [s for s, _ in tape.seen if s == "lstm_l" or s.startswith("party.")]
    assert sorted(gru_sites) == sorted(["lstm_l"] + ["party.%s.%d" % (m, q) for m in "avl" for q in range(cfg["P"])])
    assert np.abs(logp.detach().numpy() - g[name + "/log_prob"]).max() < 1e-4
    loss = O.focal_loss(logp, O.flatten_labels(b["label"], b["lengths"]), 0.5)
    assert abs(loss.item() - float(g[name + "/loss"])) < 1e-5
    loss.backward()
    live = [str(x) for x in g[name + "/live_params"]]
    assert len(live) >= 44
    for k in live:
        want = g[name + "/gd/" + k]
        got = _digest(params[k].grad)
        assert abs(got[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
    for k in params:
        if k not in live:
            assert params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, k
    full = [x[len(name) + 3:] for x in g.files if x.startswith(name + "/g/")]
    assert len(full) >= 5
    for k in full:
        want = g[name + "/g/" + k]
        assert np.abs(params[k].grad.numpy() - want).max() / np.abs(want).max() < 1e-4, k


def test_the_seeded_masks_matter():
    """The fixture is not a dropout-off run in disguise: its train-mode log-probs differ from the eval-mode oracle."""
    cfg, seed, lengths, p, _ = _site_cases()["p2_d50"]
    g = load("dropout_sites.npz")
    model = synthetic.build_model(**cfg)
    sd = synthetic.seeded_state_dict(model.state_dict(), seed)
    b = synthetic.make_batch(seed + 1, lengths=lengths, **cfg)
    with torch.no_grad():
        logp = O.forward(sd, b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"], O.default_cfg(2))
    assert np.abs(logp.numpy() - g["p2_d50/log_prob"]).max() > 1e-2


def test_graph_free_oracle_against_the_reference_golden():
    """O.forward_graph_free (the oracle side of the graph-free case of tests/test_dropout_replay_gpu.py) against what the
    reference gave for graph_type='None', concat_subsequently (tests/golden/fusion_baselines.npz): eval log-probs, the
    train-mode loss and the digest of every live gradient."""
    from test_fusion_baselines import CASES, CFG, build
    name = "concat_subsequently"
    g = load("fusion_baselines.npz")
    sd = build(name).state_dict()
    b = synthetic.make_batch(CASES[name][3] + 1, lengths=[14, 5, 9], **CFG)
    args = (b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"])
    ocfg = O.default_cfg(CFG["nlayers"])
    with torch.no_grad():
        logp = O.forward_graph_free({k: v.clone() for k, v in sd.items()}, *args, ocfg, engine="aten")
    assert np.abs(logp.numpy() - g[name + "/log_prob"]).max() < 1e-4
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logp = O.forward_graph_free(params, *args, ocfg, training=True, engine="aten")
    loss = O.focal_loss(logp, O.flatten_labels(b["label"], b["lengths"]), 0.5)
    assert abs(loss.item() - float(g[name + "/loss"])) < 1e-5
    loss.backward()
    live = [str(x) for x in g[name + "/live_params"]]
    assert len(live) >= 40
    for k in live:
        want, got = g[name + "/gd/" + k], _digest(params[k].grad)
        assert abs(got[1] - want[1]) / (want[1] + 1e-12) < 2e-4, k
    for k in params:
        if k not in live:
            assert params[k].grad is None or float(params[k].grad.abs().max()) == 0.0, k


def test_make_golden_regenerates_the_fixture_bit_for_bit(reference_available, tmp_path):
    """tests/golden/make_golden.py --dropout-sites-only, run against the reference tree in a process of its own (the
    reference shim patches torch.Tensor), writes exactly the arrays that are committed."""
    if not reference_available:
        pytest.skip("the reference tree is not on this machine")
    res = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden.py"), "--dropout-sites-only", "--out", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    new = np.load(os.path.join(str(tmp_path), "dropout_sites.npz"), allow_pickle=False)
    old = load("dropout_sites.npz")
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
