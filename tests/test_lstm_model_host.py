"""CPU: the host-side contract of LSTMModel and the K16 entry points (csrc/lstm_seq.hip): state_dict keys against the
reference's, constructor refusals, the header's declarations, the refusals of the two entry points (no device needed: they
return before any HIP call), the float64 restatement (tests/lstm_model_ref.py) against the reference's goldens and against
torch.nn.LSTM in double, and the headroom of the GPU test's figures on honest float32."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lstm_model_ref as LR
from mm_dfn_amd import LSTMModel, _hip, synthetic

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _keys(path):
    with open(path) as f:
        return [(ln.split()[0], tuple(int(d) for d in ln.split()[1:])) for ln in f if ln.strip()]


def rel_max(got, want):
    got, want = got.detach().double(), want.detach().double()
    assert tuple(got.shape) == tuple(want.shape)
    den = float(want.abs().max())
    return float((got - want).abs().max()) / den if den else float(got.abs().max())


def flat_logp(log_prob):
    return log_prob.transpose(0, 1).contiguous().view(-1, log_prob.shape[2])


def test_state_dict_keys_and_shapes_match_the_reference():
    m = LSTMModel(100, 100, 32, n_classes=6, dropout=0.5, att2=True)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _keys(os.path.join(GOLD, "state_dict_keys_lstm_model.txt"))
    wide = LSTMModel(600, 100, 100)
    assert tuple(wide.lstm.weight_ih_l0.shape) == (400, 600) and wide.smax_fc.out_features == 7
    assert not LSTMModel(100, 100, 32, att2=False).att2
    assert isinstance(m.lstm, torch.nn.LSTM) and m.lstm.dropout == 0.5 and m.dropout.p == 0.5


def test_constructor_refusals():
    with pytest.raises(NotImplementedError, match="LSTMModel"):
        LSTMModel(100, 150, 100)
    for D_m in (342, 2, 772):
        with pytest.raises(NotImplementedError, match="LSTMModel"):
            LSTMModel(D_m, 100, 100)


def test_cpu_tensors_raise():
    with pytest.raises(_hip.HipLibraryError):
        LSTMModel(100, 100, 32)(torch.zeros(3, 2, 100), torch.zeros(3, 2, 2), torch.ones(2, 3))


def test_header_declares_the_entry_points_and_the_abi_stays_23():
    assert _hip.ABI_VERSION == 23
    assert len(_hip.SIGNATURES["mmdfn_lstm_seq_fwd"]) == 9 and len(_hip.SIGNATURES["mmdfn_lstm_seq_bwd"]) == 9
    assert _hip.SIGNATURES["mmdfn_lstm_seq_fwd"] == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert _hip.SIGNATURES["mmdfn_lstm_seq_bwd"] == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert _hip.SIGNATURES["mmdfn_lstm_seq_block_steps"] == [] and _hip.RESTYPES["mmdfn_lstm_seq_fwd"] is ctypes.c_int
    # the GRU signatures are untouched
    assert len(_hip.SIGNATURES["mmdfn_gru_seq_fwd"]) == 11 and len(_hip.SIGNATURES["mmdfn_gru_seq_bwd"]) == 12


def test_refused_calls_return_minus_one_before_any_device_call():
    """Every refusal of the header's contract, one violation per call (never a valid call: nothing may launch here)."""
    P = ctypes.c_void_p(4096)                                   # a non-null value that is never dereferenced
    pair = lambda: (ctypes.c_void_p * 2)(4096, 4096)            # host arrays: these ARE read, their entries are not
    half_null = (ctypes.c_void_p * 2)(4096, None)
    T, R, H = 3, 2, 100
    assert _hip.query("mmdfn_lstm_seq_block_steps") >= 1
    fwd = lambda gi, w, b, y, st, rows, t, h: _hip.call("mmdfn_lstm_seq_fwd", gi, w, b, y, st, rows, t, h, None, allow=(-1,))
    bwd = lambda dy, y, st, w, dg, rows, t, h: _hip.call("mmdfn_lstm_seq_bwd", dy, y, st, w, dg, rows, t, h, None, allow=(-1,))
    for h, t, rows in ((64, T, R), (H, 0, R), (H, -1, R), (H, T, 0), (H, T, -2)):
        assert fwd(P, pair(), pair(), P, P, rows, t, h) == -1
        assert bwd(P, P, P, pair(), P, rows, t, h) == -1
    for k in range(5):
        args = [P, pair(), pair(), P, P]
        args[k] = None
        assert fwd(*args, R, T, H) == -1
        args = [P, P, P, pair(), P]
        args[k] = None
        assert bwd(*args, R, T, H) == -1
    assert fwd(P, half_null, pair(), P, P, R, T, H) == -1 and fwd(P, pair(), half_null, P, P, R, T, H) == -1
    assert bwd(P, P, P, half_null, P, R, T, H) == -1


def test_pairing_helper_counts_an_lstm_model_and_leaves_others_alone():
    from mm_dfn_amd import GRUModel
    from mm_dfn_amd import gru as fused_gru
    from mm_dfn_amd import lstm as fused_lstm
    assert fused_lstm._stacked_view is fused_gru._stacked_view and fused_lstm._adjacent is fused_gru._adjacent
    assert fused_lstm.pair_lstm_weights(GRUModel(100, 100, 32)) == 0
    assert fused_gru.pair_gru_weights(LSTMModel(100, 100, 32)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "lstm_model.npz"), allow_pickle=False)


def _run(name, seed, dtype, encoder=False):
    D_m, L, lengths, C, att2 = LR.CASES[name]
    sd = synthetic.seeded_state_dict(LSTMModel(D_m, LR.D_E, LR.D_H, C, 0.0, att2).state_dict(), seed)
    P = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    U, _, umask, label, weight = LR.case_inputs(name, seed + 1)
    enc = LR.torch_lstm_encoder(P) if encoder else None
    lp, alpha, emotions = LR.forward_any(P, U, umask, att2, encoder=enc)
    l1 = LR.masked_nll(flat_logp(lp), label, umask)
    l2 = LR.masked_nll(flat_logp(lp), label, umask, weight)
    l2.backward()
    return dict(lp=lp.detach(), alpha=None if alpha is None else alpha.detach(), em=emotions.detach(), l1=l1.item(), l2=l2.item(),
                grads={k: p.grad for k, p in P.items()})


@pytest.fixture(scope="module")
def results(golden):
    seed = int(golden["seed"])
    return {name: (_run(name, seed, torch.float64), _run(name, seed, torch.float32, encoder=True)) for name in LR.CASES}


def _against_golden(name, g, r, slack):
    """The figures tests/test_lstm_model_gpu.py uses against the goldens, divided by ``slack``: the worst ratio figure / bound."""
    att2 = LR.CASES[name][4]
    worst = {}
    worst["log_prob"] = np.abs(r["lp"].numpy() - g[name + "/log_prob"]).max() / 1e-4
    worst["emotions"] = np.abs(r["em"].numpy() - g[("a" if name == "c" else name) + "/emotions"]).max() / 1e-4
    if att2:
        worst["alpha"] = np.abs(r["alpha"].numpy() - g[name + "/alpha"]).max() / 1e-4
    worst["loss_plain"] = abs(r["l1"] - float(g[name + "/loss_plain"])) / 1e-5
    worst["loss_weighted"] = abs(r["l2"] - float(g[name + "/loss_weighted"])) / 1e-5
    for k, gr in r["grads"].items():
        key = name + "/digest/" + k
        if key in g.files:
            want = g[key]
            worst["digest/" + k] = abs(LR.digest(gr)[1] - want[1]) / (want[1] + 1e-12) / 2e-4
        else:
            assert k.startswith("matchatt.") and (gr is None or float(gr.abs().max()) == 0.0), k
    for key in g.files:
        if key.startswith(name + "/grad/"):
            k = key[len(name) + 6:]
            want = g[key]
            got = r["grads"][k][::LR.GRAD_ROWS[k][name]].numpy()
            worst["grad/" + k] = np.abs(got - want).max() / np.abs(want).max() / 2e-4
    bad = {k: v for k, v in worst.items() if not v * slack < 1.0}
    assert not bad, (name, slack, bad)
    return max(worst.values())


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_forward64_against_the_reference_goldens(name, golden, results):
    _against_golden(name, golden, results[name][0], 1.0)


@pytest.mark.parametrize("T,R,K", [(1, 1, 4), (7, 3, 12), (20, 2, 100)])
def test_the_explicit_loop_against_torch_lstm_in_double(T, R, K):
    torch.manual_seed(T + K)
    ref = torch.nn.LSTM(K, LR.D_E, num_layers=2, bidirectional=True).double()
    P = {"lstm." + k: v.detach() for k, v in ref.state_dict().items()}
    x = torch.randn(T, R, K, dtype=torch.float64)
    want = ref(x)[0].detach()
    got = LR.bilstm2_loop(P, x)
    assert float((got - want).abs().max()) < 1e-12
    # and layer by layer through torch._VF.lstm (the float32 restatement's encoder), with a replayed dropout mask
    keep = (torch.rand(T, R, 2 * LR.D_E) < 0.5).double()
    a, b = LR.bilstm2_loop(P, x, keep, 2.0), LR.torch_lstm_encoder(P)(x, keep, 2.0)
    assert float((a - b).abs().max()) < 1e-12 and not torch.equal(a, got)


@pytest.mark.parametrize("name", sorted(LR.CASES))
def test_the_gpu_figures_leave_a_factor_four_for_honest_float32(name, golden, results):
    """A float32 torch.nn.LSTM restatement of the case meets every model-level figure of the GPU test -- 1e-4 / 1e-5 / 2e-4
    against the goldens, rel_max < 1e-5 against float64 -- with at least a factor 4 to spare: the figures are reachable in
    float32 at these shapes, so a device miss is the device code's."""
    r64, r32 = results[name]
    ratio = _against_golden(name, golden, r32, 4.0)
    worst = {"log_prob": rel_max(r32["lp"], r64["lp"]), "emotions": rel_max(r32["em"], r64["em"]),
             "loss_plain": abs(r32["l1"] - r64["l1"]) / abs(r64["l1"]), "loss_weighted": abs(r32["l2"] - r64["l2"]) / abs(r64["l2"])}
    if r64["alpha"] is not None:
        worst["alpha"] = rel_max(r32["alpha"], r64["alpha"])
    for k, gr in r64["grads"].items():
        if gr is not None and float(gr.abs().max()) > 0:
            worst["grad " + k] = rel_max(r32["grads"][k], gr)
    print("LSTM-HEADROOM %s golden=%.3g float64=%s" % (name, ratio, {k: "%.2g" % v for k, v in worst.items()}), flush=True)
    bad = {k: v for k, v in worst.items() if not 4.0 * v < 1e-5}
    assert not bad, bad
