"""CPU: the host-side contract of DialogRNNModel / DialogueRNN and the K17 entry points (csrc/dialogue_rnn.hip): state_dict keys
against the reference's, constructor refusals and input checks, the header's declarations, the refusals of the entry points (no
device needed: they return before any HIP call), and the float64 restatement (tests/dialogue_rnn_ref.py) against every stored
array of the reference's goldens -- which is what licenses it as the yardstick of the GPU tests."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dialogue_rnn_ref as DR
from mm_dfn_amd import DialogRNNModel, DialogueRNN, _hip, dialogue_rnn, synthetic

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# The restatement in float64 against the reference's float32 outputs.  Read off the reference's own float32 error on these three
# cases (the float32 run of the SAME restatement against the float64 one, printed below as DRNN-F32): at most 5.4e-7 relative to a
# quantity's largest entry over every output and gradient (the goldens themselves are within 5.1e-7 of the float64 run), so 1e-5
# bounds the reference's error with more than the factor 4 that the last assertion asks for
# and is far below any wrong term (a dropped bypass, a history that includes g_t, a swapped gate each move outputs by > 1e-3).
REL = 1e-5


def _keys(path):
    with open(path) as f:
        return [(ln.split()[0], tuple(int(d) for d in ln.split()[1:])) for ln in f if ln.strip()]


def rel_max(got, want):
    got, want = torch.as_tensor(got).detach().double(), torch.as_tensor(want).detach().double()
    assert tuple(got.shape) == tuple(want.shape)
    den = float(want.abs().max())
    return float((got - want).abs().max()) / den if den else float(got.abs().max())


def flat_logp(log_prob):
    return log_prob.transpose(0, 1).contiguous().view(-1, log_prob.shape[2])


def test_state_dict_keys_and_shapes_match_the_reference():
    m = DialogRNNModel(100, 150, 150, 100, 32, n_classes=6, context_attention="general", att2=False)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _keys(os.path.join(GOLD, "state_dict_keys_dialog_rnn_model.txt"))
    s = DialogRNNModel(600, 150, 150, 100, 100)
    keys = list(s.state_dict())
    assert keys[12] == "dialog_rnn_f.dialogue_cell.attention.scalar.weight" and tuple(s.state_dict()[keys[12]].shape) == (1, 150)
    assert s.dropout.p == 0.5 and s.dropout_rec.p == 0.65 and s.dialog_rnn_f.dropout.p == 0.5 and s.att2
    assert isinstance(s.dialog_rnn_r, DialogueRNN) and isinstance(s.dialog_rnn_r.dialogue_cell.p_cell, torch.nn.GRUCell)
    assert tuple(s.dialog_rnn_f.dialogue_cell.g_cell.weight_ih.shape) == (450, 750) and s.smax_fc.out_features == 7
    d = DialogueRNN(100, 150, 150, 100, context_attention="general", dropout=0.25)
    assert list(d.state_dict())[0] == "dialogue_cell.g_cell.weight_ih" and list(d.state_dict())[-1] == "dialogue_cell.attention.transform.weight"


def test_constructor_refusals_name_the_argument():
    with pytest.raises(NotImplementedError, match="listener_state"):
        DialogRNNModel(100, 150, 150, 100, 32, listener_state=True)
    with pytest.raises(NotImplementedError, match="listener_state"):
        DialogueRNN(100, 150, 150, 100, listener_state=True)
    for kind in ("dot", "concat", "general2"):
        with pytest.raises(NotImplementedError, match="context_attention"):
            DialogRNNModel(100, 150, 150, 100, 32, context_attention=kind)
    for dims, word in (((100, 100, 150, 100), "D_g"), ((100, 150, 100, 100), "D_p"), ((100, 150, 150, 150), "D_e"),
                       ((342, 150, 150, 100), "D_m"), ((2, 150, 150, 100), "D_m"), ((772, 150, 150, 100), "D_m")):
        with pytest.raises(NotImplementedError, match=word):
            DialogRNNModel(*dims, 32)
        with pytest.raises(NotImplementedError, match=word):
            DialogueRNN(*dims)


def test_cpu_tensors_raise():
    with pytest.raises(_hip.HipLibraryError):
        DialogRNNModel(100, 150, 150, 100, 32)(torch.zeros(3, 2, 100), torch.zeros(3, 2, 2), torch.ones(2, 3))
    with pytest.raises(_hip.HipLibraryError):
        DialogueRNN(100, 150, 150, 100)(torch.zeros(3, 2, 100), torch.zeros(3, 2, 2))


def test_input_checks():
    """speakers() is plain tensor code: the checks run on CPU tensors as they do on the device."""
    T, B, P = 4, 3, 3
    qmask = torch.zeros(T, B, P)
    qmask[:, :, 1] = 1.0
    qmask[2, 0] = 0.0                                            # a zero row inside a dialogue is allowed (m = 0)
    full = torch.tensor([4, 2, 1], dtype=torch.int32)
    spk, upd = dialogue_rnn.speakers(qmask, full)
    assert spk.dtype == torch.int32 and spk[0, 0] == 1 and spk[2, 0] == 0 and upd[2, 0] == 0 and upd[1, 1] == 1
    bad = qmask.clone()
    bad[1, 1, 2] = 1.0                                           # two parties at once
    with pytest.raises(ValueError, match="qmask"):
        dialogue_rnn.speakers(bad, full)
    bad = qmask.clone()
    bad[0, 0, 1] = 0.5
    with pytest.raises(ValueError, match="qmask"):
        dialogue_rnn.speakers(bad, full)
    with pytest.raises(ValueError, match="length"):
        dialogue_rnn.speakers(qmask, torch.tensor([3, 2, 1], dtype=torch.int32))
    dialogue_rnn.speakers(bad, torch.tensor([3, 2, 1], dtype=torch.int32), check=False)


def test_header_declares_the_entry_points_and_the_abi_stays_23():
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _hip.ABI_VERSION == 23
    assert _hip.SIGNATURES["mmdfn_drnn_chains_per_group"] == [] and _hip.RESTYPES["mmdfn_drnn_chains_per_group"] is I
    assert _hip.SIGNATURES["mmdfn_drnn_image_floats"] == [] and _hip.RESTYPES["mmdfn_drnn_image_floats"] is ctypes.c_int64
    assert _hip.SIGNATURES["mmdfn_drnn_seq_fwd"] == [V] * 8 + [F] + [V] * 3 + [I] * 9 + [V]
    assert _hip.SIGNATURES["mmdfn_drnn_seq_bwd"] == [V] * 11 + [F] + [V] * 6 + [I] * 9 + [V]
    assert _hip.RESTYPES["mmdfn_drnn_seq_fwd"] is I and _hip.RESTYPES["mmdfn_drnn_seq_bwd"] is I
    # the LSTM / GRU signatures are untouched
    assert len(_hip.SIGNATURES["mmdfn_lstm_seq_fwd"]) == 9 and len(_hip.SIGNATURES["mmdfn_gru_seq_fwd"]) == 11


def test_refused_calls_return_minus_one_before_any_device_call():
    """Every refusal of the header's contract, one violation per call (never a valid call: nothing may launch here)."""
    Pn = ctypes.c_void_p(4096)                                  # a non-null value that is never dereferenced
    pair = lambda n=2: (ctypes.c_void_p * n)(*([4096] * n))     # host arrays: these ARE read, their entries are not
    half_null = (ctypes.c_void_p * 2)(4096, None)
    lds = lambda v=150: _hip.int_array([v, v, v, v, v, 100])
    assert 1 <= _hip.query("mmdfn_drnn_chains_per_group") <= 16
    assert _hip.query("mmdfn_drnn_image_floats") == 4 * 150 * 450 + 150 * 300 + 100 * 300 + 2 * 450 + 2 * 300 + 152

    def fwd(ptrs=None, dims=(3, 4, 2, 150, 150, 100, 900, 0, 2)):
        args = dict(pu=pair(), img=pair(), speaker=Pn, upd=Pn, lengths=Pn, kg=None, kq=None, ke=None, e=Pn, alpha=Pn, state=Pn)
        args.update(ptrs or {})
        return _hip.call("mmdfn_drnn_seq_fwd", args["pu"], args["img"], args["speaker"], args["upd"], args["lengths"], args["kg"],
                         args["kq"], args["ke"], 1.0, args["e"], args["alpha"], args["state"], *dims, None, allow=(-1,))

    def bwd(ptrs=None, dims=(3, 4, 2, 150, 150, 100, 900, 0, 2), ld=None):
        args = dict(de=Pn, pu=pair(), img=pair(), w=pair(12), ld=lds() if ld is None else ld, speaker=Pn, upd=Pn, lengths=Pn,
                    kg=None, kq=None, ke=None, alpha=Pn, state=Pn, dgate=Pn, dpu=pair(), dghist=Pn, dw=Pn)
        args.update(ptrs or {})
        return _hip.call("mmdfn_drnn_seq_bwd", args["de"], args["pu"], args["img"], args["w"], args["ld"], args["speaker"],
                         args["upd"], args["lengths"], args["kg"], args["kq"], args["ke"], 1.0, args["alpha"], args["state"],
                         args["dgate"], args["dpu"], args["dghist"], args["dw"], *dims, None, allow=(-1,))

    good = (3, 4, 2, 150, 150, 100, 900, 0, 2)                  # B T P Dg Dp De npu att ndir
    for i, v in ((0, 0), (0, -1), (1, 0), (1, 1009), (2, 0), (2, 17), (3, 100), (4, 152), (5, 150), (6, 1050), (6, 896), (7, 2),
                 (7, -1), (8, 0), (8, 3)):
        dims = list(good)
        dims[i] = v
        assert fwd(dims=tuple(dims)) == -1, (i, v)
        assert bwd(dims=tuple(dims)) == -1, (i, v)
    assert fwd(dims=(3, 4, 2, 150, 150, 100, 900, 1, 2)) == -1 and bwd(dims=(3, 4, 2, 150, 150, 100, 900, 1, 2)) == -1
    for k in ("pu", "img", "speaker", "upd", "lengths", "e", "alpha", "state"):
        assert fwd({k: None}) == -1, k
    assert fwd({"pu": half_null}) == -1 and fwd({"img": half_null}) == -1
    for k in ("de", "pu", "img", "w", "ld", "speaker", "upd", "lengths", "alpha", "state", "dgate", "dpu", "dghist", "dw"):
        assert bwd({k: None}) == -1, k
    assert bwd({"pu": half_null}) == -1 and bwd({"img": half_null}) == -1 and bwd({"dpu": half_null}) == -1
    w_null = pair(12)
    w_null[7] = None
    assert bwd({"w": w_null}) == -1
    assert bwd(ld=lds(149)) == -1 and bwd(ld=_hip.int_array([150, 150, 150, 150, 150, 99])) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement against the goldens
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "dialog_rnn_model.npz"), allow_pickle=False)


def run_restatement(name, seed, dtype):
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    sd = synthetic.seeded_state_dict(DialogRNNModel(D_m, 150, 150, 100, DR.D_H, n_classes=C, context_attention=kind,
                                                    att2=att2).state_dict(), seed)
    prm = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    U, qmask, umask, label, weight = DR.case_inputs(name, seed + 1)
    lp, alpha, emotions, af, ab = DR.forward_any(prm, U, qmask, umask, kind, att2)
    l1 = DR.masked_nll(flat_logp(lp), label, umask)
    l2 = DR.masked_nll(flat_logp(lp), label, umask, weight)
    l2.backward()
    return dict(log_prob=lp.detach(), alpha=None if alpha is None else alpha.detach(), emotions=emotions.detach(), alpha_f=af,
                alpha_b=ab, loss_plain=l1.item(), loss_weighted=l2.item(), grads={k: p.grad for k, p in prm.items()})


def compare_with_golden(name, g, r, emit=None):
    """Worst relative figure (to a quantity's largest entry) of ``r`` against every stored array of case ``name``."""
    worst = {}
    for k in ("log_prob", "alpha_f", "alpha_b", "alpha", "emotions"):
        key = name + "/" + k
        if key in g.files:
            worst[k] = rel_max(r[k], g[key])
        else:
            assert (k == "alpha" and r[k] is None) or (k == "emotions" and name == "c"), key
    if name == "c":
        worst["emotions"] = rel_max(r["emotions"], g["a/emotions"])
    for k in ("loss_plain", "loss_weighted"):
        worst[k] = abs(r[k] - float(g[name + "/" + k])) / abs(float(g[name + "/" + k]))
    for k, gr in r["grads"].items():
        key = name + "/digest/" + k
        if key in g.files:
            want = g[key]
            worst["digest/" + k] = float(np.abs(DR.digest(gr)[1:] - want[1:]).max() / want[1:].max()) if want[1] else 0.0
        else:
            assert k.startswith("matchatt.") and (gr is None or float(gr.abs().max()) == 0.0), k
    n = 0
    for key in g.files:
        if key.startswith(name + "/grad/"):
            k = key[len(name) + 6:]
            worst["grad/" + k] = rel_max(r["grads"][k][::DR.GRAD_ROWS[k][name]], g[key])
            n += 1
    assert n >= 3
    if emit:
        print("%s %s worst %.3g at %s" % (emit, name, max(worst.values()), max(worst, key=worst.get)), flush=True)
    return worst


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_float64_restatement_reproduces_every_stored_golden_array(name, golden):
    seed = int(golden["seed"])
    r64 = run_restatement(name, seed, torch.float64)
    worst = compare_with_golden(name, golden, r64, emit="DRNN-F64-vs-golden")
    bad = {k: v for k, v in worst.items() if not v < REL}
    assert not bad, bad
    # the float32 run of the same algebra against the float64 one: the size of an honest float32 error on this case
    r32 = run_restatement(name, seed, torch.float32)
    own = {k: rel_max(r32[k], r64[k]) for k in ("log_prob", "emotions", "alpha_f", "alpha_b")}
    own.update({"grad " + k: rel_max(r32["grads"][k], v) for k, v in r64["grads"].items() if v is not None and float(v.abs().max()) > 0})
    print("DRNN-F32 %s worst %.3g at %s" % (name, max(own.values()), max(own, key=own.get)), flush=True)
    assert 4.0 * max(own.values()) < REL, own
