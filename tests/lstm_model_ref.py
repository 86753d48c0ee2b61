"""Shared pieces of the LSTMModel tests: the golden cases (tests/golden/make_golden_lstm_model.py writes the reference's outputs
for exactly these; inputs and digest format are gru_model_ref's), and a float64 restatement of the model (reference
model.py:320-356) with replayable dropout flags.  The recurrence is an explicit float64 loop over the contract of
include/mmdfn_hip.h (K16), independent of torch's LSTM kernels and of oracle/:

    a = W_hh h + b_hh + (W_ih x + b_ih);  i, f, o = sig(.);  g = tanh(.);  c' = f c + i g;  h' = o tanh(c')     (gate order i f g o)
"""
import torch

import matching_attention_ref as MA
from gru_model_ref import case_inputs, digest, masked_nll  # noqa: F401  (shared, not copied)

D_E, D_H = 100, 32
# name -> (D_m, L, lengths, n_classes, att2)
CASES = {
    "a": (100, 20, [20, 13, 7], 6, True),
    "b": (600, 9, [9, 1, 4, 2], 7, True),
    "c": (100, 20, [20, 13, 7], 6, False),
}
# rows of the stored gradients (every k-th row; the digests cover every parameter in full): name -> {case: k}
GRAD_ROWS = {"matchatt.transform.weight": {"a": 4, "b": 4}, "linear.weight": {"a": 1, "b": 1, "c": 1},
             "lstm.weight_ih_l0": {"a": 4, "b": 20, "c": 4}}


def lstm_direction(x, w_ih, w_hh, b_ih, b_hh, reverse):
    """One direction of one layer, step by step, in x's dtype: x (T, R, K) -> h (T, R, H); h = c = 0 at the start."""
    T, R = x.shape[0], x.shape[1]
    Hh = w_hh.shape[1]
    gi = x @ w_ih.t() + b_ih
    h = torch.zeros(R, Hh, dtype=x.dtype)
    c = torch.zeros(R, Hh, dtype=x.dtype)
    out = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        a = h @ w_hh.t() + b_hh + gi[t]
        i, f, g, o = a[:, :Hh], a[:, Hh:2 * Hh], a[:, 2 * Hh:3 * Hh], a[:, 3 * Hh:]
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return torch.stack(out)


def bilstm2_loop(params, x, keep=None, scale=1.0, prefix="lstm."):
    """The 2-layer bidirectional LSTM on ``lstm_direction``; ``keep`` (T, R, 2H): 0 / 1 flags of the dropout between the layers."""
    for layer in range(2):
        outs = []
        for d, r in enumerate(("", "_reverse")):
            P = [params["%s%s_l%d%s" % (prefix, n, layer, r)] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            outs.append(lstm_direction(x, *P, reverse=bool(d)))
        x = torch.cat(outs, 2)
        if layer == 0 and keep is not None:
            x = x * keep.to(x.dtype).view_as(x) * scale
    return x


def attention_any(X, M, mask):
    """matching_attention_ref.closed_form(zero_rows=False) in X's dtype (that one computes in float64 whatever it is given)."""
    z = torch.einsum("tbd,sbd->tbs", X, M)
    e = (mask != 0).to(X.dtype).unsqueeze(0) * torch.exp(torch.tanh(z))
    alpha = e / e.sum(2, keepdim=True)
    return torch.einsum("tbs,sbd->tbd", alpha, M), alpha


def forward_any(params, U, umask, att2=True, lstm_keep=None, head_keep=None, p=0.0, encoder=None):
    """The model in the dtype of ``params``.  encoder (optional): a callable (x, keep, scale) -> emotions replacing the loop
    (the host test's float32 torch.nn.LSTM restatement)."""
    dt = next(iter(params.values())).dtype
    U, umask = U.to(dt), umask.to(dt)
    scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    emotions = bilstm2_loop(params, U, lstm_keep, scale) if encoder is None else encoder(U, lstm_keep, scale)
    alpha = None
    att = emotions
    if att2:
        q = emotions @ params["matchatt.transform.weight"].t() + params["matchatt.transform.bias"]
        att, alpha = MA.closed_form(q, emotions, umask, zero_rows=False) if dt == torch.float64 else attention_any(q, emotions, umask)
    hidden = torch.relu(att @ params["linear.weight"].t() + params["linear.bias"])
    if head_keep is not None:
        hidden = hidden * head_keep.to(dt).view(hidden.shape) * scale
    logits = hidden @ params["smax_fc.weight"].t() + params["smax_fc.bias"]
    return torch.log_softmax(logits, 2), alpha, emotions


def forward64(params, U, umask, att2=True, lstm_keep=None, head_keep=None, p=0.0):
    """The model in float64 on the CPU.  params: name -> float64 tensor (state_dict keys).  ``lstm_keep`` (L, B, 2 D_e) /
    ``head_keep`` (L * B, D_h): 0 / 1 keep flags of the dropout between the LSTM layers and in front of smax_fc, scaled by
    1 / (1 - p) (None: no dropout).  Returns log_prob (L, B, C), alpha (L, B, L) or None, emotions (L, B, 2 D_e)."""
    assert all(v.dtype == torch.float64 for v in params.values())
    return forward_any(params, U, umask, att2, lstm_keep, head_keep, p)


def torch_lstm_encoder(params, prefix="lstm."):
    """(x, keep, scale) -> emotions on torch's own CPU LSTM in the dtype of ``params``, layer by layer (so that the replayed
    dropout sits between the layers)."""
    def run(x, keep, scale):
        for layer in range(2):
            flat = [params["%s%s_l%d%s" % (prefix, n, layer, r)] for r in ("", "_reverse")
                    for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
            z = torch.zeros(2, x.shape[1], D_E, dtype=x.dtype)
            x = torch._VF.lstm(x, (z, z), flat, True, 1, 0.0, False, True, False)[0]
            if layer == 0 and keep is not None:
                x = x * keep.to(x.dtype).view_as(x) * scale
        return x
    return run
