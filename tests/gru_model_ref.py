"""Shared pieces of the GRUModel tests: the golden cases and their seeded inputs (tests/golden/make_golden_gru_model.py writes
the reference's outputs for exactly these), and a float64 restatement of the model (reference model.py:281-317) on torch's
own CPU GRU with replayable dropout flags."""
import numpy as np
import torch

import matching_attention_ref as MA

D_E, D_H = 100, 32
# name -> (D_m, L, lengths, n_classes, att2)
CASES = {
    "a": (100, 20, [20, 13, 7], 6, True),
    "b": (600, 9, [9, 1, 4, 2], 7, True),
    "c": (100, 20, [20, 13, 7], 6, False),
}
# rows of the stored gradients (every k-th row; the digests cover every parameter in full): name -> {case: k}
GRAD_ROWS = {"matchatt.transform.weight": {"a": 4, "b": 4}, "linear.weight": {"a": 1, "b": 1, "c": 1},
             "gru.weight_ih_l0": {"a": 4, "b": 20, "c": 4}}


def case_inputs(name, seed):
    """U (L, B, D_m), qmask (L, B, 2), umask (B, L), label (B, L) int64, class weights (C): fp32 / int64 CPU tensors drawn from
    numpy's RandomState(seed) -- a case with the same shape and seed gets the same inputs ('c' shares 'a''s)."""
    D_m, L, lengths, C, _ = CASES[name]
    B = len(lengths)
    rs = np.random.RandomState(seed)
    U = torch.from_numpy(rs.standard_normal((L, B, D_m)).astype(np.float32))
    label = torch.from_numpy(rs.randint(0, C, size=(B, L)).astype(np.int64))
    weight = torch.from_numpy(rs.uniform(0.5, 1.5, size=(C,)).astype(np.float32))
    umask = torch.zeros(B, L)
    for b, n in enumerate(lengths):
        umask[b, :n] = 1.0
    qmask = torch.zeros(L, B, 2)
    qmask[:, :, 0] = 1.0
    return U, qmask, umask, label, weight


def digest(g):
    """tests/test_oracle_golden._digest's format."""
    g = g.detach().double().reshape(-1)
    return np.array([g.sum().item(), g.abs().sum().item(), (g * g).sum().item()])


def masked_nll(pred, target, mask, weight=None):
    """sum_i m_i w[t_i] (-pred[i, t_i]) / sum_i m_i w[t_i] in pred's dtype."""
    m = mask.reshape(-1).to(pred.dtype)
    w = torch.ones_like(m) if weight is None else weight.to(pred.dtype)[target.reshape(-1)]
    picked = pred.gather(1, target.reshape(-1, 1)).reshape(-1)
    return (m * w * -picked).sum() / (m * w).sum()


def forward64(params, U, umask, att2=True, gru_keep=None, head_keep=None, p=0.0):
    """The model in float64 on the CPU.  params: name -> float64 tensor (state_dict keys).  ``gru_keep`` (L, B, 2 D_e) /
    ``head_keep`` (L * B, D_h): 0 / 1 keep flags of the dropout between the GRU layers and in front of smax_fc, scaled by
    1 / (1 - p) (None: no dropout).  Returns log_prob (L, B, C), alpha (L, B, L) or None, emotions (L, B, 2 D_e)."""
    U, umask = U.double(), umask.double()
    scale = 1.0 / (1.0 - p) if p < 1.0 else 0.0
    x = U
    for layer in range(2):
        sfx = "_l%d" % layer
        names = ["weight_ih", "weight_hh", "bias_ih", "bias_hh"]
        flat = [params["gru.%s%s%s" % (n, sfx, r)] for r in ("", "_reverse") for n in names]
        h0 = torch.zeros(2, x.shape[1], D_E, dtype=torch.float64)
        x, _ = torch._VF.gru(x, h0, flat, True, 1, 0.0, False, True, False)
        if layer == 0 and gru_keep is not None:
            x = x * gru_keep.double().view_as(x) * scale
    emotions = x
    alpha = None
    att = emotions
    if att2:
        q = emotions @ params["matchatt.transform.weight"].t() + params["matchatt.transform.bias"]
        att, alpha = MA.closed_form(q, emotions, umask, zero_rows=False)
    hidden = torch.relu(att @ params["linear.weight"].t() + params["linear.bias"])
    if head_keep is not None:
        hidden = hidden * head_keep.double().view(hidden.shape) * scale
    logits = hidden @ params["smax_fc.weight"].t() + params["smax_fc.bias"]
    return torch.log_softmax(logits, 2), alpha, emotions
