"""Shared pieces of the DialogRNNModel / K17 tests: the golden cases (tests/golden/make_golden_dialog_rnn_model.py writes the
reference's outputs for exactly these), their inputs, and a differentiable restatement of the DialogueRNN algebra (reference
model.py:168-278, 359-417) in the dtype of its parameters (float64 is the yardstick), with replayable keep flags.  It is an
explicit loop per dialogue and step over the contract of include/mmdfn_hip.h (K17), independent of torch's GRUCell and of oracle/:

    s = argmax qmask[t, b];  m = qmask[t, b, s]
    g_t = keep_g * GRU_g([U_t, q[s]], g_{t-1});   c_t = sum_{j<t} alpha_tj g_j,  alpha_t = softmax_j <x_t, g_j>,  x_t = W_att U_t | w
    qs = keep_q * GRU_p([U_t, c_t], q[s]);   q[s] = m qs + (1 - m) q[s];   e_t = keep_e * GRU_e(q[s], e_{t-1})

The reverse encoder runs a dialogue reversed within its own length and stops there.  Keep flags are in CHAIN-STEP order: row s
of a chain is its s-th processed step.
"""
import numpy as np
import torch

import lstm_model_ref as LR
from gru_model_ref import digest, masked_nll  # noqa: F401  (shared, not copied)

D_G = D_P = 150
D_E, D_H = 100, 32
# name -> (context_attention, D_m, T, lengths, P, n_classes, att2)
CASES = {
    "a": ("general", 100, 12, [12, 7, 1], 2, 6, True),
    "b": ("simple", 600, 6, [6, 2, 6, 3, 1], 9, 7, True),
    "c": ("general", 100, 12, [12, 7, 1], 2, 6, False),
}
# rows of the stored gradients (every k-th row; the digests cover every parameter in full): name -> {case: k}
GRAD_ROWS = {"linear.weight": {"a": 1, "b": 1, "c": 1},
             "dialog_rnn_f.dialogue_cell.g_cell.weight_hh": {"a": 9, "b": 9, "c": 9},
             "dialog_rnn_r.dialogue_cell.p_cell.weight_ih": {"a": 9, "b": 30, "c": 9},
             "dialog_rnn_r.dialogue_cell.e_cell.weight_ih": {"a": 6, "b": 6, "c": 6}}
PLANES = ("rg", "zg", "ng", "hng", "g", "rp", "zp", "np", "hnp", "q0", "q1", "c", "re", "ze", "ne", "hne", "e")


def make_inputs(D_m, T, lengths, P, C, seed, constant=1, zero_rows=()):
    """U (T, B, D_m), qmask (T, B, P) one-hot (zero beyond a length, as the data loaders pad), umask (B, T), label (B, T) int64,
    class weights (C): fp32 / int64 CPU tensors from numpy's RandomState(seed).  In dialogue ``constant`` the speaker never
    changes; ``zero_rows``: (t, b) whose qmask row is zero INSIDE a dialogue (m = 0: the party state passes through)."""
    B = len(lengths)
    rs = np.random.RandomState(seed)
    U = torch.from_numpy(rs.standard_normal((T, B, D_m)).astype(np.float32))
    label = torch.from_numpy(rs.randint(0, C, size=(B, T)).astype(np.int64))
    weight = torch.from_numpy(rs.uniform(0.5, 1.5, size=(C,)).astype(np.float32))
    spk = rs.randint(0, P, size=(T, B))
    if constant is not None and constant < B:
        spk[:, constant] = spk[0, constant]
    umask = torch.zeros(B, T)
    qmask = torch.zeros(T, B, P)
    for b, n in enumerate(lengths):
        umask[b, :n] = 1.0
        for t in range(n):
            qmask[t, b, spk[t, b]] = 1.0
        U[n:, b] = 0.0
    for t, b in zero_rows:
        qmask[t, b] = 0.0
    return U, qmask, umask, label, weight


def case_inputs(name, seed):
    _, D_m, T, lengths, P, C, _ = CASES[name]
    return make_inputs(D_m, T, lengths, P, C, seed)


def gru_gates(gi, gh, h):
    """(r, z, n, hn, h') of a GRU cell from its input-side and hidden-side pre-activations (gate order r z n)."""
    H = h.shape[-1]
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    hn = gh[..., 2 * H:]
    n = torch.tanh(gi[..., 2 * H:] + r * hn)
    return r, z, n, hn, (1 - z) * n + z * h


PROBES = ("gi_g", "gh_g", "gi_p", "gh_p", "gi_e", "gh_e")


def encoder(params, prefix, U, qmask, lengths, kind, reverse=False, keep=None, scale=1.0, planes=None, pu=None, probes=None):
    """One DialogueRNN encoder in the dtype of ``params`` -> (e (T, B, D_e) in time order, alpha (T, B, T) in chain-step order).
    ``lengths``: list of ints; the forward encoder runs all T steps whatever they are.  ``keep``: None or a dict g / q / e of
    0 / 1 flags (T, B, width) in chain-step order.  ``planes``: a dict that receives the saved planes of include/mmdfn_hip.h,
    name -> (T, B, width) in chain-step order (detached).  ``pu`` (T, B, 900 | 1050, time order): the projected rows of the
    header, used in place of the U halves of the g / p input contractions (+ b_ih) and of W_att U.  ``probes``: a dict PROBES
    name -> (T, B, 3 H) tensors (chain-step order) ADDED to the six gate pre-activations: zeros that require grad receive the
    gate gradients dgi / dgh of the header."""
    dt = next(iter(params.values())).dtype
    U, qmask = U.to(dt), qmask.to(dt)
    T, B, D_m = U.shape
    P = qmask.shape[2]
    c = prefix + "dialogue_cell."
    Wg, Whg, bg, bhg = (params[c + "g_cell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    Wp, Whp, bp, bhp = (params[c + "p_cell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    We, Whe, be, bhe = (params[c + "e_cell." + n] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    e_out = [[torch.zeros(D_E, dtype=dt) for _ in range(B)] for _ in range(T)]
    alpha = torch.zeros(T, B, T, dtype=dt)
    pr = (lambda n, s, b: probes[n][s, b]) if probes is not None else (lambda n, s, b: 0.0)
    if planes is not None:
        for n in PLANES:
            planes[n] = torch.zeros(T, B, D_E if n in ("re", "ze", "ne", "hne", "e") else D_G, dtype=dt)
    for b in range(B):
        n_b = int(lengths[b]) if reverse else T
        times = list(range(n_b - 1, -1, -1)) if reverse else list(range(T))
        g = torch.zeros(D_G, dtype=dt)
        e = torch.zeros(D_E, dtype=dt)
        q = [torch.zeros(D_P, dtype=dt) for _ in range(P)]
        hist = []
        for s, t in enumerate(times):
            u = U[t, b]
            spk = int(qmask[t, b].argmax())
            m = qmask[t, b, spk]
            q0 = q[spk]
            gi_g = Wg @ torch.cat([u, q0]) + bg if pu is None else pu[t, b, :3 * D_G].to(dt) + Wg[:, D_m:] @ q0
            rg, zg, ng, hng, g = gru_gates(gi_g + pr("gi_g", s, b), Whg @ g + bhg + pr("gh_g", s, b), g)
            if keep is not None:
                g = g * keep["g"][s, b].to(dt) * scale
            if hist:
                G = torch.stack(hist)
                if kind != "general":
                    x = params[c + "attention.scalar.weight"][0]
                else:
                    x = params[c + "attention.transform.weight"] @ u if pu is None else pu[t, b, 6 * D_G:].to(dt)
                a = torch.softmax(G @ x, 0)
                ctx = a @ G
                alpha[s, b, :s] = a.detach()
            else:
                ctx = torch.zeros(D_G, dtype=dt)
            gi_p = Wp @ torch.cat([u, ctx]) + bp if pu is None else pu[t, b, 3 * D_G:6 * D_G].to(dt) + Wp[:, D_m:] @ ctx
            rp, zp, np_, hnp, qs = gru_gates(gi_p + pr("gi_p", s, b), Whp @ q0 + bhp + pr("gh_p", s, b), q0)
            if keep is not None:
                qs = qs * keep["q"][s, b].to(dt) * scale
            q1 = m * qs + (1 - m) * q0
            q[spk] = q1
            re, ze, ne, hne, e = gru_gates(We @ q1 + be + pr("gi_e", s, b), Whe @ e + bhe + pr("gh_e", s, b), e)
            if keep is not None:
                e = e * keep["e"][s, b].to(dt) * scale
            hist.append(g)
            e_out[t][b] = e
            if planes is not None:
                for n, v in zip(PLANES, (rg, zg, ng, hng, g, rp, zp, np_, hnp, q0, q1, ctx, re, ze, ne, hne, e)):
                    planes[n][s, b] = v.detach()
    return torch.stack([torch.stack(r) for r in e_out]), alpha


def forward_any(params, U, qmask, umask, kind, att2=True, keeps=None, p_rec=0.0, rec_keep=None, p_out=0.0, head_keep=None, p=0.0):
    """The model in the dtype of ``params`` -> (log_prob (T, B, C), alpha (T, B, T) or None, emotions (T, B, 2 D_e), alpha_f,
    alpha_b (T, B, T) in chain-step order).  keeps: None or [dict g / q / e] per direction (probability p_rec); rec_keep: None
    or [(T, B, D_e)] per direction, the Dropout(dropout + 0.15) site (probability p_out); head_keep / p: the head's dropout."""
    dt = next(iter(params.values())).dtype
    lengths = [int(v) for v in umask.sum(1)]
    al = {}

    def enc(x, _keep, _scale):
        outs = []
        for d, pre in enumerate(("dialog_rnn_f.", "dialog_rnn_r.")):
            e, al[d] = encoder(params, pre, x, qmask, lengths, kind, reverse=bool(d), keep=None if keeps is None else keeps[d],
                               scale=1.0 / (1.0 - p_rec))
            if rec_keep is not None:
                e = e * rec_keep[d].to(dt).view_as(e) / (1.0 - p_out)
            outs.append(e)
        return torch.cat(outs, 2)

    lp, alpha, emotions = LR.forward_any(params, U, umask, att2, None, head_keep, p, encoder=enc)
    return lp, alpha, emotions, al[0], al[1]


def pack_alpha(alist, T, B):
    """The model's alpha_f / alpha_b list (entry t-1: (B, t)) as a (T, B, T) lower triangle."""
    out = torch.zeros(T, B, T, dtype=alist[0].dtype if alist else torch.float32)
    for i, a in enumerate(alist):
        out[i + 1, :, :i + 1] = a.detach().cpu()
    return out
