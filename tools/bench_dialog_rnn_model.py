"""Time an eager training step of DialogRNNModel (recurrent_models.py on K17, csrc/dialogue_rnn.hip) and the device time of its
recurrence launches, against a torch restatement of the reference's per-step loop on the same device in the same process,
alternating the forms per round:

    drnn       DialogRNNModel: forward + MaskedNLLLoss + backward + ops.join_weight_grads()
    reference  the reference's structure with torch modules (model.py:168-278, 359-417 restated, not imported: a Python loop over
               timesteps with three nn.GRUCell, the softmax over the growing history, the party select, once per direction; then
               one MatchingAttention('general2') call per timestep, Linear, ReLU, dropout, Linear, log_softmax, masked NLL)

    python tools/bench_dialog_rnn_model.py [--rounds 3] [--window 0.5] [--out FILE.md]

Per (T, B) in (110, 16), (33, 32) with D_m = 100, D_g = D_p = 150, D_e = D_h = 100, 2 parties, 7 classes, dropout 0.5 /
dropout_rec 0.5 and both attention kinds: host wall time per step (synchronised) over windows of at least ``--window`` seconds
after a warm-up of both forms, the median over the rounds and the min .. max of the rounds; and, from a device trace of 3
steps, the device time per step of ``drnn_seq_fwd`` / ``drnn_seq_bwd`` (for the reference form: the whole step's device time).
Then the batch sweep the design predicts to be near-flat: the two launches' device time at T = 33, 'simple', over B = 1 .. 256
(R = mmdfn_drnn_chains_per_group() chains share one pass over the weights, and every workgroup has a CU to itself up to B = 128 R).
No thresholds: the numbers are what they are.  Needs an MI355X: there is no CPU path."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_lstm_model import ReferenceStructure, recurrence_device_us, timed, torch_masked_nll  # noqa: E402
from mm_dfn_amd import DialogRNNModel, MaskedNLLLoss, dialogue_rnn, ops, train  # noqa: E402

SHAPES = [(110, 16), (33, 32)]
D_M, D_G, D_E, D_H, C, PARTIES, P_DROP = 100, 150, 100, 100, 7, 2, 0.5


class LoopEncoder(nn.Module):
    """One DialogueRNN of the reference restated on torch modules: the per-step loop, batched over the dialogues."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self.g_cell, self.p_cell, self.e_cell = nn.GRUCell(D_M + D_G, D_G), nn.GRUCell(D_M + D_G, D_G), nn.GRUCell(D_G, D_E)
        self.att = nn.Linear(D_G, 1, bias=False) if kind == "simple" else nn.Linear(D_M, D_G, bias=False)
        self.dropout = nn.Dropout(P_DROP)

    def forward(self, U, qmask):
        T, B, P = qmask.shape
        rows = torch.arange(B, device=U.device)
        g = U.new_zeros(B, D_G)
        e = U.new_zeros(B, D_E)
        q = U.new_zeros(B, P, D_G)
        hist, out = [], []
        for t in range(T):
            idx = qmask[t].argmax(1)
            q0 = q[rows, idx]
            g = self.dropout(self.g_cell(torch.cat([U[t], q0], 1), g))
            if hist:
                G = torch.stack(hist)
                score = self.att(G).squeeze(2) if self.kind == "simple" else torch.einsum("tbd,bd->tb", G, self.att(U[t]))
                c = torch.einsum("tb,tbd->bd", F.softmax(score, 0), G)
            else:
                c = U.new_zeros(B, D_G)
            x = torch.cat([U[t], c], 1).unsqueeze(1).expand(-1, P, -1).reshape(B * P, -1)
            qs = self.dropout(self.p_cell(x, q.reshape(B * P, D_G))).view(B, P, D_G)
            m = qmask[t].unsqueeze(2)
            q = q * (1 - m) + qs * m
            e = self.dropout(self.e_cell(q[rows, idx], e))
            hist.append(g)
            out.append(e)
        return torch.stack(out)


class ReferenceLoop(ReferenceStructure):
    """The reference's DialogRNNModel restated: two LoopEncoders, the reverse one on every dialogue reversed within its length,
    in front of bench_lstm_model.ReferenceStructure's attention / linear / head tail."""

    def __init__(self, kind):
        super().__init__(D_M)
        del self.lstm
        self.enc_f, self.enc_r = LoopEncoder(kind), LoopEncoder(kind)
        self.dropout_rec = nn.Dropout(P_DROP + 0.15)

    def forward(self, U, qmask, umask):
        T, B = U.shape[0], U.shape[1]
        lengths = umask.sum(1).long()
        t = torch.arange(T, device=U.device).unsqueeze(1)
        src = lengths.unsqueeze(0) - 1 - t                                  # (T, B): time index of reversed step t
        ok = (src >= 0).float().unsqueeze(2)
        src = src.clamp(min=0)
        rev = lambda X: X.gather(0, src.unsqueeze(2).expand(-1, -1, X.shape[2])) * ok
        ef = self.dropout_rec(self.enc_f(U, qmask))
        eb = self.dropout_rec(rev(self.enc_r(rev(U), rev(qmask))))
        emotions = torch.cat([ef, eb], 2)
        att = torch.cat([self.attend(emotions, x, umask).unsqueeze(0) for x in emotions], dim=0)
        hidden = self.dropout(F.relu(self.linear(att)))
        return F.log_softmax(self.smax_fc(hidden), 2), [], [], [], emotions


def inputs(T, B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    U = torch.randn(T, B, D_M, device="cuda", generator=g)
    lengths = torch.randint(max(1, T // 2), T + 1, (B,), device="cuda", generator=g)
    lengths[0] = T
    umask = (torch.arange(T, device="cuda").unsqueeze(0) < lengths.unsqueeze(1)).float()
    spk = torch.randint(0, PARTIES, (T, B), device="cuda", generator=g)
    qmask = F.one_hot(spk, PARTIES).float() * umask.t().unsqueeze(2)
    label = torch.randint(0, C, (B * T,), device="cuda", generator=g)
    return U, qmask, umask, label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dialog_rnn_model: needs an MI355X (no HIP device visible)")
    R = dialogue_rnn.chains_per_group()
    lines = ["chains per workgroup R = %d" % R, "",
             "| T | B | attention | form | train step us, median (min .. max) | recurrence device us / step (launches) |",
             "|---|---|---|---|---|---|"]
    notes = []
    loss_f = MaskedNLLLoss()

    def make_step(m, fused, U, qmask, umask, label):
        def step():
            m.zero_grad(set_to_none=True)
            lp = m(U, qmask, umask)[0].transpose(0, 1).contiguous().view(-1, C)
            if fused:
                train.backward(loss_f(lp, label, umask))
                ops.join_weight_grads()
            else:
                torch_masked_nll(lp, label, umask).backward()
        return step

    for T, B in SHAPES:
        for kind in ("simple", "general"):
            torch.manual_seed(T)
            data = inputs(T, B, T)
            steps = {"drnn": make_step(DialogRNNModel(D_M, D_G, D_G, D_E, D_H, n_classes=C, context_attention=kind,
                                                      dropout_rec=P_DROP, dropout=P_DROP).cuda().train(), True, *data),
                     "reference": make_step(ReferenceLoop(kind).cuda().train(), False, *data)}
            for name in steps:
                for _ in range(3):
                    steps[name]()
            torch.cuda.synchronize()
            res = {name: [] for name in steps}
            for _ in range(args.rounds):
                for name in steps:
                    res[name].append(timed(steps[name], args.window))
            dev = {"drnn": recurrence_device_us(steps["drnn"], "drnn_seq", 3), "reference": recurrence_device_us(steps["reference"], None, 3)}
            fb = [recurrence_device_us(steps["drnn"], p, 3)[0] for p in ("drnn_seq_fwd", "drnn_seq_bwd")]
            for name in steps:
                a = res[name]
                lines.append("| %d | %d | %s | %s | %.0f (%.0f .. %.0f) | %.1f (%.0f)%s |"
                             % (T, B, kind, name, statistics.median(a), min(a), max(a), dev[name][0], dev[name][1],
                                " whole step" if name == "reference" else ""))
            med = {name: statistics.median(res[name]) for name in steps}
            notes.append("(T, B, %s) = (%d, %d): train step reference / drnn = %.2f; recurrence device time %.1f us forward + %.1f us "
                         "backward = %.2f us per chain step and direction pair" % (kind, T, B, med["reference"] / med["drnn"], fb[0], fb[1],
                                                                                  (fb[0] + fb[1]) / T))
    lines += ["", "| T | B | workgroups per direction | drnn_seq_fwd us | drnn_seq_bwd us |", "|---|---|---|---|---|"]
    T = 33
    for B in (1, 4, 16, 32, 64, 128, 256):
        torch.manual_seed(B)
        m = DialogRNNModel(D_M, D_G, D_G, D_E, D_H, n_classes=C, context_attention="simple", dropout_rec=P_DROP, dropout=P_DROP).cuda().train()
        step = make_step(m, True, *inputs(T, B, B))
        for _ in range(3):
            step()
        fb = [recurrence_device_us(step, p, 3)[0] for p in ("drnn_seq_fwd", "drnn_seq_bwd")]
        lines.append("| %d | %d | %d | %.1f | %.1f |" % (T, B, (B + R - 1) // R, fb[0], fb[1]))
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
