"""Time an eager training step of LSTMModel (recurrent_models.py on K16, csrc/lstm_seq.hip) and the device time of its recurrence
launches, against two other forms on the same device in the same process, alternating the three per round:

    lstm       LSTMModel: forward + MaskedNLLLoss + backward + ops.join_weight_grads()
    gru        GRUModel at the same shape (the LSTM step has 4/3 of the GRU step's recurrent FMAs on the same dependent chain)
    reference  the reference's structure with torch modules (model.py:320-356 restated: torch.nn.LSTM, then one
               MatchingAttention('general2') call per timestep -- bmm, tanh, softmax, renormalise, bmm -- Linear, ReLU, dropout,
               Linear, log_softmax, and the masked NLL of loss.py:38-58)

    python tools/bench_lstm_model.py [--rounds 5] [--window 0.5] [--out FILE.md]

Per shape (L, B, D_m) in (110, 16, 100), (33, 32, 600) with D_e = D_h = 100, 7 classes, dropout 0.5: host wall time per step
(synchronised) over windows of at least ``--window`` seconds after a warm-up of every form at that shape, the median over the
rounds and the run-to-run spread (min .. max of the rounds); and, from a device trace of 5 steps, the device time per step of
the recurrence kernels (``lstm_seq_*`` / ``gru_seq_*``; for the reference form: every kernel MIOpen's LSTM launches is
not separable by name, so the column is the whole step's device time there).  No thresholds: the numbers are what they are.
Needs an MI355X: there is no CPU path."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mm_dfn_amd import GRUModel, LSTMModel, MaskedNLLLoss, ops, train  # noqa: E402

SHAPES = [(110, 16, 100), (33, 32, 600)]
D_E, D_H, C, P_DROP = 100, 100, 7, 0.5


class ReferenceStructure(nn.Module):
    """The reference's LSTMModel restated on torch modules (not imported from it)."""

    def __init__(self, D_m):
        super().__init__()
        self.dropout = nn.Dropout(P_DROP)
        self.lstm = nn.LSTM(input_size=D_m, hidden_size=D_E, num_layers=2, bidirectional=True, dropout=P_DROP)
        self.transform = nn.Linear(2 * D_E, 2 * D_E, bias=True)
        self.linear = nn.Linear(2 * D_E, D_H)
        self.smax_fc = nn.Linear(D_H, C)

    def attend(self, M, x, mask):
        M_ = M.permute(1, 2, 0)
        x_ = self.transform(x).unsqueeze(1)
        mask_ = mask.unsqueeze(2).repeat(1, 1, M.shape[2]).transpose(1, 2)
        M_ = M_ * mask_
        alpha_ = torch.bmm(x_, M_) * mask.unsqueeze(1)
        alpha_ = F.softmax(torch.tanh(alpha_), dim=2)
        alpha_masked = alpha_ * mask.unsqueeze(1)
        alpha = alpha_masked / torch.sum(alpha_masked, dim=2, keepdim=True)
        return torch.bmm(alpha, M.transpose(0, 1))[:, 0, :]

    def forward(self, U, qmask, umask):
        emotions, _ = self.lstm(U)
        att = torch.cat([self.attend(emotions, t, umask).unsqueeze(0) for t in emotions], dim=0)
        hidden = self.dropout(F.relu(self.linear(att)))
        return F.log_softmax(self.smax_fc(hidden), 2), [], [], [], emotions


def torch_masked_nll(pred, target, mask):
    m = mask.reshape(-1, 1)
    return F.nll_loss(pred * m, target, reduction="sum") / mask.sum()


def timed(fn, window):
    """Mean wall time per call (us), device drained, over at least ``window`` seconds of back-to-back calls."""
    n, total, calls = 4, 0.0, 0
    while total < window:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
        calls += n
        n = min(2 * n, 256)
    return total * 1e6 / calls


def recurrence_device_us(fn, pattern, steps=5):
    """(device us per step of the kernels whose name contains ``pattern`` (None: all kernels), their launches per step)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    us = n = 0
    for e in prof.key_averages():
        if pattern is None or pattern in e.key:
            us += e.device_time * e.count
            n += e.count
    return us / steps, n / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lstm_model: needs an MI355X (no HIP device visible)")
    lines = ["| L | B | D_m | form | train step us, median (min .. max) | recurrence device us / step (launches) |",
             "|---|---|---|---|---|---|"]
    notes = []
    for L, B, D_m in SHAPES:
        torch.manual_seed(L)
        g = torch.Generator(device="cuda").manual_seed(L)
        U = torch.randn(L, B, D_m, device="cuda", generator=g)
        qmask = torch.zeros(L, B, 2, device="cuda")
        lengths = torch.randint(max(1, L // 2), L + 1, (B,), device="cuda", generator=g)
        lengths[0] = L
        umask = (torch.arange(L, device="cuda").unsqueeze(0) < lengths.unsqueeze(1)).float()
        label = torch.randint(0, C, (B * L,), device="cuda", generator=g)
        models = {"lstm": LSTMModel(D_m, D_E, D_H, C, P_DROP).cuda().train(), "gru": GRUModel(D_m, D_E, D_H, C, P_DROP).cuda().train(),
                  "reference": ReferenceStructure(D_m).cuda().train()}
        loss_f = MaskedNLLLoss()

        def step(name):
            m = models[name]
            m.zero_grad(set_to_none=True)
            lp = m(U, qmask, umask)[0].transpose(0, 1).contiguous().view(-1, C)
            if name == "reference":
                torch_masked_nll(lp, label, umask).backward()
            else:
                train.backward(loss_f(lp, label, umask))
                ops.join_weight_grads()
        for name in models:                                   # warm-up of every form
            for _ in range(5):
                step(name)
        torch.cuda.synchronize()
        res = {name: [] for name in models}
        for _ in range(args.rounds):                          # alternate the forms inside every round
            for name in models:
                res[name].append(timed(lambda: step(name), args.window))
        dev = {"lstm": recurrence_device_us(lambda: step("lstm"), "lstm_seq"),
               "gru": recurrence_device_us(lambda: step("gru"), "gru_seq"),
               "reference": recurrence_device_us(lambda: step("reference"), None)}
        for name in models:
            a = res[name]
            lines.append("| %d | %d | %d | %s | %.0f (%.0f .. %.0f) | %.1f (%.0f)%s |"
                         % (L, B, D_m, name, statistics.median(a), min(a), max(a), dev[name][0], dev[name][1],
                            " whole step" if name == "reference" else ""))
        med = {name: statistics.median(res[name]) for name in models}
        notes.append("(L, B, D_m) = (%d, %d, %d): train step lstm / gru = %.2f, reference / lstm = %.2f; recurrence device time "
                     "lstm / gru = %.2f (%.1f / %.1f us per step: 2 layers x forward + backward)"
                     % (L, B, D_m, med["lstm"] / med["gru"], med["reference"] / med["lstm"], dev["lstm"][0] / dev["gru"][0],
                        dev["lstm"][0], dev["gru"][0]))
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
