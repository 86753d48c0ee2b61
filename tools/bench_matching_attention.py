"""Time the matching-attention kernels (K14, csrc/matching_attention.hip) forward and forward + backward against two torch forms
on the same device in the same process, alternating the three per round:

    loop     the reference's procedure with torch ops, one query row at a time (model.py:66-76,84: L x (bmm, tanh, softmax,
             renormalise, bmm))
    einsum   the closed formula batched: einsum, tanh, exp, masked row sum, einsum
    kernel   ops.matching_attention

    python tools/bench_matching_attention.py [--rounds 5] [--window 1.0] [--out FILE.md]

Per shape (L, B) in (110, 16), (33, 32), (512, 8) at D = 200, Tq = L: device-event time per call over windows of at least
``--window`` seconds after a warm-up of every form at that shape, the median over the rounds and the run-to-run spread
(min .. max of the rounds), the algorithmic FLOPs and bytes computed from the shapes, and the kernel's achieved rates.
Needs an MI355X: there is no CPU path."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mm_dfn_amd import ops  # noqa: E402

SHAPES = [(110, 16), (33, 32), (512, 8)]
D = 200


def algorithmic(Tq, L, B, Dm):
    """(forward FLOPs, backward FLOPs, forward bytes, backward bytes): the products the formula needs (2 per multiply-add) and
    each operand / result read or written once."""
    pair = 2.0 * Tq * L * B * Dm
    fwd_flops = 2 * pair                                 # z, pool
    bwd_flops = 4 * pair                                 # dP, dX, dz^T X, alpha^T G
    fwd_bytes = 4.0 * (Tq * B * Dm + L * B * Dm + B * L + Tq * B * Dm + 2 * Tq * B * L)
    bwd_bytes = 4.0 * (2 * Tq * B * Dm + L * B * Dm + B * L + 2 * Tq * B * L + Tq * B * Dm + L * B * Dm + 2 * Tq * B * L)
    return fwd_flops, bwd_flops, fwd_bytes, bwd_bytes


def loop_form(X, M, mask):
    mem = M.transpose(0, 1)
    masked = (mem * mask.unsqueeze(2)).transpose(1, 2)
    pools, alphas = [], []
    for t in range(X.shape[0]):
        score = torch.bmm(X[t].unsqueeze(1), masked) * mask.unsqueeze(1)
        w = torch.softmax(torch.tanh(score), dim=2) * mask.unsqueeze(1)
        alpha = w / w.sum(dim=2, keepdim=True)
        pools.append(torch.bmm(alpha, mem)[:, 0, :].unsqueeze(0))
        alphas.append(alpha[:, 0, :])
    return torch.cat(pools, 0), alphas


def einsum_form(X, M, mask):
    z = torch.einsum("tbd,sbd->tbs", X, M)
    e = torch.exp(torch.tanh(z)) * mask.unsqueeze(0)
    alpha = e / e.sum(2, keepdim=True)
    return torch.einsum("tbs,sbd->tbd", alpha, M), alpha


def kernel_form(X, M, mask):
    return ops.matching_attention(X, M, mask)


def timed(fn, window):
    """Mean device time per call (us) over at least ``window`` seconds of back-to-back calls."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total, calls = 8, 0.0, 0
    while total < window * 1e3:
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        total += start.elapsed_time(stop)
        calls += n
        n = min(4 * n, 4096)
    return total * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_matching_attention: needs an MI355X (no HIP device visible)")
    lines = ["| L | B | form | fwd us (min .. max) | fwd+bwd us (min .. max) |", "|---|---|---|---|---|"]
    notes = []
    for L, B in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(L)
        sc = (1.0 / D ** 0.5) ** 0.5
        X = (sc * torch.randn(L, B, D, device="cuda", generator=g)).requires_grad_(True)
        M = (sc * torch.randn(L, B, D, device="cuda", generator=g)).requires_grad_(True)
        G = torch.randn(L, B, D, device="cuda", generator=g)
        lengths = torch.randint(max(1, L // 2), L + 1, (B,), device="cuda", generator=g)
        lengths[0] = L
        mask = (torch.arange(L, device="cuda").unsqueeze(0) < lengths.unsqueeze(1)).float()
        forms = {"loop": loop_form, "einsum": einsum_form, "kernel": kernel_form}

        def fwd(f):
            with torch.no_grad():
                f(X.detach(), M.detach(), mask)

        def both(f):
            X.grad = M.grad = None
            f(X, M, mask)[0].backward(G)
        # the three agree at this shape (a timing of different results is no comparison)
        ref = einsum_form(X.detach().double(), M.detach().double(), mask.double())[0]
        for name, f in forms.items():
            err = float((f(X.detach(), M.detach(), mask)[0].double() - ref).abs().max() / ref.abs().max())
            assert err < 1e-5, (name, err)
        for f in forms.values():                          # warm-up of every form, both ways
            for _ in range(3):
                fwd(f)
                both(f)
        torch.cuda.synchronize()
        res = {name: ([], []) for name in forms}
        for _ in range(args.rounds):                      # alternate the forms inside every round
            for name, f in forms.items():
                res[name][0].append(timed(lambda: fwd(f), args.window))
                res[name][1].append(timed(lambda: both(f), args.window))
        for name in forms:
            a, b = res[name]
            lines.append("| %d | %d | %s | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) |"
                         % (L, B, name, statistics.median(a), min(a), max(a), statistics.median(b), min(b), max(b)))
        ff, bf, fb, bb = algorithmic(L, L, B, D)
        kf, kb = statistics.median(res["kernel"][0]), statistics.median(res["kernel"][1])
        notes.append("(L, B) = (%d, %d): forward %.1f MFLOP, %.2f MB; backward %.1f MFLOP, %.2f MB; kernel forward %.2f TFLOP/s, "
                     "%.1f GB/s; forward + backward %.2f TFLOP/s (host enqueue included: eager autograd)"
                     % (L, B, ff / 1e6, fb / 1e6, bf / 1e6, bb / 1e6, ff / kf / 1e6, fb / kf / 1e3, (ff + bf) / kb / 1e6))
    text = "\n".join(lines + [""] + notes) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
