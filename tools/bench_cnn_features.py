"""Time the K18 kernels (csrc/cnn_features.hip through cnn_features.cnn_pool: embedding gather -> Conv1d per kernel size -> ReLU
-> max over time, forward and backward) against the same block evaluated by torch eager on the same device in the same process
(its library path: an embedding gather that materialises (rows, W, D), a transpose copy, one convolution + ReLU + max per kernel
size, and autograd's backward of each), alternating the two forms per round:

    python tools/bench_cnn_features.py [--rounds 3] [--window 0.5] [--out FILE.md]

Per (rows, W, D) in (1120, 250, 300), (1120, 64, 100) with F = 50 filters, kernel sizes (3, 4, 5), a vocabulary of 20 000 and every
row live: host wall time of forward + backward (synchronised) over windows of at least ``--window`` seconds after a warm-up of
both forms, the median over the rounds and the min .. max of the rounds, with a trainable and with a frozen table; and, from a
device trace of 3 steps with the profiler on (a run of its own, after the timed windows), the device time and the launches per
step of every kernel family.  The flop count is the issue's formula, 2 D F sum_K K (W - K + 1) per row, each way counted once;
"share of the exact-f32 MFMA peak" is that count over the forward kernel's device time over 157.3 TFLOP/s (v_mfma_f32_16x16x4_f32:
32 MAC / cycle / SIMD x 1024 SIMDs x 2.4 GHz), the rate the same products would have without the bf16-piece form.
No thresholds: the numbers are what they are.  Needs an MI355X: there is no CPU path."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F_

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_lstm_model import timed  # noqa: E402
from mm_dfn_amd import cnn_features  # noqa: E402

SHAPES = [(1120, 250, 300), (1120, 64, 100)]
FILTERS, SIZES, VOCAB = 50, (3, 4, 5), 20000
F32_MFMA_PEAK = 32 * 2 * 1024 * 2.4e9
FAMILIES = ("cnn_cut", "cnn_pool_fwd", "cnn_wgrad", "cnn_table_keys", "cnn_table_bounds", "cnn_table_bwd")


def flops(rows, W, D):
    return 2.0 * D * FILTERS * sum(K * (W - K + 1) for K in SIZES) * rows


def make(rows, W, D, frozen, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    tokens = torch.randint(0, VOCAB, (rows, W), device="cuda", generator=g)
    table = (torch.randn(VOCAB, D, device="cuda", generator=g) / D ** 0.5).requires_grad_(not frozen)
    ws = [(torch.randn(FILTERS, D, K, device="cuda", generator=g) / (D * K) ** 0.5).requires_grad_(True) for K in SIZES]
    bs = [torch.zeros(FILTERS, device="cuda").requires_grad_(True) for _ in SIZES]
    mask = torch.ones(rows, device="cuda")
    dp = torch.randn(rows, len(SIZES) * FILTERS, device="cuda", generator=g)
    prm = [table] + ws + bs

    def clear():
        for p in prm:
            p.grad = None

    def fused():
        clear()
        pooled, _, _ = cnn_features.cnn_pool(tokens, table, ws, bs, mask, check=False)
        pooled.backward(dp)

    def eager():
        clear()
        emb = F_.embedding(tokens, table).transpose(1, 2).contiguous()
        pooled = torch.cat([torch.relu(F_.conv1d(emb, w, b)).max(2)[0] for w, b in zip(ws, bs)], 1)
        pooled.backward(dp)

    def fused_fwd():
        with torch.no_grad():
            cnn_features.cnn_pool(tokens, table, ws, bs, mask, check=False)

    def eager_fwd():
        with torch.no_grad():
            emb = F_.embedding(tokens, table).transpose(1, 2).contiguous()
            torch.cat([torch.relu(F_.conv1d(emb, w, b)).max(2)[0] for w, b in zip(ws, bs)], 1)
    return dict(fused=fused, eager=eager, fused_fwd=fused_fwd, eager_fwd=eager_fwd)


def trace(fn, steps=3):
    """{kernel name: (device us per step, launches per step)} of ``steps`` calls."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
    return {e.key: (e.device_time * e.count / steps, e.count / steps) for e in prof.key_averages()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cnn_features: needs an MI355X (no HIP device visible)")
    lines = ["tile words TW = %d, rows per workgroup RG = %d" % (cnn_features.tile_words(), cnn_features.rows_per_group()), "",
             "| rows | W | D | table | form | fwd + bwd us, median (min .. max) | fwd only us, median | device us / step (launches) |",
             "|---|---|---|---|---|---|---|---|"]
    detail = []
    for rows, W, D in SHAPES:
        for frozen in (False, True):
            fns = make(rows, W, D, frozen, W)
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            res = {k: [] for k in fns}
            for _ in range(args.rounds):
                for k in fns:
                    res[k].append(timed(fns[k], args.window))
            tr = {k: trace(fns[k]) for k in ("fused", "eager")}
            for form in ("fused", "eager"):
                a, f = res[form], res[form + "_fwd"]
                dev = sum(v[0] for v in tr[form].values())
                n = sum(v[1] for v in tr[form].values())
                lines.append("| %d | %d | %d | %s | %s | %.0f (%.0f .. %.0f) | %.0f | %.0f (%.0f) |"
                             % (rows, W, D, "frozen" if frozen else "trainable", form, statistics.median(a), min(a), max(a),
                                statistics.median(f), dev, n))
            fam = {p: sum(v[0] for k, v in tr["fused"].items() if p in k) for p in FAMILIES}
            other = sum(v[0] for k, v in tr["fused"].items() if not any(p in k for p in FAMILIES))
            fl = flops(rows, W, D)
            detail.append("(rows, W, D) = (%d, %d, %d), %s table: %.2f GFLOP each way; device us per step: %s, torch glue (sort, "
                          "slice, zero fill) %.1f; forward kernel %.1f TFLOP/s = %.1f %% of the exact-f32 MFMA peak; eager / fused "
                          "fwd + bwd wall time = %.2f, fwd only = %.2f"
                          % (rows, W, D, "frozen" if frozen else "trainable", fl / 1e9,
                             ", ".join("%s %.1f" % (p, fam[p]) for p in FAMILIES), other,
                             fl / fam["cnn_pool_fwd"] / 1e6, 100 * fl / (fam["cnn_pool_fwd"] * 1e-6) / F32_MFMA_PEAK,
                             statistics.median(res["eager"]) / statistics.median(res["fused"]),
                             statistics.median(res["eager_fwd"]) / statistics.median(res["fused_fwd"])))
            top = sorted(tr["eager"].items(), key=lambda kv: -kv[1][0])[:6]
            detail.append("    eager, largest kernels: " + "; ".join("%s %.1f us (%.0f)" % (k[:60], v[0], v[1]) for k, v in top))
    text = "\n".join(lines + [""] + detail) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
