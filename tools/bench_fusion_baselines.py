"""Launches of the graph-free fusion baselines at cfg2 shapes (N = 1 760 utterances): the grouped residual products
[graph_net_m(f_m) | f_m] and every launch of the LMF module each way (subnets, the 3 R factor products, csrc/lmf.hip, the
column sums, the factor-gradient gemm_tn and the input-gradient products).  Graph-captured timing; the dense stages report
their fraction of the 157.3 TF f32 MFMA peak, the pointwise kernels their HBM bytes.  The TFN legs (default widths, 101^3 =
1 030 301 fused features): the three generated-operand launches of csrc/tensor_fusion.hip with the dropout on (median and
spread of several graph replays), the peak extra device memory of one forward + backward, and for comparison the library route
-- Z materialised, F.dropout, F.linear and autograd as one unfused float32 call through torch.

    python tools/bench_fusion_baselines.py [--rows 1760] [--tfn-only] [--no-tfn]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mm_dfn_amd import _hip, ops  # noqa: E402
from mm_dfn_amd.fusion import LMF, TFN  # noqa: E402

PEAK_TF = 157.3


def gtime(fn, iters=50):
    """us per call, from two replays of a graph holding ``iters`` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (2 * iters) * 1e3


def report(name, us, flop=0.0, nbytes=0.0):
    extra = []
    if flop:
        extra.append("%.2f GFLOP, %.1f TF/s = %.3f of the f32 MFMA peak" % (flop / 1e9, flop / us / 1e6, flop / us / 1e6 / PEAK_TF))
    if nbytes:
        extra.append("%.1f MB, %.2f TB/s" % (nbytes / 1e6, nbytes / us / 1e6))
    print("%-44s %9.1f us   %s" % (name, us, "; ".join(extra)))


def gtime_spread(fn, iters=4, reps=5):
    """(median, min, max) us per call over ``reps`` timed replays of a graph holding ``iters`` calls (warmed)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def peak_extra(fn):
    """Peak device memory of ``fn()`` above what was allocated before it, in bytes (after a warm-up call)."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def tfn_legs(N, dev):
    import torch.nn.functional as F
    p = 0.4
    mod = TFN().to(dev).train()
    H = (mod.audio_hidden, mod.video_hidden, mod.text_hidden)
    W1, b1 = mod.post_fusion_layer_1.weight, mod.post_fusion_layer_1.bias
    O, K = W1.shape
    flop = 2.0 * N * K * O
    print("TFN: K = %d, O = %d, %.2f TFLOP per product, W1 %.2f GB" % (K, O, flop / 1e12, 4.0 * O * K / 1e9))
    hs = [torch.randn(N, h, device=dev) for h in H]
    lib = _hip.lib()
    state = torch.tensor([1234, 0, 0, 0], dtype=torch.int64, device=dev)
    used = torch.zeros(2, dtype=torch.int64, device=dev)
    counters = 4 * ((N * ((K + 7) // 8) + 3) // 4)
    wf = torch.empty(int(lib.mmdfn_tfn_workspace(N, H[0], H[1], H[2], O, 0)), device=dev)
    wd = torch.empty(int(lib.mmdfn_tfn_workspace(N, H[0], H[1], H[2], O, 1)), device=dev)
    y1, dy, dpre = torch.empty(N, O, device=dev), torch.randn(N, O, device=dev), torch.empty(N, O, device=dev)
    dhs = [torch.empty_like(h) for h in hs]
    dW1 = torch.empty(O, K, device=dev)
    w1, bb = W1.detach(), b1.detach()
    lds = [h.stride(0) for h in hs]
    P = _hip.ptr

    def fwd():
        _hip.check(lib.mmdfn_tfn_fwd(P(hs[0]), P(hs[1]), P(hs[2]), lds[0], lds[1], lds[2], P(w1), w1.stride(0), P(bb), P(state),
                                     P(used), counters, 1.0 - p, ops.keep_scale(p), P(y1), P(wf), N, H[0], H[1], H[2], O, 1,
                                     _hip.stream()), "mmdfn_tfn_fwd")

    def bwd_input():
        _hip.check(lib.mmdfn_tfn_bwd_input(P(dy), P(y1), 1, P(w1), w1.stride(0), P(hs[0]), P(hs[1]), P(hs[2]), lds[0], lds[1],
                                           lds[2], P(used), 1.0 - p, ops.keep_scale(p), P(dpre), P(dhs[0]), P(dhs[1]), P(dhs[2]),
                                           P(wd), N, H[0], H[1], H[2], O, _hip.stream()), "mmdfn_tfn_bwd_input")

    def bwd_weight():
        _hip.check(lib.mmdfn_tfn_bwd_weight(P(dpre), P(hs[0]), P(hs[1]), P(hs[2]), lds[0], lds[1], lds[2], P(used), 1.0 - p,
                                            ops.keep_scale(p), P(dW1), N, H[0], H[1], H[2], O, _hip.stream()),
                   "mmdfn_tfn_bwd_weight")

    for name, fn in (("TFN fused fwd (+ slab sum, bias, ReLU)", fwd), ("TFN fused dh_a, dh_v, dh_t (+ slab sum)", bwd_input),
                     ("TFN fused dW1", bwd_weight)):
        med, lo, hi = gtime_spread(fn)
        report(name, med, flop=flop)
        print("%-44s           min %.1f / max %.1f us over 5 replays of 4 calls" % ("", lo, hi))
    del dW1, wf, wd

    hg = [h.clone().requires_grad_(True) for h in hs]

    def fused_step():
        y = ops.tfn_fuse(hg[0], hg[1], hg[2], W1, b1, p, True)
        torch.autograd.grad(y, hg + [W1, b1], dy)
    slab_f = 4 * int(lib.mmdfn_tfn_workspace(N, H[0], H[1], H[2], O, 0))
    slab_d = 4 * int(lib.mmdfn_tfn_workspace(N, H[0], H[1], H[2], O, 1))
    formula = max(slab_f + 4 * N * O, 4 * N * O * 3 + slab_d + 4 * N * sum(H) + 4 * O * K + 4 * O)
    print("TFN fused forward + backward: peak extra memory %.3f GB (formula %.3f GB: dW1 %.3f GB + dgrad slabs %.3f GB + "
          "(N, O) and (N, H) results; forward slabs %.3f GB are freed before)"
          % (peak_extra(fused_step) / 1e9, formula / 1e9, 4.0 * O * K / 1e9, slab_d / 1e9, slab_f / 1e9))

    def library_step():
        one = torch.ones(N, 1, device=dev)
        a, v, t = (torch.cat([one, h], 1) for h in hg)
        Z = torch.bmm(torch.bmm(a.unsqueeze(2), v.unsqueeze(1)).view(N, -1, 1), t.unsqueeze(1)).view(N, -1)
        y = F.relu(F.linear(F.dropout(Z, p, True), W1, b1))
        torch.autograd.grad(y, hg + [W1, b1], dy)
    try:
        mem = peak_extra(library_step)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ts = []
        for _ in range(5):
            e0.record()
            library_step()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        ts.sort()
        print("TFN library route forward + backward (eager)  %9.1f us (min %.1f / max %.1f); peak extra memory %.2f GB"
              % (ts[2], ts[0], ts[-1], mem / 1e9))
    except torch.OutOfMemoryError as e:
        print("TFN library route: out of memory (%s)" % str(e).splitlines()[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        e0.record()
        fused_step()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    print("TFN fused route forward + backward (eager)    %9.1f us (min %.1f / max %.1f)" % (ts[2], ts[0], ts[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1760)
    ap.add_argument("--tfn-only", action="store_true")
    ap.add_argument("--no-tfn", action="store_true")
    args = ap.parse_args()
    N = args.rows
    dev = "cuda"
    torch.manual_seed(0)
    print("N = %d rows" % N)
    if not args.tfn_only:
        other_legs(N, dev)
    if not args.no_tfn:
        tfn_legs(N, dev)


def other_legs(N, dev):

    # residual products: 3 x (N, 200) . (200 -> 100), written into column slices of (3, N, 300)
    feats = torch.randn(3, N, 200, device=dev)
    ws = [torch.randn(100, 200, device=dev) * 0.05 for _ in range(3)]
    bs = [torch.randn(100, device=dev) for _ in range(3)]
    report("residual products fwd (1 grouped launch)", gtime(lambda: ops.residual_products(feats, ws, bs)),
           flop=3 * 2.0 * N * 200 * 100)

    mod = LMF().to(dev)
    R, O, H = mod.rank, mod.output_dim, mod.audio_hidden
    xs = [torch.randn(N, 300, device=dev, requires_grad=True) for _ in range(3)]
    facs = (mod.audio_factor, mod.video_factor, mod.text_factor)
    nets = (mod.audio_subnet, mod.video_subnet, mod.text_subnet)
    hs = [torch.randn(N, H, device=dev) for _ in range(3)]
    sub_flop = 3 * 2.0 * N * 300 * H
    prod_flop = 3 * R * 2.0 * N * H * O

    report("LMF subnets (1 grouped launch)",
           gtime(lambda: ops.linear_group_raw([dict(x=x, w=n.weight, b=n.bias) for x, n in zip(xs, nets)])), flop=sub_flop)
    P = torch.empty(N, 3 * R * O, device=dev)
    probs = [dict(x=hs[m], wk=facs[m].detach()[r, 1:, :], out=P[:, (m * R + r) * O:(m * R + r + 1) * O])
             for m in range(3) for r in range(R)]

    def products():
        ops.linear_group_raw(probs[:8])
        ops.linear_group_raw(probs[8:])
    report("LMF factor products (2 grouped launches)", gtime(products), flop=prod_flop)
    out = torch.empty(N, O, device=dev)
    f = [t.detach() for t in facs]
    w, b = mod.fusion_weights.detach(), mod.fusion_bias.detach()
    lib = _hip.lib()

    def fused_fwd():
        lib.mmdfn_lmf_fwd(_hip.ptr(P), _hip.ptr(f[0]), _hip.ptr(f[1]), _hip.ptr(f[2]), f[0].stride(0), f[1].stride(0),
                          f[2].stride(0), _hip.ptr(w), _hip.ptr(b), _hip.ptr(out), N, O, R, P.stride(0), O, _hip.stream())
    report("LMF fused fwd (csrc/lmf.hip)", gtime(fused_fwd), nbytes=4.0 * N * (2 * 3 * R * O + O))
    width = int(lib.mmdfn_lmf_bwd_width(O, R))
    D = torch.empty(N, width, device=dev)
    g = torch.randn(N, O, device=dev)

    def fused_bwd():
        lib.mmdfn_lmf_bwd(_hip.ptr(g), _hip.ptr(P), _hip.ptr(w), _hip.ptr(D), N, O, R, O, P.stride(0), D.stride(0), _hip.stream())
    report("LMF fused bwd (csrc/lmf.hip)", gtime(fused_bwd), nbytes=4.0 * N * (O + 3 * R * O + width))
    report("LMF column sums of [dP | g | T]", gtime(lambda: ops.colsum(D)), nbytes=4.0 * N * width)
    dfs = [torch.empty_like(t) for t in f]
    blk = lambda m, r: D[:, (m * R + r) * O:(m * R + r + 1) * O]
    tn = [dict(A=hs[m], B=blk(m, r), C=dfs[m][r, 1:, :]) for m in range(3) for r in range(R)]

    def factor_grads():
        ops.gemm_tn_grouped(tn[:8])
        ops.gemm_tn_grouped(tn[8:])
    report("LMF d factor (2 grouped gemm_tn)", gtime(factor_grads), flop=prod_flop)
    dhs = [torch.empty_like(h) for h in hs]

    def input_grads():
        for r in range(R):
            ops.linear_group_raw([dict(x=blk(m, r), w=f[m][r, 1:, :], out=dhs[m], accumulate=r > 0) for m in range(3)])
    report("LMF dh (%d accumulating grouped launches)" % R, gtime(input_grads), flop=prod_flop)

    # the whole module each way (autograd; weight gradients of the subnets in line)
    def whole_fwd():
        return mod(*xs)
    report("LMF module forward", gtime(lambda: whole_fwd()), flop=sub_flop + prod_flop)
    G = torch.randn(N, O, device=dev)

    def whole_step():
        y = mod(*xs)
        (dx_a, dx_v, dx_t, *_) = torch.autograd.grad(y, list(xs) + list(mod.parameters()), G)
    for _ in range(3):
        whole_step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        whole_step()
    e1.record()
    e1.synchronize()
    report("LMF module forward + backward (eager)", e0.elapsed_time(e1) / 20 * 1e3, flop=3 * (sub_flop + prod_flop))


if __name__ == "__main__":
    main()
