"""Launches of the graph-free fusion baselines at cfg2 shapes (N = 1 760 utterances): the grouped residual products
[graph_net_m(f_m) | f_m] and every launch of the LMF module each way (subnets, the 3 R factor products, csrc/lmf.hip, the
column sums, the factor-gradient gemm_tn and the input-gradient products).  Graph-captured timing; the dense stages report
their fraction of the 157.3 TF f32 MFMA peak, the pointwise kernels their HBM bytes.  TFN (tfn_only) has no kernels yet.

    python tools/bench_fusion_baselines.py [--rows 1760]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mm_dfn_amd import _hip, ops  # noqa: E402
from mm_dfn_amd.fusion import LMF  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1760)
    N = ap.parse_args().rows
    dev = "cuda"
    torch.manual_seed(0)
    print("N = %d rows" % N)

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
