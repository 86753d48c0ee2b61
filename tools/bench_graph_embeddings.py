"""What the device-side speaker / modality embeddings (ops.graph_embeddings, csrc/graph_embed.hip) cost and save.

    python tools/bench_graph_embeddings.py [--nbatches 16] [--passes 6] [--runs 3]
      Step time of the cfg2 model with use_speaker=True, use_modal=True over --nbatches different ragged batches, three legs set up
      once and then timed in turn (torch_exact, hip_exact, hip_bucketed, torch_exact, ...), --runs rounds of --passes passes, host
      clock around a device synchronise:
        torch_exact    the embeddings added by MM_GCN.forward on separate tensors (per-dialogue qmask slices, argmax, nn.Embedding,
                       in-place adds, re-stack), exact-signature StepGraphCache -- what the model did before the operator existed
        hip_exact      MM_GCN.forward_stacked with the operator, exact-signature cache
        hip_bucketed   the same model through StepGraphCache(bucket_rows=16)
      plus the launches at the embedding site (torch profiler, one eager forward + backward of the site alone, both forms) and
      device-event times of the two launches back to back at the cfg2 and cfg3 sizes.  Prints one JSON line.
    python tools/bench_graph_embeddings.py --kernels 200
      only the two launches, 200 times each at both sizes: the program of a kernel trace
      (rocprofv3 --kernel-trace --stats -- python tools/bench_graph_embeddings.py --kernels 200).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = {"cfg2": dict(M=3, N=1760, D=200, S=2), "cfg3": dict(M=3, N=1056, D=200, S=9)}


def site_inputs(M, N, D, S, dev, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    B = 16
    L = N // B
    q = torch.zeros(L, B, S)
    q[torch.arange(L)[:, None], torch.arange(B)[None, :], torch.randint(0, S, (L, B), generator=g)] = 1
    idx = (torch.arange(L)[None, :] * B + torch.arange(B)[:, None]).reshape(-1)          # full-length dialogues, dialogue-major
    return dict(X=torch.randn(M, N, D, generator=g).to(dev), G=torch.randn(M, N, D, generator=g).to(dev), q=q.to(dev),
                idx=idx.to(dev), speaker=torch.randn(S, D, generator=g).to(dev).requires_grad_(True),
                modal=torch.randn(3, D, generator=g).to(dev).requires_grad_(True), lengths=[L] * B)


def launch_pair(s, reps):
    """(forward, backward) closures that launch the kernels ``reps`` times back to back."""
    import torch
    from mm_dfn_amd import ops
    X = s["X"].clone().requires_grad_(True)

    def fwd():
        for _ in range(reps):
            Y = ops.graph_embeddings(X, s["q"], s["idx"], s["speaker"], s["modal"], "avl")
        return Y
    Y = fwd()

    def bwd():
        for _ in range(reps):
            torch.autograd.grad(Y, (s["speaker"], s["modal"]), s["G"], retain_graph=True)
    return fwd, bwd


def event_us(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def kernels_only(reps, dev):
    import torch
    out = {}
    for name, size in SIZES.items():
        fwd, bwd = launch_pair(site_inputs(dev=dev, **size), reps)
        out[name] = {"fwd_us_back_to_back": [event_us(fwd, reps) for _ in range(3)],
                     "bwd_us_back_to_back": [event_us(bwd, reps) for _ in range(3)]}
    torch.cuda.synchronize()
    return out


def device_kernels(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    short = lambda k: k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][-60:]
    return sorted((short(e.key), e.count) for e in prof.key_averages() if not e.key.startswith("hip"))


def site_launches(dev):
    """Device launches of one forward + backward of the embedding site alone at the cfg2 size: the operator on the stack against
    the adds of MM_GCN.forward on separate tensors followed by the re-stack."""
    import torch
    from mm_dfn_amd import ops
    s = site_inputs(dev=dev, **SIZES["cfg2"])

    def new():
        X = s["X"].clone().requires_grad_(True)
        Y = ops.graph_embeddings(X, s["q"], s["idx"], s["speaker"], s["modal"], "avl")
        torch.autograd.grad(Y, (X, s["speaker"], s["modal"]), s["G"])

    def old():
        X = s["X"].clone().requires_grad_(True)
        a, v, l = (t * 1.0 for t in X.unbind(0))
        flat_q = torch.cat([s["q"][:n, i, :] for i, n in enumerate(s["lengths"])], dim=0)
        l += torch.nn.functional.embedding(torch.argmax(flat_q, dim=-1), s["speaker"])
        a += s["modal"][0].reshape(1, -1)
        v += s["modal"][1].reshape(1, -1)
        l += s["modal"][2].reshape(1, -1)
        torch.autograd.grad(torch.stack([a, v, l], 0), (X, s["speaker"], s["modal"]), s["G"])
    res = {}
    for name, fn in (("operator", new), ("torch_separate_tensors", old)):
        fn()
        k = device_kernels(fn)
        # (the X.clone() of the harness and, in the torch form, the three `* 1.0` copies that stand for the encoder's outputs)
        res[name] = {"launches": sum(c for _, c in k), "kernels": k}
    return res


def make_leg(name, batches, dev):
    import torch
    from mm_dfn_amd import FocalLoss, synthetic, train
    cfg = dict(synthetic.CONFIGS["cfg2"])
    model = synthetic.build_model(dropout=0.5, use_speaker=True, use_modal=True, **cfg)
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), 2021))
    model = model.to(dev).train()
    if name == "torch_exact":
        gm = model.graph_model

        def separate(feats, dia_len, qmask, test_label=False, stacked_out=False, flat_idx=None):
            present = [k for k in "avl" if k in "".join(gm.modals)]
            parts = {k: feats[i] for i, k in enumerate(present)}          # (selects: forward() edits them in place)
            return gm(parts.get('a', []), parts.get('v', []), parts.get('l', []), dia_len, qmask, test_label, stacked_out)
        gm.forward_stacked = separate
    cache = train.StepGraphCache(model, FocalLoss(gamma=0.5), max_entries=len(batches) + 8,
                                 bucket_rows=16 if name == "hip_bucketed" else 0)

    def one_pass():
        for b in batches:
            loss, _, _ = cache.step((b["textf"], b["visuf"], b["acouf"], b["qmask"], b["umask"], b["label"]), b["lengths"], True)
        return loss

    def timed(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (passes * len(batches)) * 1e3
    one_pass()                      # captures
    one_pass()                      # the first all-replay pass (bucketed: the first retargets)
    torch.cuda.synchronize()
    return dict(timed=timed, cache=cache)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbatches", type=int, default=16)
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    import torch
    from mm_dfn_amd import synthetic
    assert torch.cuda.is_available(), "needs an MI355X: there is nothing to time without one"
    dev = torch.device("cuda", torch.cuda.current_device())
    if a.kernels:
        print(json.dumps({"reps": a.kernels, "sizes": SIZES, "device_events": kernels_only(a.kernels, dev)}))
        return
    cfg = dict(synthetic.CONFIGS["cfg2"])
    batches = [synthetic.make_batch(3000 + i, ragged=True, device=dev, **cfg) for i in range(a.nbatches)]
    names = ["torch_exact", "hip_exact", "hip_bucketed"]
    legs = {n: make_leg(n, batches, dev) for n in names}
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(legs[n]["timed"](a.passes))
    res = {"workload": "cfg2 ragged, use_speaker + use_modal, dropout 0.5, %d different batches on the device, forward + loss + "
                       "backward through StepGraphCache.step, %d passes per run, %d alternating runs"
                       % (a.nbatches, a.passes, a.runs)}
    for n in names:
        t, c = times[n], legs[n]["cache"]
        res[n] = {"ms_per_step": {"median": statistics.median(t), "min": min(t), "max": max(t), "runs": t},
                  "entries": len(c.entries), "misses": c.misses, "hits": c.hits, "fallbacks": c.fallbacks}
    res["site_launches"] = site_launches(dev)
    res["device_events"] = kernels_only(200, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
