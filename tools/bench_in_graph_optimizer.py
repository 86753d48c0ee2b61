"""What the in-graph optimizer saves in the streamed pass loop (cfg2, the workload of bench.py's ``captured_flat_adam`` leg:
32 different ragged batches from pinned host memory through train.train_or_eval_graph_model and an exact-signature
StepGraphCache, dropout 0.5).

    python tools/bench_in_graph_optimizer.py [--nbatches 32] [--passes 8] [--runs 3]
        leg A  FlatAdam outside the graph: replay, then pack + update + plane invalidation from the host (the behaviour before
               the device-state path existed)
        leg B  FlatAdam(capturable=True) inside it: StepGraphCache(optimizer=opt), a replay is the whole step
        leg C  leg B with max_grad_norm=1.0 (one more read of the flat gradient and one more launch): reported, not gated
      Each leg is set up once (its first pass captures every signature); then --runs rounds time --passes steady passes of every
      leg in turn (A, B, C, A, B, C, ...) on the same device, host clock around a device synchronise.  Prints one JSON line:
      median / min / max ms per step per leg, and ``accepted``: leg B's median is not above leg A's by more than leg A's own
      min-max spread.
    python tools/bench_in_graph_optimizer.py --leg B --passes 10
      one leg alone, for a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_in_graph_optimizer.py --leg B ...)
    python tools/bench_in_graph_optimizer.py --kernel-stats few.csv many.csv --steps K
      steady-state kernel time and launches per step from the kernel_stats.csv of two traced runs of one leg that differ by K
      steady steps (set-up, warm-up passes and captures cancel in the difference).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LEGS = {"A": dict(), "B": dict(capturable=True), "C": dict(capturable=True, max_grad_norm=1.0)}


def make_leg(name, batches, dev, dropout):
    import torch
    from mm_dfn_amd import FocalLoss, synthetic, train
    from mm_dfn_amd import data as D
    from mm_dfn_amd.optim import FlatAdam
    cfg = dict(synthetic.CONFIGS["cfg2"])
    model = synthetic.build_model(dropout=dropout, **cfg)
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), 2021))
    model = model.to(dev)
    loss_f = FocalLoss(gamma=0.5)
    opt = FlatAdam(model, lr=3e-4, weight_decay=1e-4, **LEGS[name])
    cache = train.StepGraphCache(model, loss_f, max_entries=len(batches) + 4, optimizer=opt if name != "A" else None)

    def one_pass():
        return train.train_or_eval_graph_model(model, loss_f, D.DevicePrefetcher(batches, device=dev), 0, True, opt, False,
                                               graph_cache=cache)

    def timed(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            one_pass()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (passes * len(batches)) * 1e3

    # the first pass captures every signature (leg A: twice for the ones captured before FlatAdam laid the parameters out), the
    # second one is the first all-replay pass
    one_pass()
    loss = one_pass()[2]
    torch.cuda.synchronize()
    return dict(timed=timed, cache=cache, opt=opt, loss=loss)


def kernel_stats(few, many, steps):
    def load(path):
        rows = list(csv.DictReader(open(path)))
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in rows}
    a, b = load(few), load(many)
    per = {k: ((b[k][0] - a.get(k, (0, 0.0))[0]) / steps, (b[k][1] - a.get(k, (0, 0.0))[1]) / steps / 1e3) for k in b}
    per = {k: v for k, v in per.items() if v[0] > 0}
    side = {}
    for tag in ("adam_step", "adam_prepare", "grad_sumsq", "CatArrayBatchedCopy", "cut_planes"):
        hit = [v for k, v in per.items() if tag in k]
        if hit:
            side[tag] = {"launches_per_step": round(sum(v[0] for v in hit), 2), "us_per_step": round(sum(v[1] for v in hit), 2)}
    out = {"steps": steps, "launches_per_step": round(sum(v[0] for v in per.values()), 2),
           "kernel_us_per_step": round(sum(v[1] for v in per.values()), 1), "optimizer_side": side}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nbatches", type=int, default=32)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--leg", choices=sorted(LEGS), default=None)
    ap.add_argument("--kernel-stats", nargs=2, metavar=("FEW", "MANY"), default=None)
    ap.add_argument("--steps", type=int, default=0)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats[0], a.kernel_stats[1], a.steps)
    import torch
    from mm_dfn_amd import synthetic
    assert torch.cuda.is_available(), "needs an MI355X: there is nothing to time without one"
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = dict(synthetic.CONFIGS["cfg2"])
    batches = []
    for i in range(a.nbatches):
        b = synthetic.make_batch(3000 + i, ragged=True, **cfg)
        batches.append([b["textf"].pin_memory(), b["visuf"].pin_memory(), b["acouf"].pin_memory(), b["qmask"].pin_memory(),
                        b["umask"].pin_memory(), b["label"].pin_memory(), ["b%d" % i]])
    names = [a.leg] if a.leg else sorted(LEGS)
    legs = {n: make_leg(n, batches, dev, a.dropout) for n in names}
    if a.leg:
        ms = legs[a.leg]["timed"](a.passes)
        print(json.dumps({"leg": a.leg, "steady_passes": a.passes, "steady_steps": a.passes * a.nbatches, "ms_per_step": ms}))
        return
    times = {n: [] for n in names}
    for _ in range(a.runs):
        for n in names:
            times[n].append(legs[n]["timed"](a.passes))
    res = {"workload": "cfg2 ragged, %d different batches streamed through train_or_eval_graph_model, %d passes per run, %d "
                       "alternating runs, dropout %g" % (a.nbatches, a.passes, a.runs, a.dropout)}
    for n in names:
        t = times[n]
        res[n] = {"optimizer": "FlatAdam(%s)" % ", ".join("%s=%r" % kv for kv in LEGS[n].items()),
                  "ms_per_step": {"median": statistics.median(t), "min": min(t), "max": max(t), "runs": t},
                  "steps_applied": legs[n]["opt"].t, "entries": len(legs[n]["cache"].entries),
                  "recaptures": legs[n]["cache"].recaptures, "loss_of_the_second_pass": legs[n]["loss"]}
    A, B = res["A"]["ms_per_step"], res["B"]["ms_per_step"]
    res["accepted"] = bool(B["median"] <= A["median"] + (A["max"] - A["min"]))
    res["clip_extra_ms_per_step"] = res["C"]["ms_per_step"]["median"] - B["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
