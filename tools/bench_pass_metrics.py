"""What the pass loop's book-keeping costs on the bucketed streamed pass of bench.py's streamed leg (cfg2 ragged, FlatAdam,
StepGraphCache(bucket_rows=32) pre-captured from batches drawn like the timed ones, every timed pass streams length tuples the
cache has never seen): ms per step and device launches per replayed step with ``device_metrics`` off (per-step views, clones
before an entry is reused, argmax in the graph, end-of-pass concatenation) and on (train.PassStats: one launch in the step, one
copy per pass), in ALTERNATING rounds inside one process.

    python tools/bench_pass_metrics.py [--batches 32] [--rounds 6] [--modes off,on] [--out file.json]

``--modes off`` runs on a tree without train.PassStats as well (the parent commit's figures: copy this file there).  Times are
host clocks around passes that end in a device synchronise; launch counts come from a torch.profiler trace of one further pass
per mode (kernels + copies + fills on every stream), taken after the timed rounds.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mm_dfn_amd import FocalLoss, synthetic, train  # noqa: E402
from mm_dfn_amd import data as D  # noqa: E402
from mm_dfn_amd.optim import FlatAdam  # noqa: E402


def make(cfg, seed0, n):
    out = []
    for i in range(n):
        b = synthetic.make_batch(seed0 + i, ragged=True, **cfg)
        out.append([b["textf"].pin_memory(), b["visuf"].pin_memory(), b["acouf"].pin_memory(), b["qmask"].pin_memory(),
                    b["umask"].pin_memory(), b["label"].pin_memory(), ["u%d" % i]])
    return out


class Leg:
    """One model + FlatAdam + bucketed cache, warmed the way bench.streamed_leg warms it."""

    def __init__(self, on, cfg, nbatches, dropout, dev):
        self.on, self.cfg, self.n = on, cfg, nbatches
        self.loss_f = FocalLoss(gamma=0.5)
        model = synthetic.build_model(dropout=dropout, **cfg)
        model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), 2021))
        self.model = model.to(dev)
        self.opt = FlatAdam(self.model, lr=3e-4, weight_decay=1e-4)
        kw = {}
        if on:
            kw["pass_stats"] = train.PassStats(cfg["C"], dev, ignore_index=train.StepGraphCache.IGNORE)
        self.cache = train.StepGraphCache(self.model, self.loss_f, max_entries=96, bucket_rows=32, **kw)
        self.kw = dict(device_metrics=True) if on else {}
        self.pre = D.DevicePrefetcher(make(cfg, 6000, 2), device=dev)
        self.run()                        # two real steps first: FlatAdam lays the parameters out at its first step
        for w in range(4):
            self.pre.loader = make(cfg, 7000 + 100 * w, nbatches)
            self.cache.precapture(self.pre, train_flag=True)
        torch.cuda.synchronize()

    def run(self):
        return train.train_or_eval_graph_model(self.model, self.loss_f, self.pre, 0, True, self.opt, False,
                                               graph_cache=self.cache, **self.kw)

    def timed(self, batches):
        self.pre.loader = batches
        h0, m0 = self.cache.hits, self.cache.misses
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(ms_per_step=dt / self.n * 1e3, replayed=self.cache.hits - h0, captured=self.cache.misses - m0)

    def launches(self, batches):
        from torch.profiler import ProfilerActivity, profile
        self.pre.loader = batches
        h0, m0 = self.cache.hits, self.cache.misses
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            self.run()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        steps = self.cache.hits - h0 + self.cache.misses - m0
        pick = lambda *keys: sum(1 for n in names if any(k in n.lower() for k in keys))
        return dict(device_launches_per_step=len(names) / steps, steps=steps, captured=self.cache.misses - m0,
                    argmax_per_step=pick("argmax") / steps, pass_stats_per_step=pick("pass_stats_kernel") / steps,
                    copies_per_step=pick("memcpy", "copy") / steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--config", default="cfg2")
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pass_metrics: needs an MI355X (no timing is taken on a CPU)")
    modes = [m for m in a.modes.split(",") if m]
    if "on" in modes and not hasattr(train, "PassStats"):
        raise SystemExit("bench_pass_metrics: this tree has no train.PassStats; run with --modes off")
    dev = torch.device("cuda", torch.cuda.current_device())
    cfg = dict(synthetic.CONFIGS[a.config])
    legs = {m: Leg(m == "on", cfg, a.batches, a.dropout, dev) for m in modes}
    sets = [make(cfg, 9000 + 100 * w, a.batches) for w in range(3)]      # the three unseen sets of bench.streamed_leg
    for m in modes:                                                      # one untimed pass per set: buckets still missing are captured
        for s in sets:
            legs[m].timed(s)
    rounds = []
    for r in range(a.rounds):
        rounds.append({m: legs[m].timed(sets[r % len(sets)]) for m in modes})
    res = dict(tool="bench_pass_metrics", config=a.config, batches=a.batches, rounds=rounds)
    for m in modes:
        t = sorted(x[m]["ms_per_step"] for x in rounds)
        res[m] = dict(ms_per_step_median=t[len(t) // 2] if len(t) % 2 else 0.5 * (t[len(t) // 2 - 1] + t[len(t) // 2]),
                      ms_per_step_min=t[0], ms_per_step_max=t[-1], spread_ms=t[-1] - t[0],
                      trace=legs[m].launches(sets[0]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
