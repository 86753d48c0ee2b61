"""GPU: train_or_eval_graph_model / fit with device_metrics=True (train.PassStats counted by a node of the replayed step)
against the default book-keeping on the same seed and weights -- eager, exact-signature cache, bucketed cache, bucketed cache
with an in-graph FlatAdam -- and what the statistics launch replaces in a replayed pass (no argmax, no per-step clones)."""
import numpy as np
import pytest
import torch

from mm_dfn_amd import FocalLoss, synthetic
from mm_dfn_amd import data as D
from mm_dfn_amd import train as T
from mm_dfn_amd.optim import FlatAdam

pytestmark = pytest.mark.gpu
CFG = dict(P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)        # the pass-loop model of test_trainer_gpu
NAMES = ['hap', 'sad', 'neu', 'ang', 'exc', 'fru']
LOSS = FocalLoss(gamma=0.5)


def _model(seed=21, dropout=0.1):
    m = synthetic.build_model(dropout=dropout, **CFG)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), seed))
    return m.cuda()


@pytest.fixture(scope="module")
def pickle_path(tmp_path_factory):
    return D.write_synthetic_pickle(str(tmp_path_factory.mktemp("pm") / "f.pkl"))


@pytest.fixture(scope="module", autouse=True)
def dropout_pool_hints(pickle_path):
    """The dropout flag pool (ops_flags) sizes its pooled draw from what the previous step of the same shape used: the FIRST
    eager step of a shape in a process draws per request, every later one takes slices of one pooled draw -- other masks from
    the same seed (measured on the default path: 18.9 % accuracy for a process's first run of the training pass below,
    16.61 % for each later run).  The pairs below compare two runs of one pass, so a throwaway run of each pass goes first."""
    m = _model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    tr, _, te = D.get_IEMOCAP_loaders(pickle_path, batch_size=4, valid_rate=0.0)
    T.train_or_eval_graph_model(m, LOSS, D.DevicePrefetcher(tr), 0, True, opt)
    T.train_or_eval_graph_model(m, LOSS, D.DevicePrefetcher(te), 0, False)


def _loaders(path):
    tr, _, te = D.get_IEMOCAP_loaders(path, batch_size=4, valid_rate=0.0)
    return tr, te


def _utterances(loader):
    return int(sum(int(b[4].sum()) for b in loader))


def _setup(config, on):
    m = _model()
    stats = T.PassStats(CFG["C"], "cuda", ignore_index=T.StepGraphCache.IGNORE) if on and config != "eager" else None
    if config == "bucketed+adam":
        opt = FlatAdam(m, lr=1e-3, weight_decay=1e-5, capturable=True)
    else:
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    cache = None
    if config == "exact":
        cache = T.StepGraphCache(m, LOSS, pass_stats=stats)
    elif config == "bucketed":
        cache = T.StepGraphCache(m, LOSS, bucket_rows=8, pass_stats=stats)
    elif config == "bucketed+adam":
        cache = T.StepGraphCache(m, LOSS, bucket_rows=8, optimizer=opt, pass_stats=stats)
    return m, opt, cache, stats


def check_pair(off, on, n_utts, n_batches):
    """One pass with the default book-keeping (off) and with device_metrics (on)."""
    assert on[3] == off[3] and on[6] == off[6] and on[1] == off[1] and on[0] == off[0]
    assert on[4].shape == on[5].shape == (n_utts,)
    for k in (4, 5):
        assert np.array_equal(np.bincount(on[k], minlength=CFG["C"]), np.bincount(off[k], minlength=CFG["C"]))
    l_off, l_on = off[7][1], on[7][1]
    assert l_on.dtype == np.float32 and l_off.shape == l_on.shape == (n_batches,) and l_off.tobytes() == l_on.tobytes()
    # avg_loss: float64 sum on the device against the float32 np.sum of the default path
    mean32, mean64 = float(np.sum(l_off)) / n_batches, float(np.sum(l_on.astype(np.float64))) / n_batches
    print("avg_loss off %r on %r | float32 mean %r float64 mean %r" % (off[2], on[2], mean32, mean64))
    assert abs(mean32 - mean64) <= n_batches * 2.0 ** -24 * float(np.abs(l_on.astype(np.float64)).sum())
    assert abs(on[2] - round(mean64, 4)) <= 1e-12
    assert abs(on[2] - off[2]) <= 1e-4 + 1e-9                     # one unit in the last place after round(.., 4)


@pytest.mark.parametrize("config", ["eager", "exact", "bucketed", "bucketed+adam"])
def test_pass_metrics_equal_the_default_path(config, pickle_path):
    """Two training passes (the first one captures every key in the middle of the pass) and an eval pass, off and on."""
    runs = []
    for on in (False, True):
        m, opt, cache, stats = _setup(config, on)
        tr, te = _loaders(pickle_path)
        out = []
        for e, (loader, train_flag) in enumerate(((tr, True), (tr, True), (te, False))):
            r = T.train_or_eval_graph_model(m, LOSS, D.DevicePrefetcher(loader), e, train_flag, opt if train_flag else None, False,
                                            'avl', NAMES, graph_cache=cache, device_metrics=on)
            out.append(r)
            if stats is not None:
                # every batch counted exactly once, captured mid-pass or replayed
                assert stats.rows == _utterances(loader) and stats.batches == len(loader)
                assert stats.bad_labels == 0 and stats.nan_rows == 0
                assert all(ent["pending"] is None for ent in cache.entries.values())
        runs.append((m, out, cache))
    (m0, out0, _), (m1, out1, cache) = runs
    tr, te = _loaders(pickle_path)
    for (a, b), loader in zip(zip(out0, out1), (tr, tr, te)):
        check_pair(a, b, _utterances(loader), len(loader))
    # the statistics launch draws no random numbers (dropout 0.1): the same trajectory, bit for bit
    for (k, x), (_, y) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(x, y), k
    if cache is not None:
        assert cache.hits >= 1


def test_precapture_counts_nothing_and_the_pass_after_it_counts_every_batch(pickle_path):
    m = _model().train()
    stats = T.PassStats(CFG["C"], "cuda")
    cache = T.StepGraphCache(m, LOSS, bucket_rows=8, pass_stats=stats)
    tr, _ = _loaders(pickle_path)
    T.seed_everything(2021)
    made = cache.precapture(D.DevicePrefetcher(tr), train_flag=True)
    assert made >= 1 and stats.enabled
    stats.fetch()
    assert stats.rows == 0 and stats.batches == 0 and not stats.confusion().any() and stats.loss_sum() == 0.0
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    misses = cache.misses
    T.train_or_eval_graph_model(m, LOSS, D.DevicePrefetcher(tr), 0, True, opt, False, 'avl', NAMES, graph_cache=cache,
                                device_metrics=True)
    assert cache.misses == misses
    assert stats.rows == _utterances(tr) and stats.batches == len(tr)


def _device_events(run):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        out = run()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_replayed_pass_has_no_argmax_and_no_per_step_clones():
    """Five batches of one bucket: after the first pass every step replays the same entry.  The default path then clones the
    entry's predictions, labels and loss before each reuse (three launches) and runs an argmax per step; with device_metrics
    neither exists.  Launch COUNTS from a profiler trace, not times."""
    cfg = dict(B=3, L=23, **CFG)
    tuples = [[23, 9, 17], [23, 17, 9], [19, 23, 7], [23, 5, 21], [8, 18, 23]]          # 49 utterances each: one bucket of 56
    loader = []
    for i, lengths in enumerate(tuples):
        b = synthetic.make_batch(60 + i, lengths=lengths, device="cuda", **cfg)
        loader.append((b["textf"], b["visuf"], b["acouf"], b["qmask"], b["umask"], b["label"], ["d%d" % i]))
    m = _model(dropout=0.0)
    traces, results = {}, {}
    for on in (False, True):
        stats = T.PassStats(CFG["C"], "cuda") if on else None
        cache = T.StepGraphCache(m, LOSS, bucket_rows=8, pass_stats=stats)
        run = lambda: T.train_or_eval_graph_model(m, LOSS, loader, 0, False, None, False, 'avl', NAMES, graph_cache=cache,
                                                  device_metrics=on)
        run()                                                # captures the one entry
        assert len(cache.entries) == 1 and cache.misses == 1
        seen = []
        if on:
            ent = next(iter(cache.entries.values()))
            real_step = cache.step

            def step(*a, **k):
                out = real_step(*a, **k)
                seen.append(ent["pending"])
                return out
            cache.step = step
        results[on], traces[on] = _device_events(run)
        assert cache.misses == 1 and cache.hits == 4 + 5
        if on:
            assert seen == [None] * 5                        # no pending closure is ever registered
            assert torch.equal(cache.last_pred, torch.argmax(next(iter(cache.entries.values()))["out"]["log_prob"][:49], 1))
    reuses = len(tuples) - 1
    is_argmax = lambda name: "argmax" in name.lower()
    print("device launches per pass: default %d, device_metrics %d" % (len(traces[False]), len(traces[True])))
    assert sum(map(is_argmax, traces[False])) == len(tuples)
    assert not any(map(is_argmax, traces[True]))
    assert sum("pass_stats_kernel" in n for n in traces[True]) == len(tuples)
    assert len(traces[False]) - len(traces[True]) >= 3 * reuses
    check_pair(results[False], results[True], 49 * len(tuples), len(tuples))


def test_fit_history_with_device_metrics(pickle_path):
    hists = []
    for on in (False, True):
        m = _model()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
        tr, va, te = D.get_IEMOCAP_loaders(pickle_path, batch_size=4, valid_rate=0.2)
        wrap = D.DevicePrefetcher
        out = T.fit(m, LOSS, opt, wrap(tr), wrap(va), wrap(te), n_epochs=2, patience=5, valid_rate=0.2, target_names=NAMES,
                    log=None, graph_cache=True, device_metrics=on)
        assert out["epochs_run"] == 2
        hists.append(out["history"])
    off, on = hists
    assert sorted(off) == sorted(on)
    for k in off:
        for a, b in zip(off[k], on[k]):
            if k.endswith("_loss"):
                assert abs(a - b) <= 1e-4 + 1e-9, k
            else:
                assert a == b, k
