"""K13 (csrc/pass_stats.hip) through the C entry point and through train.PassStats, compared EXACTLY with a NumPy restatement:
predictions (ties, NaN rows), the confusion matrix, the row / batch / bad-label / NaN-row counts, the float64 loss sum and the
loss history, at the launch's edges (one row .. more than two sweeps of the workgroup, 1 .. max_classes classes)."""
import numpy as np
import pytest
import torch

from mm_dfn_amd import _hip, ops
from mm_dfn_amd import train as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
IGNORE = -100
ARMED, ROWS, BATCHES, BAD, NANS = 0, 1, 2, 3, 4


def threads():
    return ops.pass_stats_threads()


class Block:
    """The accumulator of the C entry point as four device tensors."""

    def __init__(self, C, slots, armed=1):
        self.C, self.slots = C, slots
        self.counts = torch.zeros(C * C, dtype=torch.int64, device=DEV)
        self.meta = torch.zeros(8, dtype=torch.int64, device=DEV)
        self.meta[ARMED] = armed
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=DEV)
        self.loss_hist = torch.zeros(slots, dtype=torch.float32, device=DEV) if slots else None

    def arm(self, flag):
        self.meta[ARMED] = int(flag)

    def launch(self, logp, target, loss, ignore=IGNORE, query=False, override=()):
        N, C = logp.shape
        pred = torch.full((N,), -7, dtype=torch.int64, device=DEV)
        a = dict(logp=logp, target=target, loss=loss, pred=pred, counts=self.counts, meta=self.meta, loss_sum=self.loss_sum,
                 loss_hist=self.loss_hist, N=N, C=C, slots=self.slots)
        a.update(override)               # (the refusal cases: one argument replaced)
        args = [_hip.ptr(a[k]) for k in ("logp", "target", "loss", "pred", "counts", "meta", "loss_sum", "loss_hist")]
        args += [a["N"], a["C"], ignore, a["slots"], _hip.stream()]
        if query:
            return _hip.query("mmdfn_pass_stats_accumulate", *args), pred
        _hip.call("mmdfn_pass_stats_accumulate", *args)
        return pred

    def host(self):
        torch.cuda.synchronize()
        return dict(counts=self.counts.cpu().numpy().reshape(self.C, self.C), meta=self.meta.cpu().numpy(),
                    loss_sum=self.loss_sum.cpu().numpy().copy(),
                    loss_hist=np.zeros(0, np.float32) if self.loss_hist is None else self.loss_hist.cpu().numpy())

    def bytes(self):
        h = self.host()
        return b"".join(h[k].tobytes() for k in ("counts", "meta", "loss_sum", "loss_hist"))


def np_pred(logp):
    nan = np.isnan(logp)
    pred = np.where(nan, -np.inf, logp).argmax(1)                      # numpy: the first of equal maxima
    return np.where(nan.any(1), nan.argmax(1), pred).astype(np.int64), nan.any(1)


class Ref:
    """The launch's rules in NumPy on a host copy of the same block."""

    def __init__(self, C, slots, armed=1):
        self.C, self.slots = C, slots
        self.counts = np.zeros((C, C), dtype=np.int64)
        self.meta = np.zeros(8, dtype=np.int64)
        self.meta[ARMED] = armed
        self.loss_sum = np.zeros(1, dtype=np.float64)
        self.loss_hist = np.zeros(slots, dtype=np.float32)

    def launch(self, logp, target, loss, ignore=IGNORE):
        C = self.C
        pred, has_nan = np_pred(logp)
        if not self.meta[ARMED]:
            return pred
        live = target != ignore
        good = live & (target >= 0) & (target < C)
        np.add.at(self.counts, (target[good], pred[good]), 1)
        self.meta[ROWS] += good.sum()
        self.meta[BAD] += (live & ~good).sum()
        self.meta[NANS] += (live & has_nan).sum()
        k = int(self.meta[BATCHES])
        if loss is not None:
            self.loss_sum[0] += np.float64(np.float32(loss))
            if k < self.slots:
                self.loss_hist[k] = np.float32(loss)
        self.meta[BATCHES] = k + 1
        return pred

    def check(self, blk):
        h = blk.host()
        assert np.array_equal(h["counts"], self.counts)
        assert np.array_equal(h["meta"], self.meta), (h["meta"], self.meta)
        assert h["loss_sum"].tobytes() == self.loss_sum.tobytes()
        assert h["loss_hist"].tobytes() == self.loss_hist.tobytes()


def make_inputs(N, C, seed, ignore_every=0, all_ignored=False):
    """Log-probabilities on a coarse grid (many exact ties), row 0 all equal, one NaN row, labels -1 and C, ignored rows."""
    rs = np.random.RandomState(seed)
    logp = (rs.randint(-6, 3, size=(N, C)) * 0.25).astype(np.float32)
    logp[0, :] = -1.5
    target = rs.randint(0, C, size=N).astype(np.int64)
    if N > 4:
        logp[N // 2, C // 2:] = np.nan                                 # one NaN row: predicts C // 2
        target[1] = -1
        target[N - 2] = C
    if ignore_every:
        target[::ignore_every] = IGNORE
    if all_ignored:
        target[:] = IGNORE
    return logp, target


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def both(blk, ref, logp, target, loss, **kw):
    got = blk.launch(dev(logp), dev(target), None if loss is None else torch.tensor([loss], dtype=torch.float32, device=DEV), **kw)
    want = ref.launch(logp, target, loss, **kw)
    assert np.array_equal(got.cpu().numpy(), want)
    return got


def _sizes():
    Tn, mc = 1024, 64          # checked against the library in test_constants_of_the_launch
    return [(n, c) for n in (1, 63, 64, 65, Tn - 1, Tn, Tn + 1, 2 * Tn + 1) for c in (1, 2, 7, mc)]


def test_constants_of_the_launch():
    assert threads() == 1024 and ops.pass_stats_max_classes() == 64 and ops.pass_stats_max_classes() >= 16


@pytest.mark.parametrize("N,C", _sizes())
def test_one_launch_at_the_edges(N, C):
    logp, target = make_inputs(N, C, seed=N * 131 + C, ignore_every=3)
    blk, ref = Block(C, 2), Ref(C, 2)
    both(blk, ref, logp, target, 0.625)
    ref.check(blk)
    if N > 4:
        assert ref.meta[NANS] == (1 if target[N // 2] != IGNORE else 0) and ref.meta[BAD] >= 1
    # ... and through the host-side object: the same numbers from its one copy
    st = T.PassStats(C, DEV, loss_slots=2, ignore_index=IGNORE)
    pred = st.update(dev(logp), dev(target), torch.tensor(0.625, device=DEV))
    assert np.array_equal(pred.cpu().numpy(), np_pred(logp)[0])
    st.fetch()
    assert np.array_equal(st.confusion(), ref.counts)
    assert (st.rows, st.batches, st.bad_labels, st.nan_rows) == tuple(int(ref.meta[w]) for w in (ROWS, BATCHES, BAD, NANS))
    assert st.loss_sum() == 0.625 and np.array_equal(st.batch_losses(), np.array([0.625], np.float32))


def test_ties_give_the_lowest_index_and_match_torch_argmax():
    N, C = 300, 7
    logp, target = make_inputs(N, C, seed=5)
    logp = np.nan_to_num(logp, nan=-0.25)
    blk = Block(C, 0)
    pred = blk.launch(dev(logp), dev(target), None)
    assert torch.equal(pred.cpu(), torch.argmax(torch.from_numpy(logp), 1)) and int(pred[0]) == 0
    x = torch.from_numpy(logp).clone()
    x[7, 4] = x[7, 2] = float("nan")
    pred = blk.launch(x.to(DEV), dev(target), None)
    assert int(pred[7]) == 2 and torch.equal(pred.cpu(), torch.argmax(x, 1))      # torch's rule on the CPU: the first NaN


def test_every_row_ignored_and_loss_null():
    C = 7
    logp, target = make_inputs(70, C, seed=2, all_ignored=True)
    blk, ref = Block(C, 3), Ref(C, 3)
    both(blk, ref, logp, target, 1.25)
    ref.check(blk)
    assert not ref.counts.any() and ref.meta[ROWS] == 0 and ref.meta[BATCHES] == 1 and ref.meta[NANS] == 0
    logp, target = make_inputs(70, C, seed=3, ignore_every=2)
    both(blk, ref, logp, target, None)                                 # loss = NULL: the batch counts, no loss update
    ref.check(blk)
    assert ref.meta[BATCHES] == 2 and ref.loss_sum[0] == 1.25 and ref.loss_hist[1] == 0


def test_four_launches_three_slots_and_a_disarmed_launch_between():
    C, Tn = 7, threads()
    blk, ref = Block(C, 3), Ref(C, 3)
    losses = [0.1, 1e-3, 7.3333, 2.718281828]                          # float32(loss) summed in float64, in launch order
    sizes = [Tn + 1, 65, 2 * Tn + 1, 9]
    for j, (n, l) in enumerate(zip(sizes, losses)):
        logp, target = make_inputs(n, C, seed=40 + j, ignore_every=5)
        both(blk, ref, logp, target, l)
        if j == 1:                                                     # a disarmed launch: pred is written, nothing else moves
            blk.arm(False)
            before = blk.bytes()
            logp2, target2 = make_inputs(130, C, seed=77)
            pred = blk.launch(dev(logp2), dev(target2), torch.tensor([9.0], device=DEV))
            assert np.array_equal(pred.cpu().numpy(), np_pred(logp2)[0])
            assert blk.bytes() == before
            blk.arm(True)
    ref.check(blk)
    want = np.float64(0)
    for l in losses:
        want += np.float64(np.float32(l))
    h = blk.host()
    assert h["loss_sum"][0] == want and h["meta"][BATCHES] == 4
    assert np.array_equal(h["loss_hist"], np.array(losses[:3], dtype=np.float32))      # the fourth is summed, not stored


def test_two_runs_give_identical_bytes():
    C = 64
    runs = []
    for _ in range(2):
        blk = Block(C, 4)
        preds = []
        for j, n in enumerate((2 * threads() + 1, 777, 64)):
            logp, target = make_inputs(n, C, seed=90 + j, ignore_every=4)
            preds.append(blk.launch(dev(logp), dev(target), torch.tensor([0.3 * (j + 1)], device=DEV)).cpu().numpy().tobytes())
        runs.append((blk.bytes(), preds))
    assert runs[0] == runs[1]


def test_refusals_return_minus_one_and_touch_nothing():
    C = 7
    logp, target = make_inputs(20, C, seed=1)
    logp, target = dev(logp), dev(target)
    loss = torch.tensor([1.0], device=DEV)
    blk = Block(C, 2)
    blk.launch(logp, target, loss)                                     # something in the block to keep
    before = blk.bytes()
    big = ops.pass_stats_max_classes() + 1
    cases = [dict(N=0), dict(N=-3), dict(C=0), dict(C=-1), dict(C=big), dict(slots=-1), dict(logp=None), dict(target=None),
             dict(pred=None), dict(counts=None), dict(meta=None), dict(loss_sum=None), dict(loss_hist=None)]
    for over in cases:
        rc, pred = blk.launch(logp, target, loss, query=True, override=over)
        assert rc == -1, over
        assert bool((pred == -7).all()), over                          # nothing was launched
        assert blk.bytes() == before, over
    rc, _ = blk.launch(logp, target, loss, query=True, override=dict(loss_hist=None, slots=0))      # no history wanted: a null one is fine
    assert rc == 0
    with pytest.raises(_hip.HipLibraryError):
        blk.launch(logp, target, loss, override=dict(N=0))


def test_pass_stats_object_accumulates_and_resets():
    C = 6
    st = T.PassStats(C, DEV, loss_slots=3)
    ref = Ref(C, 3)
    for j, n in enumerate((40, 1025, 7)):
        logp, target = make_inputs(n, C, seed=60 + j, ignore_every=4)
        if j == 1:
            st.set_enabled(False)
            st.update(dev(logp), dev(target), torch.tensor(5.0, device=DEV))       # counts nothing
            st.set_enabled(True)
        pred = st.update(dev(logp), dev(target), torch.tensor(0.5 + j, device=DEV))
        assert np.array_equal(pred.cpu().numpy(), ref.launch(logp, target, 0.5 + j))
    st.fetch()
    assert np.array_equal(st.confusion(), ref.counts) and st.batches == 3 and st.rows == int(ref.meta[ROWS])
    assert st.loss_sum() == ref.loss_sum[0] and np.array_equal(st.batch_losses(), ref.loss_hist)
    labels, preds = st.as_arrays()
    assert abs(st.accuracy() - (labels == preds).mean()) <= 1e-12
    ptr = st._block.data_ptr()
    st.reset()
    st.fetch()
    assert st._block.data_ptr() == ptr and st.rows == 0 and st.batches == 0 and not st.confusion().any() and st.enabled
    with pytest.raises(ValueError):
        T.PassStats(ops.pass_stats_max_classes() + 1, DEV)
