"""train.PassStats on host tensors: the closed forms of the confusion matrix against scikit-learn, the torch restatement of the
device launch (csrc/pass_stats.hip) against a plain Python loop, and the argument checks of the pass loop.  No GPU."""
import numpy as np
import pytest
import torch
from sklearn.metrics import accuracy_score, confusion_matrix, f1_score

from mm_dfn_amd import ops, ops_stats
from mm_dfn_amd import train as T


def stats_of(cm):
    """A fetched PassStats that holds the matrix ``cm``."""
    cm = np.asarray(cm, dtype=np.int64)
    st = T.PassStats(cm.shape[0], "cpu")
    st._counts.copy_(torch.from_numpy(cm.ravel()))
    st._meta[ops_stats.ROWS] = int(cm.sum())
    return st.fetch()


def _matrices():
    rs = np.random.RandomState(3)
    a6, a7 = rs.randint(0, 40, size=(6, 6)), rs.randint(0, 9, size=(7, 7))
    no_row, no_col, neither = a6.copy(), a6.copy(), a7.copy()
    no_row[2, :] = 0                      # class 2 absent from the labels
    no_col[:, 4] = 0                      # class 4 never predicted
    neither[3, :] = 0
    neither[:, 3] = 0
    return {"random6": a6, "random7": a7, "zero_row": no_row, "zero_column": no_col, "zero_row_and_column": neither,
            "one_class": np.array([[17]])}


@pytest.mark.parametrize("name", sorted(_matrices()))
def test_closed_forms_equal_sklearn(name):
    cm = _matrices()[name]
    st = stats_of(cm)
    labels, preds = st.as_arrays()
    assert labels.shape == preds.shape == (int(cm.sum()),)
    C = cm.shape[0]
    assert np.array_equal(confusion_matrix(labels, preds, labels=list(range(C))), cm)      # as_arrays round-trips
    assert np.array_equal(st.confusion(), cm) and st.rows == int(cm.sum())
    acc, f1 = accuracy_score(labels, preds), f1_score(labels, preds, average='weighted')
    assert abs(st.accuracy() - acc) <= 1e-12 and abs(st.weighted_f1() - f1) <= 1e-12
    assert round(st.accuracy() * 100, 2) == round(acc * 100, 2)
    assert round(st.weighted_f1() * 100, 2) == round(f1 * 100, 2)
    per = st.per_class_accuracy()
    for c in range(C):
        sel = labels == c
        if sel.any():
            assert abs(per[c] - accuracy_score(labels[sel], preds[sel])) <= 1e-12
        else:
            assert np.isnan(per[c])


def test_empty_pass_gives_nan():
    st = T.PassStats(6, "cpu").fetch()
    assert st.rows == 0 and st.batches == 0 and st.bad_labels == 0 and st.nan_rows == 0
    assert np.isnan(st.accuracy()) and np.isnan(st.weighted_f1()) and np.isnan(st.loss_mean())
    assert st.batch_losses().shape == (0,) and st.as_arrays()[0].shape == (0,)
    assert np.isnan(st.per_class_accuracy()).all()
    with pytest.raises(RuntimeError):
        T.PassStats(6, "cpu").rows                      # nothing fetched yet


def loop_reference(calls, C, ignore, slots):
    """The launch's rules as a plain Python loop over the rows of every (logp, target, loss, armed) call."""
    cm = np.zeros((C, C), dtype=np.int64)
    rows = batches = bad = nans = 0
    loss_sum, hist, preds = 0.0, np.zeros(slots, dtype=np.float32), []
    for logp, target, loss, armed in calls:
        pred = []
        for i in range(logp.shape[0]):
            row = logp[i]
            nan_at = [c for c in range(C) if np.isnan(row[c])]
            if nan_at:
                p = nan_at[0]
            else:
                p = 0
                for c in range(1, C):
                    if row[c] > row[p]:
                        p = c
            pred.append(p)
            t = int(target[i])
            if not armed or t == ignore:
                continue
            nans += bool(nan_at)
            if 0 <= t < C:
                cm[t, p] += 1
                rows += 1
            else:
                bad += 1
        preds.append(np.array(pred, dtype=np.int64))
        if armed:
            if loss is not None:
                loss_sum += float(np.float32(loss))
                if batches < slots:
                    hist[batches] = np.float32(loss)          # (the slot of batch k; a batch without a loss leaves its slot 0)
            batches += 1
    return dict(cm=cm, rows=rows, batches=batches, bad=bad, nans=nans, loss_sum=loss_sum,
                hist=hist[:min(batches, slots)], preds=preds)


def make_calls(C=5, ignore=-100, seed=0):
    rs = np.random.RandomState(seed)
    calls = []
    for n, armed, with_loss in ((9, True, True), (6, False, True), (14, True, True), (4, True, False), (7, True, True)):
        logp = rs.randn(n, C).astype(np.float32)
        logp[0, :] = logp[0, 0]                          # every class ties: index 0
        if n > 2 and C > 2:
            logp[1, C - 1] = logp[1, 2] = logp[1].max() + 1.0      # two maxima: the lower index
        target = rs.randint(0, C, size=n).astype(np.int64)
        if n > 5:
            logp[3, 1:3] = np.nan                        # a NaN row predicts its first NaN
            logp[5, 0] = np.nan
            target[5] = ignore                           # ... an ignored one is counted nowhere
            target[2] = ignore
            target[4] = -1
            target[n - 1] = C
        calls.append((logp, target, np.float32(rs.rand() + 0.1) if with_loss else None, armed))
    return calls


def test_host_update_equals_a_python_loop():
    C, ignore, slots = 5, -100, 3
    calls = make_calls(C, ignore)
    want = loop_reference(calls, C, ignore, slots)
    st = T.PassStats(C, "cpu", loss_slots=slots, ignore_index=ignore)
    for (logp, target, loss, armed), wp in zip(calls, want["preds"]):
        st.set_enabled(armed)
        before = st._block.clone()
        pred = st.update(torch.from_numpy(logp), torch.from_numpy(target), None if loss is None else torch.tensor(loss))
        assert pred.dtype == torch.int64 and np.array_equal(pred.numpy(), wp)
        if not armed:
            assert torch.equal(st._block, before)        # a disarmed call writes its predictions and nothing else
    clean = torch.from_numpy(np.nan_to_num(calls[0][0], nan=0.0))
    assert torch.equal(ops.first_max(clean)[0], torch.argmax(clean, 1))
    st.fetch()
    assert np.array_equal(st.confusion(), want["cm"])
    assert (st.rows, st.batches, st.bad_labels, st.nan_rows) == (want["rows"], want["batches"], want["bad"], want["nans"])
    assert want["batches"] == 4 and want["bad"] > 0 and want["nans"] > 0
    assert st.loss_sum() == want["loss_sum"] and st.loss_mean() == want["loss_sum"] / 4
    assert st.batch_losses().dtype == np.float32 and np.array_equal(st.batch_losses(), want["hist"])
    assert len(want["hist"]) == 3 and want["hist"][2] == 0 and want["hist"][1] > 0      # 4 batches, 3 slots, the third without a loss
    st.reset()
    st.fetch()
    assert st.rows == 0 and st.batches == 0 and not st.confusion().any() and st.loss_sum() == 0.0 and st.enabled


def test_first_max_is_torch_argmax_on_host_rows():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(200, 7, generator=g).round(decimals=0)            # many exact ties
    assert torch.equal(ops.first_max(x)[0], torch.argmax(x, 1))
    x[5, 3] = float("nan")
    x[9, 6] = x[9, 2] = float("nan")
    x[11] = float("-inf")
    pred, has_nan = ops.first_max(x)
    assert torch.equal(pred, torch.argmax(x, 1)) and pred[5] == 3 and pred[9] == 2 and pred[11] == 0
    assert has_nan.nonzero().flatten().tolist() == [5, 9]


def test_argument_checks():
    with pytest.raises(ValueError):
        T.PassStats(0, "cpu")
    with pytest.raises(ValueError):
        T.PassStats(6, "cpu").update(torch.zeros(3, 5), torch.zeros(3, dtype=torch.int64))
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="ignore"):
        T.StepGraphCache(lin, None, pass_stats=T.PassStats(6, "cpu", ignore_index=-1))
    cache = T.StepGraphCache(lin, None)
    assert cache.pass_stats is None
    with pytest.raises(ValueError, match="pass_stats"):
        T.train_or_eval_graph_model(lin, None, [], graph_cache=cache, device_metrics=True)
    # the empty pass returns what it always did
    got = T.train_or_eval_graph_model(lin, None, [], device_metrics=True)
    assert got[0] == [] and np.isnan(got[2]) and np.isnan(got[3]) and np.isnan(got[6]) and got[7] == []


def test_eager_pass_on_host_tensors_reports_the_default_path_metrics():
    """A torch stand-in model on the CPU through the eager loop: device_metrics on and off give the same report."""
    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.randn(4, 6, generator=torch.Generator().manual_seed(0)))

        def forward(self, textf, qmask, umask, lengths, acouf, visuf, test_label=False):
            x = torch.cat([textf[:n, b] for b, n in enumerate(lengths)])
            return torch.log_softmax(x @ self.w, 1), None, None, None, None

    rs = np.random.RandomState(5)
    batches = []
    for lens in ([5, 3], [4, 4], [2, 6]):
        L, B = max(lens), len(lens)
        umask = torch.zeros(B, L)
        for b, n in enumerate(lens):
            umask[b, :n] = 1
        batches.append((torch.from_numpy(rs.randn(L, B, 4).astype(np.float32)), torch.zeros(1), torch.zeros(1), torch.zeros(1),
                        umask, torch.from_numpy(rs.randint(0, 6, size=(B, L)))))
    names = ['hap', 'sad', 'neu', 'ang', 'exc', 'fru']
    m, loss_f = Stub(), torch.nn.NLLLoss()
    want = T.train_or_eval_graph_model(m, loss_f, batches, target_names=names)
    got = T.train_or_eval_graph_model(m, loss_f, batches, target_names=names, device_metrics=True)
    assert got[0] == want[0] and got[1] == want[1] and got[3] == want[3] and got[6] == want[6]
    assert abs(got[2] - want[2]) <= 1.0001e-4
    assert np.array_equal(np.bincount(got[4], minlength=6), np.bincount(want[4], minlength=6))
    assert np.array_equal(np.bincount(got[5], minlength=6), np.bincount(want[5], minlength=6))
    assert np.array_equal(got[7][1], want[7][1])
