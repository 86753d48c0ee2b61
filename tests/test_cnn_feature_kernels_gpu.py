"""GPU: the K18 kernels (csrc/cnn_features.hip) through ``cnn_features.cnn_pool`` against the float64 reference of
tests/cnn_features_ref.py: argmax EQUAL, every pooled value and every gradient element (conv weights, biases, embedding table)
within its derived bound  (n + 16) u S + 2^-126  (see that file).  Every input is decidable everywhere (asserted on the CPU when
the case is generated: no rounding can change which window wins), so no element is excluded here.

Shapes take their edges from the library: TW = mmdfn_cnn_tile_words(), RG = mmdfn_cnn_rows_per_group().  The words sweep
{max K, max K + 1, TW - 1, TW, TW + 1, 2 TW + max K - 1} (one window of the largest size, then the halo on both sides of a tile
edge) runs for rows in {1, RG, RG + 1} at the reference's defaults (D 100, F 50, sizes 3-4-5); the D x F x sizes grid
{4, 100, 300} x {1, 50, 64} x {(3, 4, 5), (1,), (2, 8)} runs at rows = RG + 1, W = TW + 1."""
import numpy as np
import pytest
import torch

import cnn_features_ref as R
from mm_dfn_amd import cnn_features as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
W_LABELS = ("maxk", "maxk+1", "tw-1", "tw", "tw+1", "2tw+maxk-1")
ROW_LABELS = ("1", "rg", "rg+1")


def words(label, ks):
    tw, mk = C.tile_words(), max(ks)
    return {"maxk": mk, "maxk+1": mk + 1, "tw-1": max(tw - 1, mk), "tw": max(tw, mk), "tw+1": tw + 1,
            "2tw+maxk-1": 2 * tw + mk - 1}[label]


def nrows(label):
    rg = C.rows_per_group()
    return {"1": 1, "rg": rg, "rg+1": rg + 1}[label]


def run(case, frozen=False):
    """(pooled, argmax, dW list, db list, dEmb or None) of the kernels on ``case``, as numpy arrays."""
    tok = torch.from_numpy(case.tokens).to(DEV)
    table = torch.from_numpy(case.table).to(DEV).requires_grad_(not frozen)
    ws = [torch.from_numpy(w).to(DEV).requires_grad_(True) for w in case.weights]
    bs = [torch.from_numpy(b).to(DEV).requires_grad_(True) for b in case.biases]
    pooled, argmax, _ = C.cnn_pool(tok, table, ws, bs, torch.from_numpy(case.mask).to(DEV))
    pooled.backward(torch.from_numpy(case.d_pooled).to(DEV))
    torch.cuda.synchronize()
    return (pooled.detach().cpu().numpy(), argmax.cpu().numpy(), [w.grad.cpu().numpy() for w in ws],
            [b.grad.cpu().numpy() for b in bs], None if frozen else table.grad.cpu().numpy())


def reference(case):
    fwd = R.forward(case.tokens, case.table, case.weights, case.biases, case.mask)
    return fwd, R.backward(case.tokens, case.table, case.weights, fwd.argmax, case.d_pooled)


def compare(case, got=None, fwd_bound=None):
    got = run(case) if got is None else got
    fwd, bwd = reference(case)
    pooled, argmax, dws, dbs, dtable = got
    assert (argmax == fwd.argmax).all(), (case.name, np.argwhere(argmax != fwd.argmax)[:5])
    R.check(case.name + " pooled", pooled, fwd.pooled, fwd.bound if fwd_bound is None else fwd_bound)
    for i in range(len(dws)):
        R.check(case.name + " dW%d" % i, dws[i], bwd.d_weights[i], bwd.bw[i])
        R.check(case.name + " db%d" % i, dbs[i], bwd.d_biases[i], bwd.bb[i])
    if dtable is not None:
        R.check(case.name + " dEmb", dtable, bwd.d_table, bwd.bt)
    return got, fwd, bwd


@pytest.mark.parametrize("rows", ROW_LABELS)
@pytest.mark.parametrize("wl", W_LABELS)
def test_words_at_tile_edges(wl, rows):
    ks = (3, 4, 5)
    compare(R.random_case(nrows(rows), words(wl, ks), 100, 50, ks))


@pytest.mark.parametrize("ks", [(3, 4, 5), (1,), (2, 8)])
@pytest.mark.parametrize("F", [1, 50, 64])
@pytest.mark.parametrize("D", [4, 100, 300])
def test_widths_filters_and_sizes(D, F, ks):
    compare(R.random_case(nrows("rg+1"), words("tw+1", ks), D, F, ks))


@pytest.mark.parametrize("first", [0, 256])
def test_one_product_per_window_every_channel_and_tap(first):
    """Dense table, ONE non-zero tap per filter: filter j of size i holds pair number first + 64 i + j of the (c, k) sweep over
    D = 40 channels (a full and a partial 32-chunk) x 8 taps, so every window value is one product (n = 1, bias 0) and a
    missing piece product or a misplaced fragment element is tens of bounds away."""
    case = R.onehot_weights_case(40, 8, 64, 4, first)
    compare(case, fwd_bound=R.onehot_forward_bound(case))


@pytest.mark.parametrize("first", [512, 1280, 2144])
def test_one_product_per_window_at_the_widest_table(first):
    """The same family at D = 300 (ten channel chunks, the last one partial: channels 288 .. 299): 256 (c, k) pairs per launch
    from pair ``first`` on -- channels 64 .. 95, 160 .. 191 and 268 .. 299, every tap of each."""
    case = R.onehot_weights_case(300, 8, 64, 4, first)
    compare(case, fwd_bound=R.onehot_forward_bound(case))


@pytest.mark.parametrize("D", [100, 300])
def test_row_slices_of_the_weight_gradient_longer_than_one_batch(D):
    """40 rows: every row slice of the weight-gradient workgroup (8 slices at D = 100, 3 at D = 300) holds 5 / 14 rows, so its
    four-row batches take a second trip and the last batch ends inside a batch."""
    compare(R.random_case(40, 9, D, 4, (2, 3)))


@pytest.mark.parametrize("c, k", [(c, k) for c in (0, 7, 8, 31, 32, 39) for k in (0, 7)])
def test_one_table_column_and_one_tap(c, k):
    case = R.onehot_case(20, 40, 5, (2, 8), c, k, V=32)
    compare(case, fwd_bound=R.onehot_forward_bound(case))


@pytest.mark.parametrize("where", ["first", "last", "tile_end"])
def test_maximum_at_the_ends_and_at_a_tile_edge(where):
    ks = (3, 4, 5)
    tw = C.tile_words()
    W = 2 * tw + 3
    t = {"first": 0, "last": W - ks[0], "tile_end": tw - 1}[where]
    case = R.planted_case(W, 8, 4, ks, lambda K: t)
    got, fwd, _ = compare(case)
    assert (got[1][:, 0] == t).all() and (fwd.argmax[:, 0] == t).all()


def test_two_identical_windows_report_the_lowest():
    ks = (3, 4, 5)
    tw = C.tile_words()
    case = R.planted_case(2 * tw + 3, 8, 4, ks, lambda K: 5, again=lambda K: tw + 9)
    got, fwd, _ = compare(case)
    assert (got[1][:, 0] == 5).all()


def test_a_filter_without_a_positive_window():
    case = R.random_case(2, 11, 8, 3, (2, 3), negative_filter=1)
    got, fwd, _ = compare(case)
    pooled, argmax, dws, dbs, _ = got
    for i in range(2):
        assert (pooled[:, 3 * i + 1] == 0).all() and (argmax[:, 3 * i + 1] == -1).all()
        assert (dws[i][1] == 0).all() and (dbs[i][1] == 0).all()


def test_a_masked_row_between_two_live_rows():
    case = R.random_case(3, 40, 100, 50, (3, 4, 5), mask=[1, 0, 1])
    got, fwd, _ = compare(case)
    assert (got[0][1] == 0).all() and (got[1][1] == -1).all() and (got[0][[0, 2]] > 0).any()


def test_repeated_tokens_in_a_window_and_across_rows():
    case = R.random_case(4, 9, 12, 5, (2, 3), V=3)
    assert any((np.diff(case.tokens[r]) == 0).any() for r in range(4))
    compare(case)


def device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        try:
            fn()
        finally:
            torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


def test_a_frozen_table_launches_nothing_of_the_table_family():
    case = R.random_case(2, 12, 8, 4, (3, 4, 5))
    run(case)                                                # (warm up: library load, attribute calls)
    got = {}
    names = device_kernels(lambda: got.update(out=run(case, frozen=True)))
    assert any("cnn_pool_fwd" in n for n in names) and any("cnn_wgrad" in n for n in names), names
    assert not any("cnn_table" in n or "sort" in n.lower() for n in names), names
    assert got["out"][4] is None
    compare(case, got["out"])
    names = device_kernels(lambda: run(case))
    assert any("cnn_table_keys" in n for n in names) and any("cnn_table_bwd" in n for n in names), names


def test_three_runs_give_the_same_bits():
    case = R.random_case(5, 70, 100, 50, (3, 4, 5), V=11)
    runs = [run(case) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0][:2] + tuple(runs[0][2]) + tuple(runs[0][3]) + (runs[0][4],),
                        other[:2] + tuple(other[2]) + tuple(other[3]) + (other[4],)):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("bad", ["V", "-1"])
def test_an_id_outside_the_vocabulary_raises_before_any_launch(bad):
    case = R.random_case(2, 12, 8, 4, (3, 4, 5))
    run(case)
    tokens = case.tokens.copy()
    tokens[1, 7] = case.table.shape[0] if bad == "V" else -1
    broken = case._replace(tokens=tokens)

    def attempt():
        with pytest.raises(ValueError):
            run(broken)
    names = device_kernels(attempt)
    assert not any("cnn_" in n for n in names), names
