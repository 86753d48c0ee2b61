"""CPU, world_size 2 over gloo: two ranks count their shards of a fixed label / log-probability set with train.PassStats and
all_reduce(); both then hold the statistics of a single process on the whole set -- integer counts exactly, the loss sum to
its summation order."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

from mm_dfn_amd import distributed
from mm_dfn_amd import train as T

C = 6


def make_batches():
    rs = np.random.RandomState(4)
    out = []
    for n in (9, 4, 7, 12, 5, 11, 3):
        logp = torch.log_softmax(torch.from_numpy(rs.randn(n, C).astype(np.float32)), 1)
        target = torch.from_numpy(rs.randint(0, C, size=n))
        target[0] = -100                                   # an ignored row per batch
        loss = torch.tensor(np.float32(rs.rand() * 3 + 0.01))
        out.append((logp, target, loss))
    out[2][1][1] = C                                       # one bad label
    return out


def count(batches):
    st = T.PassStats(C, "cpu", loss_slots=4)
    for logp, target, loss in batches:
        st.update(logp, target, loss)
    return st


def worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    distributed.init(backend="gloo")
    mine = make_batches()[rank::world]                     # 4 and 3 batches
    st = count(mine)
    st.all_reduce()
    st.fetch()
    torch.save(dict(cm=st.confusion(), rows=st.rows, batches=st.batches, bad=st.bad_labels, nans=st.nan_rows,
                    loss_mean=st.loss_mean(), acc=st.accuracy(), f1=st.weighted_f1(), hist=st.batch_losses(),
                    local=[float(b[2]) for b in mine], armed=st.enabled), out + ".%d" % rank)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_hold_the_single_process_statistics(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "stats.pt")
    mp.spawn(worker, args=(2, port, out), nprocs=2, join=True)
    got = [torch.load(out + ".%d" % r, weights_only=False) for r in range(2)]
    batches = make_batches()
    one = count(batches).fetch()
    losses = np.array([float(b[2]) for b in batches], dtype=np.float64)
    bound = len(batches) * 2.0 ** -52 * np.abs(losses).sum()
    assert one.batches == len(batches) == 7 and one.bad_labels == 1 and one.rows == sum(b[0].shape[0] for b in batches) - 7 - 1
    for r, g in enumerate(got):
        assert np.array_equal(g["cm"], one.confusion())
        assert (g["rows"], g["batches"], g["bad"], g["nans"]) == (one.rows, one.batches, one.bad_labels, one.nan_rows)
        assert g["acc"] == one.accuracy() and g["f1"] == one.weighted_f1()
        assert abs(g["loss_mean"] - losses.sum() / one.batches) <= bound
        # the loss history stays the rank's own (its first 4 of 4 / all of 3 batches), the armed word is not summed
        assert len(g["local"]) == (4, 3)[r]
        assert g["armed"] is True and np.array_equal(g["hist"], np.array(g["local"][:4], dtype=np.float32))
    assert got[0]["acc"] == got[1]["acc"] and got[0]["f1"] == got[1]["f1"] and got[0]["loss_mean"] == got[1]["loss_mean"]
