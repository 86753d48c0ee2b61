"""CPU: the oracle restatement against outputs of the REAL reference (tests/golden/oracle_vs_reference.npz, exported by
tests/golden/make_golden.py from the reference imported live; inputs and weights are regenerated from the same seeds)."""
import os

import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd import synthetic

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_reference.npz"))


@pytest.mark.parametrize("P,nl,lengths", [(2, 2, [18, 7, 11]), (9, 3, [12, 1, 5, 9])])
def test_forward_matches_reference(P, nl, lengths):
    cfg = dict(B=len(lengths), L=max(lengths), P=P, C=6, nlayers=nl, D_t=100, D_a=48, D_v=64)
    # the reference model's state_dict has the same keys and shapes (tests/test_host_logic.py): the same seeded weights
    sd = synthetic.seeded_state_dict(synthetic.build_model(**cfg).state_dict(), 7)
    b = synthetic.make_batch(8, lengths=lengths, **cfg)
    want = torch.from_numpy(GOLDEN["logp_P%d_nl%d" % (P, nl)])
    with torch.no_grad():
        for engine in ("manual", "aten"):
            got = O.forward(sd, b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"],
                            O.default_cfg(nl), engine=engine)
            assert got.shape == want.shape
            assert (got - want).abs().max() < 1e-5


def test_adjacency_matches_reference():
    rs = np.random.RandomState(3)
    lengths = [14, 6, 1]
    feats = [torch.from_numpy(rs.randn(sum(lengths), 200).astype(np.float32)) for _ in range(3)]
    want = torch.from_numpy(GOLDEN["adj_avl"])
    got = O.create_big_adj(feats, lengths)
    assert got.shape == want.shape and (got - want).abs().max() < 2e-5
    want2 = torch.from_numpy(GOLDEN["adj_av"])
    got2 = O.create_big_adj(feats[:2], lengths)
    assert got2.shape == want2.shape and (got2 - want2).abs().max() < 2e-5
