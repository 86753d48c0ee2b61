"""TFN fusion module, host side: the reference's state_dict (tests/golden/make_golden_tfn.py) and no CPU fallback."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _keys(path):
    with open(path) as f:
        return [(ln.split()[0], tuple(int(d) for d in ln.split()[1:])) for ln in f if ln.strip()]


def test_tfn_state_dict_matches_reference_keys():
    from mm_dfn_amd.fusion import TFN
    with torch.device("meta"):                      # (the default layer-1 weight is 1.24 GB: shapes only)
        m = TFN()
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _keys(os.path.join(GOLD, "state_dict_keys_tfn.txt"))
    assert len(got) == 10
    assert isinstance(m.post_fusion_dropout, torch.nn.Dropout) and m.post_fusion_dropout.p == 0.4


def test_tfn_small_module_has_the_golden_state_dict_shapes():
    from mm_dfn_amd.fusion import TFN
    g = np.load(os.path.join(GOLD, "tfn_module.npz"), allow_pickle=False)
    m = TFN(input_dims=(12, 16, 20), hidden_dims=(5, 6, 7), dropouts=0.0, post_fusion_dim=16, output_dim=8)
    sd = m.state_dict()
    want = {k[3:]: g[k].shape for k in g.files if k.startswith("sd/")}
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in want.items()}
    assert sd["post_fusion_layer_1.weight"].shape == (16, 6 * 7 * 8)
    m.load_state_dict({k: torch.from_numpy(g["sd/" + k]) for k in sd})


def test_tfn_on_host_tensors_fails_loudly():
    from mm_dfn_amd import _hip
    from mm_dfn_amd.fusion import TFN
    m = TFN(input_dims=(12, 16, 20), hidden_dims=(5, 6, 7), post_fusion_dim=16, output_dim=8)
    with pytest.raises(_hip.HipLibraryError):
        m(torch.randn(3, 12), torch.randn(3, 16), torch.randn(3, 20))
