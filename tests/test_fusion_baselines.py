"""Graph-free fusion baselines (graph_type='None', model.py:874-883, 960-970, 984-1006, 1338-1404) and DeepGCN with 'mfn'
(model.py:1263-1293): the state_dict key / shape lists against those exported from the reference
(tests/golden/make_golden_fusion.py) and the combinations the reference cannot run."""
import os

import pytest

from mm_dfn_amd import synthetic
from test_oracle_golden import GOLD

CFG = dict(B=3, L=14, P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)
CASES = {
    # name: (graph_type, att_type, modals, seed) -- as in make_golden_fusion.py
    "concat_subsequently": ("None", "concat_subsequently", "avl", 901),
    "gated": ("None", "gated", "avl", 902),
    "mfn_only": ("None", "mfn_only", "avl", 903),
    "lmf_only": ("None", "lmf_only", "avl", 904),
    "concat_only": ("None", "concat_only", "avl", 905),
    "al_concat_subsequently": ("None", "concat_subsequently", "al", 906),
    "av_gated": ("None", "gated", "av", 907),
    "deepgcn_mfn": ("DeepGCN", "mfn", "avl", 908),
}


def build(name, dropout=0.0):
    graph_type, att_type, modals, seed = CASES[name]
    m = synthetic.build_model(dropout=dropout, graph_type=graph_type, att_type=att_type, modals=modals, reason_flag=False, **CFG)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), seed))
    return m


@pytest.mark.parametrize("name", sorted(CASES))
def test_state_dict_keys_of_the_fusion_baselines_match_the_reference(name):
    m = build(name)
    fname = "state_dict_keys_%s%s.txt" % ("none_" if CASES[name][0] == "None" else "", name)
    want = [ln.split() for ln in open(os.path.join(GOLD, fname)).read().splitlines() if ln]
    got = [[k] + [str(d) for d in v.shape] for k, v in m.state_dict().items()]
    assert sorted(map(tuple, got)) == sorted(map(tuple, want))


def test_unsupported_graph_free_combinations_say_so():
    from mm_dfn_amd.dialogue_model import DialogueGNNModel
    mk = lambda **kw: DialogueGNNModel("LSTM", 100, 150, 150, 100, 100, 100, 100, n_speakers=2, max_seq_len=200, window_past=10,
                                       window_future=10, n_classes=6, multi_modal=True, use_crn_speaker=True,
                                       speaker_weights="3-0-1", Deep_GCN_nlayers=2, reason_flag=False, **kw)
    for att in ("mfn_only", "tfn_only", "lmf_only", "concat_only"):
        with pytest.raises(NotImplementedError):
            mk(graph_type="None", modals="al", att_type=att)
    with pytest.raises(NotImplementedError):
        mk(graph_type="None", modals="avl", att_type="concat_subsequently", use_residue=False)
    with pytest.raises(NotImplementedError):
        mk(graph_type="None", modals="avl", att_type="tfn_only")
    with pytest.raises(NotImplementedError):
        mk(graph_type="None", modals="avl", att_type="mfn")
    with pytest.raises(NotImplementedError):
        mk(graph_type="None", modals="a", att_type="concat_subsequently")
    with pytest.raises(NotImplementedError):
        mk(graph_type="relation", modals="avl", att_type="concat_subsequently")
    with pytest.raises(NotImplementedError):
        mk(graph_type="GDF", modals="al", att_type="mfn")
    with pytest.raises(NotImplementedError):
        DialogueGNNModel("DialogRNN", 100, 150, 150, 100, 100, 100, 100, n_speakers=2, max_seq_len=200, window_past=10,
                         window_future=10, graph_type="None", att_type="concat_only")
    with pytest.raises(NotImplementedError):
        DialogueGNNModel("LSTM", 100, 150, 150, 100, 100, 100, 200, n_speakers=2, max_seq_len=200, window_past=10,
                         window_future=10, graph_type="None", att_type="gated", multi_modal=True)
    mk(graph_type="None", modals="avl", att_type="lmf_only")
    mk(graph_type="DeepGCN", modals="avl", att_type="mfn")
