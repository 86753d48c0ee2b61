"""Export golden vectors of the graph-free fusion baselines from the REAL reference (run only in the build container).

    python tests/golden/make_golden_fusion.py

graph_type='None' with the post-hoc fusions of --mm_fusion_mthd (model.py:874-883, 960-970, 984-1006, 1338-1404) and
graph_type='DeepGCN' with 'mfn' (model.py:1263-1293), built through oracle/ref_shim.build_reference_model.  Weights and
inputs are regenerated on both sides from seeds (mm_dfn_amd/synthetic.py); only reference outputs are stored:
eval log-probabilities, the train() loss and a digest of every live gradient with every dropout p set to 0 (the
module-level ones of MFN and MMGatedAttention included).  The MFN cases fake torch.cuda.is_available (model.py:1369,1385).
Writes fusion_baselines.npz and the state_dict key lists (keys_file) next to this file.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_shim  # noqa: E402
from mm_dfn_amd import synthetic  # noqa: E402

CFG = dict(B=3, L=14, P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)
LENGTHS = [14, 5, 9]
CASES = {
    # name: (graph_type, att_type, modals, seed)
    "concat_subsequently": ("None", "concat_subsequently", "avl", 901),
    "gated": ("None", "gated", "avl", 902),
    "mfn_only": ("None", "mfn_only", "avl", 903),
    "lmf_only": ("None", "lmf_only", "avl", 904),
    "concat_only": ("None", "concat_only", "avl", 905),
    "al_concat_subsequently": ("None", "concat_subsequently", "al", 906),
    "av_gated": ("None", "gated", "av", 907),
    "deepgcn_mfn": ("DeepGCN", "mfn", "avl", 908),
}


def keys_file(name):
    """state_dict_keys_none_<case>.txt for the graph-free cases, state_dict_keys_<case>.txt for the others."""
    return "state_dict_keys_%s%s.txt" % ("none_" if CASES[name][0] == "None" else "", name)


def grad_digest(g):
    g = g.detach().double().reshape(-1)
    return np.array([g.sum().item(), g.abs().sum().item(), (g * g).sum().item()], dtype=np.float64)


def build(graph_type, att_type, modals, seed):
    m = ref_shim.build_reference_model(CFG["D_t"], CFG["D_a"], CFG["D_v"], CFG["P"], CFG["C"], CFG["nlayers"], dropout=0.0,
                                       modals=modals, att_type=att_type, graph_type=graph_type, reason_flag=False)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), seed))
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def main():
    _, _, _, ref_loss = ref_shim.modules()
    out = {}
    real = torch.cuda.is_available
    torch.cuda.is_available = lambda: True
    try:
        for name, (graph_type, att_type, modals, seed) in CASES.items():
            batch = synthetic.make_batch(seed + 1, lengths=LENGTHS, **CFG)
            args = (batch["textf"], batch["qmask"], batch["umask"], batch["lengths"], batch["acouf"], batch["visuf"])
            m = build(graph_type, att_type, modals, seed).eval()
            with open(os.path.join(HERE, keys_file(name)), "w") as f:
                for k, v in m.state_dict().items():
                    f.write("%s %s\n" % (k, " ".join(str(d) for d in v.shape)))
            with torch.no_grad():
                out[name + "/log_prob"] = m(*args)[0].numpy()
            m.train()
            logp = m(*args)[0]
            label = torch.cat([batch["label"][j][:n] for j, n in enumerate(batch["lengths"])])
            loss = ref_loss.FocalLoss(gamma=0.5)(logp, label)
            loss.backward()
            out[name + "/loss"] = np.array(loss.item(), dtype=np.float64)
            live = []
            for k, p in m.named_parameters():
                if p.grad is not None and float(p.grad.abs().max()) > 0:
                    live.append(k)
                    out[name + "/gd/" + k] = grad_digest(p.grad)
            out[name + "/live_params"] = np.array(live)
            print(name, "loss", loss.item(), "live", len(live), "keys", len(m.state_dict()))
    finally:
        torch.cuda.is_available = real
    np.savez_compressed(os.path.join(HERE, "fusion_baselines.npz"), **out)


if __name__ == "__main__":
    main()
