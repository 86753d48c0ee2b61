"""Export golden vectors of MM_GCN with speaker and modality embeddings from the REAL reference (run only in the build container).

    python tests/golden/make_golden_embeddings.py

model_mm.MM_GCN(D, D, D, D, nlayers=2, nhidden=H, nclass=6, dropout=1e-12, lamda=0.5, alpha=0.2, variant=True,
return_feature=True, use_residue=True, n_speakers=3, use_speaker=True, use_modal=True, reason_flag=True) with (D, H) = (16, 8),
in train mode (dropout 1e-12: every element is kept and the scale is 1 in float32; at p = 0 the reference edits a ReLU output in
place), on dia_len = [5, 1, 7] with three speakers, once per ``modals`` in 'avl', 'al', 'av' -- the same weights every time.
The reference adds the embeddings to its inputs IN PLACE, so the modality inputs are passed as ``leaf * 1.0``.

Stored: the state dict (sd/), qmask, dia_len and per case <modals>/: the inputs x_<m>, the cotangent G, the output, the gradients
dx_<m> of (out * G).sum() for every input and those of the two tables, dspeaker / dmodal (absent when the reference leaves
``.grad`` None: the speaker table without 'l').  The seed is the first from 0 upward for which every ReLU's pre-activations, in
all three cases, stay away from zero (min |pre| > 1e-5 max |pre|), so that no comparison flips on a rounding.
Writes mm_gcn_embeddings.npz next to this file.
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

DIA_LEN = [5, 1, 7]
D, H, P = 16, 8, 3
CASES = ("avl", "al", "av")
CFG = dict(nlayers=2, nhidden=H, nclass=6, dropout=1e-12, lamda=0.5, alpha=0.2, variant=True, return_feature=True,
           use_residue=True, n_speakers=P, use_speaker=True, use_modal=True, reason_flag=True)


def make_qmask(gen):
    L, B = max(DIA_LEN), len(DIA_LEN)
    q = torch.zeros(L, B, P)
    for b, n in enumerate(DIA_LEN):
        spk = torch.randint(0, P, (n,), generator=gen)
        q[torch.arange(n), b, spk] = 1
    return q


def run_case(ref_mm, sd, modals, qmask, gen):
    mod = ref_mm.MM_GCN(D, D, D, D, modals=list(modals), **CFG)
    mod.load_state_dict(sd)
    mod.train()
    N = sum(DIA_LEN)
    leaves = {m: torch.randn(N, D, generator=gen).requires_grad_(True) for m in modals}
    G = torch.randn(N, len(modals) * (D + H), generator=gen)
    pres = []
    hooks = [m.register_forward_hook(lambda m, i, o: pres.append(o.detach()))
             for m in list(mod.graph_net.fcs) + list(mod.graph_net.convs)]
    args = [leaves[m] * 1.0 if m in modals else [] for m in "avl"]
    out = mod(args[0], args[1], args[2], DIA_LEN, qmask)
    for h in hooks:
        h.remove()
    assert tuple(out.shape) == tuple(G.shape)
    (out * G).sum().backward()
    margin = min(float(p.abs().min() / p.abs().max()) for p in pres)
    res = {"G": G.numpy(), "out": out.detach().numpy()}
    for m in modals:
        res["x_" + m] = leaves[m].detach().numpy()
        res["dx_" + m] = leaves[m].grad.numpy()
    for name, table in (("dspeaker", mod.speaker_embeddings), ("dmodal", mod.modal_embeddings)):
        if table.weight.grad is not None:
            res[name] = table.weight.grad.numpy()
    return res, margin


def main():
    _, ref_mm, _, _ = ref_shim.modules()
    seed = 0
    while True:
        torch.manual_seed(seed)
        gen = torch.Generator().manual_seed(1000 + seed)
        sd = {k: v.clone() for k, v in ref_mm.MM_GCN(D, D, D, D, modals=list("avl"), **CFG).state_dict().items()}
        qmask = make_qmask(gen)
        data = {"dia_len": np.array(DIA_LEN, dtype=np.int64), "qmask": qmask.numpy()}
        margins = []
        for modals in CASES:
            res, margin = run_case(ref_mm, sd, modals, qmask, gen)
            margins.append(margin)
            data.update({modals + "/" + k: v for k, v in res.items()})
        if min(margins) > 1e-5:
            break
        seed += 1
    data["seed"] = np.array(seed)
    data.update({"sd/" + k: v.numpy() for k, v in sd.items()})
    assert "av/dspeaker" not in data and float(np.abs(data["al/dmodal"][1]).max()) == 0.0
    path = os.path.join(HERE, "mm_gcn_embeddings.npz")
    np.savez_compressed(path, **data)
    print("seed", seed, "margins", margins, "arrays", len(data), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
