"""Export golden vectors of the two sparse graphs of new_graph=True from the REAL reference (run only in the build container).

    python tests/golden/make_golden_band_graphs.py

  win/<n>/  model_GCN.GCNII_lyc(nfeat=40, nlayers=2, nhidden=20, variant=True, return_feature=True, use_residue=True,
            reason_flag=True, new_graph=True) on dia_len = [1, 2, 5], [21, 22, 23] and [45]: the dense matrix of its
            message_passing_relation_graph(x, dia_len), then the module called with that matrix as adj (length 21 is the last
            fully dense tile, 22 has the first zero entry).
  spk/<n>/  model_GCN.GCNII(the same widths, new_graph=True) called with a qmask (dialogue, position, speaker); the dense
            matrix is what its message_passing_directed_speaker built inside forward.  Batch 0 has P = 2 speakers: alternating,
            only speaker 0, a dialogue where speaker 0 never speaks, a dialogue of length 1.  Batch 1 has P = 3: random
            speakers (1 and 2 share a chain), speaker 0 never, length 1.  The padded positions of qmask hold non-zero garbage
            (ones in column 0 included): the reference reads qmask[i][0:len_] only.

Train mode with dropout = 1e-12 (every element is kept, the scale is 1 in float32; with dropout 0 F.dropout hands its input
through and the reference's own backward fails: "layer_inner += q", model_GCN.py:472, then overwrites the ReLU output autograd
saved).  GCNII has no dropout between the two, so with the gate on its backward fails in every mode (make_golden.py): the spk/
gradients are those of reason_flag=False, and the forward output of the same parameters with reason_flag=True is stored next to
them as out_gate (computed under no_grad).  Stored per case: dia_len, the input x, (qmask), the state dict, a cotangent G,
the output, the dense normalised adjacency and the gradients of (out * G).sum() for x and every parameter.  As in make_golden_mmgcn2.py every
parameter is rounded to a multiple of 2^-7, every input to a multiple of 2^-6 and the cotangents to multiples of 1/4 before the
run, and the seed of a case is the first from 0 upward for which every ReLU's pre-activations stay away from zero
(min |pre| > 1e-5 max |pre|).

The script also asserts what the package's window builder relies on: the reference's edge set -- the union of the cliques on
[k - 10, k + 10] -- is exactly the band |p - q| <= 20 inside each dialogue.
Writes band_graphs.npz next to this file.
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

CFG = dict(nfeat=40, nlayers=2, nhidden=20, nclass=6, dropout=1e-12, lamda=0.5, alpha=0.2, variant=True, return_feature=True,
           use_residue=True, new_graph=True, reason_flag=True)
WINDOW = [[1, 2, 5], [21, 22, 23], [45]]
BAND = 20


def onehot(speakers, P):
    q = torch.zeros(len(speakers), P)
    q[torch.arange(len(speakers)), torch.tensor(speakers, dtype=torch.long)] = 1.0
    return q


def speaker_batches():
    g = torch.Generator().manual_seed(7)
    b0 = [[j % 2 for j in range(7)], [0] * 5, [1] * 4, [1]]
    b1 = [torch.randint(0, 3, (9,), generator=g).tolist(), [2, 1, 2], [0]]
    assert 0 in b1[0] and 1 in b1[0] and 2 in b1[0]
    out = []
    for P, dialogues in ((2, b0), (3, b1)):
        Lmax = max(len(d) for d in dialogues)
        qmask = torch.empty(len(dialogues), Lmax, P)
        qmask[:, :, 0] = 1.0            # garbage behind every dialogue's end: "speaker 0" flags and other non-zero values
        qmask[:, :, 1:] = 7.0
        for i, d in enumerate(dialogues):
            qmask[i, :len(d)] = onehot(d, P)
        out.append(([len(d) for d in dialogues], qmask))
    return out


def quantise(mod):
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.round(p * 128.0) / 128.0)


def coarse(shape, step, requires_grad=False):
    return (torch.round(torch.randn(*shape) / step) * step).requires_grad_(requires_grad)


def band_mask(dia_len):
    N = sum(dia_len)
    mask = torch.zeros(N, N, dtype=torch.bool)
    s = 0
    for L in dia_len:
        p = torch.arange(L)
        mask[s:s + L, s:s + L] = (p[:, None] - p[None, :]).abs() <= BAND
        s += L
    return mask


def run_case(make, call, dia_len):
    """First seed whose ReLU pre-activations keep their margin -> (module, x, G, out, adj)."""
    N = sum(dia_len)
    seed = 0
    while True:
        torch.manual_seed(seed)
        mod = make()
        quantise(mod)
        x = coarse((N, CFG["nfeat"]), 2.0 ** -6, True)
        G = coarse((N, CFG["nfeat"] + CFG["nhidden"]), 0.25)
        pres = []
        hooks = [m.register_forward_hook(lambda m, i, o: pres.append(o.detach())) for m in list(mod.fcs) + list(mod.convs)]
        mod.train()
        out, adj = call(mod, x)
        for h in hooks:
            h.remove()
        assert tuple(out.shape) == tuple(G.shape) and not adj.requires_grad
        if min(float(p.abs().min() / p.abs().max()) for p in pres) > 1e-5:
            return seed, mod, x, G, out, adj
        seed += 1


def export(prefix, data, dia_len, mod, x, G, out, adj, qmask=None):
    (out * G).sum().backward()
    data[prefix + "dia_len"] = np.array(dia_len, dtype=np.int64)
    data[prefix + "x"] = x.detach().numpy()
    data[prefix + "dx"] = x.grad.numpy()
    data[prefix + "G"] = G.numpy()
    data[prefix + "out"] = out.detach().numpy()
    data[prefix + "adj"] = adj.numpy()
    if qmask is not None:
        data[prefix + "qmask"] = qmask.numpy()
    for k, v in mod.state_dict().items():
        data[prefix + "sd/" + k] = v.numpy()
    for k, p in mod.named_parameters():
        if p.grad is not None:            # (the LSTM cell of a module with reason_flag=False takes no part)
            data[prefix + "grad/" + k] = p.grad.numpy()


def main():
    _, _, ref_gcn, _ = ref_shim.modules()
    data, seeds = {}, []
    for n, dia_len in enumerate(WINDOW):
        def call(mod, x):
            adj = mod.message_passing_relation_graph(x, dia_len).detach()
            return mod(x, dia_len, None, adj=adj), adj
        seed, mod, x, G, out, adj = run_case(lambda: ref_gcn.GCNII_lyc(**CFG), call, dia_len)
        # the reference's own edge set against the derivation (union of the [k - 10, k + 10] cliques = the band of half-width 20)
        assert torch.equal(adj != 0, band_mask(dia_len)), dia_len
        export("win/%d/" % n, data, dia_len, mod, x, G, out, adj)
        seeds.append(seed)
    for n, (dia_len, qmask) in enumerate(speaker_batches()):
        def call(mod, x):
            built = []
            fn = mod.message_passing_directed_speaker
            mod.message_passing_directed_speaker = lambda *a: (built.append(fn(*a)), built[-1])[1]
            out = mod(x, dia_len, qmask)
            del mod.message_passing_directed_speaker
            assert len(built) == 1
            return out, built[0].detach()
        seed, mod, x, G, out, adj = run_case(lambda: ref_gcn.GCNII(**dict(CFG, reason_flag=False)), call, dia_len)
        export("spk/%d/" % n, data, dia_len, mod, x, G, out, adj, qmask)
        gated = ref_gcn.GCNII(**CFG)
        gated.load_state_dict(mod.state_dict())
        gated.train()
        with torch.no_grad():
            data["spk/%d/out_gate" % n] = gated(x.detach(), dia_len, qmask).numpy()
        seeds.append(seed)
    path = os.path.join(HERE, "band_graphs.npz")
    np.savez_compressed(path, **data)
    print("seeds", seeds, "arrays", len(data), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
