"""Export golden vectors of the TFN fusion module from the REAL reference (run only in the build container).

    python tests/golden/make_golden_tfn.py

model_fusion.TFN(input_dims=(12, 16, 20), hidden_dims=(5, 6, 7), dropouts=0.0, post_fusion_dim=16, output_dim=8) on N = 9 rows
(K = 6 * 7 * 8 = 336), subnet weights times 3.  Stored: the inputs, the state dict, a cotangent G, the output and the gradients
of (out * G).sum() for the three inputs and every parameter.  The seed is the first from 0 upward for which the
pre-activations of both ReLUs stay away from zero (min |pre| > 1e-3 max |pre|), so that no comparison flips on a rounding.
Writes tfn_module.npz and state_dict_keys_tfn.txt (the key list of the DEFAULT TFN(), built on the meta device) next to this file.
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

CFG = dict(input_dims=(12, 16, 20), hidden_dims=(5, 6, 7), dropouts=0.0, post_fusion_dim=16, output_dim=8)
N = 9


def run(ref_fusion, seed):
    torch.manual_seed(seed)
    mod = ref_fusion.TFN(**CFG)
    with torch.no_grad():
        for net in (mod.audio_subnet, mod.video_subnet, mod.text_subnet):
            net.weight.mul_(3.0)
    xs = [torch.randn(N, d, requires_grad=True) for d in CFG["input_dims"]]
    G = torch.randn(N, CFG["output_dim"])
    pres = []
    hooks = [l.register_forward_hook(lambda m, i, o: pres.append(o.detach()))
             for l in (mod.post_fusion_layer_1, mod.post_fusion_layer_2)]
    mod.train()
    out = mod(*xs)
    for h in hooks:
        h.remove()
    margin = min(float(p.abs().min() / p.abs().max()) for p in pres)
    return mod, xs, G, out, margin


def main():
    ref_shim.install()
    import model_fusion as ref_fusion
    seed = 0
    while True:
        mod, xs, G, out, margin = run(ref_fusion, seed)
        if margin > 1e-3:
            break
        seed += 1
    assert margin > 1e-3
    (out * G).sum().backward()
    data = {"seed": np.array(seed), "G": G.numpy(), "out": out.detach().numpy()}
    for name, x in zip("avt", xs):
        data["x_" + name] = x.detach().numpy()
        data["dx_" + name] = x.grad.numpy()
    for k, v in mod.state_dict().items():
        data["sd/" + k] = v.numpy()
    for k, p in mod.named_parameters():
        data["grad/" + k] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "tfn_module.npz"), **data)
    with torch.device("meta"):
        full = ref_fusion.TFN()
    with open(os.path.join(HERE, "state_dict_keys_tfn.txt"), "w") as f:
        for k, v in full.state_dict().items():
            f.write("%s %s\n" % (k, " ".join(str(d) for d in v.shape)))
    print("seed", seed, "margin", margin, "keys", len(full.state_dict()))


if __name__ == "__main__":
    main()
