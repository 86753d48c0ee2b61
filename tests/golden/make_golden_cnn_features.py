"""Export golden vectors of CNNFeatureExtractor from the REAL reference (run only in the build container).

    python tests/golden/make_golden_cnn_features.py

model.CNNFeatureExtractor in train mode (dropout 0), once per case of tests/cnn_features_ref.MODEL_CASES:
    a   (60, 100, 100, 50, (3, 4, 5), 0), x (5, 3, 12), lengths [5, 3, 1]; "loss" = sum(features G)
    b   (40, 300, 100, 50, (3, 4, 5), 0), x (2, 2, 7), lengths [2, 1], a frozen pretrained table; the same kind of loss
    c   case a's extractor -> model.LSTMModel(100, 100, 32, n_classes=6, dropout=0) -> loss.MaskedNLLLoss(class weights)
Weights: synthetic.seeded_state_dict(reference state, seed) (case c: the LSTMModel's with seed + 7); inputs:
cnn_features_ref.model_inputs(case, seed + 1).  Only the seed and the reference's outputs are stored.  The seed is the first from
0 upward for which, in all three cases, every pre-activation of fc's ReLU stays away from zero (min |pre| > 1e-5 max |pre| over
the rows the mask keeps) and every max-pool comparison is decidable (cnn_features_ref.decidable), so that no comparison flips on
a rounding.

Stored per case <c>/: features, loss, log_prob (c only), digest/<parameter> for every parameter with a gradient
(test_oracle_golden._digest's format; case c prefixes the LSTMModel's with "lstm_model.") and grad/<parameter> for the
extractor's parameters named in cnn_features_ref.MODEL_GRAD_ROWS -- every k-th row.
Writes cnn_features.npz and state_dict_keys_cnn_features.txt next to this file.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_shim  # noqa: E402
import cnn_features_ref as CR  # noqa: E402
from mm_dfn_amd import synthetic  # noqa: E402


def run_case(ref_model, ref_loss, name, seed):
    c = CR.MODEL_CASES[name]
    torch.manual_seed(0)
    cnn = ref_model.CNNFeatureExtractor(*c["args"])
    keys = [(k, tuple(v.shape)) for k, v in cnn.state_dict().items()]
    x, qmask, umask, label, weight, G, pretrained = CR.model_inputs(name, seed + 1)
    cnn.load_state_dict(synthetic.seeded_state_dict(cnn.state_dict(), seed))
    if c["frozen"]:
        cnn.init_pretrained_embeddings_from_numpy(pretrained)
    cnn.train()
    pres = []
    hook = cnn.fc.register_forward_hook(lambda m, i, o: pres.append(o.detach()))
    features = cnn(x, umask)
    hook.remove()
    live = umask.t().reshape(-1) != 0
    pre = pres[0][live]
    margin = float(pre.abs().min() / pre.abs().max())
    decidable = CR.model_decidable({k: v.detach() for k, v in cnn.state_dict().items()}, x, umask)
    res = {"features": features.detach().numpy()}
    named = list(cnn.named_parameters())
    if c["lstm"]:
        lstm = ref_model.LSTMModel(*CR.LSTM_ARGS, n_classes=CR.N_CLASSES, dropout=0.0, att2=True)
        lstm.load_state_dict(synthetic.seeded_state_dict(lstm.state_dict(), seed + 7))
        lstm.train()
        log_prob = lstm(features, qmask, umask)[0]
        lp_ = log_prob.transpose(0, 1).contiguous().view(-1, CR.N_CLASSES)
        loss = ref_loss.MaskedNLLLoss(weight)(lp_, label.view(-1), umask)
        res["log_prob"] = log_prob.detach().numpy()
        named += [("lstm_model." + k, p) for k, p in lstm.named_parameters()]
    else:
        loss = (features * G).sum()
    loss.backward()
    res["loss"] = np.array(loss.item())
    for k, prm in named:
        if prm.grad is not None:
            res["digest/" + k] = CR.digest(prm.grad)
            step = CR.MODEL_GRAD_ROWS.get(k)
            if step:
                res["grad/" + k] = prm.grad[::step].numpy()
    return res, margin, decidable, keys


def main():
    ref_model, _, _, ref_loss = ref_shim.modules()
    seed = 0
    while True:
        data, margins, ok = {}, [], True
        for name in CR.MODEL_CASES:
            res, margin, decidable, keys = run_case(ref_model, ref_loss, name, seed)
            margins.append(margin)
            ok = ok and decidable
            data.update({name + "/" + k: v for k, v in res.items()})
            if name == "a":
                keys_a = keys
        if ok and min(margins) > 1e-5:
            break
        seed += 1
    data["seed"] = np.array(seed)
    path = os.path.join(HERE, "cnn_features.npz")
    np.savez_compressed(path, **data)
    with open(os.path.join(HERE, "state_dict_keys_cnn_features.txt"), "w") as fh:
        for k, shape in keys_a:
            fh.write(" ".join([k] + [str(s) for s in shape]) + "\n")
    print("seed", seed, "margins", margins, "arrays", len(data), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
