"""Export golden vectors of LSTMModel + MaskedNLLLoss from the REAL reference (run only in the build container).

    python tests/golden/make_golden_lstm_model.py

model.LSTMModel(D_m, 100, 32, n_classes=C, dropout=0, att2) in train mode, once per case of tests/lstm_model_ref.CASES:
    a   D_m 100, L 20, lengths [20, 13, 7], 6 classes
    b   D_m 600, L 9,  lengths [9, 1, 4, 2], 7 classes
    c   as (a) with att2=False
Weights: synthetic.seeded_state_dict(reference state, seed); inputs: gru_model_ref.case_inputs(case, seed + 1).  Only the seed
and the reference's outputs are stored.  The seed is the first from 0 upward for which every pre-activation of the ReLU, in all
three cases, stays away from zero (min |pre| > 1e-5 max |pre|), so that no comparison flips on a rounding.

Stored per case <c>/: log_prob, alpha (the list stacked, (L, B, L); absent for c), emotions (absent for c: the same LSTM on the
same inputs as a), loss_plain / loss_weighted (loss.MaskedNLLLoss without / with class weights), and of the class-weighted loss's
gradients: digest/<parameter> for every parameter (test_oracle_golden._digest's format) and grad/<parameter> for
matchatt.transform.weight, linear.weight and lstm.weight_ih_l0 -- every k-th row (lstm_model_ref.GRAD_ROWS; k = 1: the whole
gradient), which keeps the file near 300 KB.
Writes lstm_model.npz and state_dict_keys_lstm_model.txt next to this file.
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
import lstm_model_ref as LR  # noqa: E402
from mm_dfn_amd import synthetic  # noqa: E402


def run_case(ref_model, ref_loss, name, seed):
    D_m, L, lengths, C, att2 = LR.CASES[name]
    torch.manual_seed(0)
    model = ref_model.LSTMModel(D_m, LR.D_E, LR.D_H, n_classes=C, dropout=0.0, att2=att2)
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), seed))
    model.train()
    U, qmask, umask, label, weight = LR.case_inputs(name, seed + 1)
    pres = []
    hook = model.linear.register_forward_hook(lambda m, i, o: pres.append(o.detach()))
    log_prob, alpha, _, _, emotions = model(U, qmask, umask)
    hook.remove()
    margin = float(pres[0].abs().min() / pres[0].abs().max())
    lp_ = log_prob.transpose(0, 1).contiguous().view(-1, C)
    loss_plain = ref_loss.MaskedNLLLoss()(lp_, label.view(-1), umask)
    loss_weighted = ref_loss.MaskedNLLLoss(weight)(lp_, label.view(-1), umask)
    loss_weighted.backward()
    res = {"log_prob": log_prob.detach().numpy(), "loss_plain": np.array(loss_plain.item()),
           "loss_weighted": np.array(loss_weighted.item())}
    if att2:
        res["alpha"] = torch.stack(alpha).detach().numpy()
    if name != "c":
        res["emotions"] = emotions.detach().numpy()
    for k, prm in model.named_parameters():
        if prm.grad is not None:
            res["digest/" + k] = LR.digest(prm.grad)
            step = LR.GRAD_ROWS.get(k, {}).get(name)
            if step:
                res["grad/" + k] = prm.grad[::step].numpy()
    return res, margin, keys


def main():
    ref_model, _, _, ref_loss = ref_shim.modules()
    seed = 0
    while True:
        data, margins = {}, []
        for name in LR.CASES:
            res, margin, keys = run_case(ref_model, ref_loss, name, seed)
            margins.append(margin)
            data.update({name + "/" + k: v for k, v in res.items()})
        if min(margins) > 1e-5:
            break
        seed += 1
    data["seed"] = np.array(seed)
    path = os.path.join(HERE, "lstm_model.npz")
    np.savez_compressed(path, **data)
    with open(os.path.join(HERE, "state_dict_keys_lstm_model.txt"), "w") as fh:
        for k, shape in keys:
            fh.write(" ".join([k] + [str(s) for s in shape]) + "\n")
    print("seed", seed, "margins", margins, "arrays", len(data), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
