"""Export golden vectors of DialogRNNModel + MaskedNLLLoss from the REAL reference (run only in the build container, on the CPU).

    python tests/golden/make_golden_dialog_rnn_model.py

model.DialogRNNModel(D_m, 150, 150, 100, 32, n_classes=C, context_attention, dropout_rec=0, dropout=0, att2) in train mode,
with its Dropout(dropout + 0.15) site set to p = 0 (the constructor gives it 0.15 whatever ``dropout`` is), once per case of
tests/dialogue_rnn_ref.CASES:
    a   'general', D_m 100, T 12, lengths [12, 7, 1], 2 parties, 6 classes; the speaker of dialogue 1 never changes
    b   'simple',  D_m 600, T 6,  lengths [6, 2, 6, 3, 1], 9 parties, 7 classes
    c   as (a) with att2=False.  The reference's own forward raises UnboundLocalError there (it returns an ``alpha`` it never
        assigned), so this case runs that forward up to the exception and reads what it computed from forward hooks (``forward_without_att2``).
Weights: synthetic.seeded_state_dict(reference state, seed); inputs: dialogue_rnn_ref.case_inputs(case, seed + 1).  Only the
seed and the reference's outputs are stored.  The seed is the first from 0 upward for which every pre-activation of the ReLU,
in all three cases, stays away from zero (min |pre| > 1e-5 max |pre|), so that no comparison flips on a rounding.

Stored per case <c>/: log_prob, alpha (the list stacked, (T, B, T); absent for c), emotions (absent for c: the same encoders on
the same inputs as a), alpha_f / alpha_b (the lists packed into a (T, B, T) lower triangle, row t = entry t-1; rows of alpha_b
at or beyond a dialogue's length are stored as ZERO: the reference's reverse encoder runs on into its own padding there, the
package's stops), loss_plain / loss_weighted (loss.MaskedNLLLoss without / with class weights), and of the class-weighted
loss's gradients: digest/<parameter> for every parameter (test_oracle_golden._digest's format) and grad/<parameter> for the
parameters of dialogue_rnn_ref.GRAD_ROWS -- every k-th row.
Writes dialog_rnn_model.npz and state_dict_keys_dialog_rnn_model.txt next to this file.
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
import dialogue_rnn_ref as DR  # noqa: E402
from mm_dfn_amd import synthetic  # noqa: E402


def forward_without_att2(model, U, qmask, umask):
    """The reference's own forward for att2=False, run until it raises on its return statement; everything it computed by then
    is taken from forward hooks: the encoders' attention lists, the input of ``linear`` (emotions) and the logits."""
    seen = {}
    hooks = [model.dialog_rnn_f.register_forward_hook(lambda m, i, o: seen.__setitem__("alpha_f", o[1])),
             model.dialog_rnn_r.register_forward_hook(lambda m, i, o: seen.__setitem__("alpha_b", o[1])),
             model.linear.register_forward_hook(lambda m, i, o: seen.__setitem__("emotions", i[0])),
             model.smax_fc.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o))]
    try:
        model(U, qmask, umask)
        raise AssertionError("the reference's att2=False forward returned: use its result")
    except UnboundLocalError:
        pass
    finally:
        for h in hooks:
            h.remove()
    return torch.log_softmax(seen["logits"], 2), [], seen["alpha_f"], seen["alpha_b"], seen["emotions"]


def run_case(ref_model, ref_loss, name, seed):
    kind, D_m, T, lengths, P, C, att2 = DR.CASES[name]
    B = len(lengths)
    torch.manual_seed(0)
    model = ref_model.DialogRNNModel(D_m, DR.D_G, DR.D_P, DR.D_E, DR.D_H, n_classes=C, context_attention=kind, dropout_rec=0.0,
                                     dropout=0.0, att2=att2)
    model.dropout_rec.p = 0.0
    keys = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), seed))
    model.train()
    U, qmask, umask, label, weight = DR.case_inputs(name, seed + 1)
    pres = []
    hook = model.linear.register_forward_hook(lambda m, i, o: pres.append(o.detach()))
    log_prob, alpha, alpha_f, alpha_b, emotions = (model if att2 else lambda *a: forward_without_att2(model, *a))(U, qmask, umask)
    hook.remove()
    margin = float(pres[0].abs().min() / pres[0].abs().max())
    lp_ = log_prob.transpose(0, 1).contiguous().view(-1, C)
    loss_plain = ref_loss.MaskedNLLLoss()(lp_, label.view(-1), umask)
    loss_weighted = ref_loss.MaskedNLLLoss(weight)(lp_, label.view(-1), umask)
    loss_weighted.backward()
    af, ab = DR.pack_alpha(alpha_f, T, B), DR.pack_alpha(alpha_b, T, B)
    for b, n in enumerate(lengths):
        ab[n:, b] = 0.0
    res = {"log_prob": log_prob.detach().numpy(), "loss_plain": np.array(loss_plain.item()),
           "loss_weighted": np.array(loss_weighted.item()), "alpha_f": af.numpy(), "alpha_b": ab.numpy()}
    if att2:
        res["alpha"] = torch.stack(alpha).detach().numpy()
    if name != "c":
        res["emotions"] = emotions.detach().numpy()
    for k, prm in model.named_parameters():
        if prm.grad is not None:
            res["digest/" + k] = DR.digest(prm.grad)
            step = DR.GRAD_ROWS.get(k, {}).get(name)
            if step:
                res["grad/" + k] = prm.grad[::step].numpy()
    return res, margin, keys


def main():
    ref_model, _, _, ref_loss = ref_shim.modules()
    seed = 0
    while True:
        data, margins = {}, []
        for name in DR.CASES:
            res, margin, keys = run_case(ref_model, ref_loss, name, seed)
            margins.append(margin)
            data.update({name + "/" + k: v for k, v in res.items()})
        if min(margins) > 1e-5:
            break
        seed += 1
    data["seed"] = np.array(seed)
    path = os.path.join(HERE, "dialog_rnn_model.npz")
    np.savez_compressed(path, **data)
    with open(os.path.join(HERE, "state_dict_keys_dialog_rnn_model.txt"), "w") as fh:
        for k, shape in keys:
            fh.write(" ".join([k] + [str(s) for s in shape]) + "\n")
    print("seed", seed, "margins", margins, "arrays", len(data), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
