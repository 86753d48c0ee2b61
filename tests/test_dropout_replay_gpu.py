"""The dropout-on training step against the CPU oracle ON THE FLAGS THE DEVICE DREW.

Every dropout site of the HIP path draws its 0 / 1 keep flags through ``ops_flags.keep_flags``; with ``ops_flags.TAP`` set the
flags of a forward pass are recorded, ``util.dropout_tape_from_tap`` maps them onto the oracle's dropout sites
(mmdfn_oracle.DropoutTape, pinned against the reference by tests/test_dropout_sites.py) and the oracle then computes the same
function as the device -- so the bounds of the dropout-off comparisons apply unchanged: log-probs to 1e-4 absolute, every live
parameter gradient to 1e-4 of its maximum, under the protocol of test_fullsize_gradients_gpu.py (a gradient that misses may
only be explained by at most 16 ReLU units whose pre-activation is below 1e-5 and on which device and oracle took different
sides; the oracle is then differentiated on the device's side and everything must agree).

What runs: the production library with default dispatch; eager steps at small and benchmark sizes (second step of a model:
the step's flags come from the pool drawn by the rider of the first GRU launch), the benchmark's own captured step after each
of two replays, ``gru.bigru2`` alone, the DeepGCN sibling and one graph-free baseline.

``MMDFN_REPLAY_REPORT=<file>``: every case appends its measured errors as a JSON line (profiles/r08_dropout_replay.md is made
from that); ``MMDFN_REPLAY_F64=1`` adds the float32-to-float64 distance of the oracle itself on the same masks, which is also
computed and shown whenever a bound is missed."""
import json
import os

import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd import FocalLoss, gcn_stack, ops, ops_flags, synthetic, train
from mm_dfn_amd import gru as fused
from util import abs_err, check_tape_consumed, dropout_tape_from_tap, party_qmask, rel_err, relu_flips_from_tap

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREFIX = "graph_model.graph_net."


def _report(rec):
    print("dropout replay: " + json.dumps(rec))
    path = os.environ.get("MMDFN_REPLAY_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def _oracle(sd, b, ocfg, tape, loss_of, flips=None, dtype=torch.float32, forward=None):
    """The oracle's train-mode forward + backward on the given masks (and ReLU flips)."""
    params = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    probe = O.ReluProbe(flips)
    tape.seen = []
    prev_p, prev_t = O.set_relu_probe(probe), O.set_dropout_tape(tape)
    try:
        cast = lambda t: t.to(dtype)
        want = (forward or O.forward)(params, cast(b["textf"]), cast(b["qmask"]), cast(b["umask"]), b["lengths"],
                                      cast(b["acouf"]), cast(b["visuf"]), ocfg, training=True, engine="aten")
        loss_of(want).backward()
    finally:
        O.set_relu_probe(prev_p)
        O.set_dropout_tape(prev_t)
    check_tape_consumed(tape)
    return want.detach(), {k: v.grad for k, v in params.items()}, probe


def _grad_misses(dev_grads, grads):
    """(keys that miss the protocol's bounds with their error, the worst relative error and its key, gradients compared)."""
    bad, worst, checked = [], (0.0, None), 0
    for k, g in dev_grads.items():
        g_ref = grads.get(k)
        if g is None:
            if not (g_ref is None or float(g_ref.abs().max()) == 0.0):
                bad.append((k, "no device gradient"))
            continue
        if g_ref is None:
            bad.append((k, "no oracle gradient"))
            continue
        if float(g_ref.abs().max()) < 1e-6:
            if not float(g.abs().max()) < 1e-4:
                bad.append((k, "oracle 0, device %.3g" % float(g.abs().max())))
        else:
            e = rel_err(g, g_ref)
            if e > worst[0]:
                worst = (e, k)
            if not e < 1e-4:
                bad.append((k, "%.3g" % e))
        checked += 1
    return bad, worst, checked


def _compare(tag, model, sd, b, ocfg, draws, rtap, logp, dev_grads, loss_of, min_checked=44, forward=None, extra=None):
    """One device step (its tapped flags ``draws``, ReLU tap ``rtap``, log-probs and gradients) against the oracle.
    ``extra``: masks of sites that do not draw keep flags (torch's own dropout in the DeepGCN nets), by oracle site."""
    lengths = b["lengths"]
    N, M = sum(lengths), len(model.present)
    tape, keep = dropout_tape_from_tap(draws, model, lengths, int(b["textf"].shape[0]), PREFIX)
    tape.masks.update(extra or {})
    kept = float(torch.cat([m.reshape(-1) for m in tape.masks.values()]).mean())
    assert abs(kept - (1.0 - model.dropout)) < 0.02, "kept fraction %.4f at p = %g" % (kept, model.dropout)
    want, grads, probe = _oracle(sd, b, ocfg, tape, loss_of, forward=forward)
    assert logp.shape == want.shape
    lp_err = abs_err(logp, want)
    bad, worst, checked = _grad_misses(dev_grads, grads)
    nflips = 0
    if bad and model.graph_type == 'GDF':
        # some ReLU unit sits within rounding of its kink and the device is on the other linear piece: differentiate THAT piece
        assert len(rtap) == 1, "the fused graph stack did not run (no ReLU tap)"
        flips = relu_flips_from_tap(rtap[0], probe, PREFIX, M, N, keep=keep)
        nflips = sum(len(v) for v in flips.values())
        if flips:
            print("ReLU units evaluated on the device's side of the kink: %s"
                  % {k: [(int(r), int(c), float(probe.pre[k][r, c])) for r, c in v] for k, v in flips.items()})
            want2, grads, _ = _oracle(sd, b, ocfg, tape, loss_of, flips, forward=forward)
            assert abs_err(want2, want) < 1e-6       # (the forward values do not depend on the side: |pre| < 1e-5)
            bad, worst, checked = _grad_misses(dev_grads, grads)
    rec = dict(case=tag, logp_err=lp_err, worst_grad=worst[0], worst_param=worst[1], relu_flips=nflips, gradients=checked)
    if bad or not lp_err < 1e-4 or os.environ.get("MMDFN_REPLAY_F64") == "1":
        # the oracle's own float32-to-float64 distance on the same masks: what "equal" can mean for this case
        w64, g64, _ = _oracle(sd, b, ocfg, tape, loss_of, dtype=torch.float64,
                              forward=forward)
        d = [(rel_err(grads[k], g64[k]), k) for k in grads if grads[k] is not None and g64[k] is not None
             and float(g64[k].abs().max()) >= 1e-6]
        rec.update(f32_f64_logp=abs_err(want, w64), f32_f64_grad=max(d)[0], f32_f64_param=max(d)[1])
    _report(rec)
    assert lp_err < 1e-4, rec
    assert not bad, (bad, rec)
    assert checked >= min_checked, checked
    return rec


def _to_dev(b):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}


def _tapped_forward(model, dv, lengths, torch_masks=None):
    """``torch_masks``: a list; torch.nn.functional.dropout is then replaced for the duration of the forward by x * keep / (1 - p)
    with ``keep`` = the 0 / 1 mask the real function drew, appended to the list (the DeepGCN nets' dropout is torch's)."""
    import torch.nn.functional as F
    real = F.dropout

    def recording(x, p=0.5, training=True, inplace=False):
        if not training or p <= 0:
            return x
        k = (real(torch.ones_like(x), p, True) > 0).to(x.dtype)
        torch_masks.append(k.cpu())
        return x * k * (1.0 / (1.0 - p))
    ops_flags.TAP, gcn_stack.TAP = [], []
    if torch_masks is not None:
        F.dropout = recording
    try:
        logp = model(dv["textf"], dv["qmask"], dv["umask"], lengths, dv["acouf"], dv["visuf"])[0]
    finally:
        F.dropout = real
        draws, ops_flags.TAP = ops_flags.TAP, None
        rtap, gcn_stack.TAP = gcn_stack.TAP, None
    return logp, draws, rtap


def _eager_case(tag, cfg, lengths, p, seed, ragged=False, steps=(0, 1), trace=None, qmask=None, min_checked=44, forward=None,
                torch_sites=None, **model_kw):
    """Eager steps of one model, each checked: step 0 is a model's first (every site draws its own flags: no size hint yet), step 1
    takes the step's flags from one pool, drawn as riders of the first GRU launch.  The loss is sum(logp * w) for a seeded random w;
    the backward pass is the trainer's (train.backward: the weight gradients leave as the step's batch).  ``trace``: a function
    given the kernel names of step 1.  ``torch_sites``: the oracle sites, in call order, of the model's torch.nn.functional.dropout
    calls (see _tapped_forward)."""
    torch.manual_seed(seed)            # (the keep-flag generator follows torch's: the same flags in every run)
    m = synthetic.build_model(dropout=p, **model_kw, **cfg)
    sd = synthetic.seeded_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    b = synthetic.make_batch(seed + 1, ragged=ragged, lengths=lengths, **cfg)
    if qmask is not None:
        b["qmask"] = qmask(b)
    dv = _to_dev(b)
    sw = [float(x) for x in model_kw.get("speaker_weights", "3-0-1").split("-")]
    ocfg = O.default_cfg(cfg["nlayers"], dropout=p, speaker_weights=sw, reason_flag=model_kw.get("reason_flag", True))
    w = torch.from_numpy(np.random.RandomState(seed).randn(sum(b["lengths"]), cfg["C"]).astype(np.float32))
    wd = w.to(DEV)
    recs = []
    for step in range(2):
        m.zero_grad(set_to_none=True)
        prof = None
        if trace is not None and step == 1:
            from torch.profiler import ProfilerActivity, profile
            prof = profile(activities=[ProfilerActivity.CUDA])
            prof.__enter__()
        try:
            tmasks = None if torch_sites is None else []
            logp, draws, rtap = _tapped_forward(m, dv, b["lengths"], tmasks)
            train.backward((logp * wd).sum())
            torch.cuda.synchronize()
        finally:
            if prof is not None:
                prof.__exit__(None, None, None)
        if prof is not None:
            trace([e.key for e in prof.key_averages()])
        if step in steps:
            grads = {k: prm.grad for k, prm in m.named_parameters()}
            extra = None
            if torch_sites is not None:
                assert len(tmasks) == len(torch_sites), "%d torch dropout calls, %d sites" % (len(tmasks), len(torch_sites))
                extra = dict(zip(torch_sites, tmasks))
            recs.append(_compare("%s step %d" % (tag, step), m, sd, b, ocfg, draws, rtap, logp, grads, lambda lp: (lp * w).sum(),
                                 min_checked, forward, extra))
    return m, recs


SMALL = dict(B=3, L=20, P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_small_step_on_replayed_flags(p):
    _eager_case("small p=%g" % p, SMALL, [20, 13, 7], p, 3100 + int(10 * p))


def test_silent_speaker_zero_hot_and_multi_hot_rows_under_dropout():
    cfg = dict(SMALL, B=2, L=9, P=3)
    qm = lambda b: party_qmask([9, 6], 9, 3, 3110)
    q = qm(None)
    assert float(q[:, 1, 2].sum()) == 0 and bool((q.sum(2)[:6, 1] == 0).any()) and bool((q.sum(2) > 1).any())
    _eager_case("silent / zero-hot / multi-hot", cfg, [9, 6], 0.5, 3110, qmask=qm)


def test_all_three_party_encoders_carry_dropout():
    cfg = dict(SMALL, L=12, P=3)
    _eager_case("speaker weights 1-2-0.5", cfg, [12, 5, 8], 0.5, 3120, speaker_weights="1-2-0.5")


def test_four_layer_stack_under_dropout():
    _eager_case("4 layers", dict(SMALL, nlayers=4), [20, 13, 7], 0.5, 3130)


def test_one_and_two_utterance_dialogues_under_dropout():
    _eager_case("lengths 1, 1, 2", dict(SMALL, L=2), [1, 1, 2], 0.5, 3140)


def test_valid_length_party_launches_under_dropout():
    """32 short ragged dialogues of two speakers: 160 sequences, the size at which the party group runs on the valid-length
    (segmented) recurrence launches by default."""
    cfg = dict(SMALL, B=32, L=24)
    lengths = [int(x) for x in np.random.RandomState(3150).randint(3, 25, size=32)]
    lengths[5] = 24
    assert fused.wants_truncation(32 + 2 * 32 * 2) and fused.TRUNCATE == "auto"
    _eager_case("valid-length party launches", cfg, lengths, 0.5, 3150, steps=(1,))


def _forms(expect, absent):
    def check(names):
        for want in expect:
            assert any(want in n for n in names), "%s did not run: %s" % (want, sorted(names))
        for no in absent:
            assert not any(no in n for n in names), "%s ran: the form this case covers is off" % no
    return check


# the launch forms the benchmark-size cases are there to cover, by kernel name (a default switched off later fails here
# instead of silently removing the coverage): the flags drawn as riders of the first GRU launch (so: no generator launch
# of its own), the party rows stored by the projection launch (no gather launch), the inter-layer dropout inside the
# second layer's projection (no mask-scale launch), the strip-workgroup adjacency
CFG2_FORMS = _forms(["gru_seq_fwd_io_flags_kernel", "linear_planes_group_kernel", "adj_strip_fwd_kernel", "adj_strip_bwd_kernel",
                     "head_fwd_kernel"], ["keep_flags_kernel", "party_gather_kernel", "mask_scale_kernel"])
# cfg3: 1 216 sequence-directions take the MFMA recurrence (its own flag-rider form); its party projection has too few
# rows for the plane form, so the gather launch stays (profiles/r07_absorbed_launches.md)
CFG3_FORMS = _forms(["gru_seq_fwd_mfma_flags_kernel", "gru_seq_bwd_mfma", "adj_strip_fwd_kernel", "head_fwd_kernel"],
                    ["keep_flags_kernel", "mask_scale_kernel"])


@pytest.mark.parametrize("cfgname,ragged", [("cfg2", False), ("cfg2", True), ("cfg3", True)],
                         ids=["cfg2", "cfg2-ragged", "cfg3-ragged"])
def test_benchmark_size_step_on_replayed_flags(cfgname, ragged):
    """The benchmark's own setting (p = 0.5) at its batch sizes, second step of the model, with the launch forms asserted
    from a kernel trace of that same step."""
    cfg = dict(synthetic.CONFIGS[cfgname])
    seed = 3200 + 10 * list(synthetic.CONFIGS).index(cfgname) + int(ragged)
    _eager_case("%s%s" % (cfgname, " ragged" if ragged else ""), cfg, None, 0.5, seed, ragged=ragged, steps=(1,),
                trace=CFG2_FORMS if cfgname == "cfg2" else CFG3_FORMS)


@pytest.mark.parametrize("case", ["small", "cfg2"])
def test_captured_step_on_replayed_flags(case):
    """graphs.CapturedStep as bench.py builds it (FocalLoss, train.backward), captured with the taps set: the tapped tensors
    are the ones every replay rewrites.  After each of two replays the flags, log-probs and gradients are read back and
    compared with the oracle on those flags; the two replays drew different flags."""
    from mm_dfn_amd.graphs import CapturedStep
    if case == "small":
        cfg, lengths, seed = SMALL, [20, 13, 7], 3300
    else:
        cfg, lengths, seed = dict(synthetic.CONFIGS["cfg2"]), None, 3310
    torch.manual_seed(seed)
    m = synthetic.build_model(dropout=0.5, **cfg)
    sd = synthetic.seeded_state_dict(m.state_dict(), seed)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    b = synthetic.make_batch(seed + 1, lengths=lengths, **cfg)
    dv = _to_dev(b)
    label = train.flatten_labels(dv["label"], b["lengths"])
    label_cpu = O.flatten_labels(b["label"], b["lengths"])
    loss_f = FocalLoss(gamma=0.5)
    last = {}

    def fwd_bwd():
        ops_flags.TAP, gcn_stack.TAP = [], []          # (what is left after the constructor is the capture pass's own)
        logp = m(dv["textf"], dv["qmask"], dv["umask"], b["lengths"], dv["acouf"], dv["visuf"])[0]
        last.update(logp=logp, draws=ops_flags.TAP, rtap=gcn_stack.TAP)
        loss = loss_f(logp, label)
        train.backward(loss)
        return loss

    try:
        cap = CapturedStep(m, fwd_bwd, warmup=2)
    finally:
        ops_flags.TAP = gcn_stack.TAP = None
    try:
        ocfg = O.default_cfg(cfg["nlayers"], dropout=0.5)
        flags, losses = [], []
        for replay in range(2):
            loss = cap.replay()
            torch.cuda.synchronize()
            flags.append(torch.cat([d[2].reshape(-1) for d in last["draws"]]).cpu())
            grads = {k: (cap.grads[k].detach().cpu().clone() if k in cap.grads else None) for k, _ in m.named_parameters()}
            rec = _compare("captured %s replay %d" % (case, replay), m, sd, b, ocfg, last["draws"], last["rtap"],
                           last["logp"].detach().cpu().clone(), grads, lambda lp: O.focal_loss(lp, label_cpu, 0.5))
            losses.append(float(loss.detach()))
        differ = float((flags[0] != flags[1]).float().mean())
        assert 0.4 < differ < 0.6, "two replays of p = 0.5 flags differ in %.3f of their positions" % differ
        assert losses[0] != losses[1]
    finally:
        cap.close()


def _make_gru(seed):
    g = torch.nn.GRU(200, 100, num_layers=2, bidirectional=True)
    g.load_state_dict(synthetic.seeded_state_dict(g.state_dict(), seed, scale=1.5))
    return g


@pytest.mark.parametrize("shapes", [[(7, 3)], [(1, 5)], [(110, 16), (110, 96)], [(33, 40), (33, 700)], [(20, 300)],
                                    [(12, 1), (5, 2), (9, 130)]])
def test_bigru2_training_dropout_forward_backward(shapes):
    """gru.bigru2 with training=True, p = 0.5 against O.bigru2 on the tapped flags, at the shape sets and the bounds of
    test_gru_gpu.test_bigru2_forward_backward (5-wave, lane-pair and MFMA dispatch).  Second call inside one flag-pool key:
    the flags are slices of the pool the first GRU launch's riders drew."""
    p = 0.5
    torch.manual_seed(len(shapes) * 100 + shapes[0][0] + 7)
    rs = np.random.RandomState(len(shapes) * 100 + shapes[0][0] + 7)
    grus = [_make_gru(150 + i) for i in range(len(shapes))]
    xs = [torch.from_numpy(rs.randn(T, R, 200).astype(np.float32)) for T, R in shapes]
    ws = [torch.from_numpy(rs.randn(T, R, 200).astype(np.float32)) for T, R in shapes]
    gd = [g.to(DEV) for g in grus]
    for call in range(2):
        for g in gd:
            g.zero_grad(set_to_none=True)
        xg = [x.to(DEV).requires_grad_(True) for x in xs]
        ops_flags.TAP = []
        try:
            with ops.flag_pool(("bigru2-test", tuple(shapes))):
                ys = fused.bigru2(xg, gd, p, True)
        finally:
            draws, ops_flags.TAP = ops_flags.TAP, None
        sum((y * w.to(DEV)).sum() for y, w in zip(ys, ws)).backward()
    assert [(d[0], d[3]) for d in draws] == [(T * R * 200, "gru") for T, R in shapes]
    masks = [d[2].detach().cpu().view(T, R, 200) for d, (T, R) in zip(draws, shapes)]
    for mk in masks:
        assert bool(((mk == 0) | (mk == 1)).all()) and abs(float(mk.mean()) - 0.5) < 0.05
    for i, (g, x, w) in enumerate(zip(grus, xs, ws)):
        params = {"g." + k: v.detach().cpu().clone().requires_grad_(True) for k, v in g.state_dict().items()}
        xo = x.clone().requires_grad_(True)
        tape = O.DropoutTape({"g%d" % i: masks[i]})
        prev = O.set_dropout_tape(tape)
        try:
            y = O.bigru2(xo, params, "g.", p, True, engine="manual", site="g%d" % i)
        finally:
            O.set_dropout_tape(prev)
        check_tape_consumed(tape)
        (y * w).sum().backward()
        assert abs_err(ys[i], y) < 2e-6
        assert rel_err(xg[i].grad, xo.grad) < 2e-5
        for k, prm in gd[i].named_parameters():
            assert rel_err(prm.grad, params["g." + k].grad) < 5e-5, k


def test_graph_free_baseline_on_replayed_flags():
    """graph_type='None' with concat_subsequently at p = 0.5: the encoders' dropout and the ReLU-free head's mask (no graph
    stack, so no stack draw -- the helper insists on that)."""
    from test_fusion_baselines import CFG
    _eager_case("graph-free concat_subsequently", CFG, [14, 5, 9], 0.5, 3400, min_checked=40, forward=O.forward_graph_free,
                graph_type="None", att_type="concat_subsequently", reason_flag=False)


def test_deepgcn_sibling_on_replayed_flags():
    """graph_type='DeepGCN' (three unimodal GCNII nets, concat_subsequently) at p = 0.5 against O.forward_deepgcn.  The
    encoders and the head draw keep flags; the nets' own dropout (x, h0, one behind the layer loop) is torch's, recorded
    from the device run call by call.  The oracle has no ReLU probe on this path: every gradient has to agree as it is."""
    from test_oracle_golden import DEEP_CFG, DEEP_LENGTHS
    sites = ["graph_net_%s.%s" % (k, s) for k in "avl" for s in ("x", "h0", "out")]
    _eager_case("DeepGCN concat_subsequently", DEEP_CFG, DEEP_LENGTHS, 0.5, 3410, forward=O.forward_deepgcn, torch_sites=sites,
                graph_type="DeepGCN", att_type="concat_subsequently")
