"""GPU: FlatAdam on device-resident step state as the last nodes of a captured training step (graphs.CapturedStep(optimizer=...),
train.StepGraphCache(optimizer=...)) on the small lmf_only model of test_fusion_baselines_gpu (lengths [14, 5, 9], dropout 0)."""
import pytest
import torch

from mm_dfn_amd import FocalLoss, synthetic, train
from mm_dfn_amd.graphs import CapturedStep
from mm_dfn_amd.optim import FlatAdam
from test_fusion_baselines import CFG, build

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS = FocalLoss(gamma=0.5)


def batch(seed, lengths=(14, 5, 9)):
    b = synthetic.make_batch(seed, lengths=list(lengths), device=DEV, **CFG)
    return (b["textf"], b["visuf"], b["acouf"], b["qmask"], b["umask"], b["label"]), list(lengths)


def step_fn(m, inputs, lengths):
    textf, visuf, acouf, qmask, umask, label = inputs
    flat = train.flatten_labels(label, lengths)

    def fwd_bwd():
        loss = LOSS(m(textf, qmask, umask, lengths, acouf, visuf)[0], flat)
        train.backward(loss)
        return loss
    return fwd_bwd


def model():
    return build("lmf_only").to(DEV).train()


def values(m):
    return [p.detach().clone() for p in m.parameters()]


def same_bits(xs, ys):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(xs, ys))


def test_captured_step_with_the_optimizer_inside_equals_the_optimizer_outside():
    def outside():
        m = model()
        fwd_bwd = step_fn(m, *batch(931))
        m.zero_grad(set_to_none=True)
        fwd_bwd()
        opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4)
        opt.bucket.flatten()
        opt._materialise()
        cap = CapturedStep(m, fwd_bwd, warmup=2, bucket=opt.bucket)
        losses = []
        for _ in range(4):
            losses.append(float(cap.replay()))
            opt.step(grads_already_flat=True)
        return losses

    def inside():
        m = model()
        opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4, capturable=True)
        cap = CapturedStep(m, step_fn(m, *batch(931)), warmup=2, optimizer=opt)
        assert opt.t == 0                                # warm-up passes and the capture applied nothing
        losses = [float(cap.replay()) for _ in range(4)]
        assert opt.t == 4
        return losses

    want, got = outside(), inside()
    assert want[0] != want[-1]
    print("LOSSES outside %s inside %s" % (want, got))
    for a, b in zip(got, want):
        assert abs(a - b) <= 2e-5 * abs(b), (got, want)


def test_learning_rate_written_between_replays_takes_effect():
    m = model()
    opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4, capturable=True)
    cap = CapturedStep(m, step_fn(m, *batch(932)), warmup=1, optimizer=opt)
    start = values(m)
    cap.replay()
    moved = values(m)
    assert not same_bits(start, moved)
    opt.param_groups[0]["lr"] = 0.0
    cap.replay()
    cap.replay()
    assert all(torch.equal(a, b) for a, b in zip(values(m), moved))          # frozen ...
    assert opt.t == 3                                                         # ... while the step count advances
    opt.param_groups[0]["lr"] = 1e-2
    cap.replay()
    assert not same_bits(values(m), moved) and opt.t == 4


def test_two_cache_entries_alternating_follow_the_eager_flat_adam_loop():
    batches = [batch(941, (14, 5, 9)), batch(942, (11, 7, 3))]

    def eager():
        m = model()
        opt = FlatAdam(m, lr=1e-3, weight_decay=1e-5)
        fns = [step_fn(m, *b) for b in batches]
        for i in range(6):
            m.zero_grad(set_to_none=True)
            fns[i % 2]()
            opt.step()
        return m

    m0 = eager()
    m1 = model()
    opt = FlatAdam(m1, lr=1e-3, weight_decay=1e-5, capturable=True)
    cache = train.StepGraphCache(m1, LOSS, optimizer=opt)
    for i in range(6):
        inputs, lengths = batches[i % 2]
        cache.step(inputs, lengths, True)
    assert opt.t == 6
    assert len(cache.entries) == 2 and cache.misses == 2 and cache.hits == 4 and cache.recaptures == 0
    for (k, x), (_, y) in zip(m0.named_parameters(), m1.named_parameters()):
        d = (x - y).abs()
        print("DEV %s mean %.3g max %.3g" % (k, float(d.mean()), float(d.max())))
        assert float(d.mean()) < 1e-5, k
        assert float(d.max()) < 1e-3, k
    # the pass loop leaves the update to the graph: one pass over the two batches is two more steps, not four
    loader = [inputs + (["x"],) for inputs, _ in batches]
    train.train_or_eval_graph_model(m1, LOSS, loader, 0, True, opt, False, graph_cache=cache)
    assert opt.t == 8
    # an eval entry is captured without the optimizer
    before = values(m1)
    cache.step(batches[0][0], batches[0][1], False)
    assert opt.t == 8 and same_bits(values(m1), before)


def test_precapture_updates_nothing():
    m = model()
    opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4, capturable=True)
    cache = train.StepGraphCache(m, LOSS, optimizer=opt)
    inputs, lengths = batch(951)
    cache.step(inputs, lengths, True)
    cache.step(inputs, lengths, True)
    snap = [opt.flat_p.clone(), opt.m.clone(), opt.v.clone()]
    assert opt.t == 2
    made = cache.precapture([batch(952, (11, 7, 3))[0], batch(953, (6, 13))[0], inputs])
    assert made == 2 and len(cache.entries) == 3
    assert opt.t == 2 and same_bits([opt.flat_p, opt.m, opt.v], snap)
    cache.step(inputs, lengths, True)                    # enabled again afterwards
    assert opt.t == 3 and not same_bits([opt.flat_p], snap[:1])


def test_nonfinite_gradients_are_skipped_without_touching_the_weights():
    """lmf_only has no graph stack, hence no x / ||x|| (the adjacency's cosine): a zero feature row gives FINITE gradients on the
    device and that batch simply trains (checked first).  So, as the issue allows, the non-finite gradient is made directly: the
    flat bucket is poisoned before an eager ``opt.step(grads_already_flat=True)``; and, through the captured step, by a NaN in a
    feature of the static batch, which makes the loss and with it every gradient NaN inside the graph."""
    m = model()
    opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4, skip_nonfinite=True)
    inputs, lengths = batch(961)
    textf = inputs[0]
    clean = textf.clone()
    cap = CapturedStep(m, step_fn(m, inputs, lengths), warmup=1, optimizer=opt)
    textf[3, 0].zero_()                                  # one utterance's text features
    cap.replay()
    assert opt.skipped_steps == 0 and opt.t == 1 and bool(torch.isfinite(opt.grad_norm))
    assert float(opt.grad_norm) > 0
    # eager, poisoned flat bucket
    snap = [opt.flat_p.clone(), opt.m.clone(), opt.v.clone()]
    opt.bucket.flat[5] = float("nan")
    opt.step(grads_already_flat=True)
    assert opt.skipped_steps == 1 and opt.t == 1 and same_bits([opt.flat_p, opt.m, opt.v], snap)
    # in the graph, poisoned batch
    textf.copy_(clean)
    textf[3, 0, 7] = float("nan")
    loss = cap.replay()
    assert not bool(torch.isfinite(loss))
    assert opt.skipped_steps == 2 and opt.t == 1 and same_bits([opt.flat_p, opt.m, opt.v], snap)
    assert bool(torch.isfinite(opt.flat_p).all()) and not bool(torch.isfinite(opt.grad_norm))
    # the next clean batch trains
    textf.copy_(clean)
    loss = cap.replay()
    assert bool(torch.isfinite(loss)) and opt.t == 2 and opt.skipped_steps == 2
    assert not same_bits([opt.flat_p], snap[:1]) and bool(torch.isfinite(opt.flat_p).all())


def test_state_dict_round_trip_of_a_device_state_optimizer():
    kw = dict(lr=1e-2, weight_decay=1e-4, capturable=True, max_grad_norm=0.05)
    m1 = model()
    fwd1 = step_fn(m1, *batch(971))
    opt1 = FlatAdam(m1, **kw)

    def run(m, fwd, opt, k):
        for _ in range(k):
            m.zero_grad(set_to_none=True)
            fwd()
            opt.step()

    run(m1, fwd1, opt1, 3)
    assert float(opt1.grad_norm) > kw["max_grad_norm"]                      # the clip is active
    weights = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    sd = opt1.state_dict()
    assert sd["step"] == 3
    run(m1, fwd1, opt1, 2)
    # reload into a fresh model / optimizer and continue
    m2 = model()
    m2.load_state_dict(weights)
    fwd2 = step_fn(m2, *batch(971))
    opt2 = FlatAdam(m2, **kw)
    m2.zero_grad(set_to_none=True)
    fwd2()
    opt2.bucket.flatten()                                 # (load_state_dict needs the flat layout)
    opt2.load_state_dict(sd)
    assert opt2.t == 3
    run(m2, fwd2, opt2, 2)
    assert opt2.t == 5 == opt1.t
    assert same_bits(values(m1), values(m2))
    assert same_bits([opt1.m, opt1.v], [opt2.m, opt2.v])
