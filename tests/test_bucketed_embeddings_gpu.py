"""StepGraphCache(bucket_rows=g) on a DialogueGNNModel with use_speaker=True, use_modal=True -- the constructor default plus the
training script's other embedding flag -- and with either script objective: the pattern of
tests/test_trainer_gpu.py::test_bucketed_step_cache_serves_unseen_length_tuples with that test's own bounds."""
import pytest
import torch

from mm_dfn_amd import FocalLoss, NLLLoss, synthetic
from mm_dfn_amd import train as T

pytestmark = pytest.mark.gpu
CFGS = {"small": (dict(P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512), 8),
        "meld": (dict(P=9, C=7, nlayers=3, D_t=100, D_a=100, D_v=512), 16)}
TUPLES = [[23, 9, 17], [23, 17, 9], [19, 23, 4], [23, 2, 21], [8, 15, 23], [23, 23, 1], [23, 12, 12], [23, 11, 15], [5, 23, 6]]
TABLES = ("graph_model.speaker_embeddings.weight", "graph_model.modal_embeddings.weight")


def _eager_step(m, loss_f, b):
    m.zero_grad(set_to_none=True)
    logp = m(b["textf"], b["qmask"], b["umask"], b["lengths"], b["acouf"], b["visuf"])[0]
    flat = T.flatten_labels(b["label"], b["lengths"])
    loss = loss_f(logp, flat)
    T.backward(loss)
    return float(loss), logp.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _run(cfg_name, make_loss):
    cfg, g = CFGS[cfg_name]
    L, B = 23, 3
    m = synthetic.build_model(dropout=0.0, use_speaker=True, use_modal=True, **cfg)
    assert m.graph_model.use_speaker and m.graph_model.use_modal
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), 31))
    m = m.cuda().train()
    loss_f = make_loss(cfg["C"])
    cache = T.StepGraphCache(m, loss_f, bucket_rows=g, larger_bucket_fallback=False)    # (every bucket gets its own entry)
    keys = set()
    for i, lengths in enumerate(TUPLES):
        b = synthetic.make_batch(60 + i, lengths=lengths, device="cuda", B=B, L=L, **cfg)
        want_loss, want_logp, want_g = _eager_step(m, loss_f, b)
        assert set(TABLES) <= set(want_g)
        loss, logp, flat = cache.step((b["textf"], b["visuf"], b["acouf"], b["qmask"], b["umask"], b["label"]), lengths, True)
        N = sum(lengths)
        assert tuple(logp.shape) == (N, cfg["C"]) and tuple(flat.shape) == (N,)
        assert torch.equal(flat, T.flatten_labels(b["label"], lengths))
        assert torch.equal(logp, want_logp), float((logp - want_logp).abs().max())
        assert abs(float(loss) - want_loss) < 2e-6 * max(1.0, abs(want_loss))
        got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        assert set(got) == set(want_g) and set(TABLES) <= set(got)
        for k in want_g:
            den = float(want_g[k].abs().max())
            assert float((got[k] - want_g[k]).abs().max()) <= 2e-5 * den + 1e-9, (k, lengths)
        keys.add(((N + 1 + g - 1) // g) * g)
    assert all(k[0] == "bucket" for k in cache.entries)
    assert cache.misses == len(keys) < len(TUPLES) and cache.hits == len(TUPLES) - len(keys)


@pytest.mark.parametrize("cfg_name", ["small", "meld"])
def test_bucketed_step_cache_serves_models_with_speaker_and_modality_embeddings(cfg_name):
    _run(cfg_name, lambda C: FocalLoss(gamma=0.5))


def test_bucketed_step_cache_takes_the_nll_objective():
    """mm_dfn_amd.loss.NLLLoss(weight=w), ignore_index = torch's default = StepGraphCache.IGNORE: stepped as it is."""
    _run("small", lambda C: NLLLoss(weight=torch.linspace(0.5, 1.5, C)))
