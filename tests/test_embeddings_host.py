"""Host side of the speaker / modality embeddings and of NLLLoss: what needs no device."""
import pytest
import torch
import torch.nn.functional as F

from mm_dfn_amd import MM_GCN, _hip, synthetic
from mm_dfn_amd import train as T


def test_nll_loss_is_exported_and_equals_torch_on_host_tensors():
    from mm_dfn_amd import NLLLoss
    from mm_dfn_amd.loss import NLLLoss as same
    assert NLLLoss is same
    g = torch.Generator().manual_seed(0)
    logp = torch.log_softmax(torch.randn(12, 6, generator=g), 1).requires_grad_(True)
    target = torch.randint(0, 6, (12,), generator=g)
    target[3] = -100
    w = torch.rand(6, generator=g) + 0.5
    for reduction in ("mean", "sum"):
        for weight in (None, w):
            got = NLLLoss(weight=weight, reduction=reduction)(logp, target)
            want = F.nll_loss(logp, target, weight, ignore_index=-100, reduction=reduction)
            assert torch.equal(got, want)
            assert torch.equal(torch.autograd.grad(got, logp)[0], torch.autograd.grad(want, logp)[0])
    assert torch.equal(NLLLoss(weight=w.tolist(), ignore_index=2)(logp, target.clamp(min=0)),
                       F.nll_loss(logp, target.clamp(min=0), w, ignore_index=2))
    with pytest.raises(NotImplementedError):
        NLLLoss(reduction="none")
    with pytest.raises(ValueError):
        NLLLoss(reduction="batchmean")


def test_forward_stacked_accepts_embedding_models_and_fails_loudly_on_the_cpu():
    """use_speaker is the constructor default: forward_stacked serves it (it used to raise NotImplementedError before looking at
    its arguments); on host tensors the operator refuses through require_cuda, as every other one."""
    for modals, use_speaker, use_modal in (("avl", True, False), ("al", True, True), ("av", False, True)):
        net = MM_GCN(16, 16, 16, 16, 2, 8, 6, 0.0, 0.5, 0.2, True, True, True, n_speakers=2, modals=list(modals),
                     use_speaker=use_speaker, use_modal=use_modal, reason_flag=True)
        feats = torch.randn(len(modals), 5, 16)
        qmask = torch.zeros(3, 2, 2)
        with pytest.raises(_hip.HipLibraryError):
            net.forward_stacked(feats, [3, 2], qmask)
        with pytest.raises(ValueError):
            net.forward_stacked(feats[:1], [3, 2], qmask)
    # forward_streams keeps refusing embeddings
    with pytest.raises(NotImplementedError):
        net.forward_streams(feats, [3, 2], qmask)


def test_operator_argument_checks_need_no_device():
    from mm_dfn_amd import ops_embed
    assert ops_embed._slots("avl") == ([0, 1, 2], 2) and ops_embed._slots("al") == ([0, 2], 1) and ops_embed._slots("av") == ([0, 1], -1)
    assert ops_embed._slots(["v", "l"]) == ([1, 2], 1)
    for bad in ("", "aa", "ax", "avla"):
        with pytest.raises(ValueError):
            ops_embed._slots(bad)


def test_build_model_passes_the_embedding_flags_on():
    cfg = dict(P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)
    m = synthetic.build_model(**cfg)
    assert not m.use_speaker and not m.use_modal and not m.graph_model.use_speaker
    m = synthetic.build_model(use_speaker=True, use_modal=True, **cfg)
    assert m.use_speaker and m.use_modal and m.graph_model.use_speaker and m.graph_model.use_modal


def test_cache_wiring_of_the_loss_objects():
    from mm_dfn_amd import FocalLoss, NLLLoss
    m = torch.nn.Linear(2, 2)
    nll = NLLLoss(weight=torch.ones(6))
    assert T.StepGraphCache(m, nll, bucket_rows=8)._loss_ign is nll                      # ignore_index == IGNORE: as it is
    other = NLLLoss(weight=torch.ones(6), ignore_index=-1, reduction="sum")
    ign = T.StepGraphCache(m, other, bucket_rows=8)._loss_ign
    assert ign is not other and ign.ignore_index == T.StepGraphCache.IGNORE and ign.reduction == "sum" and ign.weight is other.weight
    assert T.StepGraphCache(m, torch.nn.NLLLoss(), bucket_rows=8)._loss_ign is None       # any other object: exact signatures
    assert T.StepGraphCache(m, nll)._loss_ign is None
    assert T.StepGraphCache(m, FocalLoss(gamma=0.5), bucket_rows=8)._loss_ign.ignore_index == T.StepGraphCache.IGNORE
    # a model with embeddings is bucketable now: the decision no longer looks at use_speaker / use_modal
    m.use_speaker = m.use_modal = True
    cache = T.StepGraphCache(m, nll, bucket_rows=8)

    class Fake:
        is_cuda = True
        shape = (23, 3, 4)
    assert cache._bucketable([Fake()] * 6, [23, 9, 17], False)
    assert not cache._bucketable([Fake()] * 6, [20, 9, 17], False)
