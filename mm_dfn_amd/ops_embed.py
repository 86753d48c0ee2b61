"""Speaker / modality embeddings of the graph input on the (M, N, D) modality-major stack (csrc/graph_embed.hip, K11): what
MM_GCN.forward does with per-dialogue qmask slices, an argmax, an nn.Embedding lookup and in-place adds (model_mm.py:78-93), as
one launch each way that reads the speaker indices from device memory."""
import torch

from . import _hip

MODAL_ROW = {'a': 0, 'v': 1, 'l': 2}          # rows of modal_embeddings: by identity, not by slot (model_mm.py:85-93)


def backward_rows():
    """Row groups of a backward workgroup: rows g, g + R, g + 2R, ... are summed by group g, then the groups in order."""
    return int(_hip.query("mmdfn_graph_embed_rows"))


def forward_threads():
    """16-byte lanes of the stack per forward workgroup."""
    return int(_hip.query("mmdfn_graph_embed_threads"))


def max_speakers():
    """Largest speaker table the backward launch sums in LDS; beyond it the operator takes its torch path."""
    return int(_hip.query("mmdfn_graph_embed_max_speakers"))


class _NotCovered(Exception):
    """The launch answered -2 (D % 4 != 0, a pointer off the 16-byte grid, too many speakers): nothing ran."""


def _slots(present):
    present = [k for k in present]
    if not 1 <= len(present) <= 3 or any(k not in MODAL_ROW for k in present) or len(set(present)) != len(present):
        raise ValueError("graph_embeddings: present must name distinct modalities of 'avl', got %r" % (present,))
    rows = [MODAL_ROW[k] for k in present]
    return rows, (present.index('l') if 'l' in present else -1)


class _GraphEmbeddings(torch.autograd.Function):

    @staticmethod
    def forward(ctx, feats, qmask, flat_idx, speaker, modal, rows, l_slot):
        M, N, D = feats.shape
        X = feats.contiguous()
        Y = torch.empty_like(X)
        spk = None
        P = S = LB = 0
        if speaker is not None:
            P, S = int(qmask.shape[-1]), int(speaker.shape[0])
            LB = qmask.numel() // P
            spk = torch.empty(N, dtype=torch.int32, device=X.device)
        rc = _hip.call("mmdfn_graph_embed_fwd", _hip.ptr(X), _hip.ptr(qmask), _hip.ptr(flat_idx), _hip.ptr(speaker),
                       _hip.ptr(modal), _hip.int_array(rows), l_slot, _hip.ptr(Y), _hip.ptr(spk), M, N, D, P, S, LB,
                       _hip.stream(), allow=(-2,))
        if rc == -2:
            raise _NotCovered()
        ctx.rows, ctx.l_slot, ctx.S = rows, l_slot, S
        ctx.tables = (None if speaker is None else tuple(speaker.shape), None if modal is None else tuple(modal.shape))
        ctx.save_for_backward(*([spk] if spk is not None else []))
        return Y

    @staticmethod
    def backward(ctx, dY):
        want_x, want_s, want_m = ctx.needs_input_grad[0], ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        s_shape, m_shape = ctx.tables
        want_s, want_m = want_s and s_shape is not None, want_m and m_shape is not None
        dspk = dmod = None
        if want_s or want_m:
            dY = dY.contiguous()
            M, N, D = dY.shape
            spk = ctx.saved_tensors[0] if s_shape is not None else None
            if want_s:
                dspk = torch.empty(s_shape, dtype=dY.dtype, device=dY.device)
            if want_m:
                dmod = torch.empty(m_shape, dtype=dY.dtype, device=dY.device)
            rc = _hip.call("mmdfn_graph_embed_bwd", _hip.ptr(dY), _hip.ptr(spk), _hip.ptr(dspk), _hip.ptr(dmod),
                           _hip.int_array(ctx.rows), ctx.l_slot, M, N, D, ctx.S, _hip.stream(), allow=(-2,))
            if rc == -2:
                # an upstream gradient off the 16-byte grid (a view somebody built): the sums in torch
                if want_s:
                    dspk = torch.zeros(s_shape, dtype=dY.dtype, device=dY.device).index_add_(0, spk.long(), dY[ctx.l_slot])
                if want_m:
                    dmod = torch.zeros(m_shape, dtype=dY.dtype, device=dY.device)
                    dmod[ctx.rows] = dY.sum(1)
        return (dY if want_x else None), None, None, dspk, dmod, None, None


def _torch_path(feats, qmask, flat_idx, speaker, modal, rows, l_slot):
    """The same adds in torch, in the reference's order (bit-equal; still no host slicing: the speaker index is gathered through
    flat_idx on the device)."""
    out = list(feats.unbind(0))
    if speaker is not None:
        s = torch.argmax(qmask.reshape(-1, qmask.shape[-1]).index_select(0, flat_idx), dim=-1)
        out[l_slot] = out[l_slot] + speaker[s]
    if modal is not None:
        out = [x + modal[r].reshape(1, -1) for x, r in zip(out, rows)]
    return torch.stack(out, 0)


def graph_embeddings(feats, qmask, flat_idx, speaker_weight, modal_weight, present):
    """(M, N, D) stack with the speaker embedding added to 'l' and the modality embeddings added to every modality:
    ``Y[l] = (X[l] + speaker_weight[argmax qmask[flat_idx]]) + modal_weight[2]``, ``Y[m] = X[m] + modal_weight[row(m)]`` (a 0,
    v 1).  ``present``: the stacked modalities in slot order (a subset of 'avl'); ``qmask`` (L, B, P) float, ``flat_idx`` (N,)
    int64 rows t * B + b of the stripped utterances (layout.flat_index; both are needed only with a speaker table and 'l'
    present).  A table that is None -- or the speaker table without 'l' -- is not added and receives no gradient.  Bit-equal to
    the torch adds of MM_GCN.forward; the table gradients are bit-reproducible."""
    _hip.require_cuda(feats, qmask, flat_idx, speaker_weight, modal_weight)
    _hip.require_f32(feats, speaker_weight, modal_weight)
    rows, l_slot = _slots(present)
    if feats.dim() != 3 or feats.shape[0] != len(rows):
        raise ValueError("graph_embeddings expects a (len(present), N, D) stack")
    M, N, D = feats.shape
    if l_slot < 0:
        speaker_weight = None
    if modal_weight is not None and tuple(modal_weight.shape) != (3, D):
        raise ValueError("graph_embeddings: the modality table must be (3, %d)" % D)
    if speaker_weight is not None:
        if qmask is None or flat_idx is None:
            raise ValueError("graph_embeddings: the speaker embedding needs qmask and flat_idx")
        if speaker_weight.dim() != 2 or speaker_weight.shape[1] != D:
            raise ValueError("graph_embeddings: the speaker table must be (S, %d)" % D)
        if qmask.shape[-1] > speaker_weight.shape[0]:
            # nn.Embedding raises for such an index only when a row's maximum happens to sit there
            raise ValueError("graph_embeddings: qmask has %d parties, the speaker table %d rows"
                             % (qmask.shape[-1], speaker_weight.shape[0]))
        if flat_idx.dtype != torch.int64 or tuple(flat_idx.shape) != (N,):
            raise ValueError("graph_embeddings: flat_idx must be (N,) int64")
        _hip.require_f32(qmask)
        qmask, flat_idx = qmask.contiguous(), flat_idx.contiguous()
        speaker_weight = speaker_weight.contiguous()
    else:
        qmask = flat_idx = None
    if speaker_weight is None and modal_weight is None:
        return feats
    if modal_weight is not None:
        modal_weight = modal_weight.contiguous()
    try:
        return _GraphEmbeddings.apply(feats, qmask, flat_idx, speaker_weight, modal_weight, rows, l_slot)
    except _NotCovered:
        return _torch_path(feats, qmask, flat_idx, speaker_weight, modal_weight, rows, l_slot)
