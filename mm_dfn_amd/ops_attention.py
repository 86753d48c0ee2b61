"""Matching attention over a dialogue (K14).

Part of the operator layer over the C-ABI kernels (libmmdfn_hip.so); `mm_dfn_amd.ops` re-exports every name.
Every function launches hand-written gfx950 kernels on the current HIP stream; there is no CPU / eager fallback.
"""
import torch

from . import _hip


def _operand(t):
    """Contiguous fp32 rows on a 16-byte boundary (the kernels fetch them in 16-byte units)."""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def matching_attention_supported(Tq, L, B, D):
    return int(_hip.query("mmdfn_match_att_workspace", int(Tq), int(L), int(B), int(D))) >= 0


class _MatchingAttention(torch.autograd.Function):
    """(X (Tq, B, D), M (L, B, D), mask (B, L)) -> (pool (Tq, B, D), alpha (Tq, B, L)); csrc/matching_attention.hip: one
    launch forward, two backward.  ``alpha`` is an output for the caller and is not differentiated through."""

    @staticmethod
    def forward(ctx, X, M, mask):
        _hip.require_cuda(X, M, mask)
        _hip.require_f32(X, M, mask)
        if X.dim() != 3 or M.dim() != 3 or mask.dim() != 2:
            raise ValueError("matching_attention: X (Tq, B, D), M (L, B, D), mask (B, L)")
        Tq, B, D = X.shape
        L = M.shape[0]
        if tuple(M.shape[1:]) != (B, D) or tuple(mask.shape) != (B, L):
            raise ValueError("matching_attention: X %s, M %s and mask %s do not belong together"
                             % (tuple(X.shape), tuple(M.shape), tuple(mask.shape)))
        if not matching_attention_supported(Tq, L, B, D):
            raise ValueError("matching_attention: serves D %% 4 == 0, 4 <= D <= %d, 1 <= L <= %d, 1 <= B <= 65535, Tq >= 1; "
                             "got Tq = %d, L = %d, B = %d, D = %d" % (_hip.query("mmdfn_match_att_max_width"),
                                                                   _hip.query("mmdfn_match_att_max_len"), Tq, L, B, D))
        X, M, mask = _operand(X), _operand(M), mask.contiguous()
        pool = torch.empty(Tq, B, D, dtype=torch.float32, device=X.device)
        alpha = torch.empty(Tq, B, L, dtype=torch.float32, device=X.device)
        aux = torch.empty(Tq, B, L, dtype=torch.float32, device=X.device)
        _hip.call("mmdfn_match_att_fwd", _hip.ptr(X), _hip.ptr(M), _hip.ptr(mask), _hip.ptr(pool), _hip.ptr(alpha),
                  _hip.ptr(aux), Tq, L, B, D, _hip.stream())
        ctx.save_for_backward(X, M, mask, alpha, aux)
        ctx.mark_non_differentiable(alpha)
        return pool, alpha

    @staticmethod
    def backward(ctx, dpool, _dalpha):
        X, M, mask, alpha, aux = ctx.saved_tensors
        Tq, B, D = X.shape
        L = M.shape[0]
        dpool = _operand(dpool)
        dX = torch.empty_like(X)
        dM = torch.empty_like(M)
        ws = torch.empty(int(_hip.query("mmdfn_match_att_workspace", Tq, L, B, D)), dtype=torch.float32, device=X.device)
        _hip.call("mmdfn_match_att_bwd", _hip.ptr(dpool), _hip.ptr(X), _hip.ptr(M), _hip.ptr(mask), _hip.ptr(alpha),
                  _hip.ptr(aux), _hip.ptr(dX), _hip.ptr(dM), _hip.ptr(ws), Tq, L, B, D, _hip.stream())
        return dX, dM, None


def matching_attention(X, M, mask):
    """The reference's ``MatchingAttention(att_type='general2')`` (model.py:66-76,84) for every query row of ``X`` at once:
    ``alpha[t, b, :] = softmax-like weights of exp(tanh(<X[t, b], M[s, b]>))`` over the keys the mask keeps, renormalised;
    ``pool[t, b] = sum_s alpha[t, b, s] M[s, b]``.  X (Tq, B, D), M (L, B, D), mask (B, L) fp32; returns pool (Tq, B, D) and
    alpha (Tq, B, L) (``alpha.unbind(0)`` is the reference's list of (B, L) tensors).

    The mask is read as "non-zero keeps"; values other than 0 / 1 are outside the contract (the reference multiplies by
    them).  Where it differs from the reference: a dialogue whose mask row is all zero gives zero ``pool`` / ``alpha`` and zero
    gradients (the reference: 0 / 0 = NaN).  ``alpha`` carries no gradient.  Shapes the kernel does not serve raise ValueError."""
    _hip.require_cuda(X, M, mask)
    return _MatchingAttention.apply(X, M, mask)
