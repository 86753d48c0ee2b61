"""MatchingAttention (reference model.py:32-85) on the fused all-pairs kernel (csrc/matching_attention.hip, K14).

Same constructor, parameter names (``transform.weight`` / ``transform.bias``), ``forward(M, x, mask=None)`` signature and
return shapes as the reference.  ``att_type='general2'`` -- the masked tanh form the recurrent baselines use -- is the one
built; the other types raise NotImplementedError.
"""
import torch
import torch.nn as nn

from . import ops


class MatchingAttention(nn.Module):

    def __init__(self, mem_dim, cand_dim, alpha_dim=None, att_type='general'):
        super().__init__()
        assert att_type != 'concat' or alpha_dim is not None
        assert att_type != 'dot' or mem_dim == cand_dim
        if att_type != 'general2':
            raise NotImplementedError("MatchingAttention: att_type %r is not implemented (reference model.py:58-65,77-82); "
                                      "'general2' (model.py:66-76) is" % (att_type,))
        self.mem_dim = mem_dim
        self.cand_dim = cand_dim
        self.att_type = att_type
        self.transform = nn.Linear(cand_dim, mem_dim, bias=True)

    @staticmethod
    def _mask(M, mask):
        if mask is None:
            return torch.ones(M.shape[1], M.shape[0], dtype=torch.float32, device=M.device)
        return mask if mask.dtype == torch.float32 else mask.to(torch.float32)

    def forward(self, M, x, mask=None):
        """M (seq_len, batch, mem_dim), x (batch, cand_dim), mask (batch, seq_len) of 0 / 1 -> attn_pool (batch, mem_dim),
        alpha (batch, 1, seq_len): one query per dialogue (the kernel with Tq = 1).  A dialogue whose mask row is all zero gives
        zeros (the reference: NaN); mask values other than 0 / 1 are outside the contract ("non-zero keeps")."""
        q = ops.linear(x, self.transform.weight, self.transform.bias)
        pool, alpha = ops.matching_attention(q.unsqueeze(0), M, self._mask(M, mask))
        return pool[0], alpha[0].unsqueeze(1)

    def forward_all(self, M, mask=None):
        """Every timestep of ``M`` as a query (what the reference's models loop over, model.py:306-309) in ONE launch:
        pool (seq_len, batch, mem_dim) and alpha (seq_len, batch, seq_len), alpha[t] being the (batch, seq_len) weights of query
        t.  Needs cand_dim == mem_dim."""
        if self.cand_dim != self.mem_dim:
            raise ValueError("MatchingAttention.forward_all: the memory is its own query, cand_dim must equal mem_dim")
        q = ops.linear(M, self.transform.weight, self.transform.bias)
        return ops.matching_attention(q, M, self._mask(M, mask))
