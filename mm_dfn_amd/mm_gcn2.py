"""MM_GCN2: the original MMGCN dialogue graph + GCNII stack, the graph baseline MM-DFN is compared against
(reference model_mm.py:183-296), with the reference's constructor / forward signatures and state_dict keys.

The graph is the arccos kind of the block-tile builder (ops.build_adjacency(kind='arccos')): acos(0.99999 cos) in radians within
a modality, the constant 0.99999 between the modalities of one utterance, D^-1/2 A D^-1/2.  It is built from the RAW a, v, l,
which are also the inputs of the projections: their two gradient paths meet inside the builder's backward kernel.
There is no LSTM gate in this stack; dropout sits in front of every layer and once more behind the loop.
"""
import math

import torch
import torch.nn as nn

from . import _hip, ops
from .graph_conv import GraphConvolution

CROSS_WEIGHT = 0.99999      # the cross-modal entries of MM_GCN2.create_big_adj (model_mm.py:289)


class MM_GCN2(nn.Module):
    def __init__(self, nfeat, nlayers, nhidden, nclass, dropout, lamda, alpha, variant, return_feature, use_residue,
                 new_graph=False, modals='avl', mm_graph='single'):
        super().__init__()
        if new_graph:
            raise NotImplementedError("MM_GCN2(new_graph=True): message_passing_relation_graph (reference model_mm.py:236-237, "
                                      ":335-380) is a per-edge Python loop outside the block-tile graph kinds")
        if modals != 'avl':
            raise NotImplementedError("MM_GCN2(modals=%r): the reference's 'al' branch stacks 2N rows (model_mm.py:222-227) and "
                                      "multiplies them by the 3N x 3N graph of create_big_adj (:239, :261); only 'avl' runs" % (modals,))
        if not return_feature:
            raise NotImplementedError("MM_GCN2(return_feature=False): the reference then appends the classifier as fcs[1] "
                                      "(model_mm.py:195-196), which forward applies to l as its projection (:232)")
        self.return_feature = return_feature
        self.use_residue = use_residue
        self.new_graph = new_graph
        self.convs = nn.ModuleList([GraphConvolution(nhidden, nhidden, variant=variant) for _ in range(nlayers)])
        # fcs[0] -> a, fcs[1] -> l, fcs[2] -> v (model_mm.py:230-234)
        self.fcs = nn.ModuleList([nn.Linear(nfeat, nhidden) for _ in range(3)])
        self.act_fn = nn.ReLU()
        self.dropout = dropout
        self.alpha = alpha
        self.lamda = lamda
        self.mm_graph = mm_graph
        self.modals = modals

    def create_big_adj(self, a, v, l, dia_len):
        """The normalised graph as a BlockTileAdjacency (never dense; .to_dense() gives the reference's matrix)."""
        return ops.build_adjacency(torch.stack([a, v, l], 0), [int(n) for n in dia_len], CROSS_WEIGHT, kind='arccos')

    def forward(self, a, v, l, dia_len, topicLabel):
        _hip.require_cuda(a, v, l)                    # MI355X path only: no CPU fallback
        adj = self.create_big_adj(a, v, l, dia_len)
        a, v, l = adj.stacked_feats.unbind(0)         # the tensors the graph's gradient flows back through
        N, nfeat = a.shape
        H = self.convs[0].out_features
        nl = len(self.convs)
        drop = self.training and self.dropout > 0
        a_, l_, v_ = a, l, v
        lmask = [None] * (nl + 1)
        if drop:
            # one slice of the step's flag pool, in the order the reference draws: a, l, v, the input of every layer, the output
            n_in, n_l = N * nfeat, 3 * N * H
            flags = ops.keep_flags(3 * n_in + (nl + 1) * n_l, self.dropout, a.device, site="mm_gcn2")
            scale = ops.keep_scale(self.dropout)
            a_, l_, v_ = ops.mask_scale([a, l, v], [flags[k * n_in:(k + 1) * n_in] for k in range(3)], scale)
            lflags = flags[3 * n_in:].view(nl + 1, 3 * N, H)
            lmask = [lflags[i] for i in range(nl + 1)]
        # the three projections (Linear + ReLU) as one grouped launch of the few-row kernel
        a_, l_, v_ = ops.linear_group([a_, l_, v_], [self.fcs[0].weight, self.fcs[1].weight, self.fcs[2].weight],
                                      [self.fcs[0].bias, self.fcs[1].bias, self.fcs[2].bias], act=1, hip=True)
        h0 = torch.cat([a_, v_, l_], 0)
        cur = h0 if not drop else ops.mask_scale([h0], [lmask[0].reshape(-1)], scale)[0]
        fused = all(c.variant and not c.residual for c in self.convs)
        for i, con in enumerate(self.convs):
            # the dropout in front of layer i + 1 (behind the loop for the last layer) acts on this layer's ReLU output
            if fused:
                theta = math.log(self.lamda / (i + 1) + 1)
                S2 = ops.propagate_concat(adj, cur, h0)
                P = ops.matmul_kn(S2, con.weight)
                cur = ops.gcnii_combine(P, S2, None, lmask[i + 1] * scale if drop else None, theta, self.alpha)
            else:
                cur = self.act_fn(con(cur, adj, h0, self.lamda, self.alpha, i + 1))
                if drop:
                    cur = ops.mask_scale([cur], [lmask[i + 1].reshape(-1)], scale)[0]
        out = cur.view(3, N, H).permute(1, 0, 2).reshape(N, 3 * H)      # cat([F[:N], F[N:2N], F[2N:]], -1) (model_mm.py:252)
        if self.use_residue:
            out = torch.cat([l, out], dim=-1)
        return out
