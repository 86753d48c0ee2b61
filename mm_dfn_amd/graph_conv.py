"""GraphConvolution (GCNII layer) and GCNII_lyc (GCNII stack with the LSTM
"dynamic fusion" gate) -- drop-in counterparts of reference model_GCN.py:157-189
and :412-488 with the same constructor / forward signatures and state_dict keys.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.parameter import Parameter

from . import _hip, gcn_stack, ops
from .layout import BlockTileAdjacency


class GraphConvolution(nn.Module):
    """out = theta * [A.x || h0] W + (1-theta) * ((1-alpha) A.x + alpha h0)   (variant=True)."""

    def __init__(self, in_features, out_features, residual=False, variant=False):
        super().__init__()
        self.variant = variant
        self.in_features = 2 * in_features if variant else in_features
        self.out_features = out_features
        self.residual = residual
        self.weight = Parameter(torch.empty(self.in_features, self.out_features))
        self.reset_parameters()

    def reset_parameters(self):
        bound = 1.0 / math.sqrt(self.out_features)
        with torch.no_grad():
            self.weight.uniform_(-bound, bound)

    def forward(self, input, adj, h0, lamda, alpha, l):
        _hip.require_cuda(input)                      # MI355X path only: no CPU fallback
        theta = math.log(lamda / l + 1)
        if isinstance(adj, BlockTileAdjacency):
            hi = ops.propagate(adj, input)           # HIP K6
        else:
            hi = ops.matmul_kn(adj, input)           # caller supplied a dense matrix: the package's MFMA product, no library GEMM
        if self.variant:
            support = torch.cat([hi, h0], 1)
            r = (1 - alpha) * hi + alpha * h0
        else:
            support = (1 - alpha) * hi + alpha * h0
            r = support
        out = theta * ops.matmul_kn(support, self.weight) + (1 - theta) * r
        if self.residual:
            out = out + input
        return out


def con_width(convs):
    """Output width of the (uniform) layer stack."""
    return convs[0].out_features


class GCNII_lyc(nn.Module):
    def __init__(self, nfeat, nlayers, nhidden, nclass, dropout, lamda, alpha, variant, return_feature, use_residue,
                 new_graph=False, reason_flag=False):
        super().__init__()
        self.return_feature = return_feature
        self.use_residue = use_residue
        self.new_graph = new_graph
        self.convs = nn.ModuleList([GraphConvolution(nhidden, nhidden, variant=variant) for _ in range(nlayers)])
        self.fcs = nn.ModuleList([nn.Linear(nfeat, nhidden)])
        if not return_feature:
            self.fcs.append(nn.Linear(nfeat + nhidden, nclass))
        self.act_fn = nn.ReLU()
        self.dropout = dropout
        self.alpha = alpha
        self.lamda = lamda
        self.rnn_layer = 1
        self.rnn = nn.LSTM(nhidden, nhidden, self.rnn_layer)   # one cell shared by all layers, seq_len 1
        self.reason_flag = reason_flag

    def _gate(self, q, h, c):
        """One LSTM-cell step (gate order i, f, g, o), state carried layer to layer."""
        g = ops.linear(q, self.rnn.weight_ih_l0, self.rnn.bias_ih_l0) + ops.linear(h, self.rnn.weight_hh_l0,
                                                                                  self.rnn.bias_hh_l0)
        i, f, gg, o = g.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        return h, c

    def forward(self, x, dia_len, topicLabel, adj=None, test_label=False):
        if adj is None:
            if self.new_graph:
                raise NotImplementedError("GCNII_lyc(new_graph=True) without an explicit adjacency (reference "
                                          "model_GCN.py:446-447) is not built inside forward: build the window graph with "
                                          "self.message_passing_relation_graph(x, dia_len) and pass it as adj=")
            # message_passing_wo_speaker (model_GCN.py:490-511): the M = 1 arccos graph, normalised per dialogue -- on a
            # block-diagonal matrix that is D^-1/2 A D^-1/2 of the whole
            _hip.require_cuda(x)
            adj = ops.build_adjacency(x.unsqueeze(0), [int(n) for n in dia_len], kind='arccos')
            x = adj.stacked_feats[0]                  # the tensor the adjacency gradient flows back through
        _hip.require_cuda(x)                          # MI355X path only: no CPU fallback
        fused = isinstance(adj, BlockTileAdjacency) and all(c.variant and not c.residual for c in self.convs)
        dump = self._dump_layer if test_label else None
        return self._forward_fused(x, adj, dump) if fused else self._forward_generic(x, adj, dump)

    # the two sparse graphs of new_graph=True, under the reference's names and arguments (model_GCN.py:523-584; GCNII has the
    # same two, :348-409).  Both return a BlockTileAdjacency that forward(..., adj=adj) takes; they are constants for autograd
    # (the reference computes every weight with math.acos on a Python float).
    window_size = 10

    def message_passing_relation_graph(self, x, dia_len):
        """Context window: the reference joins all pairs inside [k - window_size, k + window_size] for every k; the union of
        those cliques is the band |p - q| <= 2 window_size."""
        _hip.require_cuda(x)
        lengths = [int(n) for n in dia_len]
        return ops.build_band_adjacency(x, lengths, ops.window_keys(lengths, x.device), 2 * self.window_size)

    def message_passing_directed_speaker(self, x, dia_len, qmask):
        """Speaker chains: every utterance is joined to the previous and the next one of its own chain (chain 0: speaker 0,
        chain 1: everyone else).  qmask: (dialogue, position, speaker)."""
        _hip.require_cuda(x, qmask)
        lengths = [int(n) for n in dia_len]
        return ops.build_band_adjacency(x, lengths, ops.speaker_keys(qmask, lengths), 1)

    # the reference's --test_label activation dump (model_GCN.py:474-480): every layer's output (after dropout and the
    # residual q) is printed and saved as <test_output_dir>/1080_v1_test_output_layer_<i>.npy.  The dump needs the
    # per-layer tensors, so a forward with test_label=True takes the op-by-op path instead of the fused stack node.
    test_output_dir = "../outputs/iemocap/"

    def _dump_layer(self, i, cur):
        import os
        import numpy as np
        print('# deepGCN layer ' + str(i))
        print(cur.size())
        os.makedirs(self.test_output_dir, exist_ok=True)
        np.save(os.path.join(self.test_output_dir, "1080_v1_test_output_layer_{}".format(i)), cur.detach().cpu().numpy())

    # where the reference applies dropout around the layer loop: GCNII_lyc after every layer (model_GCN.py:470),
    # GCNII once after the loop (model_GCN.py:273-278, the per-layer call is commented out there)
    inner_dropout = True
    final_dropout = False

    def _dropout_mask(self, like):
        """Keep-mask already scaled by 1/(1-p) (one launch), or None when dropout is inactive."""
        if not self.training or self.dropout <= 0:
            return None
        return F.dropout(torch.ones_like(like), self.dropout, True)

    def _forward_stack(self, x, adj):
        """Dialogue-graph sizes: the whole stack as one autograd node of fused kernels (gcn_stack.py)."""
        R, nfeat = x.shape
        H = con_width(self.convs)
        masks, mscale = None, 1.0
        if self.training and self.dropout > 0:
            # the 0 / 1 keep flags of x, h0 and every layer: one slice of the step's flag pool; the kernels scale by 1/(1-p)
            masks = ops.keep_flags(R * nfeat + (1 + len(self.convs)) * R * H, self.dropout, x.device, site="stack")
            mscale = ops.keep_scale(self.dropout)
        cur = gcn_stack.gcn_stack(x, adj, masks, mscale, self.lamda, self.alpha, self.reason_flag, self.use_residue,
                                  self.fcs[0].weight, self.fcs[0].bias, self.rnn, [c.weight for c in self.convs])
        if not self.return_feature:
            cur = F.log_softmax(ops.linear(cur, self.fcs[-1].weight, self.fcs[-1].bias), dim=1)
        return cur

    def _stack_params(self):
        ps = [self.fcs[0].weight, self.fcs[0].bias] + [c.weight for c in self.convs]
        if self.reason_flag:
            ps += [self.rnn.weight_ih_l0, self.rnn.weight_hh_l0, self.rnn.bias_ih_l0, self.rnn.bias_hh_l0]
        return ps

    def _forward_fused(self, x, adj, dump=None):
        """MI355X path.  Dialogue-graph sizes: one fused autograd node (gcn_stack.py).  Long-dialogue batches (~10^5
        rows) and non-leaf parameters: per layer = gate GEMM(s) + fused LSTM-cell kernel + propagate (writes
        [A.x | h0] in place) + support GEMM + fused GCNII update kernel."""
        if (dump is None and self.inner_dropout and not self.final_dropout
                and gcn_stack.eligible(x, x.shape[1], con_width(self.convs), len(self.convs), self._stack_params(), self.lamda)):
            return self._forward_stack(x, adj)
        x = F.dropout(x, self.dropout, training=self.training)
        h0 = ops.linear(x, self.fcs[0].weight, self.fcs[0].bias, act=1)      # Linear + ReLU fused
        cur = F.dropout(h0, self.dropout, training=self.training)
        h = c = None
        if self.reason_flag:
            w_ih, w_hh = self.rnn.weight_ih_l0, self.rnn.weight_hh_l0
            b_ih, b_hh = self.rnn.bias_ih_l0, self.rnn.bias_hh_l0
            bsum = (b_ih + b_hh).detach()      # the gate op routes the (shared) bias gradient to both parameters
        masks = None
        if self.inner_dropout and self.training and self.dropout > 0:
            # the keep-masks of all layers in one fill + one dropout launch (already scaled by 1/(1-p))
            masks = F.dropout(torch.ones(len(self.convs), h0.shape[0], con_width(self.convs), dtype=h0.dtype,
                                         device=h0.device), self.dropout, True)
        for i, con in enumerate(self.convs):
            q = cur
            if self.reason_flag:
                G = ops.gate_linear(q, h, w_ih, w_hh, bsum, b_ih, b_hh)
                h, c = ops.lstm_pointwise(G, c)
                cur = h
            theta = math.log(self.lamda / (i + 1) + 1)
            S2 = ops.propagate_concat(adj, cur, h0)
            P = ops.matmul_kn(S2, con.weight)
            cur = ops.gcnii_combine(P, S2, q if self.reason_flag else None, None if masks is None else masks[i], theta,
                                    self.alpha)
            if dump is not None:
                dump(i, cur)
        if self.final_dropout:
            cur = F.dropout(cur, self.dropout, training=self.training)
        if self.use_residue:
            cur = torch.cat([x, cur], dim=-1)
        if not self.return_feature:
            cur = F.log_softmax(ops.linear(cur, self.fcs[-1].weight, self.fcs[-1].bias), dim=1)
        return cur

    def _forward_generic(self, x, adj, dump=None):
        """Literal op-by-op composition (dense adjacency tensors, non-variant / residual layers)."""
        x = F.dropout(x, self.dropout, training=self.training)
        h0 = ops.linear(x, self.fcs[0].weight, self.fcs[0].bias, act=1)      # Linear + ReLU (hand-written kernels here too)
        cur = F.dropout(h0, self.dropout, training=self.training)
        h = torch.zeros_like(cur)
        c = torch.zeros_like(cur)
        for i, con in enumerate(self.convs):
            q = cur
            if self.reason_flag:
                h, c = self._gate(q, h, c)
                cur = h
            cur = self.act_fn(con(cur, adj, h0, self.lamda, self.alpha, i + 1))
            if self.inner_dropout:
                cur = F.dropout(cur, self.dropout, training=self.training)
            if self.reason_flag:
                cur = cur + q
            if dump is not None:
                dump(i, cur)
        if self.final_dropout:
            cur = F.dropout(cur, self.dropout, training=self.training)
        if self.use_residue:
            cur = torch.cat([x, cur], dim=-1)
        if not self.return_feature:
            cur = F.log_softmax(ops.linear(cur, self.fcs[-1].weight, self.fcs[-1].bias), dim=1)
        return cur


class GCNII(GCNII_lyc):
    """The unimodal sibling used by graph_type='DeepGCN' (reference model_GCN.py:224-310): same layer stack and
    LSTM-cell gate as GCNII_lyc, but it builds its own single-modality adjacency from the node features
    (create_big_adj, :288-310 -- the M = 1 case of the block-tile builder: one cosine/arccos tile per dialogue, no
    cross-modal diagonals, D^-1/2 A D^-1/2) and applies dropout once after the layer loop instead of per layer."""
    inner_dropout = False
    final_dropout = True

    def create_big_adj(self, x, dia_len):
        return ops.build_adjacency(x.unsqueeze(0), [int(n) for n in dia_len])

    def forward(self, x, dia_len, qmask=None):
        if self.new_graph:
            if qmask is None:
                raise ValueError("GCNII(new_graph=True) builds the speaker-chain graph (model_GCN.py:257-258): it needs qmask")
            adj = self.message_passing_directed_speaker(x, dia_len, qmask)      # a constant: no gradient path through it
        else:
            _hip.require_cuda(x)
            adj = self.create_big_adj(x, dia_len)
            x = adj.stacked_feats[0]            # the tensor the adjacency gradient flows back through
        fused = all(c.variant and not c.residual for c in self.convs)
        return self._forward_fused(x, adj) if fused else self._forward_generic(x, adj.to_dense())
