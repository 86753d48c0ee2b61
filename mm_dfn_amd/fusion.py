"""Secondary fusion modules named by the north star, reference signatures kept:

* ``MFN`` (model_fusion.py:10-120): memory fusion network applied after the GDF graph when
  ``--mm_fusion_mthd mfn`` (model.py:1303-1326).  Non-default.  Every dense product of a timestep (three recurrent
  LSTM projections; the attention and gamma MLPs) is a grouped launch of the few-row MFMA kernel
  (csrc/linear_small.hip, forward and input gradients; weight gradients through the step's gemm_tn batch), the LSTM
  cells run on the fused gate kernel of the GCN stack (csrc/gcn_pointwise.hip) and the attention / memory update on
  csrc/fusion.hip: per step 4 grouped GEMM launches + 3 pointwise launches, no library GEMM.  The three input
  projections are hoisted out of the time loop (one grouped launch for all timesteps).
* ``MMGatedAttention`` ('general', model.py:718-781): unreachable under graph_type='GDF' in the reference
  (shape bug); provided at module level, with the reference's state_dict keys: one grouped launch
  for the three transforms, one fused kernel per modality pair (gate dot product, sigmoid, tanh, blend) each way.
* ``LMF`` (model_fusion.py:214-310): low-rank multimodal fusion, the ``lmf_only`` option of the graph-free model
  (model.py:1394-1395).  The three subnets are one grouped launch, the 3 R products [1, h_m] . factor_m grouped launches into
  column blocks of one buffer, and the rank-weighted product over modalities one fused kernel each way (csrc/lmf.hip).
  As in the reference, ``post_fusion_dropout`` is constructed and never applied.
* ``TFN`` (model_fusion.py:123-211): tensor fusion network, the ``tfn_only`` option of the reference's graph-free model.  The
  three subnets are one grouped launch; the fused tensor [1, h_a] (x) [1, h_v] (x) [1, h_t] (N x 101^3 floats by default),
  its dropout mask and its gradient are never materialised: csrc/tensor_fusion.hip generates the operand inside the three
  products against post_fusion_layer_1's (300, 1 030 301) weight and draws the dropout flags there (``ops.tfn_fuse``).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.init import xavier_normal_

from . import ops


class MFN(nn.Module):
    def __init__(self, d=300, config=None):
        super().__init__()
        self.d_l, self.d_a, self.d_v = d, d, d
        self.dh_l, self.dh_a, self.dh_v = 100, 100, 100
        total_h = self.dh_l + self.dh_a + self.dh_v
        self.mem_dim = 100
        att_in = total_h * 2
        gamma_in = att_in + self.mem_dim
        final_out = total_h + self.mem_dim
        self.lstm_l = nn.LSTMCell(self.d_l, self.dh_l)
        self.lstm_a = nn.LSTMCell(self.d_a, self.dh_a)
        self.lstm_v = nn.LSTMCell(self.d_v, self.dh_v)
        self.att1_fc1 = nn.Linear(att_in, 100)
        self.att1_fc2 = nn.Linear(100, att_in)
        self.att1_dropout = nn.Dropout(0.2)
        self.att2_fc1 = nn.Linear(att_in, 100)
        self.att2_fc2 = nn.Linear(100, self.mem_dim)
        self.att2_dropout = nn.Dropout(0.2)
        self.gamma1_fc1 = nn.Linear(gamma_in, 100)
        self.gamma1_fc2 = nn.Linear(100, self.mem_dim)
        self.gamma1_dropout = nn.Dropout(0.2)
        self.gamma2_fc1 = nn.Linear(gamma_in, 100)
        self.gamma2_fc2 = nn.Linear(100, self.mem_dim)
        self.gamma2_dropout = nn.Dropout(0.2)
        self.out_fc1 = nn.Linear(final_out, 100)      # constructed by the reference, unused in forward
        self.out_fc2 = nn.Linear(100, 1)
        self.out_dropout = nn.Dropout(0.2)

    def forward(self, x):
        """x: (T, n, 3d) -> (T, n, 400) = [h_l | h_a | h_v | mem]."""
        T, n = x.shape[0], x.shape[1]
        cells = (self.lstm_l, self.lstm_a, self.lstm_v)
        parts = (x[:, :, :self.d_l], x[:, :, self.d_l:self.d_l + self.d_a], x[:, :, self.d_l + self.d_a:])
        G = ops.linear_group
        # hoisted input projections of the three cells for all timesteps: one grouped launch, (T, n, 400) each
        gx = G([p.reshape(T * n, p.shape[-1]) for p in parts], [c.weight_ih for c in cells],
               [c.bias_ih + c.bias_hh for c in cells], hip=True)
        gx = [g.view(T, n, -1) for g in gx]
        w_hh = [c.weight_hh for c in cells]
        h = [x.new_zeros(n, 100) for _ in range(3)]
        c = None                                                            # (3 n, 100); None = zero state
        prev_cs = x.new_zeros(n, 300)
        mem = x.new_zeros(n, self.mem_dim)
        hs, mems = [], []
        for t in range(T):
            rec = G(h, w_hh, [None] * 3, hip=True)                           # h_m W_hh_m^T, gate order i, f, g, o
            gates = torch.cat([gx[m][t] + rec[m] for m in range(3)], 0)     # (3 n, 400)
            h_new, c_new = ops.lstm_pointwise(gates, c)
            new_cs = c_new.view(3, n, 100).permute(1, 0, 2).reshape(n, 300)
            c_star = torch.cat([prev_cs, new_cs], 1)
            a1 = self.att1_dropout(G([c_star], [self.att1_fc1.weight], [self.att1_fc1.bias], act=1, hip=True)[0])
            z = G([a1], [self.att1_fc2.weight], [self.att1_fc2.bias], hip=True)[0]
            attended = ops.softmax_scale(z, c_star)
            both = torch.cat([attended, mem], 1)
            y = G([attended, both, both], [self.att2_fc1.weight, self.gamma1_fc1.weight, self.gamma2_fc1.weight],
                  [self.att2_fc1.bias, self.gamma1_fc1.bias, self.gamma2_fc1.bias], act=1, hip=True)
            y = [self.att2_dropout(y[0]), self.gamma1_dropout(y[1]), self.gamma2_dropout(y[2])]
            u, v1, v2 = G(y, [self.att2_fc2.weight, self.gamma1_fc2.weight, self.gamma2_fc2.weight],
                          [self.att2_fc2.bias, self.gamma1_fc2.bias, self.gamma2_fc2.bias], hip=True)
            mem = ops.mfn_mem(u, v1, v2, mem)
            c, prev_cs = c_new, new_cs
            hv = h_new.view(3, n, 100)
            h = [hv[0], hv[1], hv[2]]
            hs.append(hv.permute(1, 0, 2).reshape(n, 300))
            mems.append(mem)
        return torch.cat([torch.stack(hs), torch.stack(mems)], -1)


class MMGatedAttention(nn.Module):
    def __init__(self, mem_dim, cand_dim, att_type='general'):
        super().__init__()
        if att_type != 'general':
            raise NotImplementedError("only att_type='general' is constructed by the reference model (model.py:982)")
        self.mem_dim, self.cand_dim, self.att_type = mem_dim, cand_dim, att_type
        self.dropouta = nn.Dropout(0.5)
        self.dropoutv = nn.Dropout(0.5)
        self.dropoutl = nn.Dropout(0.5)
        self.transform_l = nn.Linear(mem_dim, cand_dim)
        self.transform_v = nn.Linear(mem_dim, cand_dim)
        self.transform_a = nn.Linear(mem_dim, cand_dim)
        self.transform_av = nn.Linear(mem_dim * 3, 1)
        self.transform_al = nn.Linear(mem_dim * 3, 1)
        self.transform_vl = nn.Linear(mem_dim * 3, 1)

    def forward(self, a, v, l, modals=None):
        modals = modals if modals is not None else ['a', 'v', 'l']
        a = self.dropouta(a) if len(a) != 0 else a
        v = self.dropoutv(v) if len(v) != 0 else v
        l = self.dropoutl(l) if len(l) != 0 else l
        xs = {'a': a, 'v': v, 'l': l}
        tr = {'a': self.transform_a, 'v': self.transform_v, 'l': self.transform_l}
        use = [m for m in ('a', 'v', 'l') if m in modals]
        # the transforms' pre-activations in one grouped launch; tanh is applied inside the pair kernel
        pre = dict(zip(use, ops.linear_group([xs[m] for m in use], [tr[m].weight for m in use], [tr[m].bias for m in use],
                                             hip=True)))
        gate = {('a', 'v'): self.transform_av, ('a', 'l'): self.transform_al, ('v', 'l'): self.transform_vl}
        out = [ops.gated_pair(xs[m], xs[n], pre[m], pre[n], g.weight, g.bias)
               for (m, n), g in gate.items() if m in modals and n in modals]
        if len(out) == 1:
            return out[0]
        return torch.cat(out, -1)


class LMF(nn.Module):
    def __init__(self, input_dims=(300, 300, 300), hidden_dims=(300, 300, 300), dropouts=0.4, output_dim=300, rank=4,
                 use_softmax=False):
        super().__init__()
        if use_softmax:
            raise NotImplementedError("LMF(use_softmax=True) is not constructed by the reference model (model.py:1001-1003)")
        self.audio_in, self.video_in, self.text_in = input_dims
        self.audio_hidden, self.video_hidden, self.text_hidden = hidden_dims
        self.audio_subnet = nn.Linear(self.audio_in, self.audio_hidden)
        self.video_subnet = nn.Linear(self.video_in, self.video_hidden)
        self.text_subnet = nn.Linear(self.text_in, self.text_hidden)
        self.output_dim = output_dim
        self.rank = rank
        self.use_softmax = use_softmax
        self.post_fusion_dropout = nn.Dropout(p=dropouts)
        self.audio_factor = nn.Parameter(torch.empty(rank, self.audio_hidden + 1, output_dim))
        self.video_factor = nn.Parameter(torch.empty(rank, self.video_hidden + 1, output_dim))
        self.text_factor = nn.Parameter(torch.empty(rank, self.text_hidden + 1, output_dim))
        self.fusion_weights = nn.Parameter(torch.empty(1, rank))
        self.fusion_bias = nn.Parameter(torch.zeros(1, output_dim))
        for p in (self.audio_factor, self.video_factor, self.text_factor, self.fusion_weights):
            xavier_normal_(p)

    def forward(self, audio_x, video_x, text_x):
        """(N, input_dims[m]) each -> (N, output_dim); N = 1 gives (1, output_dim) as the reference's squeeze / view does."""
        nets = (self.audio_subnet, self.video_subnet, self.text_subnet)
        ha, hv, ht = ops.linear_group([audio_x, video_x, text_x], [n.weight for n in nets], [n.bias for n in nets], hip=True)
        return ops.lmf_fuse(ha, hv, ht, self.audio_factor, self.video_factor, self.text_factor, self.fusion_weights,
                            self.fusion_bias)


class TFN(nn.Module):
    def __init__(self, input_dims=(300, 300, 300), hidden_dims=(100, 100, 100), dropouts=0.4, post_fusion_dim=300, output_dim=300):
        super().__init__()
        self.audio_in, self.video_in, self.text_in = input_dims
        self.audio_hidden, self.video_hidden, self.text_hidden = hidden_dims
        self.post_fusion_dim = post_fusion_dim
        self.post_fusion_prob = dropouts
        self.audio_subnet = nn.Linear(self.audio_in, self.audio_hidden)
        self.video_subnet = nn.Linear(self.video_in, self.video_hidden)
        self.text_subnet = nn.Linear(self.text_in, self.text_hidden)
        self.post_fusion_dropout = nn.Dropout(p=self.post_fusion_prob)
        self.post_fusion_layer_1 = nn.Linear((self.text_hidden + 1) * (self.video_hidden + 1) * (self.audio_hidden + 1),
                                             self.post_fusion_dim)
        self.post_fusion_layer_2 = nn.Linear(self.post_fusion_dim, output_dim)
        self.last_keep_state = None      # the generator state of the latest training-mode forward (ops.tfn_keep_flags)

    def forward(self, audio_x, video_x, text_x):
        """(N, input_dims[m]) each -> (N, output_dim).  ``post_fusion_dropout.p`` is read at call time."""
        nets = (self.audio_subnet, self.video_subnet, self.text_subnet)
        ha, hv, ht = ops.linear_group([audio_x, video_x, text_x], [n.weight for n in nets], [n.bias for n in nets], hip=True)
        l1, l2 = self.post_fusion_layer_1, self.post_fusion_layer_2
        y1 = ops.tfn_fuse(ha, hv, ht, l1.weight, l1.bias, self.post_fusion_dropout.p,
                          self.training and self.post_fusion_dropout.training)
        self.last_keep_state = getattr(y1.grad_fn, "used_state", None)
        return ops.linear_group([y1], [l2.weight], [l2.bias], act=1, hip=True)[0]
