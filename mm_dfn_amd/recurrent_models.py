"""Recurrent comparison models of the reference on the fused kernels.

``GRUModel`` (reference model.py:281-317): a 2-layer bidirectional GRU over the utterance features, every timestep attending
over the whole dialogue through ``MatchingAttention(att_type='general2')``, then Linear + ReLU + dropout + ``smax_fc`` +
log_softmax.  Same constructor, ``forward(U, qmask, umask)`` signature, 5-tuple result and state_dict keys as the reference;
the nn.GRU / nn.Linear modules only hold the parameters.  The path is: one input projection launch (``ops.linear2``), the
fused recurrence (``gru.bigru2``), one attention launch for all L queries (K14), ``ops.linear`` and the classifier head (K9).

``LSTMModel`` (reference model.py:320-356, the training script's default ``--base_model``): the same model around a 2-layer
bidirectional LSTM (``lstm.bilstm2`` on K16, csrc/lstm_seq.hip); the attention / linear / head tail is shared.
"""
import torch
import torch.nn as nn

from . import gru as fused_gru
from . import lstm as fused_lstm
from . import ops
from .attention import MatchingAttention


class _RecurrentBaseline(nn.Module):
    """What GRUModel and LSTMModel share: the refusals, the flag-pool scope of a forward pass and the attention / linear / head
    tail.  A subclass names its recurrent module (``rnn_cls``; the attribute name is the reference's, and module registration
    order is the reference's too, so state_dict() lists the keys in its order) and implements ``_encode``."""
    rnn_cls = None
    rnn_attr = None

    def __init__(self, D_m, D_e, D_h, n_classes=7, dropout=0.5, att2=True):
        super().__init__()
        name = type(self).__name__
        if D_e != fused_gru.H:
            raise NotImplementedError("%s: the fused recurrence kernels are built for D_e = %d, got %d" % (name, fused_gru.H, D_e))
        if D_m % 4 or not 4 <= D_m <= 768:
            raise NotImplementedError("%s: the input projection serves D_m %% 4 == 0, 4 <= D_m <= 768, got %d" % (name, D_m))
        self.att2 = att2
        self.n_classes = n_classes
        self.dropout = nn.Dropout(dropout)
        setattr(self, self.rnn_attr, self.rnn_cls(input_size=D_m, hidden_size=D_e, num_layers=2, bidirectional=True,
                                                  dropout=dropout))
        self.matchatt = MatchingAttention(2 * D_e, 2 * D_e, att_type='general2')
        self.linear = nn.Linear(2 * D_e, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)

    def forward(self, U, qmask, umask):
        """U (seq_len, batch, D_m), qmask unused (as in the reference), umask (batch, seq_len) of 0 / 1 ->
        (log_prob (seq_len, batch, n_classes), [alpha_t (batch, seq_len)] * seq_len, [], [], emotions (seq_len, batch, 2 D_e)).
        Every dialogue runs at the full padded length and every timestep is a query, padded ones too, as in the reference (it
        does not pack: its reverse direction starts in the padding)."""
        if U.is_cuda:
            ops.refresh_planes()
        with ops.flag_pool((type(self).__name__, U.shape[0], U.shape[1])):
            return self._forward(U, umask)

    def _encode(self, U, p):
        raise NotImplementedError

    def _forward(self, U, umask):
        L, B = U.shape[0], U.shape[1]
        p = self.dropout.p
        emotions = self._encode(U, p)
        alpha = []
        if self.att2:
            att, alpha_all = self.matchatt.forward_all(emotions, umask)
            alpha = list(alpha_all.unbind(0))
        else:
            att = emotions
        hidden = ops.linear(att, self.linear.weight, self.linear.bias, act=1)
        log_prob = ops.head(hidden.view(L * B, -1), self.smax_fc.weight, self.smax_fc.bias, p, self.training, relu=False)
        return log_prob.view(L, B, -1), alpha, [], [], emotions


class GRUModel(_RecurrentBaseline):
    rnn_cls, rnn_attr = nn.GRU, "gru"

    def _encode(self, U, p):
        (wf, wr), (bf, br), _ = fused_gru._layer_params(self.gru, 0)
        wcat = bcat = None
        if torch.is_grad_enabled():
            wcat, bcat = fused_gru._stacked_view(wf, wr), fused_gru._stacked_view(bf, br)
        gi0 = ops.linear2(U, wf, wr, bf, br, wcat, bcat)
        return fused_gru.bigru2([None], [self.gru], p, self.training, gi0=[gi0])[0]


class LSTMModel(_RecurrentBaseline):
    rnn_cls, rnn_attr = nn.LSTM, "lstm"

    def _encode(self, U, p):
        return fused_lstm.bilstm2(U, self.lstm, p, self.training)
