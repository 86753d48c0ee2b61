"""Recurrent comparison models of the reference on the fused kernels.

``GRUModel`` (reference model.py:281-317): a 2-layer bidirectional GRU over the utterance features, every timestep attending
over the whole dialogue through ``MatchingAttention(att_type='general2')``, then Linear + ReLU + dropout + ``smax_fc`` +
log_softmax.  Same constructor, ``forward(U, qmask, umask)`` signature, 5-tuple result and state_dict keys as the reference;
the nn.GRU / nn.Linear modules only hold the parameters.  The path is: one input projection launch (``ops.linear2``), the
fused recurrence (``gru.bigru2``), one attention launch for all L queries (K14), ``ops.linear`` and the classifier head (K9).

``LSTMModel`` (reference model.py:320-356, the training script's default ``--base_model``): the same model around a 2-layer
bidirectional LSTM (``lstm.bilstm2`` on K16, csrc/lstm_seq.hip); the attention / linear / head tail is shared.

``DialogRNNModel`` (reference model.py:359-417): two DialogueRNN encoders (``dialogue_rnn.DialogueRNN`` on K17,
csrc/dialogue_rnn.hip), the reverse one on every dialogue reversed within its own length, in front of the same tail.
"""
import torch
import torch.nn as nn

from . import dialogue_rnn as fused_drnn
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

    def __init__(self, D_m, D_e, D_h, n_classes=7, dropout=0.5, att2=True, **encoder):
        super().__init__()
        name = type(self).__name__
        if D_e != fused_gru.H:
            raise NotImplementedError("%s: the fused recurrence kernels are built for D_e = %d, got %d" % (name, fused_gru.H, D_e))
        if D_m % 4 or not 4 <= D_m <= 768:
            raise NotImplementedError("%s: the input projection serves D_m %% 4 == 0, 4 <= D_m <= 768, got %d" % (name, D_m))
        self.att2 = att2
        self.n_classes = n_classes
        self.dropout = nn.Dropout(dropout)
        self._build_encoder(D_m, D_e, dropout, **encoder)
        self.matchatt = MatchingAttention(2 * D_e, 2 * D_e, att_type='general2')
        self.linear = nn.Linear(2 * D_e, D_h)
        self.smax_fc = nn.Linear(D_h, n_classes)

    def _build_encoder(self, D_m, D_e, dropout):
        setattr(self, self.rnn_attr, self.rnn_cls(input_size=D_m, hidden_size=D_e, num_layers=2, bidirectional=True,
                                                  dropout=dropout))

    def forward(self, U, qmask, umask):
        """U (seq_len, batch, D_m), qmask unused (as in the reference), umask (batch, seq_len) of 0 / 1 ->
        (log_prob (seq_len, batch, n_classes), [alpha_t (batch, seq_len)] * seq_len, [], [], emotions (seq_len, batch, 2 D_e)).
        Every dialogue runs at the full padded length and every timestep is a query, padded ones too, as in the reference (it
        does not pack: its reverse direction starts in the padding)."""
        if U.is_cuda:
            ops.refresh_planes()
        with ops.flag_pool((type(self).__name__, U.shape[0], U.shape[1])):
            return self._forward(U, umask, qmask)

    def _encode(self, U, p):
        raise NotImplementedError

    def _encode_all(self, U, p, qmask, umask):
        """(emotions, alpha_f, alpha_b): the encoders that look at qmask / umask (DialogRNNModel) override this one."""
        return self._encode(U, p), [], []

    def _forward(self, U, umask, qmask=None):
        L, B = U.shape[0], U.shape[1]
        p = self.dropout.p
        emotions, alpha_f, alpha_b = self._encode_all(U, p, qmask, umask)
        alpha = []
        if self.att2:
            att, alpha_all = self.matchatt.forward_all(emotions, umask)
            alpha = list(alpha_all.unbind(0))
        else:
            att = emotions
        hidden = ops.linear(att, self.linear.weight, self.linear.bias, act=1)
        log_prob = ops.head(hidden.view(L * B, -1), self.smax_fc.weight, self.smax_fc.bias, p, self.training, relu=False)
        return log_prob.view(L, B, -1), alpha, alpha_f, alpha_b, emotions


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


class DialogRNNModel(_RecurrentBaseline):
    """``forward(U, qmask, umask) -> (log_prob, alpha, alpha_f, alpha_b, emotions)``; alpha_f / alpha_b: T-1 tensors, entry t-1
    is (B, t), in each encoder's own step order.  The forward encoder runs all T steps of every dialogue (padded ones too, as
    in the reference); the reverse encoder stops at a dialogue's length, so rows of alpha_b at or beyond it are zero where the
    reference attends over its own padding."""

    def __init__(self, D_m, D_g, D_p, D_e, D_h, D_a=100, n_classes=7, listener_state=False, context_attention='simple',
                 dropout_rec=0.5, dropout=0.5, att2=True):
        fused_drnn.check_served(type(self).__name__, D_m, D_g, D_p, D_e, listener_state, context_attention)
        super().__init__(D_m, D_e, D_h, n_classes, dropout, att2, D_g=D_g, D_p=D_p, listener_state=listener_state,
                         context_attention=context_attention, D_a=D_a, dropout_rec=dropout_rec)

    def _build_encoder(self, D_m, D_e, dropout, D_g, D_p, listener_state, context_attention, D_a, dropout_rec):
        self.dropout_rec = nn.Dropout(dropout + 0.15)
        self.dialog_rnn_f = fused_drnn.DialogueRNN(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout_rec)
        self.dialog_rnn_r = fused_drnn.DialogueRNN(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout_rec)

    def _encode_all(self, U, p, qmask, umask):
        lengths = umask.sum(1).to(torch.int32)
        e, alpha = fused_drnn.encode([self.dialog_rnn_f, self.dialog_rnn_r], U, qmask, lengths, self.dialog_rnn_f.dropout.p,
                                     self.training)
        ef, eb = e[0], e[1]
        pr = self.dropout_rec.p
        if self.training and pr > 0:
            keep = [ops.keep_flags(ef.numel(), pr, U.device, site="drnn_rec") for _ in range(2)]
            ef, eb = ops.mask_scale([ef, eb], keep, ops.keep_scale(pr))
        return torch.cat([ef, eb], 2), fused_drnn.alpha_list(alpha[0]), fused_drnn.alpha_list(alpha[1])
