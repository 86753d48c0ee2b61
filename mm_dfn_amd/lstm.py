"""2-layer bidirectional LSTM encoder on the fused HIP recurrence (csrc/lstm_seq.hip, K16).

``bilstm2(x, lstm, ...)`` evaluates one nn.LSTM(*, 100, num_layers=2, bidirectional=True) (the reference's ``LSTMModel.lstm``,
model.py:320-356) layer by layer: per layer ONE input projection launch on the two directions' own ``weight_ih`` / ``bias_ih``
parameters (``ops.linear2``, 800 outputs) and ONE persistent recurrence launch.  The nn.LSTM module only holds the parameters
(so the state_dict keys stay the reference's); its own forward (MIOpen) is never called.
"""
import torch

from . import _hip, ops
from .gru import _adjacent, _layer_params, _stacked_view  # noqa: F401  (shape-generic: shared, not copied)

H = 100


def block_steps():
    """Timesteps per staged block of the recurrence kernels (their only launch edge besides the sequence length)."""
    return int(_hip.query("mmdfn_lstm_seq_block_steps"))


class _LstmRecurrence(torch.autograd.Function):
    """(gi (T, R, 8H), w_hh_fwd, w_hh_rev, b_hh_fwd, b_hh_rev) -> y (T, R, 2H).  The recurrent weights are the module's own
    parameters; their gradients join the step's weight-gradient batch (ops.queue_wgrad) or come back per parameter."""

    @staticmethod
    def forward(ctx, gi, wf, wr, bf, br):
        gi = gi.contiguous()
        whh = [wf.contiguous(), wr.contiguous()]
        bhh = [bf.contiguous(), br.contiguous()]
        _hip.require_cuda(gi, *whh, *bhh)
        _hip.require_f32(gi, *whh, *bhh)
        T, R = gi.shape[0], gi.shape[1]
        if gi.dim() != 3 or gi.shape[2] != 8 * H or tuple(whh[0].shape) != (4 * H, H) or tuple(whh[1].shape) != (4 * H, H):
            raise ValueError("fused LSTM recurrence: gi must be (T, rows, 800) and weight_hh (400, 100)")
        y = torch.empty(T, R, 2 * H, dtype=torch.float32, device=gi.device)
        state = torch.empty(T, R, 2, 5, H, dtype=torch.float32, device=gi.device)
        _hip.call("mmdfn_lstm_seq_fwd", _hip.ptr(gi), _hip.ptr_array(whh), _hip.ptr_array(bhh), _hip.ptr(y), _hip.ptr(state),
                  R, T, H, _hip.stream())
        ctx.refs = (wf, wr, bf, br)            # the parameter objects (leaf test of the weight-gradient queue)
        ctx.save_for_backward(y, state, *whh)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, state, w0, w1 = ctx.saved_tensors
        T, R = y.shape[0], y.shape[1]
        dy = dy.contiguous()
        dgate = torch.empty(T, R, 8 * H, dtype=torch.float32, device=y.device)
        _hip.call("mmdfn_lstm_seq_bwd", _hip.ptr(dy), _hip.ptr(y), _hip.ptr(state), _hip.ptr_array([w0, w1]), _hip.ptr(dgate),
                  R, T, H, _hip.stream())
        # dW_hh = sum_t dgate_t (x) h_{t-1}   forward: h_{t-1} = y[t-1] (row shift -R), reverse: y[t+1] (+R)
        # db_hh = sum_t dgate_t               = the column sums of the same operand (= db_ih: one pre-activation per gate)
        d2, y2 = dgate.view(T * R, 8 * H), y.view(T * R, 2 * H)
        wf, wr, bf, br = ctx.refs
        res = []
        for A, B, w, b, shift in ((d2[:, :4 * H], y2[:, :H], wf, bf, -R), (d2[:, 4 * H:], y2[:, H:], wr, br, R)):
            if ops._queueable(w, [b], 4 * H, H):
                ops.queue_wgrad(A, B, w, [b], shift)
                res.append((None, None))
            else:
                dw = torch.empty(4 * H, H, dtype=torch.float32, device=y.device)
                db = torch.empty(4 * H, dtype=torch.float32, device=y.device)
                ops.gemm_tn_grouped([dict(A=A, B=B, C=dw, colsum=db, shift=shift)])
                res.append((dw, db))
        return dgate, res[0][0], res[1][0], res[0][1], res[1][1]


def _fused(sub):
    return isinstance(sub, torch.nn.LSTM) and sub.bidirectional and sub.num_layers == 2 and sub.hidden_size == H


def pair_lstm_weights(module):
    """Lay the two directions' ``weight_ih`` / ``bias_ih`` of every fused nn.LSTM of ``module`` out adjacently NOW (what the
    first training forward would otherwise do lazily): the counterpart of ``gru.pair_gru_weights``, same caveats.  Values are
    unchanged.  Returns the number of pairs."""
    n = 0
    for sub in module.modules():
        if _fused(sub):
            for layer in range(2):
                w_ih, b_ih, _ = _layer_params(sub, layer)
                n += int(_stacked_view(*w_ih) is not None) + int(_stacked_view(*b_ih) is not None)
    return n


def bilstm2(x, lstm, dropout=0.0, training=False, gi0=None):
    """x (T, rows, input_size) -> (T, rows, 200).  gi0 (optional): the first layer's gate pre-activations
    X W_ih^T + b_ih (T, rows, 800) computed by the caller; x is then ignored."""
    if not _fused(lstm) or lstm.batch_first or getattr(lstm, "proj_size", 0):
        raise NotImplementedError("fused LSTM path supports nn.LSTM(*, 100, num_layers=2, bidirectional=True)")
    cur = x
    for layer in range(2):
        (wf, wr), (bf, br), hh = _layer_params(lstm, layer)
        if layer == 0 and gi0 is not None:
            gi = gi0
        else:
            wcat = bcat = None
            if torch.is_grad_enabled():
                # [W_ih_fwd; W_ih_rev] as ONE (800, K) operand of the input-gradient launch: a view of the adjacent parameters,
                # or a copy when another owner has laid them out differently
                wcat, bcat = _stacked_view(wf, wr), _stacked_view(bf, br)
                if wcat is None:
                    wcat = torch.cat([wf.detach(), wr.detach()])
            gi = ops.linear2(cur, wf, wr, bf, br, wcat, bcat)
        cur = _LstmRecurrence.apply(gi, *hh)
        if layer == 0 and training and dropout > 0:
            # nn.LSTM's dropout between the layers: 0 / 1 keep flags from the step's flag pool, one launch each way
            keep = ops.keep_flags(cur.numel(), dropout, cur.device, site="lstm")
            cur = ops.mask_scale([cur], [keep], ops.keep_scale(dropout))[0]
    return cur
