"""FocalLoss (reference loss.py:5-34): -(1-pt)^gamma * alpha_t * log(pt), pt detached; NLLLoss: the training script's other
objective, torch.nn.NLLLoss(class weights) (run_train_erc.py:509); MaskedNLLLoss (loss.py:38-58): the objective of the reference's
recurrent models (run_train_erc.py:92-146)."""
import torch
import torch.nn as nn


# Set by train.backward() (and only there) around ``loss.backward(one)`` when ``loss`` IS the output of the fused node below and
# ``one`` is its cached scalar 1: the node's upstream gradient is then exactly 1 and the gradient the forward launch already wrote
# is the answer.  An explicit flag, not a comparison of data pointers (an address can be reused, a seed overwritten).
UNIT_SEED_ACTIVE = [False]


def is_fused_loss_output(loss):
    """True when ``loss`` comes straight out of _FocalLossHip (so a backward seeded at ``loss`` hands the node its seed unchanged)."""
    fn = getattr(loss, "grad_fn", None)
    return fn is not None and type(fn).__name__ == "_FocalLossHipBackward"


class _FocalLossHip(torch.autograd.Function):
    """One fused launch on device tensors (csrc/focal_loss.hip): when a gradient will be wanted the forward launch also
    writes d loss / d log_prob for an upstream gradient of 1, and the backward pass launches nothing for the loss when it
    is seeded with train.backward's cached 1 (any other upstream gradient takes the backward kernel)."""

    @staticmethod
    def forward(ctx, logp, target, alpha, gamma, size_average):
        from . import _hip
        logp = logp.contiguous()
        target = target.reshape(-1).contiguous()
        N, C = logp.shape
        loss = torch.empty((), dtype=torch.float32, device=logp.device)
        coef = torch.empty(N, dtype=torch.float32, device=logp.device)
        want = ctx.needs_input_grad[0]
        dunit = torch.empty(N, C, dtype=torch.float32, device=logp.device) if want else None
        _hip.call("mmdfn_focal_loss_fwd_grad", _hip.ptr(logp), _hip.ptr(target), _hip.ptr(alpha), _hip.ptr(loss),
                  _hip.ptr(coef), _hip.ptr(dunit), N, C, float(gamma),
                  1 if size_average else 0, _hip.stream())
        ctx.save_for_backward(coef, target)
        ctx.dunit = dunit
        ctx.C = C
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from . import _hip
        if ctx.dunit is not None and UNIT_SEED_ACTIVE[0]:
            if getattr(ctx, "dunit_handed_out", False):
                return ctx.dunit.clone(), None, None, None, None     # a second pass (retain_graph): never the same tensor twice
            ctx.dunit_handed_out = True
            return ctx.dunit, None, None, None, None
        coef, target = ctx.saved_tensors
        N = coef.shape[0]
        dlogp = torch.empty(N, ctx.C, dtype=torch.float32, device=coef.device)
        dl = dloss.contiguous().to(torch.float32)
        _hip.call("mmdfn_focal_loss_bwd", _hip.ptr(coef), _hip.ptr(target), _hip.ptr(dl), _hip.ptr(dlogp), N, ctx.C,
                  _hip.stream())
        return dlogp, None, None, None, None


class _FocalLossIgnoreHip(torch.autograd.Function):
    """The fused launches with rows to leave out (csrc/focal_loss.hip, *_ignore): the row count of the mean is taken on
    the device, so a captured step serves batches with different numbers of rows that count."""

    @staticmethod
    def forward(ctx, logp, target, alpha, gamma, size_average, ignore_index):
        from . import _hip
        logp = logp.contiguous()
        target = target.reshape(-1).contiguous()
        N, C = logp.shape
        loss = torch.empty((), dtype=torch.float32, device=logp.device)
        scale = torch.empty(1, dtype=torch.float32, device=logp.device)
        coef = torch.empty(N, dtype=torch.float32, device=logp.device)
        _hip.call("mmdfn_focal_loss_fwd_ignore", _hip.ptr(logp), _hip.ptr(target), _hip.ptr(alpha), _hip.ptr(loss),
                  _hip.ptr(coef), _hip.ptr(scale), N, C, float(gamma),
                  1 if size_average else 0, int(ignore_index), _hip.stream())
        ctx.save_for_backward(coef, target, scale)
        ctx.C, ctx.ignore = C, int(ignore_index)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from . import _hip
        coef, target, scale = ctx.saved_tensors
        N = coef.shape[0]
        dlogp = torch.empty(N, ctx.C, dtype=torch.float32, device=coef.device)
        dl = dloss.contiguous().to(torch.float32)
        _hip.call("mmdfn_focal_loss_bwd_ignore", _hip.ptr(coef), _hip.ptr(target), _hip.ptr(dl), _hip.ptr(scale),
                  _hip.ptr(dlogp), N, ctx.C, ctx.ignore, _hip.stream())
        return dlogp, None, None, None, None, None


class FocalLoss(nn.Module):
    """``ignore_index`` (not in the reference, default None = the reference's behaviour): rows with that label add nothing to
    the loss or the gradient and are not counted by the mean."""

    def __init__(self, gamma=0, alpha=None, size_average=True, ignore_index=None):
        super().__init__()
        self.gamma = gamma
        self.ignore_index = ignore_index
        if isinstance(alpha, (float, int)) and not isinstance(alpha, bool):
            alpha = torch.tensor([alpha, 1 - alpha], dtype=torch.float32)
        elif isinstance(alpha, list):
            alpha = torch.tensor(alpha, dtype=torch.float32)
        self.alpha = alpha
        self.size_average = size_average

    def forward(self, input, target):
        if input.dim() > 2:
            input = input.view(input.size(0), input.size(1), -1).transpose(1, 2).contiguous().view(-1, input.size(1))
        if input.is_cuda and input.dtype == torch.float32 and input.dim() == 2 and target.dtype == torch.int64:
            alpha = self.alpha
            if alpha is not None and alpha.numel() < input.shape[1]:
                # the reference's alpha.gather(0, target) raises for such labels (loss.py:29); never read past the table
                raise IndexError("FocalLoss: alpha has %d entries for %d classes" % (alpha.numel(), input.shape[1]))
            if alpha is not None and (alpha.device != input.device or alpha.dtype != input.dtype):
                alpha = self.alpha = alpha.to(device=input.device, dtype=input.dtype)
            if self.ignore_index is not None:
                return _FocalLossIgnoreHip.apply(input, target, alpha, self.gamma, self.size_average, self.ignore_index)
            return _FocalLossHip.apply(input, target, alpha, self.gamma, self.size_average)
        # host tensors (the loss is plain glue in the reference; the gloo data-parallel test runs it on the CPU)
        if self.ignore_index is not None:
            keep = target.view(-1) != self.ignore_index
            input, target = input[keep], target.view(-1)[keep]
        target = target.view(-1, 1)
        logpt = input.gather(1, target).view(-1)
        pt = logpt.detach().exp()
        if self.alpha is not None:
            if self.alpha.device != input.device or self.alpha.dtype != input.dtype:
                self.alpha = self.alpha.to(device=input.device, dtype=input.dtype)
            logpt = logpt * self.alpha.gather(0, target.view(-1))
        loss = -1 * (1 - pt) ** self.gamma * logpt
        if self.ignore_index is not None and loss.numel() == 0:
            return loss.sum()            # every row left out: 0 with zero gradients, as the device form (not the NaN of an empty mean)
        return loss.mean() if self.size_average else loss.sum()


def nll_block_rows():
    """Rows one pass of the forward launch's single workgroup covers (csrc/nll_loss.hip)."""
    from . import _hip
    return int(_hip.query("mmdfn_nll_loss_threads"))


class _NLLLossHip(torch.autograd.Function):
    """One launch each way (csrc/nll_loss.hip): the forward writes the per-row coefficient -w[t] and 1 / (sum of the weights
    that count) on the device, so a captured step serves batches with different numbers of rows that count."""

    @staticmethod
    def forward(ctx, logp, target, weight, mean, ignore_index):
        from . import _hip
        logp = logp.contiguous()
        target = target.reshape(-1).contiguous()
        N, C = logp.shape
        loss = torch.empty((), dtype=torch.float32, device=logp.device)
        scale = torch.empty(1, dtype=torch.float32, device=logp.device)
        coef = torch.empty(N, dtype=torch.float32, device=logp.device)
        _hip.call("mmdfn_nll_loss_fwd", _hip.ptr(logp), _hip.ptr(target), _hip.ptr(weight), _hip.ptr(loss), _hip.ptr(coef),
                  _hip.ptr(scale), N, C, 1 if mean else 0, int(ignore_index), _hip.stream())
        ctx.save_for_backward(coef, target, scale)
        ctx.C, ctx.ignore = C, int(ignore_index)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from . import _hip
        coef, target, scale = ctx.saved_tensors
        N = coef.shape[0]
        dlogp = torch.empty(N, ctx.C, dtype=torch.float32, device=coef.device)
        dl = dloss.contiguous().to(torch.float32)
        _hip.call("mmdfn_nll_loss_bwd", _hip.ptr(coef), _hip.ptr(target), _hip.ptr(dl), _hip.ptr(scale), _hip.ptr(dlogp), N,
                  ctx.C, ctx.ignore, _hip.stream())
        return dlogp, None, None, None, None


class NLLLoss(nn.Module):
    """``torch.nn.NLLLoss(weight, ignore_index, reduction)`` with the arguments the reference's training script uses
    (run_train_erc.py:509, --loss NLLLoss [--class_weight]) on (N, C) log-probabilities:
    ``sum_i w[t_i] (-input[i, t_i]) / sum_i w[t_i]`` over the rows whose label is not ``ignore_index`` ('mean'; 'sum' does not
    divide).  NOT FocalLoss(gamma=0, alpha=w): that one divides by the number of rows.

    Device tensors run one fused launch each way.  Where it differs from torch, as FocalLoss's ignore_index form does: with
    every row ignored the loss is 0 with zero gradients (torch: NaN), and a label outside [0, C) that is not ``ignore_index``
    gives a NaN loss and NaN gradients (torch raises; a kernel cannot without a host synchronisation).  A weight table shorter
    than C raises IndexError.  Host tensors go to ``torch.nn.functional.nll_loss`` unchanged."""

    def __init__(self, weight=None, ignore_index=-100, reduction='mean'):
        super().__init__()
        if reduction == 'none':
            raise NotImplementedError("NLLLoss: reduction='none' is not implemented (the training script reduces)")
        if reduction not in ('mean', 'sum'):
            raise ValueError("NLLLoss: reduction must be 'mean' or 'sum', got %r" % (reduction,))
        if isinstance(weight, (list, tuple)):
            weight = torch.tensor(weight, dtype=torch.float32)
        self.weight = weight
        self.ignore_index = int(ignore_index)
        self.reduction = reduction

    def forward(self, input, target):
        weight = self.weight
        if weight is not None and (weight.device != input.device or weight.dtype != input.dtype):
            weight = self.weight = weight.to(device=input.device, dtype=input.dtype)
        if input.is_cuda and input.dtype == torch.float32 and input.dim() == 2 and target.dtype == torch.int64:
            if weight is not None and weight.numel() < input.shape[1]:
                raise IndexError("NLLLoss: weight has %d entries for %d classes" % (weight.numel(), input.shape[1]))
            if weight is not None:
                weight = weight.contiguous()
            return _NLLLossHip.apply(input, target, weight, self.reduction == 'mean', self.ignore_index)
        import torch.nn.functional as F
        return F.nll_loss(input, target, weight, ignore_index=self.ignore_index, reduction=self.reduction)


class _MaskedNLLLossHip(torch.autograd.Function):
    """One launch each way (csrc/nll_loss.hip, K15): the forward writes the per-row coefficient -m_i w[t_i] and the reciprocal
    of the denominator on the device."""

    @staticmethod
    def forward(ctx, pred, target, mask, weight):
        from . import _hip
        pred = pred.contiguous()
        target = target.reshape(-1).contiguous()
        mask = mask.reshape(-1).contiguous()
        N, C = pred.shape
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        scale = torch.empty(1, dtype=torch.float32, device=pred.device)
        coef = torch.empty(N, dtype=torch.float32, device=pred.device)
        _hip.call("mmdfn_masked_nll_fwd", _hip.ptr(pred), _hip.ptr(target), _hip.ptr(mask), _hip.ptr(weight), _hip.ptr(loss),
                  _hip.ptr(coef), _hip.ptr(scale), N, C, _hip.stream())
        ctx.save_for_backward(coef, target, mask, scale)
        ctx.C = C
        return loss

    @staticmethod
    def backward(ctx, dloss):
        from . import _hip
        coef, target, mask, scale = ctx.saved_tensors
        N = coef.shape[0]
        dpred = torch.empty(N, ctx.C, dtype=torch.float32, device=coef.device)
        dl = dloss.contiguous().to(torch.float32)
        _hip.call("mmdfn_masked_nll_bwd", _hip.ptr(coef), _hip.ptr(target), _hip.ptr(mask), _hip.ptr(dl), _hip.ptr(scale),
                  _hip.ptr(dpred), N, ctx.C, _hip.stream())
        return dpred, None, None, None


class MaskedNLLLoss(nn.Module):
    """The reference's ``MaskedNLLLoss(weight)`` (loss.py:38-58), the objective of its recurrent models: ``forward(pred, target,
    mask)`` with pred (batch * seq_len, n_classes) log-probabilities, target (batch * seq_len) and mask (batch, seq_len) of 0 / 1:
    ``sum_i m_i w[t_i] (-pred[i, t_i]) / sum_i m_i w[t_i]`` (w = 1 without a weight table).

    Device tensors run one fused launch each way; both sums are reduced in a fixed order in float64 and the denominator stays
    on the device.  Where it differs from the reference, as NLLLoss documents for its all-ignored case: with every row masked the
    loss is 0 with zero gradients (the reference: 0 / 0 = NaN), and a label outside [0, C) on a row that counts gives a NaN loss
    and a NaN gradient row (torch raises; a kernel cannot without a host synchronisation).  Gradient rows of masked positions
    are exact zeros.  A weight table shorter than C raises IndexError.  Host tensors take the reference's torch formula
    unchanged."""

    def __init__(self, weight=None):
        super().__init__()
        if isinstance(weight, (list, tuple)):
            weight = torch.tensor(weight, dtype=torch.float32)
        self.weight = weight

    def forward(self, pred, target, mask):
        weight = self.weight
        if weight is not None and (weight.device != pred.device or weight.dtype != pred.dtype):
            weight = self.weight = weight.to(device=pred.device, dtype=pred.dtype)
        if pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 2 and target.dtype == torch.int64:
            if weight is not None and weight.numel() < pred.shape[1]:
                raise IndexError("MaskedNLLLoss: weight has %d entries for %d classes" % (weight.numel(), pred.shape[1]))
            if mask.numel() != pred.shape[0] or target.numel() != pred.shape[0]:
                raise ValueError("MaskedNLLLoss: pred has %d rows, target %d, mask %d" % (pred.shape[0], target.numel(), mask.numel()))
            if weight is not None:
                weight = weight.contiguous()
            return _MaskedNLLLossHip.apply(pred, target, mask.to(torch.float32), weight)
        # host tensors: loss.py:52-58 as written
        mask_ = mask.view(-1, 1)
        nll = torch.nn.functional.nll_loss(pred * mask_, target, weight, reduction='sum')
        if weight is None:
            return nll / torch.sum(mask)
        return nll / torch.sum(weight[target] * mask_.squeeze())
