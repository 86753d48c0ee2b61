"""Pass metrics accumulated where the step runs (csrc/pass_stats.hip, K13): per step ONE launch that writes the predictions and
adds the batch to a confusion matrix, a few counters and the loss sum in device memory -- the pass loop reads them back once.
``pass_stats_update`` is the operator; host tensors run ``pass_stats_update_host``, a plain torch restatement with the same
tie, NaN, bad-label and ignore rules (the loss modules keep a host path the same way for the gloo tests)."""
import torch

from . import _hip

# words of the meta block (int64), as include/mmdfn_hip.h lays them out
META_WORDS = 8
ARMED, ROWS, BATCHES, BAD_LABELS, NAN_ROWS = 0, 1, 2, 3, 4


def pass_stats_threads():
    """Rows one sweep of the launch's single workgroup covers."""
    return int(_hip.query("mmdfn_pass_stats_threads"))


def pass_stats_max_classes():
    """Largest class count the launch's LDS histogram holds."""
    return int(_hip.query("mmdfn_pass_stats_max_classes"))


def pass_stats_update(log_prob, target, loss, counts, meta, loss_sum, loss_hist, ignore_index):
    """One launch on the current stream: returns pred (N int64) and, when ``meta[ARMED]`` is set on the device, adds the batch
    to ``counts`` (C * C int64), ``meta`` (8 int64), ``loss_sum`` (1 float64) and ``loss_hist`` (slots float32).  ``loss``: a
    one-element float32 device tensor or None.  Consumes no random numbers, keeps nothing for autograd."""
    _hip.require_cuda(log_prob, target, loss, counts, meta, loss_sum, loss_hist)
    _hip.require_f32(log_prob, loss, loss_hist)
    if log_prob.dim() != 2 or target.dtype != torch.int64 or target.numel() != log_prob.shape[0]:
        raise ValueError("pass_stats_update: log_prob (N, C) float32 with N int64 labels, got %s / %s %s"
                         % (tuple(log_prob.shape), tuple(target.shape), target.dtype))
    N, C = log_prob.shape
    if counts.numel() != C * C or counts.dtype != torch.int64 or meta.numel() != META_WORDS or meta.dtype != torch.int64 \
            or loss_sum.dtype != torch.float64:
        raise ValueError("pass_stats_update: the accumulator was laid out for another class count (%d cells for C = %d)"
                         % (counts.numel(), C))
    log_prob = log_prob.detach().contiguous()
    target = target.reshape(-1).contiguous()
    if loss is not None:
        loss = loss.detach()
    slots = 0 if loss_hist is None else int(loss_hist.numel())
    pred = torch.empty(N, dtype=torch.int64, device=log_prob.device)
    _hip.call("mmdfn_pass_stats_accumulate", _hip.ptr(log_prob), _hip.ptr(target), _hip.ptr(loss), _hip.ptr(pred),
              _hip.ptr(counts), _hip.ptr(meta), _hip.ptr(loss_sum), _hip.ptr(loss_hist), N, C, int(ignore_index), slots,
              _hip.stream())
    return pred


def first_max(log_prob):
    """torch.argmax's rule written out: the lowest index among the maxima of a row; a row that holds a NaN gives the index of
    its first NaN.  Returns (pred, has_nan)."""
    nan = torch.isnan(log_prob)
    has_nan = nan.any(1)
    C = log_prob.shape[1]
    idx = torch.arange(C, device=log_prob.device).unsqueeze(0)
    clean = torch.where(nan, torch.full_like(log_prob, float("-inf")), log_prob)
    is_max = clean == clean.max(1, keepdim=True).values
    pred = torch.where(is_max, idx, C).min(1).values
    pred = torch.where(has_nan, torch.where(nan, idx, C).min(1).values, pred)
    return pred, has_nan


def pass_stats_update_host(log_prob, target, loss, counts, meta, loss_sum, loss_hist, ignore_index):
    """The launch above in plain torch, for host tensors."""
    log_prob = log_prob.detach()
    N, C = log_prob.shape
    target = target.reshape(-1)
    pred, has_nan = first_max(log_prob)
    if int(meta[ARMED]) == 0:
        return pred
    live = target != ignore_index
    good = live & (target >= 0) & (target < C)
    cells = target[good] * C + pred[good]
    counts += torch.bincount(cells, minlength=C * C)
    meta[ROWS] += int(good.sum())
    meta[BAD_LABELS] += int((live & ~good).sum())
    meta[NAN_ROWS] += int((live & has_nan).sum())
    k = int(meta[BATCHES])
    if loss is not None:
        value = loss.detach().to(torch.float32).reshape(-1)[0]
        loss_sum[0] += value.double()
        if loss_hist is not None and k < loss_hist.numel():
            loss_hist[k] = value
    meta[BATCHES] = k + 1
    return pred
