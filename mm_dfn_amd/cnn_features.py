"""Token-level text front end on the fused embed-conv-maxpool kernels (csrc/cnn_features.hip, K18).

``CNNFeatureExtractor`` keeps the reference's constructor, ``forward(x, umask)``, ``init_pretrained_embeddings_from_numpy``,
``feature_dim`` and state_dict (model.py:1410-1443): ``embedding`` (nn.Embedding), ``convs`` (nn.Conv1d per kernel size) and
``fc`` (nn.Linear) only HOLD the parameters; their own forward is never called.  The path is one K18 launch pair (the weight cut
and the gather-conv-ReLU-max kernel: ``pooled (rows, n_k F)`` and its argmax, nothing of size rows x words x D in between),
dropout on that block as a multiply by keep flags (``ops.keep_flags(site="cnn")``), ``ops.linear(act=1)`` for fc + ReLU and the
utterance mask.  Backward: one launch for the conv weight / bias gradients and, for a trainable table only, a key launch, one
stable ``torch.sort``, a segment-bounds launch and a reduction launch -- no float atomics, so two runs give the same bits.

It composes with the recurrent baselines: ``U = cnn(x, umask); LSTMModel(D_m=output_size, ...)(U, qmask, umask)``.
"""
import torch
import torch.nn as nn

from . import _hip, ops

D_MIN, D_MAX = 4, 304
F_MAX = 64
SIZES_MAX = 4
K_MAX = 8
W_MAX = 512


def tile_words():
    """Window starts per staged tile of the forward kernel (its launch edge along the words)."""
    return int(_hip.query("mmdfn_cnn_tile_words"))


def rows_per_group():
    """Utterance rows one workgroup of the forward kernel serves."""
    return int(_hip.query("mmdfn_cnn_rows_per_group"))


def check_served(name, embedding_dim, filters, kernel_sizes):
    if embedding_dim % 4 or not D_MIN <= embedding_dim <= D_MAX:
        raise NotImplementedError("%s: the fused kernels serve embedding_dim %% 4 == 0, %d <= embedding_dim <= %d, got %d"
                                  % (name, D_MIN, D_MAX, embedding_dim))
    if not 1 <= filters <= F_MAX:
        raise NotImplementedError("%s: the fused kernels serve 1 <= filters <= %d, got %d" % (name, F_MAX, filters))
    if not 1 <= len(kernel_sizes) <= SIZES_MAX:
        raise NotImplementedError("%s: the fused kernels serve one to %d kernel sizes, got %d"
                                  % (name, SIZES_MAX, len(kernel_sizes)))
    for K in kernel_sizes:
        if not 1 <= K <= K_MAX:
            raise NotImplementedError("%s: the fused kernels serve kernel sizes 1 <= K <= %d, got %d" % (name, K_MAX, K))


def check_shape(name, rows, num_words, kernel_sizes):
    """The launch-time part of the envelope (known only at forward): raises before anything touches the device."""
    if rows < 1:
        raise NotImplementedError("%s: the fused kernels serve rows >= 1, got %d" % (name, rows))
    if not max(kernel_sizes) <= num_words <= W_MAX:
        raise NotImplementedError("%s: the fused kernels serve max(kernel_sizes) <= num_words <= %d, got num_words = %d "
                                  "with kernel sizes %s" % (name, W_MAX, num_words, tuple(kernel_sizes)))


def check_ids(tokens, vocab_size, source=None):
    """Raise ValueError for an id outside [0, vocab_size): one device reduction and one host read, skipped under stream capture
    (the kernels clamp, so a captured batch cannot fault either).  ``tokens``: the int64 ids the kernels read; ``source``: the
    float tensor they were converted from, if any -- a NaN or an infinity there converts to an unspecified integer, so it is
    refused by name."""
    if tokens.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    bad = (tokens < 0) | (tokens >= vocab_size)
    if source is not None and source.is_floating_point():
        bad = bad | ~torch.isfinite(source).reshape(tokens.shape)
    if bool(bad.any().item()):
        raise ValueError("CNNFeatureExtractor: token ids must be finite and lie in [0, %d)" % vocab_size)


class _CnnPool(torch.autograd.Function):
    """(meta, table (V, D), W_0, b_0, W_1, b_1, ...) -> pooled, FLAT with numel rounded up to a multiple of 4 (zero tail): what
    ``ops.mask_scale`` takes.  meta: tokens (rows, W) int64, row_mask (rows) fp32, ksizes."""

    @staticmethod
    def forward(ctx, meta, table, *wb):
        tokens, mask, ks = meta["tokens"], meta["row_mask"], meta["ksizes"]
        ws, bs = [w.contiguous() for w in wb[0::2]], [b.contiguous() for b in wb[1::2]]
        table = table.contiguous()
        _hip.require_cuda(tokens, mask, table, *ws, *bs)
        _hip.require_f32(mask, table, *ws, *bs)
        rows, W = tokens.shape
        V, D = table.shape
        F, n_k = ws[0].shape[0], len(ks)
        NC = n_k * F
        dev = table.device
        ksa = _hip.int_array(ks)
        planes = torch.empty(int(_hip.query("mmdfn_cnn_planes_bytes", D, F, n_k, ksa)), dtype=torch.uint8, device=dev)
        flat = torch.zeros((rows * NC + 3) & ~3, dtype=torch.float32, device=dev)
        argmax = torch.empty(rows, NC, dtype=torch.int32, device=dev)
        _hip.call("mmdfn_cnn_pool_fwd", _hip.ptr(tokens), _hip.ptr(table), _hip.ptr_array(ws), _hip.ptr_array(bs),
                  _hip.ptr(mask), _hip.ptr(planes), _hip.ptr(flat), _hip.ptr(argmax), rows, W, V, D, F, n_k, ksa, _hip.stream())
        ctx.meta = meta
        ctx.dims = (rows, W, V, D, F, n_k)
        ctx.save_for_backward(argmax, table, *ws)
        ctx.mark_non_differentiable(argmax)
        return flat, argmax

    @staticmethod
    def backward(ctx, dflat, _dargmax):
        argmax, table = ctx.saved_tensors[:2]
        ws = list(ctx.saved_tensors[2:])
        tokens, ks = ctx.meta["tokens"], ctx.meta["ksizes"]
        rows, W, V, D, F, n_k = ctx.dims
        ksa = _hip.int_array(ks)
        dflat = dflat.contiguous()
        dev = table.device
        dws = [torch.empty_like(w) for w in ws]
        dbs = [torch.empty(F, dtype=torch.float32, device=dev) for _ in ws]
        _hip.call("mmdfn_cnn_pool_bwd", _hip.ptr(dflat), _hip.ptr(argmax), _hip.ptr(tokens), _hip.ptr(table),
                  _hip.ptr_array(dws), _hip.ptr_array(dbs), rows, W, V, D, F, n_k, ksa, _hip.stream())
        dtable = None
        if ctx.needs_input_grad[1]:          # a frozen table: nothing of this family is allocated or launched
            dtable = table_grad(dflat, argmax, tokens, ws, rows, W, V, D, F, ks)
        grads = [g for pair in zip(dws, dbs) for g in pair]
        return (None, dtable, *grads)


def table_grad(dflat, argmax, tokens, ws, rows, W, V, D, F, ks):
    """dEmb (V, D): keys of the touched (row, column, tap) entries, ONE stable sort, a per-token reduction in sorted order."""
    n_k = len(ks)
    ksa = _hip.int_array(ks)
    dev = dflat.device
    n = int(_hip.query("mmdfn_cnn_table_entries", rows, F, n_k, ksa))
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    _hip.call("mmdfn_cnn_table_keys", _hip.ptr(argmax), _hip.ptr(tokens), _hip.ptr(keys), rows, W, V, F, n_k, ksa, _hip.stream())
    skeys, order = torch.sort(keys, stable=True)
    dtable = torch.empty(V, D, dtype=torch.float32, device=dev)
    bounds = torch.empty(V + 1, dtype=torch.int64, device=dev)
    _hip.call("mmdfn_cnn_table_bwd", _hip.ptr(dflat), _hip.ptr(skeys), _hip.ptr(order), _hip.ptr_array(ws), _hip.ptr(bounds),
              _hip.ptr(dtable), rows, V, D, F, n_k, ksa, _hip.stream())
    return dtable


def cnn_pool(tokens, table, weights, biases, row_mask, check=True):
    """K18 on its own: tokens (rows, W) integer ids, table (V, D), weights[i] (F, D, K_i), biases[i] (F), row_mask (rows) ->
    (pooled (rows, n_k F), argmax (rows, n_k F) int32, the flat padded block pooled is a view of)."""
    V, D = table.shape
    F = weights[0].shape[0]
    ks = [int(w.shape[2]) for w in weights]
    check_served("cnn_pool", D, F, ks)
    rows, W = tokens.shape
    if any(w.shape != (F, D, K) for w, K in zip(weights, ks)) or any(b.shape != (F,) for b in biases):
        raise ValueError("cnn_pool: every weight must be (filters, embedding_dim, K) with a bias (filters)")
    check_shape("cnn_pool", rows, W, ks)
    _hip.require_cuda(tokens, table, row_mask, *weights, *biases)
    if tokens.is_floating_point():
        raise ValueError("cnn_pool: tokens must be integer ids (CNNFeatureExtractor.forward converts float ids)")
    if check:
        check_ids(tokens, V)
    meta = dict(tokens=tokens.to(torch.int64).contiguous(), row_mask=row_mask.to(torch.float32).contiguous(), ksizes=ks)
    flat, argmax = _CnnPool.apply(meta, table, *[t for pair in zip(weights, biases) for t in pair])
    return flat[:rows * len(ks) * F].view(rows, len(ks) * F), argmax, flat


class CNNFeatureExtractor(nn.Module):
    """``forward(x (num_utt, batch, num_words) ids, float or integer, umask (batch, num_utt)) -> (num_utt, batch, output_size)``,
    exact zeros where umask is 0 (those rows are skipped, not computed and multiplied away)."""

    def __init__(self, vocab_size, embedding_dim, output_size, filters, kernel_sizes, dropout):
        super().__init__()
        kernel_sizes = tuple(int(K) for K in kernel_sizes)
        check_served(type(self).__name__, embedding_dim, filters, kernel_sizes)
        self.kernel_sizes = kernel_sizes
        self.embedding = nn.Embedding(vocab_size, embedding_dim)
        self.convs = nn.ModuleList([nn.Conv1d(in_channels=embedding_dim, out_channels=filters, kernel_size=K)
                                    for K in kernel_sizes])
        self.dropout = nn.Dropout(dropout)
        self.fc = nn.Linear(len(kernel_sizes) * filters, output_size)
        self.feature_dim = output_size

    def init_pretrained_embeddings_from_numpy(self, pretrained_word_vectors):
        self.embedding.weight = nn.Parameter(torch.from_numpy(pretrained_word_vectors).float())
        self.embedding.weight.requires_grad = False

    def forward(self, x, umask):
        num_utt, batch, num_words = x.shape
        check_shape(type(self).__name__, num_utt * batch, num_words, self.kernel_sizes)
        _hip.require_cuda(x, umask)
        tokens = x.reshape(-1, num_words).long()              # (the reference's x.long())
        check_ids(tokens, self.embedding.weight.shape[0], source=x)      # on what the kernels read, before any of them launches
        row_mask = umask.to(torch.float32).t().reshape(-1)
        p = self.dropout.p
        with ops.flag_pool((type(self).__name__, num_utt, batch)):
            pooled, _, flat = cnn_pool(tokens, self.embedding.weight, [c.weight for c in self.convs],
                                       [c.bias for c in self.convs], row_mask, check=False)
            if self.training and p > 0:
                keep = ops.keep_flags(flat.numel(), p, flat.device, site="cnn")
                flat = ops.mask_scale([flat], [keep], ops.keep_scale(p))[0]
                pooled = flat[:pooled.numel()].view(pooled.shape)
            feats = ops.linear(pooled, self.fc.weight, self.fc.bias, act=1)
        return feats.view(num_utt, batch, -1) * row_mask.view(num_utt, batch, 1)
