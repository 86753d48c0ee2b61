"""Training / evaluation pass: counterpart of ``train_or_eval_graph_model``
(reference run_train_erc.py:149-238), same argument list and 8-tuple result.

Kept from the reference: per-pass reseed (:164), batch tuple order ``textf,
visuf, acouf, qmask, umask, label`` (:169), lengths derived from umask (:194),
model call (:197), dialogue-major label flatten (:201), loss/backward/step
(:202-212), sklearn metrics (:229-236).  Changed for the device: lengths are
read back with ONE host sync per batch instead of B, and loss / prediction
syncs are deferred to the end of the pass.
"""
import random

import numpy as np
import torch

from . import ops, ops_stats


def seed_everything(seed=2021):
    """run_train_erc.py:19-26."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def lengths_from_umask(umask):
    """Index of the last 1 in each row + 1 (run_train_erc.py:194), one device->host sync."""
    L = umask.shape[1]
    pos = torch.arange(1, L + 1, device=umask.device).unsqueeze(0)
    return ((umask == 1).to(torch.int64) * pos).max(1).values.tolist()


def flatten_labels(label, lengths):
    """run_train_erc.py:201 without B slice ops: mask-select in dialogue-major order."""
    L = label.shape[1]
    keep = torch.arange(L, device=label.device).unsqueeze(0) < torch.as_tensor(lengths, device=label.device).unsqueeze(1)
    return label[keep]


_UNIT_SEED = {}      # (device, dtype) -> scalar 1; entries are never replaced (captured graphs hold their addresses)


def backward(loss):
    """``loss.backward()`` under ``ops.wgrad_batch()`` (the weight gradients of the step leave as one launch pair that
    writes ``.grad`` directly), seeded with a cached scalar 1 (autograd otherwise allocates and fills a fresh one: one
    more launch per step)."""
    key = (loss.device, loss.dtype)
    one = _UNIT_SEED.get(key)
    with ops.wgrad_batch():
        if one is None:
            if loss.is_cuda and torch.cuda.is_current_stream_capturing():
                return loss.backward()           # a tensor created under capture belongs to that graph's pool
            one = _UNIT_SEED[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
        from . import loss as _loss_mod
        # the seed is exactly 1 and, when ``loss`` is the fused FocalLoss node's own output, reaches that node unchanged: tell it
        # so (it then returns the gradient its forward launch wrote instead of launching a backward kernel)
        prev = _loss_mod.UNIT_SEED_ACTIVE[0]
        _loss_mod.UNIT_SEED_ACTIVE[0] = _loss_mod.is_fused_loss_output(loss)
        try:
            loss.backward(one)
        finally:
            _loss_mod.UNIT_SEED_ACTIVE[0] = prev


_OWN_BATCHES = 5      # word of PassStats' meta block that the launch never touches


class PassStats:
    """What a pass reports, accumulated where the step runs: a C x C confusion matrix (row = label), the counts of rows,
    batches, bad labels and NaN rows, the float64 sum of the batch losses and the first ``loss_slots`` batch losses.  ``update``
    is ONE launch per step on the device (ops.pass_stats_update, csrc/pass_stats.hip) -- a node of a captured step when a
    StepGraphCache is given this object -- and ``fetch`` the one device -> host copy of a pass.

    All of it lives in one int64 block that is allocated here and never re-pointed (a captured graph bakes its address):
    word 0 ``armed`` | words 1-4 rows, batches, bad_labels, nan_rows | 5 this process's batches + 1 once ``all_reduce`` has run
    (host-written) | 6-7 reserved | C * C counts | 1 word loss sum (float64) | loss history (float32).  ``armed`` is written by
    the host only (``set_enabled``, as FlatAdam.set_enabled): while it is 0 a launch -- the replay of a captured one included --
    writes its predictions and nothing else.  Host tensors take a plain torch restatement of the launch with the same rules."""

    def __init__(self, n_classes, device, loss_slots=4096, ignore_index=-100):
        self.n_classes, self.loss_slots, self.ignore_index = int(n_classes), int(loss_slots), int(ignore_index)
        self.device = torch.device(device)
        C = self.n_classes
        if C <= 0 or self.loss_slots < 0:
            raise ValueError("PassStats: n_classes > 0 and loss_slots >= 0, got %d / %d" % (C, self.loss_slots))
        if self.device.type == "cuda" and C > ops.pass_stats_max_classes():
            raise ValueError("PassStats: the device launch holds at most %d classes, got %d" % (ops.pass_stats_max_classes(), C))
        M = ops_stats.META_WORDS
        self._block = torch.zeros(M + C * C + 1 + (self.loss_slots + 1) // 2, dtype=torch.int64, device=self.device)
        self._meta = self._block[:M]
        self._counts = self._block[M:M + C * C]
        self._loss_sum = self._block[M + C * C:M + C * C + 1].view(torch.float64)
        self._loss_hist = self._block[M + C * C + 1:].view(torch.float32)[:self.loss_slots] if self.loss_slots else None
        self._enabled = None
        self._host = None
        self.set_enabled(True)

    def reset(self):
        """Zero everything but ``armed`` with one fill launch.  Outside any graph."""
        self._block[1:].zero_()
        self._host = None

    def set_enabled(self, flag):
        """Write ``armed`` (one tiny fill, outside any graph; nothing when the word already holds ``flag``)."""
        flag = bool(flag)
        if flag != self._enabled:
            self._meta[ops_stats.ARMED].fill_(int(flag))
            self._enabled = flag

    @property
    def enabled(self):
        return self._enabled

    def update(self, log_prob, flat_labels, loss=None):
        """Count one batch; returns its predictions (N int64; torch.argmax's rule).  Draws no random numbers, keeps nothing for
        autograd."""
        if log_prob.shape[1] != self.n_classes:
            raise ValueError("PassStats.update: built for %d classes, got log-probabilities of %d" % (self.n_classes, log_prob.shape[1]))
        args = (self._counts, self._meta, self._loss_sum, self._loss_hist, self.ignore_index)
        if self.device.type != "cuda":
            return ops.pass_stats_update_host(log_prob, flat_labels, loss, *args)
        if loss is not None:
            loss = loss.detach()
            if loss.dtype != torch.float32:
                loss = loss.to(torch.float32)
        return ops.pass_stats_update(log_prob, flat_labels, loss, *args)

    def all_reduce(self, group=None):
        """SUM of the counts, of rows / batches / bad_labels / nan_rows and of the loss sum over the process group (gloo on host
        tensors, RCCL on device tensors; never a graph node).  int64 sums are exact: every rank then derives the same metrics;
        the float64 loss sum agrees across ranks to its summation order.  ``armed`` and the loss history stay local."""
        import torch.distributed as dist
        M, C = ops_stats.META_WORDS, self.n_classes
        own = self._meta[ops_stats.BATCHES] + 1
        dist.all_reduce(self._block[1:M + C * C], op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(self._loss_sum, op=dist.ReduceOp.SUM, group=group)
        self._meta[_OWN_BATCHES].copy_(own)           # (a reserved word, zero on every rank while the sum ran)
        self._host = None

    def fetch(self):
        """ONE device -> host copy of the whole block (the only synchronising call); the accessors below read that copy."""
        self._host = self._block.cpu().numpy().copy()
        return self

    def _fetched(self):
        if self._host is None:
            raise RuntimeError("PassStats: fetch() first (the accessors read the host copy of the block)")
        return self._host

    def _word(self, w):
        return int(self._fetched()[w])

    rows = property(lambda self: self._word(ops_stats.ROWS))
    batches = property(lambda self: self._word(ops_stats.BATCHES))
    bad_labels = property(lambda self: self._word(ops_stats.BAD_LABELS))
    nan_rows = property(lambda self: self._word(ops_stats.NAN_ROWS))

    def confusion(self):
        """(C, C) int64, row = label, column = prediction."""
        M, C = ops_stats.META_WORDS, self.n_classes
        return self._fetched()[M:M + C * C].reshape(C, C).copy()

    def loss_sum(self):
        M, C = ops_stats.META_WORDS, self.n_classes
        return float(self._fetched()[M + C * C:M + C * C + 1].view(np.float64)[0])

    def loss_mean(self):
        return self.loss_sum() / self.batches if self.batches else float('nan')

    def batch_losses(self):
        """The first min(batches, loss_slots) batch losses (float32) of THIS process's pass, in step order."""
        M, C = ops_stats.META_WORDS, self.n_classes
        own = self._word(_OWN_BATCHES)
        n = own - 1 if own else self.batches
        return self._fetched()[M + C * C + 1:].view(np.float32)[:min(n, self.loss_slots)].copy()

    # closed forms of the matrix, in float64
    def accuracy(self):
        cm = self.confusion()
        n = int(cm.sum())
        return float(np.trace(cm)) / n if n else float('nan')

    def weighted_f1(self):
        """Per-class F1 = 2 tp / (2 tp + fp + fn) (0 for a class with neither predicted nor true samples) weighted by support:
        sklearn's f1_score(average='weighted') under its default zero-division rule."""
        cm = self.confusion().astype(np.float64)
        n = cm.sum()
        if n == 0:
            return float('nan')
        tp, support = np.diag(cm), cm.sum(1)
        denom = support + cm.sum(0)                # 2 tp + fn + fp
        f1 = np.divide(2.0 * tp, denom, out=np.zeros_like(tp), where=denom > 0)
        return float((f1 * support).sum() / n)

    def per_class_accuracy(self):
        """Recall of every class; nan for a class without true samples."""
        cm = self.confusion().astype(np.float64)
        support = cm.sum(1)
        return np.divide(np.diag(cm), support, out=np.full(self.n_classes, np.nan), where=support > 0)

    def as_arrays(self):
        """(labels, preds): the matrix expanded, grouped by (label, pred) -- NOT in utterance order.  Every order-invariant
        metric of these arrays is that of the pass's real sequences."""
        C = self.n_classes
        cells = self.confusion().ravel()
        return np.repeat(np.repeat(np.arange(C), C), cells), np.repeat(np.tile(np.arange(C), C), cells)


class StepGraphCache:
    """Shape-keyed hipGraph cache for the pass loop: one captured step per batch signature (dialogue lengths, padded
    shape, train / eval), replayed whenever that signature comes back.

    At IEMOCAP / MELD sizes the eager step is host-bound (a few hundred short kernels; 3.6 ms eager vs 1.45 ms replayed
    at cfg2).  The reference re-seeds before every pass (run_train_erc.py:164), so the shuffle -- and with it the
    set of batch signatures -- is the same every epoch: after the first epoch every step of a real run is a replay.
    Each entry owns static input buffers (a batch is copied in, ~5 MB), the captured forward(+loss+backward) and its
    outputs; gradients are handed to ``p.grad`` after the replay, the optimizer step stays outside the graph -- unless the
    cache is given the ``optimizer`` (a FlatAdam on device-resident step state): training entries then end with the gradient
    pack and the update, and a replay is the whole step.  Least recently used entries are dropped beyond ``max_entries``
    (each holds a private memory pool)."""

    IGNORE = -100                  # label of the padding dialogue's utterances (bucketed entries)

    def __init__(self, model, loss_f, max_entries=96, warmup=2, bucket_rows=0, larger_bucket_fallback=True, optimizer=None,
                 pass_stats=None):
        """``bucket_rows`` = g > 0: BUCKETED entries -- one captured step per (train / eval, B, padded length L, ceil((N + 1) /
        g) g) instead of per exact tuple of dialogue lengths (N = the batch's utterances).  The batch is padded to its
        bucket with ONE extra dialogue of 1..g utterances (fixed random features, labels IGNORE: dialogues never interact
        -- per-sequence GRUs, block-diagonal adjacency, row-wise stack -- so the real dialogues' results are those of the
        batch alone, the padding rows add exact zeros to every gradient, and the loss is the mean over the real
        utterances, counted on the device); before a replay the step's index arrays (dialogue lengths, row / tile
        offsets, pad-strip and label gather indices) are rewritten for the new lengths (layout.IndexScope): the kernels
        read them from device memory and their grids depend on (B, N, L) only.  A loader that reshuffles every epoch
        (run_train_erc.py:165-212 with a different seed per pass, any sampler but the reference's) then stays on replays.
        ``larger_bucket_fallback``: a batch whose own bucket has no entry yet is served by the smallest LARGER captured bucket
        of the same (B, L) that its padding dialogue can fill (at most L utterances: up to ~L / g buckets above its own)
        instead of being captured in the middle of a pass (55-90 ms at cfg2 against a few percent more rows for that step);
        ``fallbacks`` counts them, ``precapture`` still captures every bucket it meets exactly.
        Needs a mm_dfn_amd FocalLoss (its ignore_index form) or a mm_dfn_amd NLLLoss (taken as it is when its ignore_index is
        IGNORE, torch's default; otherwise a copy that ignores IGNORE steps the bucketed entries); any other loss object falls
        back to exact signatures.  use_speaker / use_modal models are served too: their embeddings are added by one row-wise
        launch that reads the speakers from qmask through the retargeted pad-strip index (ops.graph_embeddings), the padding
        dialogue is speaker 0's monologue and adds exact zeros to the table gradients.
        ``optimizer``: a device-state FlatAdam (``capturable=True`` / ``max_grad_norm`` / ``skip_nonfinite``) captured into every
        TRAINING entry, exact and bucketed (graphs.CapturedStep(optimizer=...)); eval entries are captured without it.  The pass
        loop must then not step it again (train_or_eval_graph_model does not), and ``precapture`` replays with the update
        disabled.
        ``pass_stats``: a PassStats (built with ignore_index = IGNORE, the label of the bucketed entries' padding rows).  Every
        entry, exact and bucketed, train and eval, then counts its batch with ``pass_stats.update(log_prob, labels, loss)`` as
        a node of the captured step, in place of the ``torch.argmax`` launch (``last_pred`` is that launch's output).  Only
        replays count: the block is disarmed on the device while a step is warmed up and captured and for the whole of
        ``precapture``, and armed again in front of a replay -- a miss in the middle of a pass counts its batch exactly once,
        through the replay that follows the capture."""
        from collections import OrderedDict
        if pass_stats is not None and pass_stats.ignore_index != self.IGNORE:
            raise ValueError("StepGraphCache: pass_stats must ignore the padding label (PassStats(ignore_index=%d)), got %d"
                             % (self.IGNORE, pass_stats.ignore_index))
        self.pass_stats = pass_stats
        self._stats_hold = False           # precapture: replays leave the block disarmed as well
        if optimizer is not None and not getattr(optimizer, "device_state", False):
            raise ValueError("StepGraphCache: optimizer= needs a FlatAdam on device-resident step state (capturable=True, "
                             "max_grad_norm or skip_nonfinite)")
        self.optimizer = optimizer
        self.model, self.loss_f = model, loss_f
        self.max_entries, self.warmup = max_entries, warmup
        self.bucket_rows = int(bucket_rows or 0)
        self.entries = OrderedDict()
        self.queued = {}           # signature -> batches a staging loader has announced (claim_static) and not stepped yet
        self.hits = self.misses = self.recaptures = self.fallbacks = 0
        self.larger_bucket_fallback = bool(larger_bucket_fallback)
        self._exact_buckets = False        # (precapture: every bucket it meets gets its own entry)
        self._loss_ign = None
        if self.bucket_rows:
            from .loss import FocalLoss, NLLLoss
            if isinstance(loss_f, FocalLoss) and loss_f.ignore_index is None:
                self._loss_ign = FocalLoss(gamma=loss_f.gamma, alpha=loss_f.alpha, size_average=loss_f.size_average,
                                           ignore_index=self.IGNORE)
            elif isinstance(loss_f, NLLLoss):
                # (torch's default ignore_index IS -100: the usual object is taken as it is)
                self._loss_ign = loss_f if loss_f.ignore_index == self.IGNORE else NLLLoss(
                    weight=loss_f.weight, ignore_index=self.IGNORE, reduction=loss_f.reduction)

    def _capture(self, fn, train_flag):
        """A CapturedStep of ``fn``; its eager warm-up passes and the capture itself run with the pass statistics disarmed."""
        from .graphs import CapturedStep
        if self.pass_stats is not None:
            self.pass_stats.set_enabled(False)
        return CapturedStep(self.model, fn, warmup=self.warmup, optimizer=self.optimizer if train_flag else None)

    def _replay(self, cap):
        if self.pass_stats is not None:
            self.pass_stats.set_enabled(not self._stats_hold)      # (host bookkeeping; a fill only when the word changes)
        return cap.replay()

    def _hand_over_grads(self, ent):
        """``p.grad`` = the gradient tensors the entry's graph writes (walking named_parameters() on every step cost the
        host 0.3 ms, a third of a cfg2 step: the (parameter, gradient) pairs are listed once per entry)."""
        pairs = ent.get("grad_pairs")
        if pairs is None:
            grads = ent["cap"].grads
            pairs = ent["grad_pairs"] = [(p, grads.get(name)) for name, p in self.model.named_parameters()]
        for p, g in pairs:
            p.grad = g

    def _bucketable(self, inputs, lengths, test_label):
        L = int(inputs[0].shape[0])
        return (self._loss_ign is not None and not test_label and self.bucket_rows <= L and all(t.is_cuda for t in inputs)
                and int(max(lengths)) == L)

    def _bucket_key(self, inputs, lengths, train_flag):
        g = self.bucket_rows
        B, N, L = len(lengths), int(sum(lengths)), int(inputs[0].shape[0])
        Nb = ((N + 1 + g - 1) // g) * g
        # (the padded widths of umask / label are baked into the captured label gather and the static buffers: part of the key)
        return (("bucket", bool(train_flag), B, L, Nb, int(inputs[4].shape[1]), int(inputs[5].shape[1]))
                + tuple(tuple(t.shape[2:]) for t in inputs[:4]))

    def entry_key(self, inputs, lengths, train_flag, test_label=False):
        """The cache key ``step`` would use for this batch (a bucket, or the exact signature)."""
        lengths = [int(x) for x in lengths]
        if self.bucket_rows and self._bucketable(inputs, lengths, test_label):
            return self._bucket_key(inputs, lengths, train_flag)
        return self.signature([t.shape for t in inputs], lengths, train_flag, test_label)

    def precapture(self, loader, train_flag=True, device=None):
        """Capture, BEFORE the first pass, one step for every bucket / signature ``loader``'s batches will ask for (VERDICT r05
        item 7: a pass that has to capture pays ~25 ms per new entry in the middle of its steps).  Walks the loader once --
        the loader's length histogram is what decides the set, so this is the loader the passes will use or one drawn like
        it -- and steps only the first batch of each new key (forward + loss + backward into the entry's own gradient
        buffers; no optimizer -- a cache-owned one is disabled on the device for the walk, so the replays update nothing --, no
        metrics; dropout draws are put back by CapturedStep).  Returns the number of entries
        captured; the model's ``.grad`` fields are left as they were.  Call it AFTER anything that re-points parameter storage
        (FlatAdam lays the parameters out at its first step; ``.to()``; ``load_state_dict(assign=True)``): a captured step bakes
        the storages and is captured again when they move."""
        grads = [(p, p.grad) for p in self.model.parameters()]
        made = 0
        self._exact_buckets = True
        if self.optimizer is not None:
            self.optimizer.set_enabled(False)
        stats_were = None
        if self.pass_stats is not None:
            stats_were = self.pass_stats.enabled
            self._stats_hold = True
            self.pass_stats.set_enabled(False)
        try:
            made = self._precapture_walk(loader, train_flag, device)
        finally:
            self._exact_buckets = False
            if self.optimizer is not None:
                self.optimizer.set_enabled(True)
            if self.pass_stats is not None:
                self._stats_hold = False
                self.pass_stats.set_enabled(stats_were)
        if hasattr(loader, "bind_graph_cache"):
            self.forget_queued()
        for p, g in grads:
            p.grad = g
        return made

    def _precapture_walk(self, loader, train_flag, device):
        made = 0
        for data in loader:
            tensors = list(data[:6])
            if device is not None:
                tensors = [t.to(device, non_blocking=True) for t in tensors]
            if not all(t.is_cuda for t in tensors):
                raise ValueError("StepGraphCache.precapture: batches must be on the device (pass device=...)")
            lengths = getattr(data, "lengths", None) or lengths_from_umask(tensors[4])
            if self.entry_key(tensors, lengths, train_flag) in self.entries:
                continue
            self.step(tuple(tensors), lengths, train_flag)
            if self.bucket_rows and self.entry_key(tensors, lengths, train_flag) in self.entries:
                # the first REPLAY-path step of a bucketed entry (index retarget through fresh staging buffers, the input copies)
                # costs ~10-35 ms once: paid here, not by the first batch of a pass that lands in the bucket
                self.step(tuple(tensors), lengths, train_flag)
            made += 1
        return made

    def _step_bucketed(self, inputs, lengths, train_flag):
        """One step through a bucketed entry (see __init__).  Returns (loss, log_prob[:N], flat_labels[:N])."""
        from .layout import IndexScope
        g = self.bucket_rows
        lengths = [int(x) for x in lengths]
        B, N, L = len(lengths), sum(lengths), int(inputs[0].shape[0])
        Nb = ((N + 1 + g - 1) // g) * g
        pad = Nb - N                                       # 1 .. g utterances of the padding dialogue
        lens2 = lengths + [pad]
        key = self._bucket_key(inputs, lengths, train_flag)
        ent = self.entries.get(key)
        if ent is None and self.larger_bucket_fallback and not self._exact_buckets:
            # the smallest larger captured bucket of the same (B, L) that a padding dialogue of <= L utterances reaches
            for nb2 in range(Nb + g, N + L + 1, g):
                k2 = key[:4] + (nb2,) + key[5:]
                if k2 in self.entries:
                    key, ent, Nb, pad = k2, self.entries[k2], nb2, nb2 - N
                    lens2 = lengths + [pad]
                    self.fallbacks += 1
                    break
        dev = inputs[0].device
        Lp = int(inputs[5].shape[1])

        def label_pos(lens):
            lens = np.asarray(lens, dtype=np.int64)
            start = np.cumsum(lens) - lens
            return np.arange(int(lens.sum()), dtype=np.int64) + np.repeat(np.arange(lens.size, dtype=np.int64) * Lp - start, lens)

        if ent is None:
            self.misses += 1
            gen = torch.Generator().manual_seed(20210 + B)
            static = []
            for i, t in enumerate(inputs):
                if i in ops.FEATURE_SLOTS:                 # (L, B, D) -> (L, B + 1, D): the padding dialogue's features are fixed noise
                    full = torch.cat([t, torch.randn(L, 1, t.shape[2], generator=gen).to(dev)], 1)
                    static.append(ops.pad_rows(full) if ops.is_odd_feature_tensor(full, True) else full)
                elif i == 3:                               # qmask (L, B, P): the padding dialogue is speaker 0's monologue
                    static.append(torch.cat([t, torch.zeros(L, 1, t.shape[2], dtype=t.dtype, device=dev)], 1))
                elif i == 4:                               # umask (B, L)
                    static.append(torch.cat([t, torch.zeros(1, t.shape[1], dtype=t.dtype, device=dev)], 0))
                else:                                      # label (B, L): never counted
                    static.append(torch.cat([t, torch.full((1, t.shape[1]), self.IGNORE, dtype=t.dtype, device=dev)], 0))
            textf, visuf, acouf, qmask, umask, label = static
            scope = IndexScope()
            # tri[n][t] = (t < n): the padding dialogue's masks for n utterances are one row copy each
            tri = (torch.arange(L, device=dev).unsqueeze(0) < torch.arange(L + 1, device=dev).unsqueeze(1))
            tri_q, tri_u = tri.to(qmask.dtype), tri.to(umask.dtype)
            out = {}
            model, loss_f, stats = self.model, self._loss_ign, self.pass_stats
            with scope:
                pos = scope.tensor(("labelpos", Lp), lens2, label_pos, dev)
            flat = label.reshape(-1).index_select(0, pos)
            state = dict(lens2=lens2)

            def set_padding(n):
                # the padding dialogue's speaker / utterance masks for n utterances (two tiny launches, outside the graph)
                qmask[:, B, 0].copy_(tri_q[n])
                umask[B, :L].copy_(tri_u[n])

            set_padding(pad)

            def fn():
                with scope:
                    torch.index_select(label.reshape(-1), 0, pos, out=flat)
                    out["log_prob"] = model(textf, qmask, umask, state["lens2"], acouf, visuf, False)[0]
                    if stats is None:
                        out["pred"] = torch.argmax(out["log_prob"], 1)
                    loss = loss_f(out["log_prob"], flat)
                    if stats is not None:                      # predictions + this batch's counts: one launch, no argmax
                        out["pred"] = stats.update(out["log_prob"], flat, loss)
                    if train_flag:
                        backward(loss)
                return loss

            mode = model.training
            model.train(train_flag)
            with torch.set_grad_enabled(bool(train_flag)):
                cap = self._capture(fn, train_flag)
            model.train(mode)
            ent = dict(static=static, cap=cap, out=out, flat=flat, pos=pos, pending=None, scope=scope, set_padding=set_padding,
                       state=state, bucketed=True, B=B)
            self.entries[key] = ent
            while len(self.entries) > self.max_entries:
                self.entries.popitem(last=False)
        else:
            self.hits += 1
            self.entries.move_to_end(key)
            if ent.get("pending") is not None:
                ent["pending"]()
                ent["pending"] = None
            ent["state"]["lens2"] = lens2
            ent["scope"].retarget(lens2)                   # lengths, row / tile offsets, pad-strip and label gather indices
            ent["set_padding"](pad)
            dst = [d[:, :B] if i < 4 else d[:B] for i, d in enumerate(ent["static"])]
            fl = [(d, s_) for d, s_ in zip(dst, inputs) if d.is_floating_point()]
            it = [(d, s_) for d, s_ in zip(dst, inputs) if not d.is_floating_point()]
            for grp in (fl, it):
                if grp:
                    torch._foreach_copy_([x[0] for x in grp], [x[1] for x in grp], non_blocking=True)
        cap = ent["cap"]
        try:
            loss = self._replay(cap)
        except RuntimeError as exc:
            if "storage moved" not in str(exc):
                raise
            del self.entries[key]
            self.recaptures += 1
            return self._step_bucketed(inputs, lengths, train_flag)
        if train_flag:
            self._hand_over_grads(ent)
        self.last_entry = ent
        self.last_pred = ent["out"]["pred"][:N]
        return loss, ent["out"]["log_prob"][:N], ent["flat"][:N]

    @staticmethod
    def signature(shapes, lengths, train_flag, test_label=False):
        return (bool(train_flag), bool(test_label), tuple(int(x) for x in lengths)) + tuple(tuple(s_) for s_ in shapes)

    def claim_static(self, shapes, lengths, train_flag, test_label=False):
        """For a loader that stages batches on the device (data.DevicePrefetcher(graph_cache=...)): the static input
        buffers of the captured step this batch will replay, or None (signature not captured yet, or its buffers are
        already promised to a staged batch that has not been stepped).  The caller copies the batch INTO them (after
        waiting for ``entry["done"]``, the event behind the entry's last replay) and hands exactly these tensors to
        ``step``, which then has nothing to copy."""
        key = self.signature(shapes, lengths, train_flag, test_label)
        if self.bucket_rows:
            return None               # bucketed entries serve many batches: their static buffers are filled by the step itself
        # every announced batch counts, claimed or not: the static buffers are handed out only when NO earlier batch of this
        # signature is still waiting to be stepped -- such a batch (staged elsewhere) is copied into the same buffers by its
        # step, on the compute stream, unordered with a later batch's direct copy on the loader's stream (with repeated
        # signatures inside the prefetch window the later batch's data would be overwritten, or replayed under the wrong
        # batch's name)
        ahead = self.queued.get(key, 0)
        self.queued[key] = ahead + 1
        ent = self.entries.get(key)
        if ent is None or ahead or ent.get("reserved"):
            return None
        ent["reserved"] = True
        return ent

    def forget_queued(self):
        """Drop the announcements of batches that will never be stepped (a pass abandoned mid-way)."""
        self.queued.clear()
        for ent in self.entries.values():
            ent["reserved"] = False

    def step(self, inputs, lengths, train_flag, test_label=False):
        """inputs = (textf, visuf, acouf, qmask, umask, label) on the device.  Returns (loss, log_prob, flat_labels):
        tensors owned by the cache entry -- consume (or clone) them before this signature is stepped again."""
        key = self.signature([t.shape for t in inputs], lengths, train_flag, test_label)
        if self.bucket_rows and self._bucketable(inputs, lengths, test_label):
            return self._step_bucketed(inputs, lengths, train_flag)
        ent = self.entries.get(key)
        if self.queued.get(key, 0) > 0:
            self.queued[key] -= 1
            if not self.queued[key]:
                del self.queued[key]
        if ent is not None and ent.get("reserved") and any(d is not s_ for d, s_ in zip(ent["static"], inputs)):
            # the static buffers are promised to (and being filled for) another staged batch: copying this one over them
            # would race with that copy
            raise RuntimeError("StepGraphCache.step: this signature's static inputs are reserved for a later staged batch; "
                               "step batches in the order they were announced with claim_static")
        if ent is None:
            self.misses += 1
            # (feature widths that are not multiples of 4 get row-padded static buffers: ops.py "row padding")
            static = [ops.pad_rows(t) if ops.is_odd_feature_tensor(t, i in ops.FEATURE_SLOTS) else t.clone()
                      for i, t in enumerate(inputs)]
            textf, visuf, acouf, qmask, umask, label = static
            # dialogue-major label flatten (run_train_erc.py:201) as a static gather: a boolean-mask select has a
            # data-dependent shape and cannot be captured
            Lp = label.shape[1]
            pos = torch.cat([torch.arange(int(n)) + j * Lp for j, n in enumerate(lengths)]).to(label.device)
            flat = label.reshape(-1).index_select(0, pos)
            out = {}
            model, loss_f, stats = self.model, self.loss_f, self.pass_stats

            def fn():
                torch.index_select(label.reshape(-1), 0, pos, out=flat)     # inside the graph: this batch's labels
                out["log_prob"] = model(textf, qmask, umask, lengths, acouf, visuf, test_label)[0]
                if stats is None:
                    out["pred"] = torch.argmax(out["log_prob"], 1)          # (the pass loop's per-step metric input)
                loss = loss_f(out["log_prob"], flat)
                if stats is not None:                          # predictions + this batch's counts: one launch, no argmax
                    out["pred"] = stats.update(out["log_prob"], flat, loss)
                if train_flag:
                    backward(loss)
                return loss

            mode = model.training
            model.train(train_flag)
            with torch.set_grad_enabled(bool(train_flag)):
                cap = self._capture(fn, train_flag)
            model.train(mode)
            # everything the graph reads that was allocated OUTSIDE the capture must live as long as the graph: the
            # static inputs, the label gather index and the flattened labels (the closure itself is kept by cap)
            ent = dict(static=static, cap=cap, out=out, flat=flat, pos=pos, pending=None)
            self.entries[key] = ent
            while len(self.entries) > self.max_entries:
                self.entries.popitem(last=False)
        else:
            self.hits += 1
            self.entries.move_to_end(key)
            if ent.get("pending") is not None:
                ent["pending"]()               # results of this entry's previous step are still referenced: copy them out first
                ent["pending"] = None
            # the batch goes into the entry's static buffers as ONE multi-tensor copy per dtype (two launches instead of six)
            fl = [(d, s_) for d, s_ in zip(ent["static"], inputs) if d.is_floating_point() and d is not s_]
            it = [(d, s_) for d, s_ in zip(ent["static"], inputs) if not d.is_floating_point() and d is not s_]
            for grp in (fl, it):
                if grp:
                    torch._foreach_copy_([g[0] for g in grp], [g[1] for g in grp], non_blocking=True)
        ent["reserved"] = False
        cap = ent["cap"]
        try:
            loss = self._replay(cap)
        except RuntimeError as exc:
            if "storage moved" not in str(exc):
                raise
            # the parameters were re-pointed after this entry was captured (FlatAdam lays them out in its flat buffer
            # at its first step; .to(); load_state_dict(assign=True)): the entry is stale, capture the signature again
            del self.entries[key]
            self.recaptures += 1
            return self.step(inputs, lengths, train_flag, test_label)
        if train_flag:
            self._hand_over_grads(ent)
        self.last_entry = ent
        self.last_pred = ent["out"]["pred"]
        if loss.is_cuda:
            done = ent.get("done")
            if done is None:
                done = ent["done"] = torch.cuda.Event()
            done.record(torch.cuda.current_stream(loss.device))       # the static inputs may be refilled after this
        return loss, ent["out"]["log_prob"], ent["flat"]


def train_or_eval_graph_model(model, loss_f, dataloader, epoch=0, train_flag=False, optimizer=None, cuda_flag=False,
                              modals=None, target_names=None, test_label=False, tensorboard=False, seed=2021,
                              step_hook=None, graph_cache=None, device_metrics=False, reduce_group=None):
    """``graph_cache``: a StepGraphCache (or None = launch every step eagerly, as before).  A cache that owns its optimizer
    (StepGraphCache(optimizer=...)) steps it inside the replayed graph: ``optimizer`` must be that object, there is no place
    for a ``step_hook`` between backward and update, and only steps that bypass the cache (``test_label``) call
    ``optimizer.step()`` here.
    ``device_metrics=True``: the pass keeps no per-step predictions, labels or losses.  Every step adds its batch to a PassStats
    -- ``graph_cache.pass_stats``, counted by a node of the replayed step, or a private one for the eager loop (classes from the
    first ``log_prob``, device from the batch) -- which is read back ONCE at the end; accuracy, weighted F1 and the per-class
    figures are closed forms of its confusion matrix, ``avg_loss`` the float64 mean of the batch losses.  Same 8-tuple, but
    positions 4 and 5 hold the matrix expanded (PassStats.as_arrays: grouped by (label, prediction), NOT in utterance order --
    metrics that need the order, ``vids`` alignment, keep the default path).  ``reduce_group``: a process group the statistics
    are summed over before they are read (data parallelism: every rank then reports the same global metrics; the per-batch
    losses of the last position stay this rank's).  A cache without a ``pass_stats`` raises ValueError."""
    losses, preds, labels = [], [], []
    stats, nsteps = None, 0
    if device_metrics:
        if graph_cache is not None:
            stats = getattr(graph_cache, "pass_stats", None)
            if stats is None:
                raise ValueError("train_or_eval_graph_model: device_metrics=True needs a StepGraphCache built with pass_stats= "
                                 "(its captured steps would keep the per-step book-keeping otherwise)")
            stats.set_enabled(True)
            stats.reset()
    assert not train_flag or optimizer is not None
    in_graph_opt = graph_cache is not None and getattr(graph_cache, "optimizer", None) is not None
    if in_graph_opt and train_flag:
        if optimizer is not graph_cache.optimizer:
            raise ValueError("train_or_eval_graph_model: graph_cache steps its own optimizer inside the captured step; pass that "
                             "object as optimizer")
        if step_hook is not None:
            raise ValueError("train_or_eval_graph_model: step_hook cannot run between backward and an optimizer step that are "
                             "nodes of one captured graph (StepGraphCache(optimizer=...))")
    model.train() if train_flag else model.eval()
    seed_everything(seed)
    vids = []
    if hasattr(dataloader, "bind_graph_cache"):
        # a device-staging loader copies every batch whose signature is already captured straight into that step's static
        # input buffers (data.DevicePrefetcher): nothing is left to copy on the device
        dataloader.bind_graph_cache(graph_cache if not test_label else None, train_flag)
    for data in dataloader:
        if train_flag and graph_cache is None:
            optimizer.zero_grad()         # (a replayed step hands over fresh gradient tensors: nothing to reset)
        textf, visuf, acouf, qmask, umask, label = [d.cuda() for d in data[:6]] if cuda_flag else data[:6]
        lengths = getattr(data, "lengths", None) or lengths_from_umask(umask)
        stepped_in_graph = False
        if graph_cache is not None and not test_label:      # (the --test_label dumps call .cpu() / np.save: never captured)
            stepped_in_graph = in_graph_opt and train_flag
            loss, log_prob, flat = graph_cache.step((textf, visuf, acouf, qmask, umask, label), lengths, train_flag,
                                                    test_label)
            nsteps += 1
            # (device_metrics: the replayed step counted this batch itself -- nothing of the entry is referenced after the step)
            if stats is None:
                # metrics are deferred to the end of the pass: the step's predictions, labels and loss stay where the graph
                # wrote them (no per-step copy launches) unless this cache entry is stepped again before the pass ends, in
                # which case they are copied out first (StepGraphCache runs the entry's ``pending`` closure)
                ent = graph_cache.last_entry
                slot = len(preds)
                preds.append(graph_cache.last_pred)
                labels.append(flat)
                losses.append(loss.detach())

                def materialise(slot=slot):
                    preds[slot], labels[slot], losses[slot] = preds[slot].clone(), labels[slot].clone(), losses[slot].clone()
                ent["pending"] = materialise
        else:
            log_prob, e_i, e_n, e_t, e_l = model(textf, qmask, umask, lengths, acouf, visuf, test_label)
            flat = flatten_labels(label, lengths)
            loss = loss_f(log_prob, flat)
            nsteps += 1
            if device_metrics:
                if stats is None:         # no cache: a private block, sized by the first batch
                    stats = PassStats(log_prob.shape[1], log_prob.device)
                stats.update(log_prob, flat, loss)
            else:
                preds.append(torch.argmax(log_prob, 1))
                labels.append(flat)
                losses.append(loss.detach())
            if train_flag:
                backward(loss)
        if train_flag:
            ops.join_weight_grads()       # weight gradients still queued are written to .grad here
            if not stepped_in_graph:      # (else the replayed graph ended with the pack and the update)
                if step_hook is not None:
                    step_hook(model)          # e.g. data-parallel gradient all-reduce
                optimizer.step()
        if len(data) > 6:
            vids = data[6]
    if not nsteps:
        return [], [], float('nan'), float('nan'), [], [], float('nan'), []
    if graph_cache is not None:
        for ent in graph_cache.entries.values():
            ent["pending"] = None             # everything is consumed right below
    from sklearn import metrics
    from sklearn.metrics import accuracy_score, f1_score
    if device_metrics:
        if reduce_group is not None:
            stats.all_reduce(reduce_group)
        stats.fetch()                         # the pass's one device -> host copy
        labels, preds = stats.as_arrays()
        losses = stats.batch_losses()
        avg_loss = round(stats.loss_mean(), 4)
        avg_accuracy = round(stats.accuracy() * 100, 2)
        avg_fscore = round(stats.weighted_f1() * 100, 2)
    else:
        preds = torch.cat(preds).cpu().numpy()
        labels = torch.cat(labels).cpu().numpy()
        losses = torch.stack(losses).cpu().numpy()
        avg_loss = round(float(np.sum(losses)) / len(losses), 4)
        avg_accuracy = round(accuracy_score(labels, preds) * 100, 2)
        avg_fscore = round(f1_score(labels, preds, average='weighted') * 100, 2)
    all_each, all_acc = "", ["ACC"]
    if target_names is not None:
        all_each = metrics.classification_report(labels, preds, target_names=target_names, digits=4,
                                                 labels=list(range(len(target_names))), zero_division=0)
        for i, name in enumerate(target_names):
            sel = labels == i
            acc = accuracy_score(labels[sel], preds[sel]) if sel.any() else float('nan')
            all_acc.append("{}: {:.4f}".format(name, acc))
    return all_each, all_acc, avg_loss, avg_accuracy, labels, preds, avg_fscore, [np.array(vids), losses]


def train_or_eval_model(model, loss_f, dataloader, epoch=0, train_flag=False, optimizer=None, cuda_flag=False,
                        target_names=None, tensorboard=False):
    """The pass loop of the reference's recurrent models (run_train_erc.py:92-146: GRUModel and friends with MaskedNLLLoss):
    same arguments, same 9-tuple ``(all_each, all_acc, avg_loss, avg_accuracy, labels, preds, masks, avg_fscore, [alphas,
    alphas_f, alphas_b, vids])``.  Kept: batch tuple order (:106), the model call (:107), the dialogue-major flatten of the
    log-probabilities (:108), metrics weighted by the utterance mask (:137-139), attention weights collected in evaluation
    passes only (:125-128).  Changed for the device: the step runs eagerly through ``backward`` (the step's weight gradients
    leave as one batch) and ``ops.join_weight_grads()`` in front of ``optimizer.step()``; predictions, labels, masks and
    losses stay on the device and are copied to the host once at the end of the pass.  ``tensorboard`` is accepted and ignored
    (the reference's writer is a global of its script)."""
    losses, preds, labels, masks = [], [], [], []
    alphas, alphas_f, alphas_b, vids = [], [], [], []
    assert not train_flag or optimizer is not None
    model.train() if train_flag else model.eval()
    for data in dataloader:
        if train_flag:
            optimizer.zero_grad()
        textf, visuf, acouf, qmask, umask, label = [d.cuda() for d in data[:-1]] if cuda_flag else data[:-1]
        log_prob, alpha, alpha_f, alpha_b, _ = model(textf, qmask, umask)
        lp_ = log_prob.transpose(0, 1).contiguous().view(-1, log_prob.size()[2])
        labels_ = label.view(-1)
        loss = loss_f(lp_, labels_, umask)
        preds.append(torch.argmax(lp_.detach(), 1))
        labels.append(labels_)
        masks.append(umask.reshape(-1))
        losses.append(loss.detach())
        if train_flag:
            backward(loss)
            ops.join_weight_grads()       # weight gradients still queued are written to .grad here
            optimizer.step()
        else:
            alphas += alpha
            alphas_f += alpha_f
            alphas_b += alpha_b
            vids += data[-1]
    if not preds:
        return [], [], float('nan'), float('nan'), [], [], [], float('nan'), []
    # the pass's one round of device -> host copies
    counts = torch.stack([m.to(torch.float64).sum() for m in masks]).cpu().numpy()       # (run_train_erc.py:117)
    preds = torch.cat(preds).cpu().numpy()
    labels = torch.cat(labels).cpu().numpy()
    masks = torch.cat(masks).cpu().numpy()
    losses = torch.stack(losses).to(torch.float64).cpu().numpy()
    from sklearn import metrics
    from sklearn.metrics import accuracy_score, f1_score
    avg_loss = round(float(np.sum(losses * counts)) / float(np.sum(masks)), 4)
    avg_accuracy = round(accuracy_score(labels, preds, sample_weight=masks) * 100, 2)
    avg_fscore = round(f1_score(labels, preds, sample_weight=masks, average='weighted') * 100, 2)
    all_each, all_acc = "", ["ACC"]
    if target_names is not None:
        all_each = metrics.classification_report(labels, preds, target_names=target_names, digits=4,
                                                 labels=list(range(len(target_names))), zero_division=0)
        for i, name in enumerate(target_names):
            sel = labels == i
            acc = accuracy_score(labels[sel], preds[sel]) if sel.any() else float('nan')
            all_acc.append("{}: {:.4f}".format(name, acc))
    return all_each, all_acc, avg_loss, avg_accuracy, labels, preds, masks, avg_fscore, [alphas, alphas_f, alphas_b, vids]


def fit(model, loss_f, optimizer, train_loader, valid_loader, test_loader, n_epochs, patience=10, valid_rate=0.1,
        cuda_flag=False, modals=None, target_names=None, run_pass=None, log=print, step_hook=None, graph_cache=None,
        device_metrics=False, reduce_group=None):
    """The epoch loop of run_train_erc.py:531-660: train / valid / test pass per epoch, model selection on the
    validation weighted-F1 (on the test split when valid_rate == 0), and the DUAL-patience early stop -- the run
    ends only when neither the F1 (strict improvement, :614-618) nor the loss (:619-627) has improved for
    ``patience`` epochs (:637).  Returns the history and the test metrics at the two selected epochs (:641-660).

    ``graph_cache=True`` replays a captured step per batch signature (StepGraphCache) instead of launching eagerly.
    ``device_metrics`` / ``reduce_group``: handed to every pass (train_or_eval_graph_model); ``graph_cache=True`` then builds
    the cache with a PassStats (classes from ``model.smax_fc``).  With ``reduce_group`` the stopping rule sees the same global
    F1 and loss on every rank.
    ``run_pass(loader, epoch, train_flag) -> (all_each, all_acc, loss, acc, labels, preds, fscore, extras)``
    defaults to ``train_or_eval_graph_model``; tests drive the stopping rule with a stub."""
    if graph_cache is True:
        stats = None
        if device_metrics:
            stats = PassStats(model.smax_fc.out_features, next(model.parameters()).device, ignore_index=StepGraphCache.IGNORE)
        graph_cache = StepGraphCache(model, loss_f, pass_stats=stats)
    if run_pass is None:
        def run_pass(loader, epoch, train_flag):
            return train_or_eval_graph_model(model, loss_f, loader, epoch=epoch, train_flag=train_flag,
                                             optimizer=optimizer if train_flag else None, cuda_flag=cuda_flag,
                                             modals=modals, target_names=target_names, step_hook=step_hook,
                                             graph_cache=graph_cache, device_metrics=device_metrics,
                                             reduce_group=reduce_group)
    hist = dict(train_loss=[], train_fscore=[], valid_loss=[], valid_fscore=[], test_loss=[], test_acc=[], test_fscore=[])
    best_epoch, best_epoch2, pat, pat2, best_eval_fscore, best_eval_loss = -1, -1, 0, 0, 0, None
    last = None
    for e in range(n_epochs):
        for ld in (train_loader, valid_loader, test_loader):
            bs = getattr(ld, "batch_sampler", None)
            if hasattr(bs, "set_epoch"):
                bs.set_epoch(e)
        _, _, train_loss, train_acc, _, _, train_fscore, _ = run_pass(train_loader, e, True)
        _, _, valid_loss, valid_acc, _, _, valid_fscore, _ = run_pass(valid_loader, e, False)
        last = run_pass(test_loader, e, False)
        all_each, all_acc, test_loss, test_acc, test_label, test_pred, test_fscore, _ = last
        for k, v in (("train_loss", train_loss), ("train_fscore", train_fscore), ("valid_loss", valid_loss),
                     ("valid_fscore", valid_fscore), ("test_loss", test_loss), ("test_acc", test_acc),
                     ("test_fscore", test_fscore)):
            hist[k].append(v)
        eval_loss, eval_fscore = (valid_loss, valid_fscore) if valid_rate > 0 else (test_loss, test_fscore)
        if e == 0 or best_eval_fscore < eval_fscore:
            pat, best_epoch, best_eval_fscore = 0, e, eval_fscore
        else:
            pat += 1
        if best_eval_loss is None:
            best_eval_loss, best_epoch2 = eval_loss, 0
        elif eval_loss < best_eval_loss:
            best_epoch2, best_eval_loss, pat2 = e, eval_loss, 0
        else:
            pat2 += 1
        if log is not None:
            log('epoch: {}, train_loss: {}, train_acc: {}, train_fscore: {}, valid_loss: {}, valid_acc: {}, valid_fscore: {}, '
                'test_loss: {}, test_acc: {}, test_fscore: {}'.format(e, train_loss, train_acc, train_fscore, valid_loss,
                                                                      valid_acc, valid_fscore, test_loss, test_acc, test_fscore))
        if pat >= patience and pat2 >= patience:
            if log is not None:
                log('Early stoping... {} {}'.format(pat, pat2))
            break
    pick = lambda ep, key: hist[key][ep] if ep >= 0 else 0
    return dict(history=hist, epochs_run=len(hist["test_fscore"]), patience=(pat, pat2),
                by_f1=dict(epoch=best_epoch, eval_fscore=best_eval_fscore, test_acc=pick(best_epoch, "test_acc"),
                           test_fscore=pick(best_epoch, "test_fscore")),
                by_loss=dict(epoch=best_epoch2, eval_loss=best_eval_loss, test_acc=pick(best_epoch2, "test_acc"),
                             test_fscore=pick(best_epoch2, "test_fscore")),
                last_test=last)


def load_reference_weights(model, source, strict=True):
    """Loads weights trained with the reference into ``model``.  ``source`` is a state_dict or the path of a file
    holding one (``torch.save(model.state_dict(), path)`` on the reference side: the key set is identical, see
    tests/golden/state_dict_keys_iemocap.txt).  The reference's own ``torch.save(model)`` files (opened with torch.load at run_train_erc.py:532)
    are pickles of ITS classes and can only be opened where that code is importable; convert them there with
    ``torch.save(torch.load(p).state_dict(), q)``."""
    sd = torch.load(source, map_location="cpu") if isinstance(source, (str, bytes)) else source
    if not isinstance(sd, dict):
        sd = sd.state_dict()
    return model.load_state_dict(sd, strict=strict)
