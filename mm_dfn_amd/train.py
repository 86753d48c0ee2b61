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

from . import ops


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

    def __init__(self, model, loss_f, max_entries=96, warmup=2, bucket_rows=0, larger_bucket_fallback=True, optimizer=None):
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
        disabled."""
        from collections import OrderedDict
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
        try:
            made = self._precapture_walk(loader, train_flag, device)
        finally:
            self._exact_buckets = False
            if self.optimizer is not None:
                self.optimizer.set_enabled(True)
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
        from .graphs import CapturedStep
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
            model, loss_f = self.model, self._loss_ign
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
                    out["pred"] = torch.argmax(out["log_prob"], 1)
                    loss = loss_f(out["log_prob"], flat)
                    if train_flag:
                        backward(loss)
                return loss

            mode = model.training
            model.train(train_flag)
            with torch.set_grad_enabled(bool(train_flag)):
                cap = CapturedStep(model, fn, warmup=self.warmup, optimizer=self.optimizer if train_flag else None)
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
            loss = cap.replay()
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
        from .graphs import CapturedStep
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
            model, loss_f = self.model, self.loss_f

            def fn():
                torch.index_select(label.reshape(-1), 0, pos, out=flat)     # inside the graph: this batch's labels
                out["log_prob"] = model(textf, qmask, umask, lengths, acouf, visuf, test_label)[0]
                out["pred"] = torch.argmax(out["log_prob"], 1)          # (the pass loop's per-step metric input)
                loss = loss_f(out["log_prob"], flat)
                if train_flag:
                    backward(loss)
                return loss

            mode = model.training
            model.train(train_flag)
            with torch.set_grad_enabled(bool(train_flag)):
                cap = CapturedStep(model, fn, warmup=self.warmup, optimizer=self.optimizer if train_flag else None)
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
            loss = cap.replay()
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
                              step_hook=None, graph_cache=None):
    """``graph_cache``: a StepGraphCache (or None = launch every step eagerly, as before).  A cache that owns its optimizer
    (StepGraphCache(optimizer=...)) steps it inside the replayed graph: ``optimizer`` must be that object, there is no place
    for a ``step_hook`` between backward and update, and only steps that bypass the cache (``test_label``) call
    ``optimizer.step()`` here."""
    losses, preds, labels = [], [], []
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
    if not preds:
        return [], [], float('nan'), float('nan'), [], [], float('nan'), []
    if graph_cache is not None:
        for ent in graph_cache.entries.values():
            ent["pending"] = None             # everything is consumed right below
    preds = torch.cat(preds).cpu().numpy()
    labels = torch.cat(labels).cpu().numpy()
    losses = torch.stack(losses).cpu().numpy()
    avg_loss = round(float(np.sum(losses)) / len(losses), 4)
    from sklearn import metrics
    from sklearn.metrics import accuracy_score, f1_score
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


def fit(model, loss_f, optimizer, train_loader, valid_loader, test_loader, n_epochs, patience=10, valid_rate=0.1,
        cuda_flag=False, modals=None, target_names=None, run_pass=None, log=print, step_hook=None, graph_cache=None):
    """The epoch loop of run_train_erc.py:531-660: train / valid / test pass per epoch, model selection on the
    validation weighted-F1 (on the test split when valid_rate == 0), and the DUAL-patience early stop -- the run
    ends only when neither the F1 (strict improvement, :614-618) nor the loss (:619-627) has improved for
    ``patience`` epochs (:637).  Returns the history and the test metrics at the two selected epochs (:641-660).

    ``graph_cache=True`` replays a captured step per batch signature (StepGraphCache) instead of launching eagerly.
    ``run_pass(loader, epoch, train_flag) -> (all_each, all_acc, loss, acc, labels, preds, fscore, extras)``
    defaults to ``train_or_eval_graph_model``; tests drive the stopping rule with a stub."""
    if graph_cache is True:
        graph_cache = StepGraphCache(model, loss_f)
    if run_pass is None:
        def run_pass(loader, epoch, train_flag):
            return train_or_eval_graph_model(model, loss_f, loader, epoch=epoch, train_flag=train_flag,
                                             optimizer=optimizer if train_flag else None, cuda_flag=cuda_flag,
                                             modals=modals, target_names=target_names, step_hook=step_hook,
                                             graph_cache=graph_cache)
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
