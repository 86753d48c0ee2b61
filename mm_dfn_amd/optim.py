"""FlatAdam: the reference's optimizer (torch.optim.Adam(lr, weight_decay=l2), run_train_erc.py:512) as ONE
fused HIP launch per step over flat buffers.

All parameters that receive gradients are re-pointed at slices of one contiguous fp32 buffer and their
gradients are packed into a matching flat buffer (the same bucket the data-parallel all-reduce uses), so the
update is a single elementwise kernel (csrc/optimizer.hip).  Parameters the MM-DFN configuration never reaches
get no gradient and are left untouched, exactly like torch.optim.Adam skips ``grad is None``.

Device-state path (``capturable`` / ``max_grad_norm`` / ``skip_nonfinite``, csrc/optimizer_state.hip): the step count, the bias
corrections, lr / weight decay, the global gradient norm, its clip factor and the skip decision live in a 64-byte block of
device memory (``_hip.AdamState``), so ``step()`` launches nothing whose arguments change from step to step -- it can be captured
behind the backward pass (graphs.CapturedStep(optimizer=...)) -- and clipping / skipping cost no host synchronisation.
"""
import ctypes

import torch

from . import _hip
from .distributed import GradientBucket, register_slots, slot_pieces, slot_size, slot_view


class FlatAdam:
    PARTIALS = 1024                # doubles of the norm's workspace: one per workgroup of mmdfn_grad_sumsq

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, bucket=None, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False):
        """``capturable`` / ``max_grad_norm`` / ``skip_nonfinite``: any of them selects the device-state path (module docstring).
        ``max_grad_norm``: global-norm clipping, torch.nn.utils.clip_grad_norm_'s factor min(1, max / (norm + 1e-6));
        ``skip_nonfinite``: a step whose flat gradient holds an inf / NaN leaves parameters, moments and the step count alone
        and is counted in ``skipped_steps``."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("FlatAdam: max_grad_norm must be positive (None = no clipping), got %r" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.device_state = bool(capturable) or self.max_grad_norm is not None or self.skip_nonfinite
        self._state = self._partials = None      # the device block (16 int32 words) and the norm's workspace
        self._pushed = None                      # (lr, weight_decay) the block holds
        self._enabled = True
        self._captured_args = None               # (betas, eps) baked into captured launches of step()
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.bucket = bucket if bucket is not None else GradientBucket(model, average=True)
        self._t = 0
        self.flat_p = self.m = self.v = None
        # torch.optim-style handle for LR schedulers: ``step`` reads lr / weight_decay from here
        self.param_groups = [dict(params=[p for p in model.parameters() if p.requires_grad], lr=self.lr,
                                  betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)]

    # ---- the step count: a host integer, or (device-state path, once the block exists) the block's counter
    @property
    def t(self):
        if self._state is not None:
            return int(self._state[_hip.adam_state_word("step")].item())       # (a device -> host sync)
        return self._t

    @t.setter
    def t(self, value):
        self._t = int(value)
        if self._state is not None:
            self._state[_hip.adam_state_word("step")].fill_(self._t)

    def _ensure_state(self, device):
        if self._state is not None:
            return
        grp = self.param_groups[0]
        lr, wd = float(grp["lr"]), float(grp["weight_decay"])
        host = _hip.AdamState(step=self._t, enabled=int(self._enabled), skip_nonfinite=int(self.skip_nonfinite), lr=lr,
                              weight_decay=wd, max_norm=self.max_grad_norm or 0.0, scale=1.0)
        words = torch.frombuffer(bytearray(bytes(host)), dtype=torch.int32)
        assert words.numel() * 4 == int(_hip.query("mmdfn_adam_state_bytes"))
        self._state = words.to(device)
        self._partials = torch.zeros(self.PARTIALS, dtype=torch.float64, device=device)
        self._pushed = (lr, wd)

    def _push_hyper(self):
        """lr / weight_decay of ``param_groups[0]`` into the block: one small stream-ordered copy, only when they changed since
        the last one (an LR scheduler).  Never under stream capture -- CapturedStep.replay() calls it in front of the launch."""
        grp = self.param_groups[0]
        now = (float(grp["lr"]), float(grp["weight_decay"]))
        if self._state is None or now == self._pushed:
            return
        w = _hip.adam_state_word("lr")
        self._state[w:w + 2].copy_(torch.tensor(now, dtype=torch.float32).view(torch.int32), non_blocking=True)
        self._pushed = now

    def set_enabled(self, flag):
        """``False``: every launch of ``step()`` -- replays of a captured one included -- leaves parameters, moments and the
        step count untouched (StepGraphCache.precapture replays its entries this way)."""
        self._enabled = bool(flag)
        if self._state is not None:
            self._state[_hip.adam_state_word("enabled")].fill_(int(self._enabled))

    @property
    def grad_norm(self):
        """Global norm of the latest step's flat gradient (before clipping) as a 0-dim device tensor: a view of the block, no
        sync.  Computed only with ``max_grad_norm`` / ``skip_nonfinite``; 0 otherwise."""
        self._need_state("grad_norm")
        w = _hip.adam_state_word("grad_norm")
        return self._state[w:w + 1].view(torch.float32)[0]

    @property
    def skipped_steps(self):
        self._need_state("skipped_steps")
        return int(self._state[_hip.adam_state_word("skipped")].item())        # (a device -> host sync)

    def _need_state(self, what):
        if not self.device_state:
            raise RuntimeError("FlatAdam.%s needs the device-state path (capturable / max_grad_norm / skip_nonfinite)" % what)
        if self._state is None:
            self._ensure_state(next(p for p in self.model.parameters() if p.requires_grad).device)

    def prepare_for_capture(self):
        """Everything ``step()`` would set up on its first call, without an update: packs the gradients of the backward pass that
        has just run (the flat layout is the set of parameters that received one), re-points the parameters into the flat buffer,
        creates the device block.  Afterwards ``step(grads_already_flat=True)`` only launches (capturable)."""
        if self.bucket.flat is None:
            self.bucket.flatten()
        _hip.require_cuda(self.bucket.flat)
        if self.flat_p is None:
            self._materialise()
        if self.device_state:
            self._ensure_state(self.bucket.flat.device)
            if not torch.cuda.is_current_stream_capturing():
                self._push_hyper()

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad(set_to_none=True)

    def _materialise(self):
        params = self.bucket.params
        # one slot per parameter (16-byte aligned starts; a row-padded block for weights of odd contraction width,
        # distributed.slot_size): the same layout as the gradient bucket, so the update is one elementwise pass
        flat = torch.cat([piece for p in params for piece in slot_pieces(p.detach(), p)])
        register_slots(flat, params)
        off = 0
        for p in params:
            p.data = slot_view(flat, off, p)
            p._mmdfn_flat = True       # this storage layout is owned here: nobody may re-point the parameter
            off += slot_size(p)
        self.flat_p = flat
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)

    @torch.no_grad()
    def step(self, grads_already_flat=False):
        """Pack gradients (unless the caller already did, e.g. after the data-parallel all-reduce) and update."""
        if not grads_already_flat:
            # (single process: nothing reads the gradients as views of the bucket, so they are only packed)
            self.bucket.flatten(attach=self.flat_p is None)
        g = self.bucket.flat
        _hip.require_cuda(g)
        if self.flat_p is None:
            self._materialise()
        if self.device_state:
            return self._step_device_state(g)
        self._t += 1
        grp = self.param_groups[0]
        _hip.call("mmdfn_adam_step", _hip.ptr(self.flat_p), _hip.ptr(g), _hip.ptr(self.m), _hip.ptr(self.v),
                  g.numel(), float(grp["lr"]), self.betas[0], self.betas[1], self.eps,
                  float(grp["weight_decay"]), self._t, _hip.stream())
        # the kernel wrote the parameters behind autograd's version counters: piece planes cut from them are stale now
        from . import ops
        ops.invalidate_planes()

    def _step_device_state(self, g):
        """[sum of squares ->] prepare -> update: no argument depends on the step, lr / weight decay are read from the block."""
        self._ensure_state(g.device)
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            self._captured_args = (self.betas, self.eps)
        else:
            self._push_hyper()
        st, stream = _hip.ptr(self._state), _hip.stream()
        partials, nparts = None, 0
        if self.max_grad_norm is not None or self.skip_nonfinite:
            count = ctypes.c_int(0)
            _hip.call("mmdfn_grad_sumsq", _hip.ptr(g), g.numel(), _hip.ptr(self._partials), self.PARTIALS, ctypes.byref(count), stream)
            partials, nparts = _hip.ptr(self._partials), count.value
        _hip.call("mmdfn_adam_prepare", st, partials, nparts, self.betas[0], self.betas[1], stream)
        _hip.call("mmdfn_adam_step_state", _hip.ptr(self.flat_p), _hip.ptr(g), _hip.ptr(self.m), _hip.ptr(self.v), g.numel(), st,
                  self.betas[0], self.betas[1], self.eps, stream)
        if not capturing:
            # (a captured step's weights change at every REPLAY: CapturedStep.replay() invalidates behind its launch)
            from . import ops
            ops.invalidate_planes()

    # ---- checkpointing: per-parameter moments under the parameter NAMES (layout-independent, loads into a bucket
    # whose flat order differs), plus the step count and the hyper-parameters
    def state_dict(self):
        names = {id(p): n for n, p in self.model.named_parameters()}
        state = {}
        if self.flat_p is not None:
            off = 0
            for p in self.bucket.params:
                state[names[id(p)]] = dict(exp_avg=slot_view(self.m, off, p).contiguous().clone(),
                                           exp_avg_sq=slot_view(self.v, off, p).contiguous().clone())
                off += slot_size(p)
        grp = self.param_groups[0]
        return dict(step=self.t, lr=float(grp["lr"]), betas=self.betas, eps=self.eps,
                    weight_decay=float(grp["weight_decay"]), state=state)

    def load_state_dict(self, sd):
        """Needs the bucket layout, i.e. call after one backward pass (or pass a bucket that has been flattened).
        betas and eps are plain kernel arguments: a captured ``step()`` holds the values of its capture, so a checkpoint with
        other values is refused once a step has been captured -- load it first, or capture again with a new optimizer."""
        betas, eps = (float(sd["betas"][0]), float(sd["betas"][1])), float(sd["eps"])
        if self._captured_args is not None and (betas, eps) != self._captured_args:
            raise RuntimeError("FlatAdam.load_state_dict: betas / eps %r differ from %r, which captured steps of this optimizer "
                               "hold as kernel arguments; load the checkpoint before capturing" % ((betas, eps), self._captured_args))
        self.t = int(sd["step"])
        self.betas, self.eps = betas, eps
        self.param_groups[0]["lr"] = self.lr = float(sd["lr"])
        self.param_groups[0]["weight_decay"] = self.weight_decay = float(sd["weight_decay"])
        if not sd["state"]:
            return
        if self.bucket.params is None:
            raise RuntimeError("FlatAdam.load_state_dict: run one backward pass first (the flat layout is the set of "
                               "parameters that receive gradients)")
        if self.flat_p is None:
            self._materialise()
        names = {id(p): n for n, p in self.model.named_parameters()}
        off = 0
        for p in self.bucket.params:
            st = sd["state"][names[id(p)]]
            slot_view(self.m, off, p).copy_(st["exp_avg"].view_as(p))
            slot_view(self.v, off, p).copy_(st["exp_avg_sq"].view_as(p))
            off += slot_size(p)
