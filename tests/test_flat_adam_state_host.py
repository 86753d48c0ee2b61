"""Host side of FlatAdam on device-resident step state: constructor validation, the combinations CapturedStep / StepGraphCache /
the pass loop refuse, and the layout of ``mmdfn_adam_state`` in the header against its ctypes mirror (no device needed)."""
import ctypes
import os
import re

import pytest

from mm_dfn_amd import FocalLoss, _hip, train
from mm_dfn_amd.graphs import CapturedStep
from mm_dfn_amd.optim import FlatAdam
from test_fusion_baselines import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_selects_the_device_state_path_and_validates_the_clip_norm():
    m = build("lmf_only")
    assert not FlatAdam(m).device_state
    assert FlatAdam(m, capturable=True).device_state
    assert FlatAdam(m, max_grad_norm=1.0).device_state and FlatAdam(m, max_grad_norm=1.0).max_grad_norm == 1.0
    assert FlatAdam(m, skip_nonfinite=True).device_state
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FlatAdam(m, max_grad_norm=bad)
    # the step count is a plain host integer until a device block exists; the plain path's accessors say what they need
    opt = FlatAdam(m, capturable=True)
    opt.t = 7
    assert opt.t == 7 and opt.state_dict()["step"] == 7
    with pytest.raises(RuntimeError, match="device-state"):
        FlatAdam(m).skipped_steps
    with pytest.raises(RuntimeError, match="device-state"):
        FlatAdam(m).grad_norm


def test_checkpoint_with_other_betas_is_refused_once_a_step_was_captured():
    """betas / eps are kernel arguments of the captured launches (what a capture records is marked here by hand)."""
    m = build("lmf_only")
    opt = FlatAdam(m, capturable=True)
    sd = opt.state_dict()
    other = dict(sd, betas=(0.8, 0.999))
    opt.load_state_dict(other)                           # nothing captured yet: taken
    assert opt.betas == (0.8, 0.999)
    opt._captured_args = (opt.betas, opt.eps)
    opt.load_state_dict(other)                           # the captured values: fine
    with pytest.raises(RuntimeError, match="before capturing"):
        opt.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="before capturing"):
        opt.load_state_dict(dict(other, eps=1e-6))
    assert opt.betas == (0.8, 0.999) and opt.eps == 1e-8


def test_captured_step_refuses_what_it_cannot_capture():
    m = build("lmf_only")
    fn = lambda: None
    with pytest.raises(ValueError, match="reduce_in_graph"):
        CapturedStep(m, fn, optimizer=FlatAdam(m, capturable=True), reduce_in_graph=True)
    with pytest.raises(ValueError, match="device-resident"):
        CapturedStep(m, fn, optimizer=FlatAdam(m))
    opt = FlatAdam(m, capturable=True)
    from mm_dfn_amd.distributed import GradientBucket
    with pytest.raises(ValueError, match="bucket"):
        CapturedStep(m, fn, optimizer=opt, bucket=GradientBucket(m))
    with pytest.raises(ValueError, match="device-resident"):
        train.StepGraphCache(m, FocalLoss(gamma=0.5), optimizer=FlatAdam(m))


def test_pass_loop_refuses_a_step_hook_or_another_optimizer_with_a_cache_owned_optimizer():
    m = build("lmf_only")
    loss_f = FocalLoss(gamma=0.5)
    opt = FlatAdam(m, capturable=True)
    cache = train.StepGraphCache(m, loss_f, optimizer=opt)
    assert cache.optimizer is opt
    with pytest.raises(ValueError, match="step_hook"):
        train.train_or_eval_graph_model(m, loss_f, [], 0, True, opt, False, step_hook=lambda model: None, graph_cache=cache)
    with pytest.raises(ValueError, match="optimizer"):
        train.train_or_eval_graph_model(m, loss_f, [], 0, True, FlatAdam(m, capturable=True), False, graph_cache=cache)
    # an evaluation pass has no optimizer to compare, and an empty loader returns the empty result
    assert train.train_or_eval_graph_model(m, loss_f, [], 0, False, None, False, graph_cache=cache)[0] == []


def test_state_block_in_the_header_is_64_bytes_and_matches_the_ctypes_mirror():
    text = open(os.path.join(ROOT, "include", "mmdfn_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+mmdfn_adam_state\s*\{(.*?)\}\s*mmdfn_adam_state\s*;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind, names = decl.split(None, 1)
        for name in names.split(","):
            arr = re.match(r"\s*(\w+)\s*\[(\d+)\]\s*$", name)
            fields.append((arr.group(1), ctype[kind] * int(arr.group(2))) if arr else (name.strip(), ctype[kind]))
    header = type("HeaderState", (ctypes.Structure,), {"_fields_": fields})
    assert ctypes.sizeof(header) == 64 == ctypes.sizeof(_hip.AdamState)
    assert [n for n, _ in fields] == [n for n, _ in _hip.AdamState._fields_]
    for name, _ in fields:
        a, b = getattr(header, name), getattr(_hip.AdamState, name)
        assert (a.offset, a.size) == (b.offset, b.size), name
    for (_, a), (_, b) in zip(fields, _hip.AdamState._fields_):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is b or a._type_ is b._type_)
    assert _hip.adam_state_word("lr") + 1 == _hip.adam_state_word("weight_decay")      # (pushed as one two-word copy)
