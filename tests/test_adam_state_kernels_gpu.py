"""GPU: FlatAdam's kernels on device-resident step state (csrc/optimizer_state.hip: mmdfn_grad_sumsq, mmdfn_adam_prepare,
mmdfn_adam_step_state) called directly through the C ABI, against float64 restatements.  The update reuses the input recipe and
the bounds of test_loss_optimizer_kernels_gpu.test_adam_step_against_float64; u = 2^-24."""
import ctypes
import math

import numpy as np
import pytest
import torch

from mm_dfn_amd import _hip
from test_loss_optimizer_kernels_gpu import ADAM_CASES, BETA1, BETA2, EPS, F32, adam_inputs, adam_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
PAD = 8
SENTINEL = (3.5, -1.25, 7.0, 9.0)
CAP = 1024


def make_state(step=0, enabled=1, skip=0, lr=1e-3, wd=0.0, max_norm=0.0, **more):
    host = _hip.AdamState(step=step, enabled=enabled, skip_nonfinite=skip, lr=lr, weight_decay=wd, max_norm=max_norm, **more)
    return torch.frombuffer(bytearray(bytes(host)), dtype=torch.int32).to(DEV)


def read_state(st):
    return _hip.AdamState.from_buffer_copy(st.cpu().numpy().tobytes())


def padded(tensors):
    return [torch.cat([t, torch.full((PAD,), s)]).to(DEV) for t, s in zip(tensors, SENTINEL)]


def sumsq(g, n, partials):
    count = ctypes.c_int(0)
    rc = _hip.lib().mmdfn_grad_sumsq(_hip.ptr(g), n, _hip.ptr(partials), CAP, ctypes.byref(count), _hip.stream())
    return rc, count.value


def full_step(dev, n, st, partials=None):
    """[sumsq ->] prepare -> step_state, as optim.FlatAdam issues them; ``partials``: the norm's workspace (None = not wanted)."""
    lib = _hip.lib()
    nparts = 0
    if partials is not None:
        rc, nparts = sumsq(dev[1], n, partials)
        assert rc == 0
    assert lib.mmdfn_adam_prepare(_hip.ptr(st), _hip.ptr(partials), nparts, BETA1, BETA2, _hip.stream()) == 0
    assert lib.mmdfn_adam_step_state(*(_hip.ptr(t) for t in dev), n, _hip.ptr(st), BETA1, BETA2, EPS, _hip.stream()) == 0


def check_update(tag, dev, p, g, m, v, n, lr, wd, step, scale=None, zero=None):
    """The bounds of test_adam_step_against_float64 on what ``dev`` holds after one call; ``scale``: the kernel's own clip factor
    (the float64 restatement clips with exactly that float, so the factor's own error is judged apart)."""
    g64 = g.double() if scale is None else g.double() * float(scale)
    dp, m2, v2, m_mag, v_mag = adam_reference(p, g64, m, v, lr, wd, step)
    pg, gg, mg, vg = (t.cpu() for t in dev)
    for t, s in zip((pg, gg, mg, vg), SENTINEL):
        assert bool((t[n:] == s).all()), tag
    assert torch.equal(gg[:n], g), tag
    pg, mg, vg = pg[:n].double(), mg[:n].double(), vg[:n].double()
    assert bool(torch.isfinite(pg).all() and torch.isfinite(mg).all() and torch.isfinite(vg).all())
    dp_got = pg - p.double()
    dp_b = 16 * U * dp.abs() + U * (p.double().abs() + (p.double() + dp).abs())
    tiny = 1e-300
    r_p = float(((dp_got - dp).abs() / dp_b.clamp_min(tiny)).max())
    r_m = float(((mg - m2).abs() / (8 * U * m_mag).clamp_min(tiny)).max())
    r_v = float(((vg - v2).abs() / (8 * U * v_mag).clamp_min(tiny)).max())
    print("RATIO adam_state[%s] dp %.3f m %.3f v %.3f" % (tag, r_p, r_m, r_v))
    assert r_p <= 1.0 and r_m <= 1.0 and r_v <= 1.0, (tag, r_p, r_m, r_v)
    if zero is not None:
        still = zero & ((p == 0) | torch.tensor(F32(wd) == 0.0))
        if bool(still.any()):
            assert bool((dp_got[still] == 0).all()) and bool((mg[still] == 0).all()) and bool((vg[still] == 0).all())
    if lr == 0.0:
        assert bool((dp_got == 0).all())


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("n,step,wd,lr", ADAM_CASES)
def test_update_against_float64(n, step, wd, lr):
    """The cases of test_adam_step_against_float64 (ADAM_CASES), the block preset to step - 1.  Every n in {1, 3, 4, 5, 7, 1023,
    1024, 1025, 2048 * 256 * 4 + 5}, every step in {1, 2, 3, 5, 10, 100, 100000}, both wd in {0, 1e-4} and both lr in {1e-3, 0}
    occur, but NOT as a cross product (that would be 252 cases, 28 of them 2 M floats against float64 on the host): each small n
    once with rotating step / wd, n = 1025 (two blocks and a tail) with every step x wd, lr = 0 at n = 1023 and 7, and the size
    past the block cap at steps 1 and 2 only -- the step enters the kernel only through bc1 / bc2_sqrt, which do not depend on
    n."""
    p, g, m, v, zero = adam_inputs(n, step, 17 * step + n % 1000)
    dev = padded((p, g, m, v))
    st = make_state(step=step - 1, lr=lr, wd=wd)
    full_step(dev, n, st)
    torch.cuda.synchronize()
    got = read_state(st)
    assert (got.step, got.last_skipped, got.skipped, got.scale, got.grad_norm) == (step, 0, 0, 1.0, 0.0)
    b1, b2 = F32(BETA1), F32(BETA2)
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    assert abs(got.bc1 - bc1) <= ulp32(bc1) and abs(got.bc2_sqrt - bc2s) <= ulp32(bc2s), (got.bc1, bc1, got.bc2_sqrt, bc2s)
    check_update("n=%d,step=%d,wd=%g,lr=%g" % (n, step, wd, lr), dev, p, g, m, v, n, lr, wd, step, zero=zero)


def norm_inputs(n, seed):
    """Magnitudes log-uniform in [1e-20, 1e18], random signs: the squares leave float's range at both ends, not double's."""
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (-20.0 + 38.0 * torch.rand(n, generator=gen, dtype=torch.float64))
    sign = 1.0 - 2.0 * (torch.rand(n, generator=gen) < 0.5).double()
    return (mag * sign).float()


@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 257, 1024 * 256 * 4 + 5])
def test_norm_against_float64_and_bit_reproducible(n):
    g = norm_inputs(n, 5 + n % 1000)
    want = math.sqrt(float((g.double() ** 2).sum()))
    gd = torch.cat([g, torch.full((PAD,), float("nan"))]).to(DEV)          # (a read past n would poison the sum)
    runs = []
    for fill in (0.0, float("nan")):
        partials = torch.full((CAP + PAD,), fill, dtype=torch.float64, device=DEV)
        st = make_state(step=0, max_norm=1.0)
        rc, nparts = sumsq(gd, n, partials)
        assert rc == 0 and nparts == min(max((n // 4 + 255) // 256, 1), CAP)
        assert _hip.lib().mmdfn_adam_prepare(_hip.ptr(st), _hip.ptr(partials), nparts, BETA1, BETA2, _hip.stream()) == 0
        torch.cuda.synchronize()
        tail = partials[nparts:].cpu()
        assert bool(torch.isnan(tail).all() if math.isnan(fill) else (tail == fill).all())     # only nparts doubles written
        runs.append((read_state(st), partials[:nparts].cpu()))
    got = runs[0][0].grad_norm
    print("RATIO grad_norm[n=%d] %.3f" % (n, abs(got - want) / (2 * U * want)))
    assert abs(got - want) <= 2 * U * want, (got, want)
    assert bytes(runs[0][0]) == bytes(runs[1][0])
    assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))


def test_clipping_scale_and_clipped_update():
    n, step, lr, wd = 1025, 3, 1e-3, 1e-4
    p, g, m, v, zero = adam_inputs(n, step, 77)
    norm = math.sqrt(float((g.double() ** 2).sum()))
    partials = torch.zeros(CAP, dtype=torch.float64, device=DEV)
    # above the threshold
    max_norm = F32(1.0)
    assert norm > 10 * max_norm
    dev = padded((p, g, m, v))
    st = make_state(step=step - 1, lr=lr, wd=wd, max_norm=max_norm)
    full_step(dev, n, st, partials)
    torch.cuda.synchronize()
    got = read_state(st)
    want = max_norm / (norm + 1e-6)
    print("RATIO clip scale %.3f" % (abs(got.scale - want) / (4 * U * want)))
    assert abs(got.scale - want) <= 4 * U * want and got.scale < 1.0, (got.scale, want)
    assert abs(got.grad_norm - norm) <= 2 * U * norm and got.step == step
    check_update("clipped", dev, p, g, m, v, n, lr, wd, step, scale=got.scale, zero=zero)
    # below it: the factor is exactly 1 and the update is the unclipped one, bit for bit
    outs = []
    for mx in (F32(1e6), 0.0):
        dev = padded((p, g, m, v))
        st = make_state(step=step - 1, lr=lr, wd=wd, max_norm=mx)
        full_step(dev, n, st, partials)
        torch.cuda.synchronize()
        assert read_state(st).scale == 1.0 and read_state(st).step == step
        outs.append([t.cpu() for t in dev])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("index,value", [(1026, float("inf")), (0, float("nan")), (512, float("-inf"))])
def test_nonfinite_gradient_is_skipped_and_the_next_step_applies(index, value):
    """index 1026: the scalar tail of n = 1027; 0 and 512: the float4 body."""
    n, step, lr, wd = 1027, 5, 1e-3, 1e-4
    p, g, m, v, zero = adam_inputs(n, step, 31)
    bad = g.clone()
    bad[index] = value
    dev = padded((p, bad, m, v))
    before = [t.clone() for t in dev]
    partials = torch.zeros(CAP, dtype=torch.float64, device=DEV)
    st = make_state(step=step - 1, skip=1, lr=lr, wd=wd)
    full_step(dev, n, st, partials)
    torch.cuda.synchronize()
    got = read_state(st)
    assert (got.step, got.skipped, got.last_skipped) == (step - 1, 1, 1)
    for a, b in zip(dev, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a finite gradient next: step `step` is applied, the flag clears, the count stays
    dev[1][:n].copy_(g)
    full_step(dev, n, st, partials)
    torch.cuda.synchronize()
    got = read_state(st)
    assert (got.step, got.skipped, got.last_skipped, got.scale) == (step, 1, 0, 1.0)
    check_update("after skip", dev, p, g, m, v, n, lr, wd, step, zero=zero)
    # without skip_nonfinite the same gradient is NOT held back (the plain kernel's behaviour: the caller asked for no check)
    dev = padded((p, bad, m, v))
    st = make_state(step=step - 1, skip=0, lr=lr, wd=wd)
    full_step(dev, n, st, partials)
    torch.cuda.synchronize()
    assert read_state(st).step == step and read_state(st).skipped == 0


def test_disabled_state_and_bad_arguments_change_nothing():
    n = 1025
    p, g, m, v, _ = adam_inputs(n, 3, 9)
    dev = padded((p, g, m, v))
    before = [t.clone() for t in dev]
    partials = torch.zeros(CAP, dtype=torch.float64, device=DEV)
    st = make_state(step=2, enabled=0, skip=1, max_norm=0.5, grad_norm=4.0, scale=0.25, bc1=0.5, bc2_sqrt=0.5)
    st0 = st.clone()
    full_step(dev, n, st, partials)
    lib, s = _hip.lib(), _hip.stream()
    P = _hip.ptr
    count = ctypes.c_int(-7)
    # n <= 0, null pointers, no room for a partial, a state block or a float buffer that is not 16-byte aligned
    odd = torch.zeros(20, dtype=torch.int32, device=DEV)[1:17]
    assert odd.data_ptr() % 16 == 4
    off = [t[1:] for t in dev]                                            # 4 bytes past an aligned start
    assert all(t.data_ptr() % 16 == 4 for t in off)
    live = make_state(step=2)                                             # (enabled: a launch WOULD update)
    live0 = live.clone()
    bad = [lib.mmdfn_grad_sumsq(P(dev[1]), 0, P(partials), CAP, ctypes.byref(count), s),
           lib.mmdfn_grad_sumsq(P(dev[1]), -4, P(partials), CAP, ctypes.byref(count), s),
           lib.mmdfn_grad_sumsq(None, n, P(partials), CAP, ctypes.byref(count), s),
           lib.mmdfn_grad_sumsq(P(dev[1]), n, None, CAP, ctypes.byref(count), s),
           lib.mmdfn_grad_sumsq(P(dev[1]), n, P(partials), 0, ctypes.byref(count), s),
           lib.mmdfn_grad_sumsq(P(dev[1]), n, P(partials), CAP, None, s),
           lib.mmdfn_adam_prepare(None, P(partials), 1, BETA1, BETA2, s),
           lib.mmdfn_adam_prepare(P(odd), P(partials), 1, BETA1, BETA2, s),
           lib.mmdfn_adam_prepare(P(st), P(partials), 0, BETA1, BETA2, s),
           lib.mmdfn_adam_prepare(P(st), P(partials), CAP + 1, BETA1, BETA2, s),
           lib.mmdfn_adam_step_state(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), 0, P(st), BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), -1, P(st), BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(None, P(dev[1]), P(dev[2]), P(dev[3]), n, P(st), BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(P(dev[0]), None, P(dev[2]), P(dev[3]), n, P(st), BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(P(dev[0]), P(dev[1]), None, P(dev[3]), n, P(st), BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(P(dev[0]), P(dev[1]), P(dev[2]), None, n, P(st), BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), n, None, BETA1, BETA2, EPS, s),
           lib.mmdfn_adam_step_state(P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), n, P(odd), BETA1, BETA2, EPS, s),
           lib.mmdfn_grad_sumsq(P(off[1]), n, P(partials), CAP, ctypes.byref(count), s)]
    for k in range(4):
        args = [P(off[i]) if i == k else P(dev[i]) for i in range(4)]
        bad.append(lib.mmdfn_adam_step_state(*args, n, P(live), BETA1, BETA2, EPS, s))
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert count.value == -7
    assert int(lib.mmdfn_adam_state_bytes()) == 64
    assert torch.equal(st, st0) and torch.equal(live, live0) and not bool(odd.any())
    for a, b in zip(dev, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_captured_launches_replay_like_eager_calls():
    """A graph that holds only sumsq -> prepare -> step_state, replayed over 5 gradients copied into its static buffer: the
    parameters, the moments and the step count are those of 5 eager calls, bit for bit (clipping on: the norm, the factor and the
    bias corrections are all recomputed on the device at every replay)."""
    n, lr, wd, max_norm = 1025, 1e-3, 1e-4, 1.0
    p, g0, m, v, _ = adam_inputs(n, 1, 41)
    grads = [g0] + [adam_inputs(n, 1, 42 + i)[1] for i in range(4)]

    def fresh():
        return padded((p, g0, m, v)), make_state(lr=lr, wd=wd, max_norm=max_norm), torch.zeros(CAP, dtype=torch.float64, device=DEV)

    dev_e, st_e, part_e = fresh()
    for g in grads:
        dev_e[1][:n].copy_(g)
        full_step(dev_e, n, st_e, part_e)
    dev_w, st_w, part_w = fresh()
    full_step(dev_w, n, st_w, part_w)                    # (the kernels' code objects are loaded before the capture)
    torch.cuda.synchronize()
    dev_c, st_c, part_c = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        full_step(dev_c, n, st_c, part_c)
    torch.cuda.synchronize()
    assert read_state(st_c).step == 0                    # capturing ran nothing
    for g in grads:
        dev_c[1][:n].copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert read_state(st_c).step == 5 and read_state(st_c).scale < 1.0
    assert bytes(read_state(st_c)) == bytes(read_state(st_e))
    for a, b in zip(dev_c, dev_e):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
