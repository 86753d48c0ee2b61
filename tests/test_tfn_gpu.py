"""TFN tensor fusion on the device (csrc/tensor_fusion.hip, ops.tfn_fuse, fusion.TFN): the module against the reference golden
(tests/golden/make_golden_tfn.py), the three generated-operand products against float64 restatements (torch on the device,
tests only), the in-kernel dropout against its exported flags, 64-bit indexing, determinism, graph capture, no library kernels.
Errors are max |got - want| / max |want|."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from mm_dfn_amd import FocalLoss, ops, train
from mm_dfn_amd.fusion import TFN

DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def err(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max() / want.abs().max())


def fuse_ref(ha, hv, ht, W1, b1, mask=None, scale=1.0, relu=False):
    """act(dropout(Z) W1^T + b1) in the dtype of its arguments, Z materialised (model_fusion.py:189-206)."""
    one = lambda h: torch.cat([torch.ones(h.shape[0], 1, dtype=h.dtype, device=h.device), h], 1)
    a, v, t = one(ha), one(hv), one(ht)
    Z = ((a[:, :, None] * v[:, None, :]).reshape(a.shape[0], -1, 1) * t[:, None, :]).reshape(a.shape[0], -1)
    if mask is not None:
        Z = Z * mask.to(Z.dtype) * scale
    pre = Z @ W1.t() + b1
    return torch.relu(pre) if relu else pre


def make(N, H, O, seed, wscale=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    K = (H[0] + 1) * (H[1] + 1) * (H[2] + 1)
    hs = [torch.randn(N, h, device=DEV, generator=g).requires_grad_(True) for h in H]
    W1 = (torch.randn(O, K, device=DEV, generator=g) * (wscale if wscale is not None else K ** -0.5)).requires_grad_(True)
    b1 = torch.randn(O, device=DEV, generator=g).requires_grad_(True)
    G = torch.randn(N, O, device=DEV, generator=g)
    return hs, W1, b1, G, K


def run_kernel(hs, W1, b1, G, p=0.0, training=False, relu=False):
    for t in hs + [W1, b1]:
        t.grad = None
    out = ops.tfn_fuse(hs[0], hs[1], hs[2], W1, b1, p, training, relu)
    state = out.grad_fn.used_state
    (out * G).sum().backward()
    return out.detach(), [t.grad for t in hs + [W1, b1]], state


def run_ref(hs, W1, b1, G, dtype, mask=None, scale=1.0, relu=False, want_w=True):
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in hs] + [W1.detach().to(dtype).requires_grad_(want_w),
                                                                        b1.detach().to(dtype).requires_grad_(want_w)]
    out = fuse_ref(*leaves, mask=mask, scale=scale, relu=relu)
    (out * G.to(dtype)).sum().backward()
    return out.detach(), [t.grad for t in leaves]


NAMES = ["dha", "dhv", "dht", "dW1", "db1"]


# ---- 1. the module against the reference golden -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tfn_module_against_reference_golden():
    g = np.load(os.path.join(GOLD, "tfn_module.npz"), allow_pickle=False)
    m = TFN(input_dims=(12, 16, 20), hidden_dims=(5, 6, 7), dropouts=0.0, post_fusion_dim=16, output_dim=8).to(DEV).train()
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith("sd/")})
    xs = [torch.from_numpy(g["x_" + n]).to(DEV).requires_grad_(True) for n in "avt"]
    out = m(*xs)
    assert tuple(out.shape) == g["out"].shape
    (out * torch.from_numpy(g["G"]).to(DEV)).sum().backward()
    e = err(out, torch.from_numpy(g["out"]).to(DEV))
    print("out", e)
    assert e < 1e-5
    grads = {"dx_" + n: x.grad for n, x in zip("avt", xs)}
    grads.update({"grad/" + k: p.grad for k, p in m.named_parameters()})
    assert len(grads) == 13
    for k, got in grads.items():
        assert got is not None, k
        e = err(got, torch.from_numpy(g[k]).to(DEV))
        print(k, e)
        assert got.shape == g[k].shape and e < 1e-5, (k, e)


# ---- 2. the affine kernels against float64 -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H,O", [((5, 6, 7), 16), ((20, 21, 22), 300), ((20, 21, 22), 64)])
@pytest.mark.parametrize("N", [1, 37, 300])
def test_tfn_affine_kernels_against_float64(H, O, N):
    hs, W1, b1, G, K = make(N, H, O, 17 * N + O)
    out, grads, state = run_kernel(hs, W1, b1, G)
    assert state is None and tuple(out.shape) == (N, O)
    want_out, want = run_ref(hs, W1, b1, G, torch.float64)
    e = err(out, want_out)
    print("out", e)
    assert e < 1e-5
    for n, a, b in zip(NAMES, grads, want):
        e = err(a, b)
        print(n, e)
        assert a.shape == b.shape and e < 1e-5, (n, e)


# ---- 3. the ReLU form ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tfn_relu_form():
    hs, W1, b1, G, K = make(37, (20, 21, 22), 300, 5)
    out, grads, _ = run_kernel(hs, W1, b1, G, relu=True)
    want_pre, _ = run_ref(hs, W1, b1, G, torch.float64)
    assert err(out, torch.relu(want_pre)) < 1e-5
    assert float((out == 0).float().mean()) > 0.2            # the ReLU does cut
    # backward = the affine backward fed dy (.) (y1 > 0) with the kernel's own y1
    _, grads_aff, _ = run_kernel(hs, W1, b1, G * (out > 0).float())
    for n, a, b in zip(NAMES, grads, grads_aff):
        assert torch.equal(a, b) or err(a, b) < 1e-6, n


# ---- 4. dropout inside the kernels ------------------------------------------------------------------------------------------------
def _dropout_call(seed):
    hs, W1, b1, G, K = make(37, (20, 21, 22), 300, 23)
    torch.manual_seed(seed)
    out, grads, state = run_kernel(hs, W1, b1, G, p=0.4, training=True)
    return hs, W1, b1, G, K, out, grads, state.clone()


@pytest.mark.gpu
def test_tfn_dropout_matches_its_exported_flags():
    hs, W1, b1, G, K, out, grads, state = _dropout_call(1234)
    N = 37
    M = ops.tfn_keep_flags(state, N, K, 0.4, 0, N)
    assert tuple(M.shape) == (N, K) and bool(((M == 0) | (M == 1)).all())
    frac, sigma = float(M.double().mean()), (0.24 / (N * K)) ** 0.5
    print("kept", frac, "sigma", sigma)
    assert abs(frac - 0.6) < 5 * sigma
    want_out, want = run_ref(hs, W1, b1, G, torch.float64, mask=M, scale=1.0 / 0.6)
    e = err(out, want_out)
    print("out", e)
    assert e < 1e-5
    for n, a, b in zip(NAMES, grads, want):
        e = err(a, b)
        print(n, e)
        assert e < 1e-5, (n, e)
    # a window of rows of the same call gives the same flags
    assert torch.equal(ops.tfn_keep_flags(state, N, K, 0.4, 30, 5), M[30:35])
    # a second call draws other flags
    out2, _, state2 = run_kernel(hs, W1, b1, G, p=0.4, training=True)
    M2 = ops.tfn_keep_flags(state2, N, K, 0.4, 0, N)
    assert not torch.equal(M, M2) and not torch.equal(out, out2)
    assert abs(float((M * M2).double().mean()) - 0.36) < 0.01          # independent draws, not a shifted copy
    # the seed reproduces flags and bits
    hs3, W13, b13, G3, _, out3, grads3, state3 = _dropout_call(1234)
    assert torch.equal(state3, state) and torch.equal(ops.tfn_keep_flags(state3, N, K, 0.4, 0, N), M)
    assert torch.equal(out3, out) and all(torch.equal(a, b) for a, b in zip(grads3, grads))


@pytest.mark.gpu
def test_tfn_without_dropout_consumes_no_counters():
    hs, W1, b1, G, K = make(5, (5, 6, 7), 16, 3)
    idx = torch.cuda.current_device()
    run_kernel(hs, W1, b1, G, p=0.4, training=True)                  # (sets the generator state up)
    gen = torch.cuda.default_generators[idx]
    before = (ops.flags_consumed(idx), gen.get_offset())
    out_eval, _, s1 = run_kernel(hs, W1, b1, G, p=0.4, training=False)
    out_p0, _, s2 = run_kernel(hs, W1, b1, G, p=0.0, training=True)
    assert s1 is None and s2 is None and torch.equal(out_eval, out_p0)
    assert (ops.flags_consumed(idx), gen.get_offset()) == before
    run_kernel(hs, W1, b1, G, p=0.4, training=True)
    counters = 4 * ((5 * ((K + 7) // 8) + 3) // 4)
    assert (ops.flags_consumed(idx), gen.get_offset()) == (before[0] + counters, before[1] + counters)
    # p >= 1: everything dropped, scale 0 (no inf * 0)
    out_all, grads_all, _ = run_kernel(hs, W1, b1, G, p=1.0, training=True)
    assert torch.equal(out_all, b1.detach().expand(5, 16))
    assert all(bool(torch.isfinite(g).all()) for g in grads_all) and float(grads_all[3].abs().max()) == 0.0


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tfn_same_seed_same_bits():
    a = _dropout_call(77)
    b = _dropout_call(77)
    assert torch.equal(a[5], b[5])
    for n, x, y in zip(NAMES, a[6], b[6]):
        assert torch.equal(x, y), n


# ---- autograd contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tfn_second_backward_accumulates_and_train_backward_agrees():
    hs, W1, b1, G, K = make(5, (5, 6, 7), 16, 11)
    leaves = hs + [W1, b1]
    out = ops.tfn_fuse(hs[0], hs[1], hs[2], W1, b1, 0.4, True)
    loss = (out * G).sum()
    loss.backward(retain_graph=True)
    first = [t.grad.clone() for t in leaves]
    loss.backward()                                   # no zero_grad: .grad accumulates (the saved state gives the same flags)
    for n, a, t in zip(NAMES, first, leaves):
        assert float(a.abs().max()) > 0 and torch.equal(t.grad, a + a), n
    _, plain, _ = run_kernel(hs, W1, b1, G, relu=True)
    for t in leaves:
        t.grad = None
    train.backward((ops.tfn_fuse(hs[0], hs[1], hs[2], W1, b1, 0.0, False) * G).sum())
    for n, a, t in zip(NAMES, plain, leaves):
        assert torch.equal(t.grad, a), n


# ---- bad widths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tfn_refuses_widths_the_kernels_do_not_take():
    hs, W1, b1, G, K = make(3, (5, 6, 7), 16, 1)
    with pytest.raises(ValueError):
        ops.tfn_fuse(hs[0], hs[1], hs[2], W1[:, :-1], b1, 0.0, False)
    with pytest.raises(ValueError):
        ops.tfn_fuse(hs[0], hs[1], hs[2], torch.zeros(320, K, device=DEV), torch.zeros(320, device=DEV), 0.0, False)


# ---- 5 / 6. default widths -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def default_weight():
    g = torch.Generator(device=DEV).manual_seed(101)
    K = 101 ** 3
    W1 = torch.randn(300, K, device=DEV, generator=g) * K ** -0.5
    b1 = torch.randn(300, device=DEV, generator=g)
    return W1, b1, K


def _bound(name, got, want64, want32):
    e_ref, e = err(want32, want64), err(got, want64)
    print("%s: kernel %.3e  float32 torch (e_ref) %.3e" % (name, e, e_ref))
    return e, max(1e-5, 4 * e_ref)


@pytest.mark.gpu
def test_tfn_default_widths_against_float64(default_weight):
    W1, b1, K = default_weight
    N = 3
    g = torch.Generator(device=DEV).manual_seed(7)
    hs = [torch.randn(N, 100, device=DEV, generator=g).requires_grad_(True) for _ in range(3)]
    G = torch.randn(N, 300, device=DEV, generator=g)
    W1 = W1.detach().requires_grad_(True)
    b1 = b1.detach().requires_grad_(True)
    out, grads, _ = run_kernel(hs, W1, b1, G)
    o64, g64 = run_ref(hs, W1, b1, G, torch.float64)
    o32, g32 = run_ref(hs, W1, b1, G, torch.float32)
    e, bound = _bound("out", out, o64, o32)
    assert e < bound
    for n, a, b64, b32 in zip(NAMES, grads, g64, g32):
        e, bound = _bound(n, a, b64, b32)
        assert e < bound, (n, e, bound)


@pytest.mark.gpu
def test_tfn_indices_past_2_to_31(default_weight):
    """N K > 2^31 (N = 2 112 at the default widths), dropout on: the LAST four rows of the output and of dh_a / dh_v / dh_t
    against the restatement of those rows alone, with their flags from the export (rows are independent in these results).
    Nothing of size N K is allocated here."""
    W1, b1, K = default_weight
    N, R = 2112, 4
    assert N * K > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(9)
    hs = [torch.randn(N, 100, device=DEV, generator=g).requires_grad_(True) for _ in range(3)]
    G = torch.randn(N, 300, device=DEV, generator=g)
    torch.manual_seed(5)
    out = ops.tfn_fuse(hs[0], hs[1], hs[2], W1, b1, 0.4, True, False)          # (W1 takes no gradient: no 1.24 GB dW1)
    state = out.grad_fn.used_state
    (out * G).sum().backward()
    M = ops.tfn_keep_flags(state, N, K, 0.4, N - R, R)
    assert abs(float(M.double().mean()) - 0.6) < 5 * (0.24 / (R * K)) ** 0.5
    tail = [h.detach()[N - R:] for h in hs]
    o64, g64 = run_ref(tail, W1, b1, G[N - R:], torch.float64, mask=M, scale=1.0 / 0.6, want_w=False)
    o32, g32 = run_ref(tail, W1, b1, G[N - R:], torch.float32, mask=M, scale=1.0 / 0.6, want_w=False)
    e, bound = _bound("out[-4:]", out.detach()[N - R:], o64, o32)
    assert e < bound
    for n, h, b64, b32 in zip(NAMES, hs, g64, g32):
        e, bound = _bound(n + "[-4:]", h.grad[N - R:], b64, b32)
        assert e < bound, (n, e, bound)


# ---- 8. captured = eager ---------------------------------------------------------------------------------------------------------
class _Net(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.tfn = TFN(hidden_dims=(20, 21, 22), dropouts=p)
        self.fc = nn.Linear(300, 6)

    def forward(self, a, v, t):
        return torch.log_softmax(self.fc(self.tfn(a, v, t)), 1)


def _net_setup(p, seed=41):
    torch.manual_seed(seed)
    m = _Net(p).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    xs = [torch.randn(37, 300, device=DEV, generator=g) for _ in range(3)]
    label = torch.randint(0, 6, (37,), device=DEV, generator=g)
    loss_f = FocalLoss(gamma=0.5)

    def fwd_bwd():
        loss = loss_f(m(*xs), label)
        train.backward(loss)
        return loss
    return m, fwd_bwd, xs, label


def _captured(p):
    from mm_dfn_amd.graphs import CapturedStep
    from mm_dfn_amd.optim import FlatAdam
    m, fwd_bwd, xs, label = _net_setup(p)
    m.zero_grad(set_to_none=True)
    fwd_bwd()
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    opt.bucket.flatten()
    opt._materialise()
    return m, CapturedStep(m, fwd_bwd, warmup=2, bucket=opt.bucket), opt, xs, label


@pytest.mark.gpu
def test_tfn_captured_step_equals_eager_over_flat_adam_steps():
    from mm_dfn_amd.optim import FlatAdam
    m, fwd_bwd, _, _ = _net_setup(0.0)
    opt = FlatAdam(m, lr=1e-3, weight_decay=1e-4)
    want = []
    for _ in range(4):
        m.zero_grad(set_to_none=True)
        want.append(float(fwd_bwd()))
        opt.step()
    m, cap, opt, _, _ = _captured(0.0)
    got = []
    for _ in range(4):
        got.append(float(cap.replay()))
        opt.step(grads_already_flat=True)
    assert want[0] != want[-1]
    for a, b in zip(got, want):
        assert abs(a - b) <= 2e-5 * abs(b), (got, want)


@pytest.mark.gpu
def test_tfn_captured_replays_draw_fresh_flags_and_match_their_state():
    m, cap, opt, xs, label = _captured(0.4)
    l1 = float(cap.replay())
    s1 = m.tfn.last_keep_state.clone()
    l2 = float(cap.replay())
    s2 = m.tfn.last_keep_state.clone()
    assert l1 != l2 and not torch.equal(s1, s2)
    # the gradients of the second replay against the float64 restatement built from ITS state tensor
    K = 21 * 22 * 23
    M = ops.tfn_keep_flags(s2, 37, K, 0.4, 0, 37)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in m.named_parameters()}
    lin = lambda x, n: x @ sd[n + ".weight"].t() + sd[n + ".bias"]
    hs = [lin(x.double(), "tfn." + n) for x, n in zip(xs, ("audio_subnet", "video_subnet", "text_subnet"))]
    y1 = fuse_ref(hs[0], hs[1], hs[2], sd["tfn.post_fusion_layer_1.weight"], sd["tfn.post_fusion_layer_1.bias"], mask=M,
                  scale=1.0 / 0.6, relu=True)
    logp = torch.log_softmax(lin(torch.relu(lin(y1, "tfn.post_fusion_layer_2")), "fc"), 1)
    lp = logp.gather(1, label.view(-1, 1)).view(-1)
    loss = (-(1 - lp.detach().exp()) ** 0.5 * lp).mean()
    loss.backward()
    assert abs(l2 - float(loss)) < 1e-5 * abs(float(loss))
    for k, p in m.named_parameters():
        e = err(cap.grads[k], sd[k].grad)
        print(k, e)
        assert e < 1e-5, (k, e)


# ---- 9. no library kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tfn_forward_backward_runs_no_library_kernels():
    from torch.profiler import ProfilerActivity, profile
    m = TFN(hidden_dims=(20, 21, 22)).to(DEV).train()
    xs = [torch.randn(37, 300, device=DEV, requires_grad=True) for _ in range(3)]

    def step():
        m.zero_grad(set_to_none=True)
        train.backward(m(*xs).square().sum())
    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    for k in ("tfn_fwd_kernel", "tfn_wgrad_kernel", "tfn_dgrad_kernel"):
        assert any(k in n for n in names), (k, names)
    bad = [n for n in names if n.startswith("Cijk_") or "rocblas" in n.lower() or "miopen" in n.lower()
           or "hipblaslt" in n.lower() or ("gemm" in n.lower() and "gemm_tn" not in n)]
    assert not bad, bad
