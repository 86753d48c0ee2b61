"""GPU: the kernels of csrc/fusion.hip (softmax_scale, mfn_mem, gated_pair, rowscale_colsum) and csrc/lmf.hip driven directly at
their launch edges -- rows past the first workgroup, a partial last workgroup, widths around the 64-lane wave, the grid-stride
loops -- and the MFN / MMGatedAttention / LMF modules off their default shapes, all against float64 restatements on the CPU
(or, for LMF, float64 on the device as test_fusion_baselines_gpu.py does).

Bounds of the kernel tests are derived, not tuned.  With u = 2^-24 every test computes in float64 the wanted value and a
magnitude ``mag`` (the same formula with every summed term replaced by its absolute value; |want| for a pointwise output) and
asserts elementwise

    |got - want| <= (n + 16) u mag  (+ 2^-126)

n = the number of terms the kernel sums for that element (0 pointwise, W for a softmax row, 3 D for the gate pre-activation, C for
dpre, R for the weight-gradient contraction); the 16 covers a handful of pointwise roundings and the 1-2 ulp of the device's expf /
tanhf.  An output that depends on an earlier reduced quantity (the gate z through the sigmoid, dpre, the softmax row dot in dz)
adds that quantity's bound times the float64 derivative magnitude; dz uses a factor 2 on its mag.  The additive 2^-126 (the smallest
normal float32) is the one term the format forces: the -80 entry next to a +80 one has att = e^-160, a sigmoid of -100 is 4e-44, and
no float32 kernel can return either (they underflow to zero or to a subnormal).  Where such a quantity is stored in float32 and
multiplied afterwards (att, the saved gates, z, dpre), the 2^-126 is carried through those factors like any other bound.
Every test prints its worst error-to-bound ratio per output (profiles/r08_fusion_loss_optimizer_parity.md records them)."""
import numpy as np
import pytest
import torch

import mmdfn_oracle as O
from mm_dfn_amd import MFN, MMGatedAttention, ops, synthetic
from mm_dfn_amd.fusion import LMF

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
TINY = 2.0 ** -126


def check(name, got, want, bound):
    """Elementwise |got - want| <= bound; prints and returns the worst ratio."""
    got = got.detach().double().cpu()
    want = want.detach()
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), "%s: not finite" % name
    ratio = float(((got - want).abs() / bound).max())
    print("RATIO %s %.3f" % (name, ratio))
    assert ratio <= 1.0, "%s: error / bound = %.3f" % (name, ratio)
    return ratio


def rel_max(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert tuple(got.shape) == tuple(want.shape), (tuple(got.shape), tuple(want.shape))
    den = float(want.abs().max())
    if den == 0.0:                                  # (a gradient that is identically zero: MFN's recurrent weights at T = 1)
        return float(got.abs().max())
    return float((got - want).abs().max()) / den


def leaf(t):
    return t.detach().double().cpu().requires_grad_(True)


# ---- softmax_scale -------------------------------------------------------------------------------------------------------------
def softmax_scale_reference(z, c, dout):
    """{name: (want, bound)} of att, out = att * c and the gradients dz, dc for the upstream gradient dout; float64 autograd on
    the plain formula for the values, the formula with absolute terms for the bounds."""
    W = z.shape[1]
    z, c, d = leaf(z), leaf(c), dout.detach().double().cpu()
    att = torch.softmax(z, 1)
    out = att * c
    dz, dc = torch.autograd.grad(out, (z, c), d)
    a = att.detach()
    S = (d * c * a).abs().sum(1, keepdim=True)
    k = (W + 16) * U
    dc_abs = (d * c).abs().detach()
    # (the TINY terms: att is stored in float32, so an entry below 2^-126 reaches out, dc, dz and the row dot flushed)
    return {"att": (a, k * a + TINY), "out": (out.detach(), k * out.detach().abs() + TINY * (1 + c.detach().abs())),
            "dc": (dc, k * dc.abs() + TINY * (1 + d.abs())),
            "dz": (dz, 2 * k * a * (dc_abs + S.detach()) + TINY * (1 + dc_abs + dc_abs.sum(1, keepdim=True)))}


def softmax_inputs(R, W, seed, special):
    g = torch.Generator().manual_seed(seed)
    z = 8.0 * torch.randn(R, W, generator=g)
    if special == "peak":                            # +80 next to -80: only the max subtraction keeps the row finite
        z[0, 0] = 80.0
        z[0, W - 1] = -80.0 if W > 1 else 80.0
    if special == "const" or (special == "peak" and R > 1):
        z[R - 1] = 3.25                              # a constant row: att = 1 / W
    return z, torch.randn(R, W, generator=g), torch.randn(R, W, generator=g)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 600])
@pytest.mark.parametrize("R", [1, 4, 5, 9])
def test_softmax_scale_against_float64(R, W):
    for special in (("peak", "const") if R == 1 else ("peak",)):
        z, c, dout = softmax_inputs(R, W, 1000 * R + W, special)
        ref = softmax_scale_reference(z, c, dout)
        zd, cd = z.to(DEV).requires_grad_(True), c.to(DEV).requires_grad_(True)
        out = ops.softmax_scale(zd, cd)
        att = out.grad_fn.saved_tensors[0]
        out.backward(dout.to(DEV))
        tag = "softmax_scale[R=%d,W=%d,%s] " % (R, W, special)
        for name, got in (("att", att), ("out", out), ("dz", zd.grad), ("dc", cd.grad)):
            check(tag + name, got, *ref[name])
        rowsum = att.double().sum(1).cpu()
        assert float((rowsum - 1.0).abs().max()) <= W * U, (tag, rowsum)
        const = R - 1 if (special == "const" or R > 1) else None
        if const is not None:
            assert float((att[const].double().cpu() - 1.0 / W).abs().max()) <= 2 * U / W, tag


# ---- mfn_mem -------------------------------------------------------------------------------------------------------------------
def mfn_mem_reference(u, v1, v2, mem, dout):
    u, v1, v2, mem, d = leaf(u), leaf(v1), leaf(v2), leaf(mem), dout.detach().double().cpu()
    ch, g1, g2 = torch.tanh(u), torch.sigmoid(v1), torch.sigmoid(v2)
    out = g1 * mem + g2 * ch
    du, dv1, dv2, dmem = torch.autograd.grad(out, (u, v1, v2, mem), d)
    ch, g1, g2, m = ch.detach(), g1.detach(), g2.detach(), mem.detach()
    k = 16 * U
    # (the TINY terms: a gate below 2^-126 is saved flushed and multiplied by what follows)
    return {"out": (out.detach(), k * ((g1 * m).abs() + (g2 * ch).abs()) + TINY * (2 + m.abs())),
            "du": (du, k * (d * g2).abs() * (1 + ch * ch) + TINY * (1 + d.abs())),
            "dv1": (dv1, k * (d * m * g1).abs() * (1 + g1) + TINY * (1 + (d * m).abs())),
            "dv2": (dv2, k * (d * ch * g2).abs() * (1 + g2) + TINY * (1 + d.abs())),
            "dmem": (dmem, k * dmem.abs() + TINY * (1 + d.abs()))}


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 * 256 + 3])
def test_mfn_mem_against_float64(n):
    g = torch.Generator().manual_seed(n)
    u, v1, v2 = (60.0 * torch.rand(n, generator=g) - 30.0 for _ in range(3))
    mem, dout = torch.randn(n, generator=g), torch.randn(n, generator=g)
    if n >= 255:                                     # +-100: expf overflows; the gates must saturate, not turn into NaN
        idx = [0, 7, n // 2, n - 1]
        for t, vals in ((u, (100.0, -100.0, 100.0, -100.0)), (v1, (-100.0, 100.0, 100.0, -100.0)),
                        (v2, (100.0, 100.0, -100.0, -100.0))):
            t[idx] = torch.tensor(vals)
    ref = mfn_mem_reference(u, v1, v2, mem, dout)
    dev = [t.to(DEV).requires_grad_(True) for t in (u, v1, v2, mem)]
    out = ops.mfn_mem(*dev)
    out.backward(dout.to(DEV))
    for name, got in (("out", out), ("du", dev[0].grad), ("dv1", dev[1].grad), ("dv2", dev[2].grad), ("dmem", dev[3].grad)):
        check("mfn_mem[n=%d] %s" % (n, name), got, *ref[name])
    if n >= 255:
        o = out.detach().cpu()
        assert abs(float(o[0]) - 1.0) <= 16 * U                       # g1 = 0, g2 = 1, cHat = 1
        assert abs(float(o[7]) - (float(mem[7]) - 1.0)) <= 16 * U * (abs(float(mem[7])) + 1.0)   # g1 = 1, g2 = 1, cHat = -1
        assert abs(float(o[n // 2]) - float(mem[n // 2])) <= 16 * U * abs(float(mem[n // 2]))    # g1 = 1, g2 = 0
        assert abs(float(o[n - 1])) <= TINY                           # g1 = g2 = 0


# ---- gated_pair + rowscale_colsum ----------------------------------------------------------------------------------------------
def gated_pair_reference(xm, xn, pm, pn, w, b, dout):
    D, C, R = xm.shape[1], pm.shape[1], xm.shape[0]
    xm, xn, pm, pn, w, b = (leaf(t) for t in (xm, xn, pm, pn, w, b))
    d = dout.detach().double().cpu()
    terms = torch.cat([xm, xn, xm * xn], 1) * w                         # (R, 3 D) the summed terms of the gate pre-activation
    z = torch.sigmoid(terms.sum(1, keepdim=True) + b)
    hm, hn = torch.tanh(pm), torch.tanh(pn)
    out = z * hm + (1 - z) * hn
    grads = torch.autograd.grad(out, (xm, xn, pm, pn, w, b), d)
    with torch.no_grad():
        k = 16 * U
        s_b = (3 * D + 16) * U * (terms.abs().sum(1, keepdim=True) + b.abs())
        z_b = s_b * z * (1 - z) + k * z + TINY                      # (z and dpre are stored in float32: flushed below 2^-126)
        out_b = k * (z * hm.abs() + (1 - z) * hn.abs()) + z_b * (hm - hn).abs()
        dpm_b = k * (z * d).abs() * (1 + hm * hm) + z_b * (d * (1 - hm * hm)).abs()
        dpn_b = k * ((1 - z) * d).abs() * (1 + hn * hn) + z_b * (d * (1 - hn * hn)).abs()
        acc = (d * (hm - hn)).sum(1, keepdim=True)
        dpre = acc * z * (1 - z)
        dpre_b = (C + 16) * U * (d.abs() * (hm.abs() + hn.abs())).sum(1, keepdim=True) * z * (1 - z) + z_b * (acc * (1 - 2 * z)).abs() + TINY
        w1, w2, w3 = w[:, :D], w[:, D:2 * D], w[:, 2 * D:]
        dxm_b = k * dpre.abs() * (w1.abs() + (w3 * xn).abs()) + dpre_b * (w1 + w3 * xn).abs()
        dxn_b = k * dpre.abs() * (w2.abs() + (w3 * xm).abs()) + dpre_b * (w2 + w3 * xm).abs()
        X = torch.cat([xm, xn, xm * xn], 1).abs()
        dw_b = ((R + 16) * U * (dpre.abs() * X).sum(0, keepdim=True) + (dpre_b * X).sum(0, keepdim=True))
        db_b = ((R + 16) * U * dpre.abs().sum() + dpre_b.sum()).view(1)
        bounds = (dxm_b, dxn_b, dpm_b, dpn_b, dw_b, db_b)
        ref = {"out": (out.detach(), out_b + TINY)}
        for name, gr, bd in zip(("dxm", "dxn", "dpm", "dpn", "dw", "db"), grads, bounds):
            ref[name] = (gr, bd + TINY)
        # the manual dpre agrees with autograd's db (a check of this function's own algebra)
        assert abs(float(dpre.sum() - grads[5][0])) <= 1e-12 * (1.0 + float(dpre.abs().sum()))
    return ref


def gated_inputs(R, D, C, seed, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    xm, xn = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    pm, pn = 2.0 * torch.randn(R, C, generator=g), 2.0 * torch.randn(R, C, generator=g)
    w = wscale * torch.randn(1, 3 * D, generator=g) / D ** 0.5
    b = torch.tensor([0.375])
    return xm, xn, pm, pn, w, b, torch.randn(R, C, generator=g)


def run_gated_pair(tag, inputs):
    ref = gated_pair_reference(*inputs)
    dev = [t.to(DEV).requires_grad_(True) for t in inputs[:6]]
    out = ops.gated_pair(*dev)
    out.backward(inputs[6].to(DEV))
    assert tuple(dev[4].grad.shape) == tuple(inputs[4].shape) and tuple(dev[5].grad.shape) == (1,)
    for name, got in zip(("out", "dxm", "dxn", "dpm", "dpn", "dw", "db"), [out] + [t.grad for t in dev]):
        check(tag + name, got, *ref[name])
    return out


# every value of each axis (R: 1 4 5 9 37; D: 1 63 64 65 300; C: 1 64 65 100), D != C, and D = 300 with C = 100
GATED_SHAPES = [(1, 300, 100), (4, 1, 64), (5, 63, 1), (9, 64, 65), (37, 65, 100), (5, 300, 100), (37, 300, 100), (9, 1, 100),
                (4, 64, 1), (37, 63, 64)]


@pytest.mark.parametrize("R,D,C", GATED_SHAPES)
def test_gated_pair_against_float64(R, D, C):
    run_gated_pair("gated_pair[R=%d,D=%d,C=%d] " % (R, D, C), gated_inputs(R, D, C, 10000 * R + 100 * D + C))


def test_gated_pair_with_saturated_gates():
    """w scaled until the gate pre-activations reach +-50 and beyond: z is 1 or ~0 in float32 on rows of both kinds."""
    inputs = gated_inputs(37, 65, 100, 4242, wscale=40.0)
    s = torch.cat([inputs[0], inputs[1], inputs[0] * inputs[1]], 1).double() @ inputs[4].double().t() + 0.375
    assert float(s.max()) > 40.0 and float(s.min()) < -40.0
    run_gated_pair("gated_pair[saturated] ", inputs)


def test_gated_pair_weight_gradient_over_many_rows():
    """R = 1000 with D = 65: each of the four waves of rowscale_colsum takes 250 rows, the second column block holds one column."""
    run_gated_pair("gated_pair[R=1000,D=65,C=4] ", gated_inputs(1000, 65, 4, 777))


# ---- non-contiguous inputs -----------------------------------------------------------------------------------------------------
def _views(shape, g):
    """A column slice of a wider matrix and a transposed view, both of ``shape`` and neither contiguous (where the shape allows)."""
    r, c = shape
    wide = torch.randn(r, c + 5, generator=g).to(DEV)
    return wide[:, 3:3 + c], torch.randn(c, r, generator=g).to(DEV).t()


@pytest.mark.parametrize("kind", [0, 1])
def test_fusion_operators_take_non_contiguous_inputs(kind):
    """A column slice (kind 0) or a transposed view (kind 1) through each operator: the result and the gradients have the
    shapes and exactly the values of the call on contiguous copies."""
    g = torch.Generator().manual_seed(31 + kind)
    R, D, C = 9, 65, 12
    cases = {
        "softmax_scale": (ops.softmax_scale, [(R, D), (R, D)]),
        "mfn_mem": (ops.mfn_mem, [(R, C)] * 4),
        "gated_pair": (ops.gated_pair, [(R, D), (R, D), (R, C), (R, C), (1, 3 * D)]),
    }
    for name, (fn, shapes) in cases.items():
        views = [_views(s, g)[kind] for s in shapes]
        extra = [torch.tensor([0.25], device=DEV)] if name == "gated_pair" else []
        dout = _views(shapes[0] if name != "gated_pair" else (R, C), g)[kind]
        assert not dout.is_contiguous() and not views[0].is_contiguous()
        a = [v.detach().requires_grad_(True) for v in views + extra]          # leaves that keep the views' strides
        b = [v.detach().contiguous().clone().requires_grad_(True) for v in views + extra]
        assert a[0].stride() == views[0].stride()
        ya, yb = fn(*a), fn(*b)
        ya.backward(dout)
        yb.backward(dout.contiguous())
        assert torch.equal(ya, yb), name
        for i, (p, q) in enumerate(zip(a, b)):
            assert p.grad.shape == p.shape and torch.equal(p.grad, q.grad), (name, i)


# ---- the modules against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(1, 1), (3, 5), (2, 9)])
def test_mfn_module_against_float64_oracle(T, n):
    """MFN in eval mode; n = 5 and n = 9 put real rows into the second and third workgroup of the row kernels.  Output, dx and
    the gradient of every parameter that takes part; out_fc1 / out_fc2 are constructed and unused (model_fusion.py:58-59)."""
    seed = 800 + 10 * T + n
    mod = MFN()
    mod.load_state_dict(synthetic.seeded_state_dict(mod.state_dict(), seed))
    params = {k: v.detach().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    mod = mod.to(DEV).eval()
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randn(T, n, 900).astype(np.float32))
    G = torch.from_numpy(rs.randn(T, n, 400).astype(np.float32))
    xd = x.to(DEV).requires_grad_(True)
    y = mod(xd)
    assert tuple(y.shape) == (T, n, 400)
    (y * G.to(DEV)).sum().backward()
    xo = x.double().requires_grad_(True)
    want = O.mfn(xo, params)
    (want * G.double()).sum().backward()
    worst = {"y": rel_max(y, want), "dx": rel_max(xd.grad, xo.grad)}
    for k, p in mod.named_parameters():
        if k.startswith(("out_fc1.", "out_fc2.")):
            assert p.grad is None and params[k].grad is None, k
            continue
        assert p.grad is not None and params[k].grad is not None, k
        worst[k] = rel_max(p.grad, params[k].grad)
    print("RATIO mfn_module[T=%d,n=%d] worst %s %.3g (of 1e-5)" % (T, n, max(worst, key=worst.get), max(worst.values())))
    for k, v in worst.items():
        assert v < 1e-5, (k, v)


@pytest.mark.parametrize("modals", ["avl", "av", "al", "vl"])
@pytest.mark.parametrize("R", [1, 5, 37])
def test_gated_attention_module_against_float64_oracle(R, modals):
    """MMGatedAttention(300, 100) 'general' in eval mode, three modalities and each pair: output, input gradients and every live
    parameter's gradient (the transforms of the modalities in use, the gate weights and biases of the pairs in use)."""
    seed = 900 + R
    mod = MMGatedAttention(300, 100, att_type='general')
    mod.load_state_dict(synthetic.seeded_state_dict(mod.state_dict(), seed))
    params = {k: v.detach().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    mod = mod.to(DEV).eval()
    rs = np.random.RandomState(seed)
    xs = {m: torch.from_numpy(rs.randn(R, 300).astype(np.float32)) for m in "avl"}
    npairs = 3 if modals == "avl" else 1
    G = torch.from_numpy(rs.randn(R, 100 * npairs).astype(np.float32))
    dev = {m: xs[m].to(DEV).requires_grad_(True) if m in modals else [] for m in "avl"}
    y = mod(dev["a"], dev["v"], dev["l"], list(modals))
    assert tuple(y.shape) == (R, 100 * npairs)
    (y * G.to(DEV)).sum().backward()
    xo = {m: xs[m].double().requires_grad_(True) for m in "avl"}
    want = O.gated_attention_general(xo["a"], xo["v"], xo["l"], params, prefix="", modals=modals)
    (want * G.double()).sum().backward()
    worst = {"y": rel_max(y, want)}
    for m in modals:
        worst["d" + m] = rel_max(dev[m].grad, xo[m].grad)
    live = ["transform_" + m for m in modals] + ["transform_" + p for p in ("av", "al", "vl") if p[0] in modals and p[1] in modals]
    for k, p in mod.named_parameters():
        if k.rsplit(".", 1)[0] in live:
            assert p.grad is not None and params[k].grad is not None, k
            worst[k] = rel_max(p.grad, params[k].grad)
        else:
            assert p.grad is None and params[k].grad is None, k
    print("RATIO gated_module[R=%d,%s] worst %s %.3g (of 1e-5)" % (R, modals, max(worst, key=worst.get), max(worst.values())))
    for k, v in worst.items():
        assert v < 1e-5, (k, v)


# ---- LMF off its defaults ------------------------------------------------------------------------------------------------------
LMF_CASES = {
    "rank1": (dict(rank=1), 5),
    "rank3": (dict(rank=3), 5),                                      # 9 grouped problems: the last chunk holds one
    "rank8": (dict(rank=8), 5),                                      # the kernels' limit; [dP | g | T] is 7 508 columns wide
    "unequal_hidden": (dict(hidden_dims=(4, 36, 100), output_dim=8), 5),
    "out260": (dict(output_dim=260), 5),                             # one full trip of the 256-thread column loop and a short one
    "rows4097": (dict(output_dim=8, rank=2, hidden_dims=(4, 4, 4)), 4097),      # the grid-stride over rows
}


@pytest.mark.parametrize("case", sorted(LMF_CASES))
def test_lmf_off_defaults_against_float64(case):
    kw, N = LMF_CASES[case]
    torch.manual_seed(sorted(LMF_CASES).index(case) + 50)
    mod = LMF(**kw).to(DEV)
    with torch.no_grad():
        mod.fusion_bias.normal_()
        for net in (mod.audio_subnet, mod.video_subnet, mod.text_subnet):
            net.weight.mul_(3.0)
    xs = [torch.randn(N, 300, device=DEV, requires_grad=True) for _ in range(3)]
    G = torch.randn(N, mod.output_dim, device=DEV, dtype=torch.float64)
    out = mod(*xs)
    assert tuple(out.shape) == (N, mod.output_dim)
    (out.double() * G).sum().backward()
    got = [x.grad.clone() for x in xs] + [p.grad.clone() for p in mod.parameters()]
    ref = {k: v.detach().double().requires_grad_(True) for k, v in mod.state_dict().items()}
    xd = [x.detach().double().requires_grad_(True) for x in xs]
    want_out = O.lmf(xd, ref)
    (want_out * G).sum().backward()
    want = [x.grad for x in xd] + [ref[k].grad for k, _ in mod.named_parameters()]
    worst = {"out": float((out.double() - want_out).abs().max() / want_out.abs().max())}
    names = ["dx_a", "dx_v", "dx_t"] + [k for k, _ in mod.named_parameters()]
    for n, a, b in zip(names, got, want):
        assert a.shape == b.shape, n
        worst[n] = float((a.double() - b).abs().max() / b.abs().max())
    print("RATIO lmf[%s] worst %s %.3g (of 1e-5)" % (case, max(worst, key=worst.get), max(worst.values())))
    for k, v in worst.items():
        assert v < 1e-5, (k, v)


def test_lmf_refuses_what_its_kernels_do_not_take():
    torch.manual_seed(5)
    xs = [torch.randn(3, 300, device=DEV) for _ in range(3)]
    with pytest.raises(ValueError, match=r"rank 9 is outside the kernels' range 1\.\.8"):
        LMF(rank=9).to(DEV)(*xs)
    with pytest.raises(ValueError, match="multiples of 4"):
        LMF(output_dim=6).to(DEV)(*xs)
    with pytest.raises(ValueError, match="multiples of 4"):
        LMF(hidden_dims=(300, 30, 300)).to(DEV)(*xs)
