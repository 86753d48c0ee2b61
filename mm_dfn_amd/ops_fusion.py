"""Kernels of the fusion modules (MFN, MMGatedAttention, LMF) and of the graph-free model's per-modality products.

Part of the operator layer over the C-ABI kernels (libmmdfn_hip.so); `mm_dfn_amd.ops` re-exports every name.
Every function launches hand-written gfx950 kernels on the current HIP stream; there is no CPU / eager fallback.
"""
import torch

from . import _hip
from .ops_linear import linear_group_raw
from .ops_pad import weight_operand
from .ops_wgrad import _wgrad, colsum, gemm_tn_grouped

_GROUP = 8          # problems per grouped launch (linear_small.hip SG_MAX, gemm_tn.hip TN_MAXG)


def _chunks(xs):
    return [xs[i:i + _GROUP] for i in range(0, len(xs), _GROUP)]


class _SoftmaxScale(torch.autograd.Function):
    """out = softmax(z, dim=1) * c (MFN attention, model_fusion.py:96-97)."""

    @staticmethod
    def forward(ctx, z, c):
        _hip.require_cuda(z, c)
        z, c = z.contiguous(), c.contiguous()
        att, out = torch.empty_like(z), torch.empty_like(z)
        _hip.check(_hip.lib().mmdfn_softmax_scale_fwd(_hip.ptr(z), _hip.ptr(c), _hip.ptr(att), _hip.ptr(out), z.shape[0],
                                                      z.shape[1], _hip.stream()), "mmdfn_softmax_scale_fwd")
        ctx.save_for_backward(att, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        att, c = ctx.saved_tensors
        dout = dout.contiguous()
        dz, dc = torch.empty_like(att), torch.empty_like(att)
        _hip.check(_hip.lib().mmdfn_softmax_scale_bwd(_hip.ptr(att), _hip.ptr(c), _hip.ptr(dout), _hip.ptr(dz), _hip.ptr(dc),
                                                      att.shape[0], att.shape[1], _hip.stream()), "mmdfn_softmax_scale_bwd")
        return dz, dc


def softmax_scale(z, c):
    return _SoftmaxScale.apply(z, c)


class _MfnMem(torch.autograd.Function):
    """mem' = sigmoid(v1) mem + sigmoid(v2) tanh(u)  (model_fusion.py:98-102)."""

    @staticmethod
    def forward(ctx, u, v1, v2, mem):
        _hip.require_cuda(u, v1, v2, mem)
        u, v1, v2, mem = u.contiguous(), v1.contiguous(), v2.contiguous(), mem.contiguous()
        out = torch.empty_like(mem)
        saved = torch.empty(3, mem.numel(), dtype=mem.dtype, device=mem.device)
        _hip.check(_hip.lib().mmdfn_mfn_mem_fwd(_hip.ptr(u), _hip.ptr(v1), _hip.ptr(v2), _hip.ptr(mem), _hip.ptr(out),
                                                _hip.ptr(saved), mem.numel(), _hip.stream()), "mmdfn_mfn_mem_fwd")
        ctx.save_for_backward(saved, mem)
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, mem = ctx.saved_tensors
        dout = dout.contiguous()
        du, dv1, dv2, dmem = (torch.empty_like(mem) for _ in range(4))
        _hip.check(_hip.lib().mmdfn_mfn_mem_bwd(_hip.ptr(saved), _hip.ptr(mem), _hip.ptr(dout), _hip.ptr(du), _hip.ptr(dv1),
                                                _hip.ptr(dv2), _hip.ptr(dmem), mem.numel(), _hip.stream()), "mmdfn_mfn_mem_bwd")
        return du, dv1, dv2, dmem


def mfn_mem(u, v1, v2, mem):
    return _MfnMem.apply(u, v1, v2, mem)


class _GatedPair(torch.autograd.Function):
    """h = z tanh(p_m) + (1 - z) tanh(p_n), z = sigmoid(w . [x_m | x_n | x_m * x_n] + b)  (model.py:766-781); w: (1, 3D)."""

    @staticmethod
    def forward(ctx, xm, xn, pm, pn, w, b):
        _hip.require_cuda(xm, xn, pm, pn, w, b)
        xm, xn, pm, pn, w = xm.contiguous(), xn.contiguous(), pm.contiguous(), pn.contiguous(), w.contiguous()
        R, D = xm.shape
        C = pm.shape[1]
        out = torch.empty_like(pm)
        zs = torch.empty(R, dtype=xm.dtype, device=xm.device)
        _hip.check(_hip.lib().mmdfn_gated_pair_fwd(_hip.ptr(xm), _hip.ptr(xn), _hip.ptr(w), _hip.ptr(b), _hip.ptr(pm), _hip.ptr(pn),
                                                   _hip.ptr(out), _hip.ptr(zs), R, D, C, _hip.stream()), "mmdfn_gated_pair_fwd")
        ctx.save_for_backward(xm, xn, pm, pn, w, zs)
        return out

    @staticmethod
    def backward(ctx, dout):
        xm, xn, pm, pn, w, zs = ctx.saved_tensors
        dout = dout.contiguous()
        R, D = xm.shape
        C = pm.shape[1]
        dxm, dxn, dpm, dpn = torch.empty_like(xm), torch.empty_like(xn), torch.empty_like(pm), torch.empty_like(pn)
        dpre = torch.empty(R, dtype=xm.dtype, device=xm.device)
        lib = _hip.lib()
        _hip.check(lib.mmdfn_gated_pair_bwd(_hip.ptr(xm), _hip.ptr(xn), _hip.ptr(w), _hip.ptr(pm), _hip.ptr(pn), _hip.ptr(zs),
                                            _hip.ptr(dout), _hip.ptr(dxm), _hip.ptr(dxn), _hip.ptr(dpm), _hip.ptr(dpn),
                                            _hip.ptr(dpre), R, D, C, _hip.stream()), "mmdfn_gated_pair_bwd")
        dwb = torch.empty(3 * D + 1, dtype=xm.dtype, device=xm.device)
        _hip.check(lib.mmdfn_rowscale_colsum(_hip.ptr(dpre), _hip.ptr(xm), _hip.ptr(xn), _hip.ptr(dwb), R, D, _hip.stream()),
                   "mmdfn_rowscale_colsum")
        return dxm, dxn, dpm, dpn, dwb[:3 * D].view(1, 3 * D), dwb[3 * D:].view(1)


def gated_pair(xm, xn, pm, pn, w, b):
    return _GatedPair.apply(xm, xn, pm, pn, w, b)


class _ResidualProducts(torch.autograd.Function):
    """E[m] = [f_m W_m^T + b_m | f_m] for the M modalities of the graph-free model (reference model.py:1376-1384: the
    linear output first).  feats (M, N, D) -> E (M, N, H + D): the M products are one grouped launch of the few-row kernel
    writing the left column block of each E[m] in place; the right blocks take f_m by one strided copy (the only copy E
    needs).  Backward: dF_m = dE_m[:, H:] + dE_m[:, :H] W_m as one grouped launch that reads both column blocks of dE in
    place (the right block as the kernel's addend); dW_m / db_m = dE_m[:, :H]^T f_m through the step's weight-gradient batch
    (or in line), on the row-strided block as well."""

    @staticmethod
    def forward(ctx, feats, *params):
        _hip.require_cuda(feats)
        M, N, D = feats.shape
        ws, bs = params[:M], params[M:]
        H = ws[0].shape[0]
        feats = feats.contiguous()
        E = torch.empty(M, N, H + D, dtype=feats.dtype, device=feats.device)
        E[:, :, H:].copy_(feats)
        linear_group_raw([dict(x=feats[m], w=ws[m], b=bs[m], out=E[m][:, :H]) for m in range(M)])
        ctx.H = H
        ctx.param_refs = list(zip(ws, bs))
        ctx.save_for_backward(feats, *ws)
        return E

    @staticmethod
    def backward(ctx, dE):
        feats, *ws = ctx.saved_tensors
        M, H = feats.shape[0], ctx.H
        dE = dE.contiguous()
        dF = torch.empty_like(feats)
        linear_group_raw([dict(x=dE[m][:, :H], wk=weight_operand(ws[m]), out=dF[m], addend=dE[m][:, H:]) for m in range(M)])
        wg = [_wgrad(dE[m][:, :H], feats[m], *ctx.param_refs[m]) for m in range(M)]
        return (dF,) + tuple(r[0] for r in wg) + tuple(r[1] for r in wg)


def residual_products(feats, weights, biases):
    """[cat([Linear_m(f_m), f_m], -1) for m] as one (M, N, H + D) tensor (see _ResidualProducts)."""
    return _ResidualProducts.apply(feats, *weights, *biases)


class _Lmf(torch.autograd.Function):
    """Low-rank fusion of LMF (reference model_fusion.py:274-310) after its subnets:
    out = sum_r w_r prod_m ([1, h_m] . factor_m[r]) + bias, modalities a, v, t.  The 3 R products h_m . factor_m[r, 1:, :]
    are grouped launches of the few-row kernel into column blocks of one (N, 3 R O) buffer P; csrc/lmf.hip adds the constant
    rows and forms the rank-weighted product.  Backward: csrc/lmf.hip writes [dP | g | T], one column-sum launch gives
    d factor_m[r, 0, :], d bias and d w, grouped gemm_tn launches give d factor_m[r, 1:, :] = h_m^T dP_m,r, and R accumulating
    grouped launches give dh_m = sum_r dP_m,r factor_m[r, 1:, :]^T."""

    @staticmethod
    def forward(ctx, ha, hv, ht, fa, fv, ft, w, bias):
        hs, fs = [h.contiguous() for h in (ha, hv, ht)], (fa, fv, ft)
        _hip.require_cuda(*hs, *fs, w, bias)
        _hip.require_f32(*hs, *fs, w, bias)
        fs = tuple(f.contiguous() for f in fs)
        R, O, N = fs[0].shape[0], fs[0].shape[2], hs[0].shape[0]
        if O % 4 or any(h.shape[1] % 4 for h in hs):
            raise ValueError("lmf_fuse: output and hidden widths must be multiples of 4")
        P = torch.empty(N, 3 * R * O, dtype=torch.float32, device=hs[0].device)
        probs = [dict(x=hs[m], wk=fs[m][r, 1:, :], out=P[:, (m * R + r) * O:(m * R + r + 1) * O])
                 for m in range(3) for r in range(R)]
        for c in _chunks(probs):
            linear_group_raw(c)
        w, bias = w.contiguous(), bias.contiguous()
        out = torch.empty(N, O, dtype=torch.float32, device=P.device)
        _hip.check(_hip.lib().mmdfn_lmf_fwd(_hip.ptr(P), _hip.ptr(fs[0]), _hip.ptr(fs[1]), _hip.ptr(fs[2]), fs[0].stride(0),
                                            fs[1].stride(0), fs[2].stride(0), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(out), N, O, R,
                                            P.stride(0), O, _hip.stream()), "mmdfn_lmf_fwd")
        ctx.save_for_backward(P, *hs, *fs, w)
        return out

    @staticmethod
    def backward(ctx, g):
        P, ha, hv, ht, fa, fv, ft, w = ctx.saved_tensors
        hs, fs = (ha, hv, ht), (fa, fv, ft)
        R, O, N = fa.shape[0], fa.shape[2], P.shape[0]
        g = g.contiguous()
        lib = _hip.lib()
        width = int(lib.mmdfn_lmf_bwd_width(O, R))
        D = torch.empty(N, width, dtype=torch.float32, device=P.device)
        _hip.check(lib.mmdfn_lmf_bwd(_hip.ptr(g), _hip.ptr(P), _hip.ptr(w), _hip.ptr(D), N, O, R, g.stride(0), P.stride(0),
                                     D.stride(0), _hip.stream()), "mmdfn_lmf_bwd")
        sums = colsum(D)
        blk = lambda m, r: D[:, (m * R + r) * O:(m * R + r + 1) * O]
        dfs = [torch.empty_like(f) for f in fs]
        for m in range(3):
            dfs[m][:, 0, :].copy_(sums[m * R * O:(m + 1) * R * O].view(R, O))
        probs = [dict(A=hs[m], B=blk(m, r), C=dfs[m][r, 1:, :]) for m in range(3) for r in range(R)]
        for c in _chunks(probs):
            gemm_tn_grouped(c)
        dhs = [torch.empty_like(h) for h in hs]
        for r in range(R):
            linear_group_raw([dict(x=blk(m, r), w=fs[m][r, 1:, :], out=dhs[m], accumulate=r > 0) for m in range(3)])
        dbias = sums[3 * R * O:3 * R * O + O].view(1, O)
        dw = sums[3 * R * O + O:3 * R * O + O + R].view(1, R)
        return dhs[0], dhs[1], dhs[2], dfs[0], dfs[1], dfs[2], dw, dbias


def lmf_fuse(ha, hv, ht, fa, fv, ft, w, bias):
    """(N, O) = sum_r w[0, r] prod_m ([1, h_m] . factor_m[r]) + bias (see _Lmf)."""
    return _Lmf.apply(ha, hv, ht, fa, fv, ft, w, bias)
