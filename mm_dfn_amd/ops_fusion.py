"""Kernels of the fusion modules (MFN, MMGatedAttention, LMF, TFN) and of the graph-free model's per-modality products.

Part of the operator layer over the C-ABI kernels (libmmdfn_hip.so); `mm_dfn_amd.ops` re-exports every name.
Every function launches hand-written gfx950 kernels on the current HIP stream; there is no CPU / eager fallback.
"""
import torch

from . import _hip
from .ops_flags import keep_scale, reserve_counters
from .ops_linear import linear_group_raw
from .ops_pad import weight_operand
from .ops_wgrad import _wgrad, colsum, gemm_tn_grouped

_GROUP = 8          # problems per grouped launch (linear_small.hip SG_MAX, gemm_tn.hip TN_MAXG)
_LMF_RANK_MAX = 8   # csrc/lmf.hip LMF_RMAX
_COLSUM_COLS = 4096 # columns per column-sum launch (csrc/encoder_glue.hip mmdfn_colsum: 64 blocks of 64 columns)


def _chunks(xs):
    return [xs[i:i + _GROUP] for i in range(0, len(xs), _GROUP)]


def _colsum_wide(D):
    """colsum of a matrix of any width (a multiple of 4): one launch per 4096 columns, each on its column block in place."""
    if D.shape[1] <= _COLSUM_COLS:
        return colsum(D)
    return torch.cat([colsum(D[:, i:i + _COLSUM_COLS]) for i in range(0, D.shape[1], _COLSUM_COLS)])


class _SoftmaxScale(torch.autograd.Function):
    """out = softmax(z, dim=1) * c (MFN attention, model_fusion.py:96-97)."""

    @staticmethod
    def forward(ctx, z, c):
        _hip.require_cuda(z, c)
        z, c = z.contiguous(), c.contiguous()
        att, out = torch.empty_like(z), torch.empty_like(z)
        _hip.call("mmdfn_softmax_scale_fwd", _hip.ptr(z), _hip.ptr(c), _hip.ptr(att), _hip.ptr(out), z.shape[0],
                  z.shape[1], _hip.stream())
        ctx.save_for_backward(att, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        att, c = ctx.saved_tensors
        dout = dout.contiguous()
        dz, dc = torch.empty_like(att), torch.empty_like(att)
        _hip.call("mmdfn_softmax_scale_bwd", _hip.ptr(att), _hip.ptr(c), _hip.ptr(dout), _hip.ptr(dz), _hip.ptr(dc),
                  att.shape[0], att.shape[1], _hip.stream())
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
        _hip.call("mmdfn_mfn_mem_fwd", _hip.ptr(u), _hip.ptr(v1), _hip.ptr(v2), _hip.ptr(mem), _hip.ptr(out),
                  _hip.ptr(saved), mem.numel(), _hip.stream())
        ctx.save_for_backward(saved, mem)
        return out

    @staticmethod
    def backward(ctx, dout):
        saved, mem = ctx.saved_tensors
        dout = dout.contiguous()
        du, dv1, dv2, dmem = (torch.empty_like(mem) for _ in range(4))
        _hip.call("mmdfn_mfn_mem_bwd", _hip.ptr(saved), _hip.ptr(mem), _hip.ptr(dout), _hip.ptr(du), _hip.ptr(dv1),
                  _hip.ptr(dv2), _hip.ptr(dmem), mem.numel(), _hip.stream())
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
        _hip.call("mmdfn_gated_pair_fwd", _hip.ptr(xm), _hip.ptr(xn), _hip.ptr(w), _hip.ptr(b), _hip.ptr(pm), _hip.ptr(pn),
                  _hip.ptr(out), _hip.ptr(zs), R, D, C, _hip.stream())
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
        _hip.call("mmdfn_gated_pair_bwd", _hip.ptr(xm), _hip.ptr(xn), _hip.ptr(w), _hip.ptr(pm), _hip.ptr(pn), _hip.ptr(zs),
                  _hip.ptr(dout), _hip.ptr(dxm), _hip.ptr(dxn), _hip.ptr(dpm), _hip.ptr(dpn),
                  _hip.ptr(dpre), R, D, C, _hip.stream())
        dwb = torch.empty(3 * D + 1, dtype=xm.dtype, device=xm.device)
        _hip.call("mmdfn_rowscale_colsum", _hip.ptr(dpre), _hip.ptr(xm), _hip.ptr(xn), _hip.ptr(dwb), R, D, _hip.stream())
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
    rows and forms the rank-weighted product.  Backward: csrc/lmf.hip writes [dP | g | T], one column-sum launch per 4096
    columns of it gives d factor_m[r, 0, :], d bias and d w, grouped gemm_tn launches give d factor_m[r, 1:, :] = h_m^T dP_m,r,
    and R accumulating grouped launches give dh_m = sum_r dP_m,r factor_m[r, 1:, :]^T."""

    @staticmethod
    def forward(ctx, ha, hv, ht, fa, fv, ft, w, bias):
        hs, fs = [h.contiguous() for h in (ha, hv, ht)], (fa, fv, ft)
        _hip.require_cuda(*hs, *fs, w, bias)
        _hip.require_f32(*hs, *fs, w, bias)
        fs = tuple(f.contiguous() for f in fs)
        R, O, N = fs[0].shape[0], fs[0].shape[2], hs[0].shape[0]
        if not 1 <= R <= _LMF_RANK_MAX:
            raise ValueError("lmf_fuse: rank %d is outside the kernels' range 1..%d" % (R, _LMF_RANK_MAX))
        if O % 4 or any(h.shape[1] % 4 for h in hs):
            raise ValueError("lmf_fuse: output and hidden widths must be multiples of 4")
        P = torch.empty(N, 3 * R * O, dtype=torch.float32, device=hs[0].device)
        probs = [dict(x=hs[m], wk=fs[m][r, 1:, :], out=P[:, (m * R + r) * O:(m * R + r + 1) * O])
                 for m in range(3) for r in range(R)]
        for c in _chunks(probs):
            linear_group_raw(c)
        w, bias = w.contiguous(), bias.contiguous()
        out = torch.empty(N, O, dtype=torch.float32, device=P.device)
        _hip.call("mmdfn_lmf_fwd", _hip.ptr(P), _hip.ptr(fs[0]), _hip.ptr(fs[1]), _hip.ptr(fs[2]), fs[0].stride(0),
                  fs[1].stride(0), fs[2].stride(0), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(out), N, O, R,
                  P.stride(0), O, _hip.stream())
        ctx.save_for_backward(P, *hs, *fs, w)
        return out

    @staticmethod
    def backward(ctx, g):
        P, ha, hv, ht, fa, fv, ft, w = ctx.saved_tensors
        hs, fs = (ha, hv, ht), (fa, fv, ft)
        R, O, N = fa.shape[0], fa.shape[2], P.shape[0]
        g = g.contiguous()
        width = int(_hip.query("mmdfn_lmf_bwd_width", O, R))
        D = torch.empty(N, width, dtype=torch.float32, device=P.device)
        _hip.call("mmdfn_lmf_bwd", _hip.ptr(g), _hip.ptr(P), _hip.ptr(w), _hip.ptr(D), N, O, R, g.stride(0), P.stride(0),
                  D.stride(0), _hip.stream())
        sums = _colsum_wide(D)       # (rank 5 and up at the default 300 outputs: more than one launch's 4096 columns)
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


def _tfn_rows(h):
    """(N, H) fp32 rows with unit inner stride (a column slice of a wider matrix is read in place)."""
    return h if h.stride(1) == 1 and h.stride(0) >= h.shape[1] else h.contiguous()


def _tfn_workspace(N, H, O, which, device):
    n = int(_hip.query("mmdfn_tfn_workspace", N, H[0], H[1], H[2], O, which))
    if n < 0:
        raise ValueError("tfn_fuse: hidden widths %s with %d outputs are not taken by the kernels (at most 304 outputs; the three "
                         "[1, h] rows of 64 utterances must fit the LDS next to a weight tile)" % (tuple(H), O))
    return torch.empty(n, dtype=torch.float32, device=device)


class _Tfn(torch.autograd.Function):
    """Tensor fusion of TFN (reference model_fusion.py:189-206) after its subnets: out = act(dropout_p(Z) W1^T + b1) with
    Z[n, (i V1 + j) T1 + k] = [1, h_a][n, i] [1, h_v][n, j] [1, h_t][n, k].  Neither Z nor its dropout mask nor dZ exists:
    csrc/tensor_fusion.hip regenerates the fragments it needs in each of the three products (forward, dW1, dh_m), the keep
    flags as a function of the generator state the forward call read (saved as a 2-word device tensor) and the element's
    position.  Backward returns dh_a, dh_v, dh_t, dW1, db1 to autograd."""

    @staticmethod
    def forward(ctx, ha, hv, ht, W1, b1, p, training, relu):
        _hip.require_cuda(ha, hv, ht, W1, b1)
        _hip.require_f32(ha, hv, ht, W1, b1)
        if any(h.dim() != 2 or h.shape[0] != ha.shape[0] or h.shape[1] < 1 for h in (ha, hv, ht)) or ha.shape[0] < 1:
            raise ValueError("tfn_fuse: ha, hv, ht must be (N, H_m) matrices with the same N >= 1")
        hs = [_tfn_rows(h) for h in (ha, hv, ht)]
        N, H = hs[0].shape[0], [h.shape[1] for h in hs]
        K = (H[0] + 1) * (H[1] + 1) * (H[2] + 1)
        if W1.dim() != 2 or W1.shape[1] != K or b1.shape != (W1.shape[0],):
            raise ValueError("tfn_fuse: W1 must be (O, %d) and b1 (O,)" % K)
        O = W1.shape[0]
        if W1.stride(1) != 1 or W1.stride(0) < K:
            W1 = W1.contiguous()
        b1 = b1.contiguous()
        p = float(p)
        ws = _tfn_workspace(N, H, O, 0, ha.device)
        drop = bool(training) and p > 0.0
        used = state = None
        counters = 0
        if drop:
            state, counters = reserve_counters(N * ((K + 7) // 8), ha.device)
            used = torch.empty(2, dtype=torch.int64, device=ha.device)
        keep = max(0.0, 1.0 - p) if drop else 1.0
        scale = keep_scale(p) if drop else 1.0
        out = torch.empty(N, O, dtype=torch.float32, device=ha.device)
        _hip.call("mmdfn_tfn_fwd", _hip.ptr(hs[0]), _hip.ptr(hs[1]), _hip.ptr(hs[2]), hs[0].stride(0), hs[1].stride(0),
                  hs[2].stride(0), _hip.ptr(W1), W1.stride(0), _hip.ptr(b1), _hip.ptr(state), _hip.ptr(used),
                  counters, keep, scale, _hip.ptr(out), _hip.ptr(ws), N, H[0], H[1], H[2], O, int(bool(relu)),
                  _hip.stream())
        ctx.keep, ctx.scale, ctx.relu, ctx.drop = keep, scale, bool(relu), drop
        ctx.save_for_backward(hs[0], hs[1], hs[2], W1, out if relu else None, used)
        ctx.used_state = used                        # (tests: the flags of this call through ops.tfn_keep_flags)
        return out

    @staticmethod
    def backward(ctx, dy):
        ha, hv, ht, W1, y1, used = ctx.saved_tensors
        N, H, O, K = ha.shape[0], [ha.shape[1], hv.shape[1], ht.shape[1]], W1.shape[0], W1.shape[1]
        dy = dy.contiguous()
        ws = _tfn_workspace(N, H, O, 1, dy.device)
        dpre = torch.empty(N, O, dtype=torch.float32, device=dy.device)
        dhs = [torch.empty(N, h, dtype=torch.float32, device=dy.device) for h in H]
        _hip.call("mmdfn_tfn_bwd_input", _hip.ptr(dy), _hip.ptr(y1), int(ctx.relu), _hip.ptr(W1), W1.stride(0), _hip.ptr(ha),
                  _hip.ptr(hv), _hip.ptr(ht), ha.stride(0), hv.stride(0), ht.stride(0), _hip.ptr(used),
                  ctx.keep, ctx.scale, _hip.ptr(dpre), _hip.ptr(dhs[0]), _hip.ptr(dhs[1]),
                  _hip.ptr(dhs[2]), _hip.ptr(ws), N, H[0], H[1], H[2], O, _hip.stream())
        dW1 = db1 = None
        if ctx.needs_input_grad[3]:
            dW1 = torch.empty(O, K, dtype=torch.float32, device=dy.device)
            _hip.call("mmdfn_tfn_bwd_weight", _hip.ptr(dpre), _hip.ptr(ha), _hip.ptr(hv), _hip.ptr(ht), ha.stride(0),
                      hv.stride(0), ht.stride(0), _hip.ptr(used), ctx.keep, ctx.scale, _hip.ptr(dW1), N,
                      H[0], H[1], H[2], O, _hip.stream())
        if ctx.needs_input_grad[4]:
            db1 = colsum(dpre)
        return dhs[0], dhs[1], dhs[2], dW1, db1, None, None, None


def tfn_fuse(ha, hv, ht, W1, b1, p, training, relu=True):
    """(N, O) = act(dropout_p([1, h_a] (x) [1, h_v] (x) [1, h_t]) W1^T + b1), act = ReLU unless ``relu`` is False; the dropout
    (training mode, p > 0) draws from the package's keep-flag generator inside the kernels (see _Tfn)."""
    return _Tfn.apply(ha, hv, ht, W1, b1, p, training, relu)


def tfn_keep_flags(used_state, N, K, p, row0, rows):
    """Test / debug: the (rows, K) 0 / 1 keep flags that a training-mode ``tfn_fuse`` call of N rows whose generator state
    was ``used_state`` (2 int64 on the device: the tensor the call saved) applies to rows row0 .. row0 + rows - 1."""
    _hip.require_cuda(used_state)
    out = torch.empty(int(rows), int(K), dtype=torch.float32, device=used_state.device)
    _hip.call("mmdfn_tfn_keep_flags", _hip.ptr(used_state), max(0.0, 1.0 - float(p)), _hip.ptr(out), int(N), int(K),
              int(row0), int(rows), _hip.stream())
    return out
