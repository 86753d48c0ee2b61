"""Weight fragment images of the GCN stack kernels (csrc/stack_images.hip, csrc/stack_image_map.h, the *_img entry points of
csrc/gcn_stack.hip, ops_linear.stack_image, gcn_stack.STACK_IMAGES).

An image stores, for every (column block, tile, K-chunk, lane), the float4 that the consumer lane of the staging kernels reads
from the padded LDS copy of its weight slice.  The kernels' image forms take their B fragments from it and run the same MFMAs
on the same values, so every check here is BIT equality, not a tolerance:
  * the host index function against a numpy restatement of the staging kernels' LDS copy and fragment addressing (no GPU),
  * each *_img entry against the entry without the suffix on the same operands,
  * the registry: images follow in-place weight updates, FlatAdam steps around a captured step, and leave with their parameter,
  * the whole autograd node with the switch on against the switch off.
"""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
KINDS = dict(input_fwd=0, input_bwd=1, layer_bwd=2, gate_fwd=3, gate_bwd=4)
UB, CBW = 32, 64


def frag_row(i):
    return 2 * i if i < 4 else (2 * (i - 4) + 1 if i < 12 else 2 * (i - 12) + 8)


def frag_unit(g):
    return ((g & 1) << 1) | (g >> 1)


def lds_stride(K):
    ld = ((K + 15) & ~15) + 4
    return ld + 4 if ((ld >> 2) & 1) == 0 else ld


def image_dims(kind, H, F, has_h):
    """(column blocks, tiles per column block, K chunks), restated from the kernels' launch geometry."""
    c16 = lambda v: (v + 15) // 16
    if kind == 0:
        return 1, c16(H), c16(F)
    if kind == 1:
        return 1, c16(F), c16(H)
    if kind == 2:
        return 1, c16(2 * H), c16(H)
    if kind == 3:
        return (H + UB - 1) // UB, 4 * UB // 16, c16(2 * H if has_h else H)
    nb = (H + CBW - 1) // CBW
    return (2 * nb if has_h else nb), CBW // 16, c16(4 * H)


def lds_copies(kind, H, F, has_h, w1, w2):
    """The zero-padded LDS weight slice of every column block as the staging kernels build it (WeightStager::commit and the
    two lstm_gate_*_ws prologues): k-contiguous rows of stride lds_stride(K), pads and missing rows zero."""
    ncb, ntiles, nk = image_dims(kind, H, F, has_h)
    out = []
    for cb in range(ncb):
        if kind == 0:                                  # KMAJOR = false, W0 (H, F)
            K = F
            sW = np.zeros((16 * ntiles, lds_stride(K)), np.float64)
            sW[:H, :K] = w1
        elif kind == 1:                                # KMAJOR = true, W0 (H, F): sW[n][k] = W0[k][n]
            K = H
            sW = np.zeros((16 * ntiles, lds_stride(K)), np.float64)
            sW[:F, :K] = w1.T
        elif kind == 2:                                # KMAJOR = false, W (2H, H)
            K = H
            sW = np.zeros((16 * ntiles, lds_stride(K)), np.float64)
            sW[:2 * H, :K] = w1
        elif kind == 3:                                # rows (gate, ul) <- [W_ih | W_hh] row gate * H + u0 + ul
            K = 2 * H if has_h else H
            sW = np.zeros((4 * UB, lds_stride(K)), np.float64)
            u0 = cb * UB
            nu = min(UB, H - u0)
            for gate in range(4):
                sW[gate * UB:gate * UB + nu, :H] = w1[gate * H + u0:gate * H + u0 + nu]
                if has_h:
                    sW[gate * UB:gate * UB + nu, H:2 * H] = w2[gate * H + u0:gate * H + u0 + nu]
        else:                                          # W_ih / W_hh (4H, H) column block n0: sW[n][k] = W[k][n0 + n]
            K = 4 * H
            nb = (H + CBW - 1) // CBW
            src = w2 if cb >= nb else w1
            n0 = (cb - nb if cb >= nb else cb) * CBW
            ncols = min(CBW, H - n0)
            sW = np.zeros((CBW, lds_stride(K)), np.float64)
            sW[:ncols, :K] = src[:, n0:n0 + ncols].T
        out.append(sW)
    return out


def expected_image(kind, H, F, has_h, w1, w2):
    """What contract<NT> reads: ld4(sW + (16 t + frag_row(l & 15)) * ldw + 4 frag_unit(l >> 4) + 16 kc), as [cb, t, kc, l, j]."""
    ncb, ntiles, nk = image_dims(kind, H, F, has_h)
    rows = np.array([frag_row(l & 15) for l in range(64)])
    cols = np.array([4 * frag_unit(l >> 4) for l in range(64)])
    img = np.zeros((ncb, ntiles, nk, 64, 4), np.float64)
    for cb, sW in enumerate(lds_copies(kind, H, F, has_h, w1, w2)):
        for t in range(ntiles):
            for kc in range(nk):
                for j in range(4):
                    img[cb, t, kc, :, j] = sW[16 * t + rows, 16 * kc + cols + j]
    return img


def labelled_weights(kind, H, F):
    """Matrices whose every element is a distinct non-zero number (w2's continue w1's), exact in float32."""
    shape = (H, F) if kind < 2 else ((2 * H, H) if kind == 2 else (4 * H, H))
    n = shape[0] * shape[1]
    w1 = np.arange(1, n + 1, dtype=np.float64).reshape(shape)
    return w1, w1 + n


_MAPS = {}


def host_map(kind, H, F, has_h):
    """(src, row, col) arrays [cb, t, kc, l, j] from the library's host index function (the one the cut kernel evaluates)."""
    key = (kind, H, F if kind < 2 else 0, has_h if kind >= 3 else 0)
    if key in _MAPS:
        return _MAPS[key]
    from mm_dfn_amd import _hip
    fn = _hip.lib().mmdfn_stack_image_source
    ncb, ntiles, nk = image_dims(kind, H, F, has_h)
    assert _hip.query("mmdfn_stack_images_workspace", kind, H, F, has_h) == ncb * ntiles * nk * 64 * 16
    src = np.zeros((ncb, ntiles, nk, 64, 4), np.int64)
    row, col = np.zeros_like(src), np.zeros_like(src)
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    pr, pc = ctypes.byref(r), ctypes.byref(c)
    for cb in range(ncb):
        for t in range(ntiles):
            for kc in range(nk):
                for l in range(64):
                    for j in range(4):
                        s = fn(kind, H, F, has_h, cb, t, kc, l, j, pr, pc)
                        src[cb, t, kc, l, j], row[cb, t, kc, l, j], col[cb, t, kc, l, j] = s, r.value, c.value
    _MAPS[key] = (src, row, col)
    return _MAPS[key]


MAP_CASES = ([(k, H, F, 0) for k in (0, 1) for H in (4, 36, 100) for F in (4, 200, 256)]
             + [(2, H, 4, 0) for H in (4, 36, 100)]
             + [(k, H, 4, has_h) for k in (3, 4) for H in (4, 36, 100) for has_h in (0, 1)])


@pytest.mark.parametrize("kind,H,F,has_h", MAP_CASES)
def test_host_index_function_restates_the_staged_slice(kind, H, F, has_h):
    from mm_dfn_amd import build
    import os
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    w1, w2 = labelled_weights(kind, H, F)
    want = expected_image(kind, H, F, has_h, w1, w2 if (kind >= 3 and has_h) else None)
    src, row, col = host_map(kind, H, F, has_h)
    assert src.min() >= 0 and src.max() <= (2 if (kind >= 3 and has_h) else 1)
    got = np.where(src == 1, w1[row.clip(0, w1.shape[0] - 1), col.clip(0, w1.shape[1] - 1)], 0.0)
    got = np.where(src == 2, w2[row.clip(0, w2.shape[0] - 1), col.clip(0, w2.shape[1] - 1)], got)
    assert (src == 0).sum() == (want == 0).sum()
    assert np.array_equal(got, want)
    # every parameter element the slices cover appears (the image drops nothing)
    covered = np.unique(got[got != 0])
    if kind < 3:
        assert covered.size == w1.size
    elif kind == 3:
        assert covered.size == (2 if has_h else 1) * w1.size
    else:
        assert covered.size == (2 if has_h else 1) * w1.size


def test_host_index_function_rejects_positions_outside_the_image():
    from mm_dfn_amd import _hip, build
    import os
    if not os.path.exists(build.LIBPATH):
        pytest.skip("libmmdfn_hip.so not built here (hipcc unavailable?)")
    fn = _hip.lib().mmdfn_stack_image_source
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    ok = (0, 100, 200, 0, 0, 6, 12, 63, 3)
    assert fn(*ok, ctypes.byref(r), ctypes.byref(c)) in (0, 1)
    for i, bad in ((0, 5), (1, 104), (1, 102), (2, 260), (4, 1), (5, 7), (6, 13), (7, 64), (8, 4), (5, -1)):
        args = list(ok)
        args[i] = bad
        assert fn(*args, ctypes.byref(r), ctypes.byref(c)) == -1, (i, bad)
    assert _hip.query("mmdfn_stack_images_workspace", 5, 100, 200, 0) == -1
    assert _hip.query("mmdfn_stack_images_workspace", 0, 100, 258, 0) == -1


# ---------------------------------------------------------------------------------------------------------------- GPU side
def _t(rs, *sh, scale=1.0):
    return torch.from_numpy((rs.randn(*sh) * scale).astype(np.float32)).to(DEV)


def _flags(rs, *sh):
    return torch.from_numpy((rs.uniform(size=sh) > 0.3).astype(np.float32)).to(DEV)


def _nan(*sh):
    return torch.full(sh, float("nan"), device=DEV)


def _bits(a):
    return a.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def cut_image(kind, w1, w2, H, F, has_h):
    from mm_dfn_amd import _hip
    nbytes = _hip.query("mmdfn_stack_images_workspace", kind, H, F, has_h)
    assert nbytes > 0
    img = torch.full((nbytes // 4,), float("nan"), device=DEV)
    _hip.call("mmdfn_cut_stack_images", 1, _hip.int_array([kind]), _hip.ptr_array([w1]), _hip.ptr_array([w2]),
              _hip.int_array([H]), _hip.int_array([F]), _hip.int_array([has_h]), _hip.ptr_array([img]), _hip.stream())
    return img


@gpu
@pytest.mark.parametrize("kind,H,F,has_h", [(0, 100, 200, 0), (1, 100, 200, 0), (2, 100, 4, 0), (3, 100, 4, 1), (3, 36, 4, 0),
                                             (4, 100, 4, 1), (4, 36, 4, 0)])
def test_cut_image_holds_the_parameter_bits_or_zero(kind, H, F, has_h):
    rs = np.random.RandomState(17 + kind + H)
    shape = (H, F) if kind < 2 else ((2 * H, H) if kind == 2 else (4 * H, H))
    w1, w2 = _t(rs, *shape), (_t(rs, *shape) if kind >= 3 else None)
    img = cut_image(kind, w1, w2 if has_h else None, H, F, has_h).cpu().numpy()
    src, row, col = host_map(kind, H, F, has_h)
    a1 = w1.cpu().numpy()
    want = np.where(src == 1, a1[row.clip(0, a1.shape[0] - 1), col.clip(0, a1.shape[1] - 1)], np.float32(0.0))
    if w2 is not None:
        a2 = w2.cpu().numpy()
        want = np.where(src == 2, a2[row.clip(0, a2.shape[0] - 1), col.clip(0, a2.shape[1] - 1)], want)
    assert np.array_equal(img.view(np.int32), want.astype(np.float32).reshape(-1).view(np.int32))


ROWS = [1, 16, 17, 47, 330]


@gpu
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("H", [36, 100])
def test_input_kernels_image_form_is_bit_equal(R, H):
    from mm_dfn_amd import _hip
    P, st = _hip.ptr, _hip.stream()
    for F in (20, 200):
        for masked in (False, True):
            rs = np.random.RandomState(R + 3 * H + F)
            x, W0, b0 = _t(rs, R, F), _t(rs, H, F, scale=0.2), _t(rs, H)
            mx, m0 = (_flags(rs, R, F), _flags(rs, R, H)) if masked else (None, None)
            ms = 1.0 / 0.7 if masked else 1.0
            ldxd = F + H
            img = cut_image(0, W0, None, H, F, 0)
            outs = []
            for image in (None, img):
                xd, h0, cur = _nan(R, ldxd), _nan(R, H), _nan(R, H)
                if image is None:
                    _hip.call("mmdfn_gcn_input_fwd", P(x), P(mx), P(W0), P(b0), P(m0), P(xd), P(h0), P(cur), R, F, H, ldxd, ms, st)
                else:
                    _hip.call("mmdfn_gcn_input_fwd_img", P(x), P(mx), P(W0), P(b0), P(m0), P(xd), P(h0), P(cur), R, F, H, ldxd, ms,
                              P(image), st)
                outs.append((xd, h0, cur))
            torch.cuda.synchronize()
            assert not torch.isnan(outs[0][1]).any()
            for a, b in zip(*outs):
                assert same_bits(a, b), ("input_fwd", R, H, F, masked)
            # backward of the same stage; dxd with a row stride > F (the residue output's gradient) or absent
            h0 = outs[0][1]
            dcur, dh0 = _t(rs, R, H), _t(rs, R, H)
            dxd = _t(rs, R, F + H) if masked else None
            img = cut_image(1, W0, None, H, F, 0)
            outs = []
            for image in (None, img):
                dpre, dx = _nan(R, H), _nan(R, F)
                args = (P(dcur), P(m0), P(dh0), P(h0), P(W0), P(dxd), P(mx), P(dpre), P(dx), R, F, H, F + H if masked else 0, ms)
                if image is None:
                    _hip.call("mmdfn_gcn_input_bwd", *args, st)
                else:
                    _hip.call("mmdfn_gcn_input_bwd_img", *args, P(image), st)
                outs.append((dpre, dx))
            torch.cuda.synchronize()
            assert not torch.isnan(outs[0][1]).any()
            for a, b in zip(*outs):
                assert same_bits(a, b), ("input_bwd", R, H, F, masked)


@gpu
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("H", [36, 100])
def test_layer_backward_image_form_is_bit_equal(R, H):
    from mm_dfn_amd import _hip
    P, st = _hip.ptr, _hip.stream()
    for acc_h0, wide in ((0, False), (1, True)):
        rs = np.random.RandomState(R + 5 * H + acc_h0)
        lddo, lddhi = (H + 12, 2 * H) if wide else (H, H)
        dout, gmask, W = _t(rs, R, lddo), _flags(rs, R, H) * 1.25, _t(rs, 2 * H, H, scale=0.2)
        dh0_init = _t(rs, R, H)
        theta, alpha = math.log(0.5 / 2 + 1), 0.1
        img = cut_image(2, W, None, H, 4, 0)
        outs = []
        for image in (None, img):
            dP, dhi, dh0 = _nan(R, H), _nan(R, lddhi), dh0_init.clone()
            args = (P(dout), P(gmask), P(W), P(dP), P(dhi), P(dh0), theta, alpha, R, H, lddo, acc_h0, lddhi)
            if image is None:
                _hip.call("mmdfn_gcnii_layer_bwd_ld", *args, st)
            else:
                _hip.call("mmdfn_gcnii_layer_bwd_ld_img", *args, P(image), st)
            outs.append((dP, dhi, dh0))
        torch.cuda.synchronize()
        assert not torch.isnan(outs[0][1][:, :H]).any()
        for a, b in zip(*outs):
            assert same_bits(a, b), ("layer_bwd", R, H, acc_h0)


@gpu
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("H", [36, 100])
def test_gate_kernels_image_form_is_bit_equal(R, H):
    from mm_dfn_amd import _hip
    P, st = _hip.ptr, _hip.stream()
    for has_h in (0, 1):
        rs = np.random.RandomState(R + 7 * H + has_h)
        q, Wih, Whh = _t(rs, R, H), _t(rs, 4 * H, H, scale=0.2), _t(rs, 4 * H, H, scale=0.2)
        b1, b2 = _t(rs, 4 * H), _t(rs, 4 * H)
        ldh = 2 * H                                          # the layers' hidden states are column blocks of one buffer
        hbuf = _t(rs, R, ldh)
        h, c = (hbuf[:, :H], _t(rs, R, H)) if has_h else (None, None)
        img = cut_image(3, Wih, Whh if has_h else None, H, 4, has_h)
        outs = []
        for image in (None, img):
            gates, hout, cout = _nan(R, 4 * H), _nan(R, ldh), _nan(R, H)
            args = (P(q), P(h), P(c), P(Wih), P(Whh), P(b1), P(b2), P(gates), P(hout[:, H:]), P(cout), R, H, ldh, None)
            if image is None:
                _hip.call("mmdfn_lstm_gate_fwd_pre", *args, st)
            else:
                _hip.call("mmdfn_lstm_gate_fwd_pre_img", *args, P(image), st)
            outs.append((gates, hout, cout))
        torch.cuda.synchronize()
        assert not torch.isnan(outs[0][0]).any()
        for a, b in zip(*outs):
            assert same_bits(a, b), ("gate_fwd", R, H, has_h)
        gates, c_new = outs[0][0], outs[0][2]
        # backward: dres with a row stride > H on the first pass, absent on the second; one image serves has_h = 0 and 1
        img = cut_image(4, Wih, Whh, H, 4, 1)
        for with_res in (True, False):
            dh_a, dh_b, dc_next = _t(rs, R, H), (_t(rs, R, H) if with_res else None), (_t(rs, R, H) if has_h else None)
            lddres = H + 20
            dres = _t(rs, R, lddres) if with_res else None
            outs = []
            for image in (None, img):
                dG, dq = _nan(R, 4 * H), _nan(R, H)
                dcp, dhp = (_nan(R, H), _nan(R, H)) if has_h else (None, None)
                args = (P(gates), P(c), P(c_new), P(dh_a), P(dh_b), P(dc_next), P(Wih), P(Whh), P(dres), P(dG), P(dcp), P(dq), P(dhp),
                        R, H, has_h, lddres if with_res else 0)
                if image is None:
                    _hip.call("mmdfn_lstm_gate_bwd", *args, st)
                else:
                    _hip.call("mmdfn_lstm_gate_bwd_img", *args, P(image), st)
                outs.append([t for t in (dG, dq, dcp, dhp) if t is not None])
            torch.cuda.synchronize()
            assert not torch.isnan(outs[0][1]).any()
            for a, b in zip(*outs):
                assert same_bits(a, b), ("gate_bwd", R, H, has_h, with_res)


@gpu
def test_image_entries_answer_minus_two_outside_their_shapes():
    from mm_dfn_amd import _hip
    P, st = _hip.ptr, _hip.stream()
    rs = np.random.RandomState(5)
    R, H, F = 16, 36, 256                                   # 16 K-chunks: more than the held fragments of the input forward cover
    x, W0 = _t(rs, R, F), _t(rs, H, F)
    img = cut_image(0, W0, None, H, F, 0)
    xd, h0, cur = _nan(R, F), _nan(R, H), _nan(R, H)
    rc = _hip.call("mmdfn_gcn_input_fwd_img", P(x), None, P(W0), None, None, P(xd), P(h0), P(cur), R, F, H, F, 1.0, P(img), st,
                   allow=(-2,))
    torch.cuda.synchronize()
    assert rc == -2 and torch.isnan(h0).all()               # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the node
def _stack_net(seed=0, nl=2):
    from mm_dfn_amd import GCNII_lyc
    torch.manual_seed(seed)
    return GCNII_lyc(nfeat=200, nlayers=nl, nhidden=100, nclass=6, dropout=0.0, lamda=0.5, alpha=0.1, variant=True,
                     return_feature=True, use_residue=True, reason_flag=True).to(DEV).train()


def _stack_pass(net, feats, lengths, backward=True):
    from mm_dfn_amd import ops
    M, N = feats.shape[0], feats.shape[1]
    x = feats.clone().requires_grad_(True)
    adj = ops.build_adjacency(x, lengths, 1.0)
    out = net(adj.stacked_feats.reshape(M * N, 200), lengths, None, adj)
    if backward:
        net.zero_grad(set_to_none=True)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).view_as(out)).sum().backward()
    return out.detach().clone(), (x.grad.clone() if backward else None)


@gpu
def test_whole_node_is_bit_equal_with_the_switch_on_and_off(monkeypatch):
    """_GcnStack forward + backward at R = 47, two layers: outputs, input gradient and every operand the node queues for the
    weight-gradient batch."""
    from mm_dfn_amd import gcn_stack, ops
    rs = np.random.RandomState(11)
    lengths = [30, 17]
    feats = _t(rs, 1, sum(lengths), 200)
    net = _stack_net()
    assert gcn_stack.STACK_IMAGES and gcn_stack.STACK_IMAGE_KERNELS <= frozenset(gcn_stack.STACK_IMAGE_ALL)
    default = frozenset(gcn_stack.STACK_IMAGE_KERNELS)
    res = []
    for on, kernels in ((True, gcn_stack.STACK_IMAGE_ALL), (True, default), (False, gcn_stack.STACK_IMAGE_ALL)):
        monkeypatch.setattr(gcn_stack, "STACK_IMAGES", on)
        monkeypatch.setattr(gcn_stack, "STACK_IMAGE_KERNELS", frozenset(kernels))
        queued = []
        monkeypatch.setattr(ops, "wgrad_batching", lambda: True)
        monkeypatch.setattr(ops, "queue_wgrad", lambda A, B, w, biases=(), rows=None: queued.append((A.clone(), B.clone(), rows)))
        used = []
        real = ops.stack_image
        monkeypatch.setattr(ops, "stack_image", lambda *a, **k: used.append(a[0]) or real(*a, **k))
        out, dx = _stack_pass(net, feats, lengths)
        monkeypatch.setattr(ops, "stack_image", real)
        res.append((out, dx, queued, used))
    (o1, g1, q1, u1), (o2, g2, q2, u2), (o0, g0, q0, u0) = res
    assert sorted(set(u1)) == sorted(gcn_stack.STACK_IMAGE_ALL) and u0 == []
    assert set(u2) == set(default)                                # the default: the kernels that measured faster
    for o, g, q in ((o1, g1, q1), (o2, g2, q2)):
        assert same_bits(o, o0) and same_bits(g, g0)
        assert len(q) == len(q0) and len(q) >= 8
        for (a1, b1, r1), (a0, b0, r0) in zip(q, q0):
            assert r1 == r0 and same_bits(a1, a0) and same_bits(b1, b0)


@gpu
def test_images_follow_an_in_place_weight_update_and_leave_with_the_parameter(monkeypatch):
    from mm_dfn_amd import gcn_stack, ops, ops_linear
    rs = np.random.RandomState(12)
    lengths = [30, 17]
    feats = _t(rs, 1, sum(lengths), 200)
    net = _stack_net(1)
    monkeypatch.setattr(gcn_stack, "STACK_IMAGES", True)
    monkeypatch.setattr(gcn_stack, "STACK_IMAGE_KERNELS", frozenset(gcn_stack.STACK_IMAGE_ALL))
    before = _stack_pass(net, feats, lengths)
    mine = lambda: [e for e in ops_linear._PLANES.values() if e.image is not None and e.w1() is not None
                    and any(e.w1() is p for p in net.parameters())]
    assert len(mine()) == 7                                  # input fwd / bwd, 2 layer bwd, gate fwd without / with h, gate bwd
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.sign(p))
    assert all(not ops_linear._plane_fresh(e, ops_linear._plane_params(e)) for e in mine())
    got = _stack_pass(net, feats, lengths)
    assert all(ops_linear._plane_fresh(e, ops_linear._plane_params(e)) for e in mine())
    monkeypatch.setattr(gcn_stack, "STACK_IMAGES", False)    # the staging path reads the parameters themselves
    want = _stack_pass(net, feats, lengths)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    assert not same_bits(got[0], before[0])
    # every image equals a fresh cut of its parameters
    for e in mine():
        k, H, F, has_h = e.image
        w1, w2 = ops_linear._plane_params(e)
        assert same_bits(e.buf.view(torch.float32), cut_image(k, w1, w2, H, F, has_h))
    ids = [id(e) for e in mine()]
    del net, e, w1, w2
    gc.collect()
    ops.refresh_planes()
    assert not any(id(e) in ids for e in ops_linear._PLANES.values())


@gpu
def test_images_are_recut_in_front_of_a_replay_that_follows_a_flat_adam_step():
    """replay, FlatAdam step, replay of a captured fwd + bwd step of the graph model against the eager sequence on the staging
    path (which reads the parameters themselves), and the images the captured step reads against fresh cuts."""
    from mm_dfn_amd import FocalLoss, gcn_stack, ops_linear, synthetic, train
    from mm_dfn_amd.graphs import CapturedStep
    from mm_dfn_amd.optim import FlatAdam
    cfg = dict(B=3, L=20, P=2, C=6, nlayers=2, D_t=100, D_a=100, D_v=512)
    lengths = [20, 13, 7]
    b = synthetic.make_batch(8, lengths=lengths, device=DEV, **cfg)
    loss_fn = FocalLoss(gamma=0.5)
    flat = train.flatten_labels(b["label"], lengths)

    def run(images, captured):
        gcn_stack.STACK_IMAGES = images
        m = synthetic.build_model(**cfg)
        m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), 7))
        m = m.to(DEV).train()

        def fwd_bwd():
            loss = loss_fn(m(b["textf"], b["qmask"], b["umask"], lengths, b["acouf"], b["visuf"])[0], flat)
            train.backward(loss)
            return loss
        m.zero_grad(set_to_none=True)
        fwd_bwd()
        opt = FlatAdam(m, lr=1e-2, weight_decay=1e-4)
        opt.bucket.flatten()
        opt._materialise()
        cap = CapturedStep(m, fwd_bwd, warmup=2, bucket=opt.bucket) if captured else None
        losses = []
        for _ in range(3):
            if captured:
                losses.append(float(cap.replay()))
                opt.step(grads_already_flat=True)
            else:
                m.zero_grad(set_to_none=True)
                losses.append(float(fwd_bwd()))
                opt.step()
        if captured and images:
            ents = list(cap._images)
            assert len(ents) >= 7
            assert all(not ops_linear._plane_fresh(e, ops_linear._plane_params(e)) for e in ents)     # the step just ran
            cap.replay()
            for e in ents:
                k, H, F, has_h = e.image
                w1, w2 = ops_linear._plane_params(e)
                assert same_bits(e.buf.view(torch.float32), cut_image(k, w1, w2, H, F, has_h))
        if cap is not None:
            cap.close()
        return losses

    prev = gcn_stack.STACK_IMAGES, gcn_stack.STACK_IMAGE_KERNELS
    gcn_stack.STACK_IMAGE_KERNELS = frozenset(gcn_stack.STACK_IMAGE_ALL)
    try:
        got, want = run(True, True), run(False, False)
    finally:
        gcn_stack.STACK_IMAGES, gcn_stack.STACK_IMAGE_KERNELS = prev
    assert want[0] != want[-1]
    for a, w in zip(got, want):
        assert abs(a - w) <= 2e-5 * abs(w), (got, want)      # (the bound of the captured-against-eager FlatAdam test)
