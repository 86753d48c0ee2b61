"""DialogueRNN encoder on the fused HIP recurrence (csrc/dialogue_rnn.hip, K17).

``DialogueRNN`` keeps the reference's constructor and state_dict (model.py:168-278): ``dialogue_cell.g_cell / p_cell / e_cell``
are nn.GRUCell modules and ``dialogue_cell.attention`` a SimpleAttention / MatchingAttention('general') that only HOLD the
parameters; their own forward is never called.  ``encode(rnns, U, qmask, lengths, ...)`` evaluates one encoder (a DialogueRNN
on its own) or the two directions of ``DialogRNNModel`` together: per encoder ONE projection launch (``ops.linear``: the
U halves of the g / p cells' input contractions with their b_ih, and W_att U for 'general'), then ONE recurrence launch for
every chain of both directions.  Weight gradients of the six state-side matrices and their biases are contractions of the
saved planes with the gate gradients (``ops.gemm_tn_grouped``, one launch pair per direction; the h_{s-1} operands by a row
shift of -B); the U halves and W_att get theirs from the projection's backward, and autograd's ``cat`` / slice backward assemble
the two halves of a ``weight_ih`` gradient.
"""
import torch
import torch.nn as nn

from . import _hip, ops
from . import ops_linear

D_G = D_P = 150
D_E = 100
P_MAX = 16
T_MAX = 1008
PW = 152            # row width of the saved planes
GW = 452            # row width of the gate-gradient planes
N_PLANES = 17
(P_RG, P_ZG, P_NG, P_HNG, P_G, P_RP, P_ZP, P_NP, P_HNP, P_Q0, P_Q1, P_C, P_RE, P_ZE, P_NE, P_HNE, P_E) = range(N_PLANES)
ATT_KINDS = {"simple": 0, "general": 1}


def chains_per_group():
    """Chains one workgroup of the recurrence kernels serves (their launch edge in the batch dimension)."""
    return int(_hip.query("mmdfn_drnn_chains_per_group"))


class SimpleAttention(nn.Module):
    """Parameter holder of the reference's SimpleAttention (model.py:14-29): ``scalar``, Linear(D_g, 1, bias=False)."""

    def __init__(self, input_dim):
        super().__init__()
        self.input_dim = input_dim
        self.scalar = nn.Linear(input_dim, 1, bias=False)


class GeneralAttention(nn.Module):
    """Parameter holder of the reference's MatchingAttention(D_g, D_m, att_type='general') (model.py:32-85): ``transform``,
    Linear(D_m, D_g, bias=False)."""

    def __init__(self, mem_dim, cand_dim):
        super().__init__()
        self.mem_dim, self.cand_dim, self.att_type = mem_dim, cand_dim, "general"
        self.transform = nn.Linear(cand_dim, mem_dim, bias=False)


class DialogueRNNCell(nn.Module):
    def __init__(self, D_m, D_g, D_p, D_e, listener_state=False, context_attention="simple", D_a=100, dropout=0.5):
        super().__init__()
        self.D_m, self.D_g, self.D_p, self.D_e = D_m, D_g, D_p, D_e
        self.listener_state = listener_state
        self.g_cell = nn.GRUCell(D_m + D_p, D_g)
        self.p_cell = nn.GRUCell(D_m + D_g, D_p)
        self.e_cell = nn.GRUCell(D_p, D_e)
        self.dropout = nn.Dropout(dropout)
        self.attention = SimpleAttention(D_g) if context_attention == "simple" else GeneralAttention(D_g, D_m)


def check_served(name, D_m, D_g, D_p, D_e, listener_state, context_attention):
    if listener_state:
        raise NotImplementedError("%s: listener_state=True (the listener cell) is not built" % name)
    if context_attention not in ATT_KINDS:
        raise NotImplementedError("%s: context_attention must be 'simple' or 'general', got %r" % (name, context_attention))
    if (D_g, D_p, D_e) != (D_G, D_P, D_E):
        raise NotImplementedError("%s: the fused DialogueRNN kernels are built for D_g = D_p = %d, D_e = %d, got D_g = %d, "
                                  "D_p = %d, D_e = %d" % (name, D_G, D_E, D_g, D_p, D_e))
    if D_m % 4 or not 4 <= D_m <= 768:
        raise NotImplementedError("%s: the input projection serves D_m %% 4 == 0, 4 <= D_m <= 768, got %d" % (name, D_m))


class DialogueRNN(nn.Module):
    """One direction of the reference's DialogueRNN: ``forward(U (T, B, D_m), qmask (T, B, P)) -> (e (T, B, D_e), [alpha_t (B, t)]
    for t = 1 .. T-1)``.  Every dialogue runs all T steps, as in the reference."""

    def __init__(self, D_m, D_g, D_p, D_e, listener_state=False, context_attention="simple", D_a=100, dropout=0.5):
        super().__init__()
        check_served(type(self).__name__, D_m, D_g, D_p, D_e, listener_state, context_attention)
        self.D_m, self.D_g, self.D_p, self.D_e = D_m, D_g, D_p, D_e
        self.context_attention = context_attention
        self.dropout = nn.Dropout(dropout)
        self.dialogue_cell = DialogueRNNCell(D_m, D_g, D_p, D_e, listener_state, context_attention, D_a, dropout)

    def forward(self, U, qmask):
        _hip.require_cuda(U, qmask)
        if U.is_cuda:
            ops.refresh_planes()
        T, B = U.shape[0], U.shape[1]
        lengths = torch.full((B,), T, dtype=torch.int32, device=U.device)
        with ops.flag_pool((type(self).__name__, T, B)):
            e, alpha = encode([self], U, qmask, lengths, self.dropout.p, self.training)
        return e[0], alpha_list(alpha[0])


def alpha_list(alpha):
    """(T, B, T) lower-triangular rows -> the reference's list: entry t-1 is (B, t)."""
    return [alpha[t, :, :t] for t in range(1, alpha.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------------
# forward weight images: the six state-side matrices transposed (k-major, the order the lanes stream them) and the hidden-side
# biases, cut once per weight version.  Stamped like the plane and stack images (ops_linear): tensor versions and storage, and the
# registry's epoch, which FlatAdam bumps (invalidate_planes) when its kernel writes the parameters behind autograd's back.
# ---------------------------------------------------------------------------------------------------------------------------
_IMAGES = {}      # id(cell) -> [weakref(cell), stamp, image]


def _image_params(cell):
    att = cell.attention
    return [cell.g_cell.weight_ih, cell.g_cell.weight_hh, cell.p_cell.weight_ih, cell.p_cell.weight_hh, cell.e_cell.weight_ih,
            cell.e_cell.weight_hh, cell.g_cell.bias_hh, cell.p_cell.bias_hh, cell.e_cell.bias_ih, cell.e_cell.bias_hh,
            att.scalar.weight if isinstance(att, SimpleAttention) else att.transform.weight]


def _stamp(prm):
    return (ops_linear._PLANE_EPOCH[0],) + tuple((p._version, p.data_ptr()) for p in prm)


def weight_image(cell):
    """The forward image of ``cell`` (mmdfn_drnn_image_floats() floats, layout in include/mmdfn_hip.h), re-cut when stale."""
    import weakref
    prm = _image_params(cell)
    ent = _IMAGES.get(id(cell))
    stamp = _stamp(prm)
    if ent is not None and ent[0]() is cell and ent[1] == stamp and ent[2].device == prm[0].device:
        return ent[2]
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("the DialogueRNN weight image is stale inside a stream capture: it is never cut in a captured step")
    for k in [k for k, v in _IMAGES.items() if v[0]() is None]:
        del _IMAGES[k]
    D_m = cell.D_m
    with torch.no_grad():
        img = torch.zeros(int(_hip.query("mmdfn_drnn_image_floats")), dtype=torch.float32, device=prm[0].device)
        mats = [prm[0][:, D_m:], prm[1], prm[2][:, D_m:], prm[3], prm[4], prm[5]]
        o = 0
        for w in mats:
            n = w.numel()
            img[o:o + n].view(w.shape[1], w.shape[0]).copy_(w.t())
            o += n
        for b in prm[6:10]:
            img[o:o + b.numel()].copy_(b)
            o += b.numel()
        if isinstance(cell.attention, SimpleAttention):
            img[o:o + D_G].copy_(prm[10].view(-1))
    _IMAGES[id(cell)] = [weakref.ref(cell), stamp, img]
    return img


def speakers(qmask, lengths, check=True):
    """(speaker (T, B) int32 = argmax of qmask, upd (T, B) float = qmask at the speaker).  ``check``: rows of qmask must be one-hot
    or all zero and at least one dialogue must have length T (one device reduction, one host read; skipped under capture)."""
    T = qmask.shape[0]
    spk = qmask.argmax(2)
    upd = qmask.gather(2, spk.unsqueeze(2)).squeeze(2).to(torch.float32).contiguous()
    if check and not (qmask.is_cuda and torch.cuda.is_current_stream_capturing()):
        bad_rows = (((qmask != 0) & (qmask != 1)).any() | (qmask.sum(2) > 1).any()).to(torch.int32)
        bad_len = ((lengths.max() != T) | (lengths.min() < 0)).to(torch.int32)
        code = int((bad_rows + 2 * bad_len).item())
        if code & 1:
            raise ValueError("DialogueRNN: every row of qmask must be one-hot or all zero")
        if code & 2:
            raise ValueError("DialogueRNN: umask must give at least one dialogue the full length %d (and no negative length)" % T)
    return spk.to(torch.int32).contiguous(), upd


class _DrnnRecurrence(torch.autograd.Function):
    """(meta, pu_0 [, pu_1], then per direction: W_ih_g[:, D_m:], W_hh_g, W_ih_p[:, D_m:], W_hh_p, W_ih_e, W_hh_e, b_hh_g, b_hh_p,
    b_ih_e, b_hh_e, scalar.weight or None) -> (e (ndir, T, B, D_e) in time order, alpha (ndir, T, B, T) in chain-step order)."""

    @staticmethod
    def forward(ctx, meta, *args):
        nd = meta["ndir"]
        pu = [a.contiguous() for a in args[:nd]]
        prm = [args[nd + 11 * d: nd + 11 * (d + 1)] for d in range(nd)]
        _hip.require_cuda(*pu)
        _hip.require_f32(*pu)
        T, B, npu = pu[0].shape
        dev = pu[0].device
        att, P = meta["att"], meta["P"]
        e = torch.zeros(2, T, B, D_E, dtype=torch.float32, device=dev)
        alpha = torch.zeros(2, T, B, T, dtype=torch.float32, device=dev)
        state = torch.zeros(2, N_PLANES, T, B, PW, dtype=torch.float32, device=dev)
        keeps = [None if meta[k] is None else _hip.ptr_array(meta[k]) for k in ("keep_g", "keep_q", "keep_e")]
        _hip.call("mmdfn_drnn_seq_fwd", _hip.ptr_array(pu), _hip.ptr_array(meta["img"]), _hip.ptr(meta["speaker"]),
                  _hip.ptr(meta["upd"]), _hip.ptr(meta["lengths"]), keeps[0], keeps[1], keeps[2], float(meta["scale"]),
                  _hip.ptr(e), _hip.ptr(alpha), _hip.ptr(state), B, T, P, D_G, D_P, D_E, npu, att, nd, _hip.stream())
        ctx.meta = meta
        # the backward kernel reads the matrices in place (no image), the forward read the image cut from them: an in-place
        # change in between would mix weights, and these views are not saved tensors, so their versions are checked by hand
        ctx.prm = prm
        ctx.versions = [[None if w is None else w._version for w in d] for d in prm]
        ctx.save_for_backward(alpha, state, *pu)
        e_out, alpha_out = e[:nd], alpha[:nd]
        ctx.mark_non_differentiable(alpha_out)
        return e_out, alpha_out

    @staticmethod
    def backward(ctx, de, _dalpha):
        meta, prm = ctx.meta, ctx.prm
        if ctx.versions != [[None if w is None else w._version for w in d] for d in prm]:
            raise RuntimeError("fused DialogueRNN: a cell parameter was modified in place between forward and backward")
        alpha, state = ctx.saved_tensors[:2]
        pu = list(ctx.saved_tensors[2:])
        nd = meta["ndir"]
        T, B, npu = pu[0].shape
        dev = pu[0].device
        att, P = meta["att"], meta["P"]
        de_full = torch.zeros(2, T, B, D_E, dtype=torch.float32, device=dev)
        de_full[:nd].copy_(de)
        dgate = torch.zeros(2, 6, T, B, GW, dtype=torch.float32, device=dev)
        dpu = [torch.zeros(T, B, npu, dtype=torch.float32, device=dev) for _ in range(nd)]
        dghist = torch.zeros(2, T, B, PW, dtype=torch.float32, device=dev)
        dw_part = torch.zeros(2, B, PW, dtype=torch.float32, device=dev)
        mats = [w for d in range(nd) for w in prm[d][:6]]
        for w in mats:
            if w.stride(1) != 1:
                raise ValueError("fused DialogueRNN: the cell matrices must have unit inner stride")
        ld = [w.stride(0) for w in prm[0][:6]]
        for d in range(nd):
            if [w.stride(0) for w in prm[d][:6]] != ld:
                raise ValueError("fused DialogueRNN: the two directions' matrices must share their row strides")
        keeps = [None if meta[k] is None else _hip.ptr_array(meta[k]) for k in ("keep_g", "keep_q", "keep_e")]
        _hip.call("mmdfn_drnn_seq_bwd", _hip.ptr(de_full), _hip.ptr_array(pu), _hip.ptr_array(meta["img"]), _hip.ptr_array(mats),
                  _hip.int_array(ld), _hip.ptr(meta["speaker"]), _hip.ptr(meta["upd"]), _hip.ptr(meta["lengths"]), keeps[0],
                  keeps[1], keeps[2], float(meta["scale"]), _hip.ptr(alpha), _hip.ptr(state), _hip.ptr(dgate),
                  _hip.ptr_array(dpu), _hip.ptr(dghist), _hip.ptr(dw_part), B, T, P, D_G, D_P, D_E, npu, att, nd, _hip.stream())
        # dW = sum_s dgate_s (x) operand_s over the saved planes (chain-step order in both directions: h_{s-1} is a shift of -B rows)
        grads = []
        R = T * B
        for d in range(nd):
            dg = dgate[d].view(6, R, GW)
            pl = state[d].view(N_PLANES, R, PW)
            C = [torch.empty(GW, PW, dtype=torch.float32, device=dev) for _ in range(4)]
            C += [torch.empty(3 * D_E, PW, dtype=torch.float32, device=dev), torch.empty(3 * D_E, D_E, dtype=torch.float32, device=dev)]
            cs = [torch.empty(GW, dtype=torch.float32, device=dev) for _ in range(2)]
            cs += [torch.empty(3 * D_E, dtype=torch.float32, device=dev) for _ in range(2)]
            problems = [dict(A=dg[0], B=pl[P_Q0], C=C[0]),
                        dict(A=dg[1], B=pl[P_G], C=C[1], colsum=cs[0], shift=-B),
                        dict(A=dg[2], B=pl[P_C], C=C[2]),
                        dict(A=dg[3], B=pl[P_Q0], C=C[3], colsum=cs[1]),
                        dict(A=dg[4][:, :3 * D_E], B=pl[P_Q1], C=C[4], colsum=cs[2]),
                        dict(A=dg[5][:, :3 * D_E], B=pl[P_E][:, :D_E], C=C[5], colsum=cs[3], shift=-B)]
            ops.gemm_tn_grouped(problems)
            g = [C[i][:3 * D_G, :D_G] for i in range(4)] + [C[4][:, :D_P], C[5]]
            g += [cs[0][:3 * D_G], cs[1][:3 * D_G], cs[2], cs[3]]
            g.append(None if att else dw_part[d].sum(0)[:D_G].view(1, D_G))
            grads += g
        return (None, *dpu, *grads)


def encode(rnns, U, qmask, lengths, p=0.0, training=False, check=True):
    """Run the encoders ``rnns`` ([forward] or [forward, reverse]) on U (T, B, D_m), qmask (T, B, P), lengths (B) int32:
    -> e (ndir, T, B, D_e) in time order (reverse rows beyond a length are zero), alpha (ndir, T, B, T) in chain-step order."""
    _hip.require_cuda(U, qmask, lengths)
    _hip.require_f32(U)
    nd = len(rnns)
    T, B, P = qmask.shape
    kind = rnns[0].context_attention
    if any(r.context_attention != kind for r in rnns):
        raise NotImplementedError("DialogueRNN: context_attention must be the same in both directions")
    if not 1 <= P <= P_MAX:
        raise NotImplementedError("DialogueRNN: the kernels serve 1 <= P (parties, qmask.shape[2]) <= %d, got %d" % (P_MAX, P))
    if not 1 <= T <= T_MAX:
        raise NotImplementedError("DialogueRNN: the kernels serve 1 <= T (seq_len) <= %d, got %d" % (T_MAX, T))
    att = ATT_KINDS[kind]
    speaker, upd = speakers(qmask, lengths, check)
    D_m = rnns[0].D_m
    pus, prm, imgs = [], [], []
    for r in rnns:
        c = r.dialogue_cell
        ws = [c.g_cell.weight_ih[:, :D_m], c.p_cell.weight_ih[:, :D_m]]
        bs = [c.g_cell.bias_ih, c.p_cell.bias_ih]
        if att:
            ws.append(c.attention.transform.weight)
            bs.append(torch.zeros(D_G, dtype=torch.float32, device=U.device))
        pus.append(ops.linear(U, torch.cat(ws), torch.cat(bs)))
        prm += [c.g_cell.weight_ih[:, D_m:], c.g_cell.weight_hh, c.p_cell.weight_ih[:, D_m:], c.p_cell.weight_hh,
                c.e_cell.weight_ih, c.e_cell.weight_hh, c.g_cell.bias_hh, c.p_cell.bias_hh, c.e_cell.bias_ih, c.e_cell.bias_hh,
                None if att else c.attention.scalar.weight]
        imgs.append(weight_image(c))
    meta = dict(ndir=nd, att=att, P=P, speaker=speaker, upd=upd, lengths=lengths.to(torch.int32).contiguous(), img=imgs,
                keep_g=None, keep_q=None, keep_e=None, scale=1.0)
    if training and p > 0:
        for site, width in (("g", D_G), ("q", D_P), ("e", D_E)):
            meta["keep_" + site] = [ops.keep_flags(T * B * width, p, U.device, site="drnn_" + site) for _ in range(nd)]
        meta["scale"] = ops.keep_scale(p)
    return _DrnnRecurrence.apply(meta, *pus, *prm)
