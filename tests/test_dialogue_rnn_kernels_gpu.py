"""GPU: the K17 entry points (csrc/dialogue_rnn.hip: mmdfn_drnn_seq_fwd / mmdfn_drnn_seq_bwd), called directly, against the
float64 restatement tests/dialogue_rnn_ref.py, step by step.

FORWARD, TEACHER-FORCED.  Every saved plane of a step is a function of the projected rows and of planes the kernel wrote
earlier (g_{s-1}, the history g_{<s}, q_{s-1}[speaker], e_{s-1}).  The float64 step is evaluated ON THE KERNEL'S OWN earlier
planes, so errors do not compound and every element has a local bound.  u = 2^-24; |.| elementwise; a contraction of K terms
accumulated in any order, with or without FMA, errs by at most (K + 1) u sum |w| |x|.
  pre-activations   a_i = in + W_i x,  a_h = W_h h + b:      E_a = (K + 2) u (|in or b| + |W| |x|)      K = 150 (100: W_hh_e)
  r, z = sig(a_i + a_h)    E_s = (E_ai + E_ah + u |a_i + a_h|) / 4 + 4 u     (|sig'| <= 1/4; libm expf within 1 ulp moves sig by
                            <= u / 2, rounding 1 + e and the correctly rounded quotient by <= u each: 2.5 u <= 4 u)
  hn = a_h (n block)       E_hn = E_ah
  n = tanh(a_i + r hn)     E_n = E_ai + |hn| E_r + |r| E_hn + E_r E_hn + u (|a_i| + 2 |r hn| + |a_i + r hn|) + 6 u
                            (|tanh'| <= 1; libm tanhf within 2 ulp of a result in [-1, 1]: 4 u <= 6 u)
  h' = (1 - z) n + z h     E_h' = |n - h| E_z + (1 - z) E_n + E_z E_n + 4 u (|n| + |h|);  with keep flags (x keep x scale, two
                            roundings): scale E_h' + 2 u |h'|
  q_s[speaker] = m qs + (1 - m) q_{s-1}[speaker], m in {0, 1}: a selection, E = m E_qs (+ 0: products by 0 / 1 and a sum with 0 are exact)
  scores  sc_j = <x, g_j>  E_sc = 151 u sum |x| |g_j|
  alpha   = exp(sc_j - max) / sum:   relative error of a term  rho_j = 2 max_j E_sc + u (|sc_j - max| + 2)  (argument error, its
            rounding, expf's ulp);  of the sum  max_j rho_j + s u;  E_alpha_j = alpha_j (rho_j + max rho + (s + 1) u)
  c       = sum_j alpha_j g_j        E_c = sum_j E_alpha_j |g_j| + (s + 1) u sum_j alpha_j |g_j|
Every bound also carries 2^-126.  q_{s-1}[speaker] (plane q0) is a copy: it must equal, bit for bit, the q_s'[speaker] the
kernel saved at the speaker's previous step s' (zero if there is none); the e output is the e plane scattered to time order.

BACKWARD, LOCAL (T = 1, 2: test_backward_local_bounds).  The last step processed has de = de_out exactly and dq = dg = 0.  A
GRU cell's gate gradients from the gradient dh of its output (bound E_dh) and the SAVED r, z, n, hn, h_prev (exact inputs):
    B = 1 - n^2:  E_B = u (n^2 + |B|)  (the absolute form, as for tc in the LSTM file)
    dnp = dh (1-z) B          E_dnp = E_dh |(1-z) B| + |dh (1-z)| E_B + 6 u |dnp|
    dz  = dh (h_prev - n) z (1-z)      E_dz = E_dh |(h_prev - n) z (1-z)| + 6 u |dz|
    dr  = dnp hn r (1-r)      E_dr = E_dnp |hn r (1-r)| + 6 u |dr|
    dgi = [dr, dz, dnp],  dgh = [dr, dz, dnp r]:  E = E_dnp r + 2 u |dnp r|;   dh_prev (direct) = dh z:  E = E_dh z + u |dh z|
A keep flag multiplies dh by keep x scale (one rounding): E_dh scale + u |dh|.  What one cell hands to the next is a contraction
of the kernel's OWN gate gradients (read back, so their error does not compound) with a stored matrix, J = 300 or 450 terms in
three partial sums: E = (J + 4) u |dgate| |W|.  So at the last step  dq_s[speaker] = dgi_e W_ih_e  and  dqs = m dq (x keep):
dgi_e / dgh_e and dgi_p / dgh_p have elementwise bounds; nothing depends on g of the last step (its gate gradients must be
exactly zero).  At T = 2 the step processed second sees
    de = de_out + (d_1 z_1 + dgh_e,1 W_hh_e)            d_1 (not an output): the float64 value with its own bound
    dq[speaker] = dgi_e W_ih_e + [same speaker] ((1 - m_1) dq_1 + dqs_1 z_1 + dgh_p,1 W_hh_p)
    dg = dG_hist[0] = dc_1 = dgi_p,1 W_ih_p[:, D_m:]   (alpha_10 = 1, dscore = 0: the kernel's dG_hist row is read back, and is
                                                        itself checked against the contraction under (454) u |dgi_p| |W|)
with one more u |sum| per addition.  dx_att and dw are exactly zero at T <= 2, and the projected rows' gradient blocks are bit
copies of dgi_g / dgi_p in time order.  Every bound also carries 2^-126.

BACKWARD, AT LENGTH.  dg, dq, de of an inner step are not outputs, so no local bound exists.  As in
tests/test_lstm_recurrence_kernels_gpu.py the kernel is calibrated against honest fp32: the kernels (forward + backward) and a
float32 CPU run of the restatement (forward + autograd) are both compared with the float64 run, max-norm per tensor, and the
kernel's error must be <= 4 e_ref + 8 u max |want| (the projected rows' gradient per column block: g, p, x_att).  The gate gradients come out of the restatement as the gradients of zero
probes added to the six gate pre-activations.

Properties: a chain's bits do not depend on its workgroup slot (batch permuted), two runs give the same bits, reverse rows at or
beyond a length are exactly zero in every output, alpha rows sum to 1 within 4 ulp and are zero on and above the diagonal.
Measured ratios: profiles/dialogue_rnn_parity.md (the tests print them: pytest -s).
"""
import numpy as np
import pytest
import torch

import dialogue_rnn_ref as DR
from mm_dfn_amd import _hip, dialogue_rnn as K

gpu = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
TINY = 2.0 ** -126
DG, DE, PW, GW = 150, 100, 152, 452
CELLS = ("g_cell", "p_cell", "e_cell")


def _say(tag, **kv):
    print("DRNN-PARITY %s %s" % (tag, " ".join("%s=%.3g" % (k, v) for k, v in kv.items())), flush=True)


def _ratio(got, want, bound):
    err = (got.double() - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isfinite(got.double()), q, torch.full_like(q, float("inf")))
    return float(q.max()) if q.numel() else 0.0


def make_params(D_m, kind, seed):
    """Two directions' parameters, fp32 CPU, under the model's state_dict names; nn.GRUCell's initialisation range."""
    rs = np.random.RandomState(seed)
    P = {}
    for pre in ("dialog_rnn_f.", "dialog_rnn_r."):
        c = pre + "dialogue_cell."
        for cell, (nin, H) in zip(CELLS, ((D_m + DG, DG), (D_m + DG, DG), (DG, DE))):
            k = 1.0 / np.sqrt(H)
            for n, shape in (("weight_ih", (3 * H, nin)), ("weight_hh", (3 * H, H)), ("bias_ih", (3 * H,)), ("bias_hh", (3 * H,))):
                P[c + cell + "." + n] = torch.from_numpy(rs.uniform(-k, k, shape).astype(np.float32))
        if kind == "general":
            P[c + "attention.transform.weight"] = torch.from_numpy(rs.uniform(-0.1, 0.1, (DG, D_m)).astype(np.float32))
        else:
            P[c + "attention.scalar.weight"] = torch.from_numpy(rs.uniform(-0.5, 0.5, (1, DG)).astype(np.float32))
    return P


def image_of(P, pre, D_m, kind):
    """The forward weight image by the header's layout."""
    c = pre + "dialogue_cell."
    parts = [P[c + "g_cell.weight_ih"][:, D_m:].t(), P[c + "g_cell.weight_hh"].t(), P[c + "p_cell.weight_ih"][:, D_m:].t(),
             P[c + "p_cell.weight_hh"].t(), P[c + "e_cell.weight_ih"].t(), P[c + "e_cell.weight_hh"].t(), P[c + "g_cell.bias_hh"],
             P[c + "p_cell.bias_hh"], P[c + "e_cell.bias_ih"], P[c + "e_cell.bias_hh"],
             P[c + "attention.scalar.weight"][0] if kind == "simple" else torch.zeros(DG), torch.zeros(2)]
    img = torch.cat([p.contiguous().reshape(-1) for p in parts])
    assert img.numel() == _hip.query("mmdfn_drnn_image_floats")
    return img


def projected_rows(P, pre, U, kind):
    """pu (T, B, 900 | 1050) in fp32 (the rounded values are what kernel and restatement both read)."""
    D_m = U.shape[2]
    c = pre + "dialogue_cell."
    cols = [U.double() @ P[c + "g_cell.weight_ih"][:, :D_m].double().t() + P[c + "g_cell.bias_ih"].double(),
            U.double() @ P[c + "p_cell.weight_ih"][:, :D_m].double().t() + P[c + "p_cell.bias_ih"].double()]
    if kind == "general":
        cols.append(U.double() @ P[c + "attention.transform.weight"].double().t())
    return torch.cat(cols, 2).float().contiguous()


class Problem:
    def __init__(self, kind, B, T, Pn, flags, seed, lengths=None, zero_rows=()):
        self.kind, self.B, self.T, self.Pn, self.D_m = kind, B, T, Pn, 8
        self.lengths = list(lengths) if lengths is not None else [T] * B
        self.P = make_params(self.D_m, kind, seed)
        self.U, self.qmask, _, _, _ = DR.make_inputs(self.D_m, T, self.lengths, Pn, 3, seed + 1, constant=1, zero_rows=zero_rows)
        self.pu = [projected_rows(self.P, pre, self.U, kind) for pre in ("dialog_rnn_f.", "dialog_rnn_r.")]
        self.img = [image_of(self.P, pre, self.D_m, kind) for pre in ("dialog_rnn_f.", "dialog_rnn_r.")]
        self.scale = 1.25 if flags else 1.0
        rs = np.random.RandomState(seed + 2)
        self.keep = None
        if flags:
            self.keep = [{k: torch.from_numpy((rs.uniform(size=(T, B, w)) < 0.8).astype(np.float32)) for k, w in
                          (("g", DG), ("q", DG), ("e", DE))} for _ in range(2)]
        self.de = torch.from_numpy(rs.standard_normal((2, T, B, DE)).astype(np.float32))
        for b, n in enumerate(self.lengths):
            self.de[1, n:, b] = 0.0
        self.spk, self.upd = K.speakers(self.qmask, torch.tensor(self.lengths, dtype=torch.int32))

    def permuted(self, perm):
        """The same chains in another batch order."""
        import copy
        o = copy.copy(self)
        o.lengths = [self.lengths[i] for i in perm]
        o.U, o.qmask, o.spk, o.upd = self.U[:, perm], self.qmask[:, perm], self.spk[:, perm].contiguous(), self.upd[:, perm].contiguous()
        o.pu = [p[:, perm].contiguous() for p in self.pu]
        o.de = self.de[:, :, perm].contiguous()
        if self.keep is not None:
            o.keep = [{k: v[:, perm].contiguous() for k, v in d.items()} for d in self.keep]
        return o


def run_kernels(pb, backward=True):
    T, B, npu, att = pb.T, pb.B, pb.pu[0].shape[2], K.ATT_KINDS[pb.kind]
    dev = lambda t: t.to(DEV).contiguous()
    pu, img = [dev(p) for p in pb.pu], [dev(i) for i in pb.img]
    spk, upd, lens = dev(pb.spk), dev(pb.upd), dev(torch.tensor(pb.lengths, dtype=torch.int32))
    keeps = [None] * 3
    held = []
    if pb.keep is not None:
        for i, k in enumerate(("g", "q", "e")):
            ts = [dev(pb.keep[d][k]) for d in range(2)]
            held.append(ts)
            keeps[i] = _hip.ptr_array(ts)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    out = dict(e=z(2, T, B, DE), alpha=z(2, T, B, T), state=z(2, 17, T, B, PW))
    dims = (B, T, pb.Pn, DG, DG, DE, npu, att, 2)
    _hip.call("mmdfn_drnn_seq_fwd", _hip.ptr_array(pu), _hip.ptr_array(img), _hip.ptr(spk), _hip.ptr(upd), _hip.ptr(lens), *keeps,
              pb.scale, _hip.ptr(out["e"]), _hip.ptr(out["alpha"]), _hip.ptr(out["state"]), *dims, _hip.stream())
    if backward:
        names = [("g_cell.weight_ih", True), ("g_cell.weight_hh", False), ("p_cell.weight_ih", True), ("p_cell.weight_hh", False),
                 ("e_cell.weight_ih", False), ("e_cell.weight_hh", False)]
        ws = []
        for pre in ("dialog_rnn_f.", "dialog_rnn_r."):
            for n, sliced in names:
                w = dev(pb.P[pre + "dialogue_cell." + n])
                held.append(w)
                ws.append(w[:, pb.D_m:] if sliced else w)
        ld = [w.stride(0) for w in ws[:6]]
        out.update(dgate=z(2, 6, T, B, GW), dpu=[z(T, B, npu), z(T, B, npu)], dghist=z(2, T, B, PW), dw=z(2, B, PW))
        de = dev(pb.de)
        _hip.call("mmdfn_drnn_seq_bwd", _hip.ptr(de), _hip.ptr_array(pu), _hip.ptr_array(img), _hip.ptr_array(ws),
                  _hip.int_array(ld), _hip.ptr(spk), _hip.ptr(upd), _hip.ptr(lens), *keeps, pb.scale, _hip.ptr(out["alpha"]),
                  _hip.ptr(out["state"]), _hip.ptr(out["dgate"]), _hip.ptr_array(out["dpu"]), _hip.ptr(out["dghist"]),
                  _hip.ptr(out["dw"]), *dims, _hip.stream())
    torch.cuda.synchronize()
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# forward: teacher-forced float64 steps with local bounds
# ---------------------------------------------------------------------------------------------------------------------
def _contract(w, x, extra, K_):
    """(a, E_a) of a = extra + x W^T in float64 for x (..., K), w (J, K)."""
    a = x @ w.t() + extra
    mag = x.abs() @ w.abs().t() + extra.abs()
    return a, (K_ + 2) * U32 * mag + TINY


def _cell(ai, Eai, ah, Eah, h, keep, scale):
    """Float64 GRU cell from its pre-activations and their bounds -> {r z n hn h'} values and bounds (module docstring)."""
    H = h.shape[-1]
    val, E = {}, {}
    for k, sl in (("r", slice(0, H)), ("z", slice(H, 2 * H))):
        val[k] = torch.sigmoid(ai[..., sl] + ah[..., sl])
        E[k] = (Eai[..., sl] + Eah[..., sl] + U32 * (ai[..., sl] + ah[..., sl]).abs()) / 4 + 4 * U32
    n_sl = slice(2 * H, 3 * H)
    val["hn"], E["hn"] = ah[..., n_sl], Eah[..., n_sl]
    r, hn, ain = val["r"], val["hn"], ai[..., n_sl]
    val["n"] = torch.tanh(ain + r * hn)
    E["n"] = (Eai[..., n_sl] + hn.abs() * E["r"] + r.abs() * E["hn"] + E["r"] * E["hn"] +
              U32 * (ain.abs() + 2 * (r * hn).abs() + (ain + r * hn).abs()) + 6 * U32)
    z, n = val["z"], val["n"]
    hp = (1 - z) * n + z * h
    Eh = (n - h).abs() * E["z"] + (1 - z) * E["n"] + E["z"] * E["n"] + 4 * U32 * (n.abs() + h.abs()) + TINY
    if keep is not None:
        hp = hp * keep.double() * scale
        Eh = scale * Eh * keep.double() + 2 * U32 * hp.abs() + TINY
    val["h"], E["h"] = hp, Eh
    return val, E


def forward_ratios(pb, out):
    """Worst |kernel - float64 step| / bound per plane, over both directions; plus the exact checks of the docstring."""
    T, B = pb.T, pb.B
    worst = {}
    for d, pre in enumerate(("dialog_rnn_f.", "dialog_rnn_r.")):
        c = pre + "dialogue_cell."
        W = {k: v.double() for k, v in pb.P.items() if k.startswith(c)}
        st = {n: out["state"][d, i].double() for i, n in enumerate(DR.PLANES)}
        for n in DR.PLANES:       # padding columns stay zero
            w = DE if n in ("re", "ze", "ne", "hne", "e") else DG
            assert float(st[n][..., w:].abs().max()) == 0.0, n
            st[n] = st[n][..., :w]
        lens = pb.lengths if d else [T] * B
        valid = torch.zeros(T, B, dtype=torch.bool)
        tmap = torch.zeros(T, B, dtype=torch.long)
        for b, n in enumerate(lens):
            valid[:n, b] = True
            tmap[:n, b] = torch.arange(n - 1, -1, -1) if d else torch.arange(n)
        bidx = torch.arange(B).expand(T, B)
        pu = pb.pu[d].double()[tmap, bidx]                       # chain-step order
        keep = None if pb.keep is None else pb.keep[d]
        prev = lambda x: torch.cat([torch.zeros_like(x[:1]), x[:-1]])
        # q0: a bit-exact copy of the speaker's previous q1
        spk = pb.spk.long()[tmap, bidx]
        m = pb.upd.double()[tmap, bidx].unsqueeze(2)
        for b in range(B):
            last = {}
            for s in range(lens[b]):
                want = last.get(int(spk[s, b]), torch.zeros(DG, dtype=torch.float64))
                assert torch.equal(st["q0"][s, b], want), ("q0", d, s, b)
                last[int(spk[s, b])] = st["q1"][s, b]
        D_m = pb.D_m
        # g cell
        ai, Eai = _contract(W[c + "g_cell.weight_ih"][:, D_m:], st["q0"], pu[..., :3 * DG], DG)
        ah, Eah = _contract(W[c + "g_cell.weight_hh"], prev(st["g"]), W[c + "g_cell.bias_hh"].expand(T, B, -1), DG)
        gv, gE = _cell(ai, Eai, ah, Eah, prev(st["g"]), None if keep is None else keep["g"], pb.scale)
        # attention on the kernel's history
        cv = torch.zeros(T, B, DG, dtype=torch.float64)
        cE = torch.full((T, B, DG), TINY, dtype=torch.float64)
        al_w = torch.zeros(T, B, T, dtype=torch.float64)
        al_E = torch.full((T, B, T), TINY, dtype=torch.float64)
        for b in range(B):
            for s in range(1, lens[b]):
                x = pu[s, b, 6 * DG:] if pb.kind == "general" else W[c + "attention.scalar.weight"][0]
                G = st["g"][:s, b]
                sc = G @ x
                Esc = 151 * U32 * (G.abs() @ x.abs())
                a = torch.softmax(sc, 0)
                rho = 2 * Esc.max() + U32 * ((sc - sc.max()).abs() + 2)
                Ea = a * (rho + rho.max() + (s + 1) * U32) + TINY
                al_w[s, b, :s], al_E[s, b, :s] = a, Ea
                cv[s, b] = a @ G
                cE[s, b] = Ea @ G.abs() + (s + 1) * U32 * (a @ G.abs()) + TINY
        # p cell on the kernel's c and q0
        ai, Eai = _contract(W[c + "p_cell.weight_ih"][:, D_m:], st["c"], pu[..., 3 * DG:6 * DG], DG)
        ah, Eah = _contract(W[c + "p_cell.weight_hh"], st["q0"], W[c + "p_cell.bias_hh"].expand(T, B, -1), DG)
        pv, pE = _cell(ai, Eai, ah, Eah, st["q0"], None if keep is None else keep["q"], pb.scale)
        q1 = m * pv["h"] + (1 - m) * st["q0"]
        q1E = m * pE["h"] + TINY
        # e cell on the kernel's q1 and e
        ai, Eai = _contract(W[c + "e_cell.weight_ih"], st["q1"], W[c + "e_cell.bias_ih"].expand(T, B, -1), DG)
        ah, Eah = _contract(W[c + "e_cell.weight_hh"], prev(st["e"]), W[c + "e_cell.bias_hh"].expand(T, B, -1), DE)
        ev, eE = _cell(ai, Eai, ah, Eah, prev(st["e"]), None if keep is None else keep["e"], pb.scale)
        checks = [("rg", gv["r"], gE["r"]), ("zg", gv["z"], gE["z"]), ("ng", gv["n"], gE["n"]), ("hng", gv["hn"], gE["hn"]),
                  ("g", gv["h"], gE["h"]), ("c", cv, cE), ("rp", pv["r"], pE["r"]), ("zp", pv["z"], pE["z"]), ("np", pv["n"], pE["n"]),
                  ("hnp", pv["hn"], pE["hn"]), ("q1", q1, q1E), ("re", ev["r"], eE["r"]), ("ze", ev["z"], eE["z"]),
                  ("ne", ev["n"], eE["n"]), ("hne", ev["hn"], eE["hn"]), ("e", ev["h"], eE["h"])]
        vm = valid.unsqueeze(2)
        for n, want, bound in checks:
            got = st[n]
            assert float((got * (~vm)).abs().max()) == 0.0, (n, "rows at or beyond a length must stay zero")
            worst[n] = max(worst.get(n, 0.0), _ratio(got[valid], want[valid], bound[valid]))
        alpha = out["alpha"][d].double()
        assert float((alpha * (~vm)).abs().max()) == 0.0
        assert float(torch.triu(alpha.permute(1, 0, 2)).abs().max()) == 0.0, "alpha must be zero on and above the diagonal"
        worst["alpha"] = max(worst.get("alpha", 0.0), _ratio(alpha, al_w, al_E))
        rowsum = out["alpha"][d].double().sum(2)
        has = valid.clone()
        has[0] = False
        if has.any():
            assert float((rowsum[has] - 1.0).abs().max()) <= 4 * 2.0 ** -23, "alpha rows must sum to 1 within 4 ulp"
        assert float(rowsum[~has].abs().max()) == 0.0 if (~has).any() else True
        # the e output: the e plane in time order, zero beyond a length
        e_want = torch.zeros(T, B, DE)
        e_want[tmap[valid], bidx[valid]] = out["state"][d, 16][..., :DE][valid]
        assert torch.equal(out["e"][d], e_want), "e output"
    return worst


# (kind, B as an offset from R, T, parties, flags, lengths or None, zero qmask rows)
def _cases():
    return [("general", 1, 1, 2, False), ("simple", "R-1", 2, 9, True), ("general", "R", 3, 2, True), ("simple", "R+1", 9, 9, False),
            ("general", "R+1", 9, 2, True), ("simple", "R", 9, 2, True), ("general", "R-1", 9, 9, False), ("simple", 1, 3, 2, False)]


def _shape(Bspec, T):
    R = K.chains_per_group()
    B = {"R-1": max(R - 1, 1), "R": R, "R+1": R + 1}.get(Bspec, Bspec)
    lengths = [T, 1, T, max(T // 2, 1), max(T - 3, 1), T, 2, T][:B] if B > 1 else [T]
    lengths = [min(n, T) for n in lengths]
    zero_rows = [(2, 0)] if T >= 3 else []
    if T >= 9 and B >= 3:
        zero_rows.append((5, 2))
    return B, lengths, zero_rows


@gpu
@pytest.mark.parametrize("case", range(8))
def test_forward_planes_against_float64_steps(case):
    kind, Bspec, T, Pn, flags = _cases()[case]
    B, lengths, zero_rows = _shape(Bspec, T)
    pb = Problem(kind, B, T, Pn, flags, 100 + case, lengths, zero_rows)
    worst = forward_ratios(pb, run_kernels(pb, backward=False))
    _say("fwd case=%d %s B=%d T=%d P=%d flags=%d" % (case, kind, B, T, Pn, flags), **worst)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def restatement_grads(pb, dtype):
    """Forward + autograd of the restatement in ``dtype`` on the projected rows -> the backward entry point's outputs."""
    Pd = {k: v.to(dtype).clone() for k, v in pb.P.items()}
    T, B = pb.T, pb.B
    res = dict(dgate=torch.zeros(2, 6, T, B, 3 * DG, dtype=dtype), dpu=[], dw=torch.zeros(2, DG, dtype=dtype), e=[], alpha=[])
    for d, pre in enumerate(("dialog_rnn_f.", "dialog_rnn_r.")):
        pu = pb.pu[d].to(dtype).requires_grad_(True)
        probes = {n: torch.zeros(T, B, 3 * (DE if n.endswith("_e") else DG), dtype=dtype, requires_grad=True) for n in DR.PROBES}
        if pb.kind == "simple":
            Pd[pre + "dialogue_cell.attention.scalar.weight"].requires_grad_(True)
        e, alpha = DR.encoder(Pd, pre, pb.U, pb.qmask, pb.lengths, pb.kind, reverse=bool(d), keep=None if pb.keep is None else pb.keep[d],
                              scale=pb.scale, pu=pu, probes=probes)
        (e * pb.de[d].to(dtype)).sum().backward()
        for i, n in enumerate(DR.PROBES):
            g = probes[n].grad
            if g is not None:             # (None: nothing depends on it -- the g cell at T = 1)
                res["dgate"][d, i, :, :, :g.shape[2]] = g
        res["dpu"].append(pu.grad)
        if pb.kind == "simple":
            gw = Pd[pre + "dialogue_cell.attention.scalar.weight"].grad
            if gw is not None:
                res["dw"][d] = gw[0]
        res["e"].append(e.detach())
        res["alpha"].append(alpha)
    return res


def _gate_grad64(dh, Edh, r, z, n, hn, hp):
    """Float64 gate gradients of one GRU cell and their bounds (module docstring) -> (dgi, E_dgi, dgh, E_dgh, direct, E_direct)."""
    Bn = 1 - n * n
    EB = U32 * (n * n + Bn.abs())
    dnp = dh * (1 - z) * Bn
    Ednp = Edh * ((1 - z) * Bn).abs() + (dh * (1 - z)).abs() * EB + 6 * U32 * dnp.abs() + TINY
    dz = dh * (hp - n) * z * (1 - z)
    Edz = Edh * ((hp - n) * z * (1 - z)).abs() + 6 * U32 * dz.abs() + TINY
    dr = dnp * hn * r * (1 - r)
    Edr = Ednp * (hn * r * (1 - r)).abs() + 6 * U32 * dr.abs() + TINY
    dnh = dnp * r
    Ednh = Ednp * r + 2 * U32 * dnh.abs() + TINY
    direct = dh * z
    return (torch.cat([dr, dz, dnp]), torch.cat([Edr, Edz, Ednp]), torch.cat([dr, dz, dnh]), torch.cat([Edr, Edz, Ednh]),
            direct, Edh * z + U32 * direct.abs() + TINY)


def _contract_t64(d, W):
    """(d W, bound) for the kernel's own gate gradients d (J) and a stored matrix W (J, K)."""
    return d @ W, (W.shape[0] + 4) * U32 * (d.abs() @ W.abs()) + TINY


def backward_local_ratios(pb, out):
    """T <= 2: worst |kernel - float64 step| / bound per backward output, chain by chain, and the exact checks."""
    T, B, D_m = pb.T, pb.B, pb.D_m
    assert T <= 2
    worst = {}

    def note(k, got, want, bound):
        worst[k] = max(worst.get(k, 0.0), _ratio(got, want, bound))
    for d, pre in enumerate(("dialog_rnn_f.", "dialog_rnn_r.")):
        c = pre + "dialogue_cell."
        W = {k[len(c):]: v.double() for k, v in pb.P.items() if k.startswith(c)}
        Wie, Whe = W["e_cell.weight_ih"], W["e_cell.weight_hh"]
        Wpc, Wph = W["p_cell.weight_ih"][:, D_m:], W["p_cell.weight_hh"]
        Wgq = W["g_cell.weight_ih"][:, D_m:]
        st = {n: out["state"][d, i].double() for i, n in enumerate(DR.PLANES)}
        dg = out["dgate"][d]                                   # (6, T, B, 452) float32, the kernel's own
        for b in range(B):
            n_b = pb.lengths[b] if d else T
            times = list(range(n_b - 1, -1, -1)) if d else list(range(T))
            ks = lambda name, s, w: (pb.keep[d][name][s, b].double() * pb.scale) if pb.keep is not None else torch.ones(w, dtype=torch.float64)
            zero = lambda w: torch.zeros(w, dtype=torch.float64)
            de_c, Ede_c = zero(DE), zero(DE)
            dq_c = {}
            for s in range(n_b - 1, -1, -1):
                t = times[s]
                spk, m = int(pb.spk[t, b]), float(pb.upd[t, b])
                last = s == n_b - 1
                # ---- e cell
                dh = pb.de[d, t, b].double() + de_c
                Edh = Ede_c + (0 if last else U32 * dh.abs())
                k_e = ks("e", s, DE)
                Edh = Edh * k_e + (U32 * (dh * k_e).abs() if pb.keep is not None else 0)
                dh = dh * k_e
                hp = st["e"][s - 1, b, :DE] if s > 0 else zero(DE)
                gi, Egi, gh, Egh, dire, Edire = _gate_grad64(dh, Edh, st["re"][s, b, :DE], st["ze"][s, b, :DE], st["ne"][s, b, :DE],
                                                             st["hne"][s, b, :DE], hp)
                note("dgi_e", dg[4, s, b, :3 * DE], gi, Egi)
                note("dgh_e", dg[5, s, b, :3 * DE], gh, Egh)
                k4, k5 = dg[4, s, b, :3 * DE].double(), dg[5, s, b, :3 * DE].double()
                dq1, Edq1 = _contract_t64(k4, Wie)
                if spk in dq_c:
                    dq1 = dq1 + dq_c[spk][0]
                    Edq1 = Edq1 + dq_c[spk][1] + U32 * dq1.abs()
                v, Ev = _contract_t64(k5, Whe)
                de_c, Ede_c = dire + v, Edire + Ev + U32 * (dire + v).abs()
                # ---- p cell
                k_q = ks("q", s, DG)
                dqs = m * dq1 * k_q
                Edqs = m * Edq1 * k_q + (U32 * dqs.abs() if pb.keep is not None else 0)
                gi, Egi, gh, Egh, dirp, Edirp = _gate_grad64(dqs, Edqs, st["rp"][s, b, :DG], st["zp"][s, b, :DG], st["np"][s, b, :DG],
                                                             st["hnp"][s, b, :DG], st["q0"][s, b, :DG])
                note("dgi_p", dg[2, s, b, :3 * DG], gi, Egi)
                note("dgh_p", dg[3, s, b, :3 * DG], gh, Egh)
                k2, k3 = dg[2, s, b, :3 * DG].double(), dg[3, s, b, :3 * DG].double()
                v, Ev = _contract_t64(k3, Wph)
                dq0 = (1 - m) * dq1 + dirp + v
                Edq0 = (1 - m) * Edq1 + Edirp + Ev + 3 * U32 * dq0.abs()
                # ---- attention of step 1 over its one-entry history: dG_hist[0] = dc, nothing else
                hist = out["dghist"][d, :, b, :DG].double()
                if s == 1:
                    dc, Edc = _contract_t64(k2, Wpc)
                    note("dghist", out["dghist"][d, 0, b, :DG], dc, Edc + U32 * dc.abs())
                # ---- g cell: dg = dG_hist[s] (the kernel's own row) exactly; zero at the last step
                if last:
                    assert float(hist[s].abs().max()) == 0.0 and float(dg[0:2, s, b].abs().max()) == 0.0, ("g at the last step", d, b)
                    dq_c = {spk: (dq0, Edq0)}
                else:
                    k_g = ks("g", s, DG)
                    dgt = hist[s] * k_g
                    Edgt = (U32 * dgt.abs() if pb.keep is not None else zero(DG)) + TINY
                    gi, Egi, gh, Egh, _, _ = _gate_grad64(dgt, Edgt, st["rg"][s, b, :DG], st["zg"][s, b, :DG], st["ng"][s, b, :DG],
                                                          st["hng"][s, b, :DG], zero(DG))
                    note("dgi_g", dg[0, s, b, :3 * DG], gi, Egi)
                    note("dgh_g", dg[1, s, b, :3 * DG], gh, Egh)
                # ---- the projected rows' gradient: bit copies in time order, dx_att exactly zero
                row = out["dpu"][d][t, b]
                assert torch.equal(row[:3 * DG], dg[0, s, b, :3 * DG]) and torch.equal(row[3 * DG:6 * DG], dg[2, s, b, :3 * DG]), "dpu"
                assert float(row[6 * DG:].abs().max()) == 0.0 if row.numel() > 6 * DG else True
            for s in range(n_b, T):
                assert float(dg[:, s, b].abs().max()) == 0.0
        assert float(out["dw"][d].abs().max()) == 0.0
    return worst


@gpu
@pytest.mark.parametrize("kind,B,T,Pn,flags", [("general", 1, 1, 2, False), ("simple", 3, 1, 9, True), ("general", 3, 2, 2, True),
                                               ("simple", 3, 2, 9, False), ("general", 2, 2, 9, False), ("simple", 1, 2, 2, True)])
def test_backward_local_bounds(kind, B, T, Pn, flags):
    lengths = [T, 1, T][:B]
    pb = Problem(kind, B, T, Pn, flags, 300 + 10 * T + B, lengths)
    worst = backward_local_ratios(pb, run_kernels(pb))
    _say("bwd-local %s B=%d T=%d P=%d flags=%d" % (kind, B, T, Pn, flags), **worst)
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@gpu
@pytest.mark.parametrize("case", range(8))
def test_backward_against_float64_calibrated_on_float32(case):
    kind, Bspec, T, Pn, flags = _cases()[case]
    B, lengths, zero_rows = _shape(Bspec, T)
    pb = Problem(kind, B, T, Pn, flags, 100 + case, lengths, zero_rows)
    out = run_kernels(pb)
    r64, r32 = restatement_grads(pb, torch.float64), restatement_grads(pb, torch.float32)
    assert float(out["dgate"][..., 3 * DG:].abs().max()) == 0.0
    got = {"dgate/" + n: out["dgate"][:, i, :, :, :3 * DG] for i, n in enumerate(DR.PROBES)}
    want = {"dgate/" + n: (r64["dgate"][:, i], r32["dgate"][:, i]) for i, n in enumerate(DR.PROBES)}
    blocks = [("g", 0, 3 * DG), ("p", 3 * DG, 6 * DG)] + ([("x_att", 6 * DG, 7 * DG)] if kind == "general" else [])
    for d in range(2):            # the projected rows' gradient per column block: dx_att is small next to the gate gradients
        for n, c0, c1 in blocks:
            got["dpu/%d/%s" % (d, n)] = out["dpu"][d][..., c0:c1]
            want["dpu/%d/%s" % (d, n)] = (r64["dpu"][d][..., c0:c1], r32["dpu"][d][..., c0:c1])
    if kind == "simple":
        got["dw"] = out["dw"][:, :, :DG].double().sum(1)
        want["dw"] = (r64["dw"], r32["dw"])
        assert float(out["dw"][:, :, DG:].abs().max()) == 0.0
    worst = {}
    for k, g in got.items():
        w64, w32 = want[k]
        top = float(w64.abs().max())
        err = float((g.double() - w64).abs().max())
        if top == 0:
            # an exact zero of the float64 gradient is a zero of the algebra, and the kernel must give an exact zero too: a
            # softmax over at most one entry has no gradient (dw, dx_att at T <= 2; the kernel's dscore = alpha (da - da)),
            # nothing depends on g_0 at T = 1, and a zero qmask row (m = 0) at the last step with a history cuts dc off
            assert err == 0, k
            worst[k] = 0.0
            continue
        ref = float((w32.double() - w64).abs().max())
        worst[k] = err / (4 * ref + 8 * U32 * top)
    _say("bwd case=%d %s B=%d T=%d P=%d flags=%d" % (case, kind, B, T, Pn, flags), **worst)
    # reverse rows at or beyond a length: exactly zero in every backward output
    for b, n in enumerate(lengths):
        assert float(out["dgate"][1, :, n:, b].abs().max()) == 0.0 if n < T else True
        assert float(out["dpu"][1][n:, b].abs().max()) == 0.0 if n < T else True
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


@gpu
@pytest.mark.parametrize("kind,flags", [("general", True), ("simple", False)])
def test_bits_do_not_depend_on_the_slot_or_the_run(kind, flags):
    R = K.chains_per_group()
    B, T = max(2 * R + 1, 5), 9
    lengths = ([T, 1, 5, T, 3, 7, 2, T, 4] * 2)[:B]
    pb = Problem(kind, B, T, 9, flags, 7, lengths, [(2, 0), (4, 3)])
    a, again = run_kernels(pb), run_kernels(pb)
    perm = [(3 * i + 1) % B for i in range(B)] if B % 3 else list(range(B - 1, -1, -1))
    assert sorted(perm) == list(range(B)) and any(p // R != i // R or p % R != i % R for i, p in enumerate(perm))
    pm = run_kernels(pb.permuted(perm))
    for k in ("e", "alpha", "state", "dgate", "dghist", "dw"):
        assert torch.equal(a[k], again[k]), ("two runs", k)
        axis = 1 if k == "dw" else (3 if k in ("state", "dgate") else 2)
        assert torch.equal(a[k].index_select(axis, torch.tensor(perm)), pm[k]), ("slot", k)
    for d in range(2):
        assert torch.equal(a["dpu"][d], again["dpu"][d]) and torch.equal(a["dpu"][d][:, perm], pm["dpu"][d])
    for b, n in enumerate(lengths):      # reverse outputs at or beyond a length
        if n < T:
            assert float(a["e"][1, n:, b].abs().max()) == 0.0 and float(a["alpha"][1, n:, b].abs().max()) == 0.0
            assert float(a["state"][1, :, n:, b].abs().max()) == 0.0


@gpu
def test_operator_image_matches_the_header_layout():
    from mm_dfn_amd import DialogueRNN
    for kind in ("simple", "general"):
        torch.manual_seed(3)
        m = DialogueRNN(8, 150, 150, 100, context_attention=kind).to(DEV)
        P = {"dialog_rnn_f." + k: v.detach().cpu() for k, v in m.state_dict().items()}
        img = K.weight_image(m.dialogue_cell)
        assert torch.equal(img.cpu(), image_of(P, "dialog_rnn_f.", 8, kind))
        assert K.weight_image(m.dialogue_cell) is img
        with torch.no_grad():
            m.dialogue_cell.e_cell.bias_hh.add_(1.0)
        again = K.weight_image(m.dialogue_cell)
        assert again is not img and not torch.equal(again, img)
