"""The fused GRU recurrence (K2: csrc/gru.hip, csrc/gru_mfma.hip) against a float64 restatement, step by step.

The C entry points are called directly (mmdfn_gru_seq_fwd / _bwd, their _seg forms, mmdfn_gru_tab_reduce); the reference
is the contract of include/mmdfn_hip.h restated here in float64 on the CPU, independent of oracle/:

    a = W_hh h + b_hh;  r = sig(gi_r + a_r);  z = sig(gi_z + a_z);  ghn = a_n;  n = tanh(gi_n + r ghn);  h' = (1-z) n + z h
    dn = dh (1-z)(1-n^2);  dz = dh (h-n) z (1-z);  dr = dn ghn r (1-r)
    dgi = [dr, dz, dn];  dgh = [dr, dz, dn r];  dh_prev = dgh W_hh + z dh

Nothing below is fitted to what the kernels return.  u = 2^-24 is the fp32 unit roundoff, one ulp of a result is <= 2u
of it, K = H = 100.

FORWARD: ONE-STEP RESIDUALS.  A 110-step trajectory amplifies legitimate rounding, so whole trajectories are not compared.
For every (t, row, direction) the kernel's OWN previous output (as float64) is h, one float64 step is evaluated, and the
kernel's r, z, ghn, n, y_t are compared element by element.  If every step is locally right the trajectory is a valid fp32
trajectory of any length.  With S = |W_hh| |h| + |b_hh| (per gate row):

  E_a   a K-term fp32 dot product in any order (FMA or not) is within K u sum|w h| of the exact one, the bias adds one
        rounding, one u is slack: (K + 2) u S.  The MFMA form cuts every fp32 operand into three bf16 pieces by truncation
        (8 + 8 + 8 bits: exact) and forms six of the nine piece products; the dropped ones, (p2 q3, p3 q2, p3 q3), are at
        most (2^-24 + 2^-24 + 2^-32) |w h| = (2 + 2^-8) u |w h| per term: (K + 5) u S.
  E_r = E_z   the pre-activation x = gi + a carries E_a and one rounding u |x| <= u (|gi| + S); |sig'| <= 1/4.  The
        evaluation rcp(1 + exp(-x)): exp's argument scaling and its ulp move e = exp(-x) by (|x| + 2) u relative, i.e. sig
        by sig (1 - sig) (|x| + 2) u <= 0.73 u; rounding 1 + e moves sig by <= u; rcp's ulp is <= u of a result in
        (0, 1]: 2.73 u, stated as 4 u.        E_r = (E_a + u (|gi| + S)) / 4 + 4 u.
  E_n   x_n = gi_n + r ghn from the kernel's own r, ghn: E_a |r| + E_r |ghn|, two roundings 2 u (|gi_n| + |r ghn|);
        |tanh'| <= 1.  The evaluation 1 - 2 rcp(1 + exp(2x)) with t = 2 / (1 + e) in [0, 2]: e's relative error moves t by
        t (1 - t/2) (|2x| + 2) u <= 1.45 u, rounding 1 + e by <= 2 u, rcp's ulp by <= 2 u, the final subtraction by
        u / 2: 5.95 u, stated as 6 u.   E_n = E_a |r| + E_r |ghn| + 2 u (|gi_n| + |r ghn|) + 6 u.
  E_y   from z and n: E_z |n - h| + E_n |1 - z|; (1 - z), two products and one sum: 3 u (|n| + |h|).
A float32 numpy restatement of the same formulas stays well inside these bounds and well above zero
(test_bounds_hold_for_a_float32_restatement: no device needed), so they are neither violated by honest fp32 nor vacuous.

BACKWARD, LOCAL (T = 1, 2; y, gates, dy are plain inputs, so they are synthetic here).  The first step processed has
dh = dy exactly (E_dh = 0).  With A = 1 - z (one rounding) and B = 1 - n^2 (n^2 rounded, then subtracted: absolute error
u (n^2 + |B|), which is NOT small next to B when |n| -> 1):
    E_dn  = E_dh |A B| + |dh A| u (n^2 + |B|) + 6 u |dn|              (three more roundings; 6 u covers any order)
    E_dz  = E_dh |(h-n) z A| + 6 u |dz|                               (five roundings, all relative)
    E_dr  = E_dn |ghn r (1-r)| + 6 u |dr|                             (four more roundings)
    E_dgn = E_dn |r| + 2 u |dn r|
At T = 2 the second step sees dh = dy + carry, carry = dgh W_hh + z dh_1: one 300-term contraction of the kernel's OWN
dgh of the first step (read back, so its error does not compound) plus one product and two sums:
    E_carry = (3H + 4) u (|dgh| |W_hh| + |z dh_1|)   [(3H + 7) for the MFMA form, as above],
    E_dh = E_carry + u (|dy| + |dgh| |W_hh| + |z dh_1|)   (the sum with dy).
Every bound also carries 2^-126 (results below the smallest normal fp32 may be flushed).

BACKWARD AT LENGTH (T = 33, 110).  No local bound exists (dh of an inner step is not an output, and an absolute-value
propagated bound grows beyond 1e26), so the kernel is calibrated against honest fp32: both the kernel and a float32 CPU
restatement of the same recurrence run on the kernel's own saved forward values and are compared with float64, max-norm
per tensor; the kernel's error must be <= 4 e_ref + 8 u max|want| (factor 4: the precedent of
test_lstm_gate_forward_bf16_piece_form_against_the_exact_f32_form).

mmdfn_gru_tab_reduce is a plain sum: (rows + 2) u sum|terms|.

Saturation: sig is exactly 1 at pre-activations of +30 and +100 and exactly 0 at -100 (exp overflows to inf, rcp(inf) = 0);
at -30 the exact value is 9.4e-14, which fp32 represents, so there the tests assert the E_r bound and 0 < sig < 1e-9, not
an exact zero.  tanh is exactly +-1 at all four.

Measured ratios of every check: profiles/r10_gru_recurrence_parity.md (the tests print them: pytest -s).
"""
import numpy as np
import pytest
import torch

from mm_dfn_amd import _hip

gpu = pytest.mark.gpu
DEV = "cuda"
H = 100
U = 2.0 ** -24
TINY = 2.0 ** -126
NAN = float("nan")


def _say(tag, **kv):
    print("GRU-PARITY %s %s" % (tag, " ".join("%s=%.3g" % (k, v) for k, v in kv.items())), flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement and bounds (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _shift(yd, d):
    """h_{t-1} of every step of direction d from the outputs yd (T, R, H): zero initial state, direction 1 runs backwards."""
    z = torch.zeros_like(yd[:1])
    return torch.cat([z, yd[:-1]]) if d == 0 else torch.cat([yd[1:], z])


def step64(gi, h, W, b, mfma=False):
    """One float64 step for gi (..., 3H), h (..., H): ({r, z, ghn, n, y}, the per-element bounds of the module docstring)."""
    gi, h, W, b = gi.double(), h.double(), W.double(), b.double()
    a = h @ W.t() + b
    S = h.abs() @ W.abs().t() + b.abs()
    Ea = (H + (5 if mfma else 2)) * U * S
    g = lambda x, k: x[..., k * H:(k + 1) * H]
    r, z = torch.sigmoid(g(gi, 0) + g(a, 0)), torch.sigmoid(g(gi, 1) + g(a, 1))
    Er = 0.25 * (g(Ea, 0) + U * (g(gi, 0).abs() + g(S, 0))) + 4 * U
    Ez = 0.25 * (g(Ea, 1) + U * (g(gi, 1).abs() + g(S, 1))) + 4 * U
    ghn = g(a, 2)
    n = torch.tanh(g(gi, 2) + r * ghn)
    En = g(Ea, 2) * r.abs() + Er * ghn.abs() + 2 * U * (g(gi, 2).abs() + (r * ghn).abs()) + 6 * U
    y = (1 - z) * n + z * h
    Ey = Ez * (n - h).abs() + En * (1 - z).abs() + 3 * U * (n.abs() + h.abs())
    return dict(r=r, z=z, ghn=ghn, n=n, y=y), dict(r=Er, z=Ez, ghn=g(Ea, 2), n=En, y=Ey)


def _ratio(got, want, bound, mask=None):
    """max over the (masked) elements of |got - want| / bound; 0 / 0 counts as 0, a non-finite value as inf."""
    got = got.double()
    err = (got - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isfinite(got), q, torch.full_like(q, float("inf")))
    if mask is not None:
        q = torch.where(mask.unsqueeze(-1).expand_as(q), q, torch.zeros_like(q))
    return float(q.max()) if q.numel() else 0.0


def forward_ratios(gi, Ws, bs, y, gates, mfma=False, mask=None):
    """Teacher-forced residuals of one group: {quantity: worst |kernel - float64 step| / bound}.  mask (T, R, 2): the
    positions to judge (the segmented launches do not visit every position)."""
    T, R = gi.shape[:2]
    gi4 = gi.reshape(T, R, 2, 3 * H)
    out = {}
    for d in range(2):
        yd = y[..., d * H:(d + 1) * H]
        want, bound = step64(gi4[:, :, d], _shift(yd, d), Ws[d], bs[d], mfma)
        got = dict(r=gates[:, :, d, 0], z=gates[:, :, d, 1], n=gates[:, :, d, 2], ghn=gates[:, :, d, 3], y=yd)
        for k in want:
            out[k] = max(out.get(k, 0.0), _ratio(got[k], want[k], bound[k], None if mask is None else mask[:, :, d]))
    return out


def fwd32(gi, Ws, bs):
    """float32 numpy restatement of the forward recurrence with the kernels' gate formulas: (y, gates)."""
    gi = gi.numpy()
    T, R = gi.shape[:2]
    gi4 = gi.reshape(T, R, 2, 3 * H)
    y = np.zeros((T, R, 2 * H), np.float32)
    gates = np.zeros((T, R, 2, 4, H), np.float32)
    one, two = np.float32(1), np.float32(2)
    with np.errstate(over="ignore"):
        for d in range(2):
            W, b = Ws[d].numpy(), bs[d].numpy()
            h = np.zeros((R, H), np.float32)
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                a = h @ W.T + b
                g = gi4[t, :, d]
                r = one / (one + np.exp(-(g[:, :H] + a[:, :H])))
                z = one / (one + np.exp(-(g[:, H:2 * H] + a[:, H:2 * H])))
                ghn = a[:, 2 * H:]
                n = one - two / (one + np.exp(two * (g[:, 2 * H:] + r * ghn)))
                h = (one - z) * n + z * h
                y[t, :, d * H:(d + 1) * H] = h
                for k, v in enumerate((r, z, n, ghn)):
                    gates[t, :, d, k] = v
    return torch.from_numpy(y), torch.from_numpy(gates)


def _bwd_step(dh, r, z, n, ghn, hp):
    dn = dh * (1 - z)
    dz = dh * (hp - n)
    dnp = dn * (1 - n * n)
    drp = dnp * ghn * r * (1 - r)
    dzp = dz * z * (1 - z)
    return drp, dzp, dnp, dnp * r


def bwd_ref(dy, y, gates, Ws, dtype, visited=None):
    """The backward recurrence in ``dtype`` on the given saved values: (dgi, dgh (T, R, 2, 3H), dhinit (R, 2, H) = the
    gradient wrt the state every chain started from).  visited (T, R, 2) bool: the steps that ran (segmented launches)."""
    T, R = dy.shape[:2]
    dgi = torch.zeros(T, R, 2, 3 * H, dtype=dtype)
    dgh = torch.zeros_like(dgi)
    dhinit = torch.zeros(R, 2, H, dtype=dtype)
    gates = torch.nan_to_num(gates.to(dtype), nan=0.0)
    for d in range(2):
        W = Ws[d].to(dtype)
        yd = y[..., d * H:(d + 1) * H].to(dtype)
        hp = _shift(yd, d)
        carry = torch.zeros(R, H, dtype=dtype)
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        for i, t in enumerate(order):
            v = torch.ones(R, 1, dtype=torch.bool) if visited is None else visited[t, :, d].unsqueeze(-1)
            nxt = torch.zeros(R, 1, dtype=torch.bool) if i + 1 == T else (
                v if visited is None else visited[order[i + 1], :, d].unsqueeze(-1))
            dh = dy[t, :, d * H:(d + 1) * H].to(dtype) + carry
            r, z, n, ghn = (gates[t, :, d, k] for k in range(4))
            drp, dzp, dnp, dgn = _bwd_step(dh, r, z, n, ghn, hp[t])
            gi_t, gh_t = torch.cat([drp, dzp, dnp], -1), torch.cat([drp, dzp, dgn], -1)
            new = gh_t @ W + dh * z
            zero3 = torch.zeros_like(gi_t)
            dgi[t, :, d] = torch.where(v, gi_t, zero3)
            dgh[t, :, d] = torch.where(v, gh_t, zero3)
            carry = torch.where(v, new, torch.zeros_like(new))
            dhinit[:, d] = torch.where(v & ~nxt, new, dhinit[:, d])
    return dgi, dgh, dhinit


def bwd_local_ratios(dy, y, gates, Ws, dgi, dgh, mfma=False):
    """T <= 2: every element of dgi / dgh against the float64 step under the local bounds of the module docstring."""
    T, R = dy.shape[:2]
    assert T <= 2
    dy, y, gates = dy.double(), y.double(), gates.double()
    dgi, dgh = dgi.reshape(T, R, 2, 3 * H), dgh.reshape(T, R, 2, 3 * H)
    out = {}
    for d in range(2):
        W = Ws[d].double()
        yd = y[..., d * H:(d + 1) * H]
        hp = _shift(yd, d)
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        dh, Edh = dy[order[0], :, d * H:(d + 1) * H], torch.zeros(R, H, dtype=torch.float64)
        for i, t in enumerate(order):
            if i == 1:
                t1 = order[0]
                dgk = dgh[t1, :, d].double()
                z1 = gates[t1, :, d, 1]
                mag = dgk.abs() @ W.abs() + (z1 * dh).abs()
                carry = dgk @ W + z1 * dh
                dyt = dy[t, :, d * H:(d + 1) * H]
                Edh = (3 * H + (7 if mfma else 4)) * U * mag + U * (dyt.abs() + mag)
                dh = dyt + carry
            r, z, n, ghn = (gates[t, :, d, k] for k in range(4))
            A, B = 1 - z, 1 - n * n
            drp, dzp, dnp, dgn = _bwd_step(dh, r, z, n, ghn, hp[t])
            Edn = Edh * (A * B).abs() + (dh * A).abs() * U * (n * n + B.abs()) + 6 * U * dnp.abs() + TINY
            Edz = Edh * ((hp[t] - n) * z * A).abs() + 6 * U * dzp.abs() + TINY
            Edr = Edn * (ghn * r * (1 - r)).abs() + 6 * U * drp.abs() + TINY
            Edg = Edn * r.abs() + 2 * U * dgn.abs() + TINY
            for name, got, want, bound in (("dgi_r", dgi[t, :, d, :H], drp, Edr), ("dgi_z", dgi[t, :, d, H:2 * H], dzp, Edz),
                                           ("dgi_n", dgi[t, :, d, 2 * H:], dnp, Edn), ("dgh_r", dgh[t, :, d, :H], drp, Edr),
                                           ("dgh_z", dgh[t, :, d, H:2 * H], dzp, Edz), ("dgh_n", dgh[t, :, d, 2 * H:], dgn, Edg)):
                key = name if i == 0 else name + "@2"
                out[key] = max(out.get(key, 0.0), _ratio(got, want, bound))
    return out


def bwd_long_ratios(dy, y, gates, Ws, dgi, dgh, visited=None, dhinit=None, tdir=None):
    """Section 3: {tensor: (kernel error / e_ref, passes)} with e_ref the error of the float32 CPU restatement against
    float64 on the same inputs; passes: kernel error <= 4 e_ref + 8 u max|want|."""
    T, R = dy.shape[:2]
    want = list(bwd_ref(dy, y, gates, Ws, torch.float64, visited))
    ref = list(bwd_ref(dy, y, gates, Ws, torch.float32, visited))
    if dhinit is not None:
        want[2], ref[2] = want[2][:, tdir], ref[2][:, tdir]
    got = [dgi.reshape(T, R, 2, 3 * H), dgh.reshape(T, R, 2, 3 * H)] + ([] if dhinit is None else [dhinit])
    out = {}
    for name, g, w, f in zip(("dgi", "dgh", "dhinit"), got, want, ref):
        assert bool(torch.isfinite(g).all()), name
        ek, er, top = float((g.double() - w).abs().max()), float((f.double() - w).abs().max()), float(w.abs().max())
        out[name] = (ek / er if er > 0 else (0.0 if ek == 0 else float("inf")), ek <= 4 * er + 8 * U * top)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_weights(seed, wscale, bscale=None):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    return [f(3 * H, H) * wscale for _ in range(2)], [f(3 * H) * (wscale if bscale is None else bscale) for _ in range(2)]


def make_gi(seed, T, R, scales=(0.01, 1.0, 1.0, 30.0), zero_row=True):
    """randn times a per-element scale drawn from ``scales`` (tiny, ordinary and saturating pre-activations side by side);
    one row of all zeros next to the ordinary ones."""
    g = torch.Generator().manual_seed(seed)
    gi = torch.randn(T, R, 6 * H, generator=g)
    sc = torch.tensor(scales)[torch.randint(len(scales), (T, R, 6 * H), generator=g)]
    gi = gi * sc
    if zero_row and R >= 2:
        gi[:, R // 2] = 0.0
    return gi


def make_saved(seed, T, R, edges=True):
    """Synthetic (dy, y, gates) for the backward: r, z in [0, 1], n, y in [-1, 1], ghn ~ N(0, 1); with ``edges`` the
    exactly saturated values in fixed unit ranges and one row of all zeros."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(T, R, 2 * H, generator=g)
    y = torch.rand(T, R, 2 * H, generator=g) * 2 - 1
    gates = torch.rand(T, R, 2, 4, H, generator=g)
    gates[:, :, :, 2] = gates[:, :, :, 2] * 2 - 1
    gates[:, :, :, 3] = torch.randn(T, R, 2, H, generator=g)
    if edges:
        gates[:, :, :, 0, 0:5] = 0.0          # r = 0
        gates[:, :, :, 0, 5:10] = 1.0         # r = 1
        gates[:, :, :, 1, 10:20] = 1.0        # z = 1
        gates[:, :, :, 1, 20:30] = 0.0        # z = 0
        gates[:, :, :, 2, 30:35] = 1.0        # n = +-1
        gates[:, :, :, 2, 35:40] = -1.0
        gates[:, :, :, 2, 40:45] = 1.0 - 2.0 ** -24       # 1 - n^2 is all cancellation
        gates[:, :, :, 1, 45:50] = 1.0 - 2.0 ** -24
        if R >= 2:
            dy[:, R // 2] = 0.0
            y[:, R // 2] = 0.0
            gates[:, R // 2] = 0.0
    return dy, y, gates


# ---------------------------------------------------------------------------------------------------------------------
# launches: every output sits inside a larger buffer whose margins hold a fixed bit pattern and is prefilled with NaN
# ---------------------------------------------------------------------------------------------------------------------
PATTERN = 0x5A5AA5A5
MARGIN = 256          # floats: keeps the 16-byte alignment the kernels' float4 stores need


class Guarded:
    def __init__(self, shape, fill=NAN):
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), PATTERN, dtype=torch.int32, device=DEV)
        inner = self.buf[MARGIN:MARGIN + n]
        if isinstance(fill, int):
            self.t = inner.view(shape)
        else:
            self.t = inner.view(torch.float32).view(shape)
        self.t.fill_(fill)

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == PATTERN).all()) and bool((self.buf[MARGIN + self.n:] == PATTERN).all())


def _dev(ts):
    return [None if t is None else t.to(DEV).contiguous() for t in ts]


def _finish(outs):
    torch.cuda.synchronize()
    for o in outs:
        assert o.margins_intact(), "a kernel wrote outside its output"
    return [o.t.cpu() for o in outs]


def launch_fwd(groups, seg=None, n=None, rows=None, Ts=None, Hval=H, rc_want=0):
    """groups: [(gi, Ws, bs)] on the CPU -> [(y, gates)] on the CPU.  seg = dict(rank, P, BP, tdir, ytab) of per-group
    lists selects mmdfn_gru_seq_fwd_seg.  n / rows / Ts / Hval override what is passed (the refusals)."""
    gis = _dev([g[0] for g in groups])
    Wd = _dev([w for g in groups for w in g[1]])
    bd = _dev([b for g in groups for b in g[2]])
    shp = [(g[0].shape[0], g[0].shape[1]) for g in groups]
    ys = [Guarded((T, R, 2 * H)) for T, R in shp]
    gs = [Guarded((T, R, 2, 4, H)) for T, R in shp]
    n = len(groups) if n is None else n
    rows = [R for _, R in shp] if rows is None else rows
    Ts = [T for T, _ in shp] if Ts is None else Ts
    common = (n, _hip.ptr_array(gis), _hip.ptr_array(Wd), _hip.ptr_array(bd), _hip.ptr_array([o.t for o in ys]),
              _hip.ptr_array([o.t for o in gs]), _hip.int_array(rows), _hip.int_array(Ts), Hval)
    if seg is None:
        rc = _hip.lib().mmdfn_gru_seq_fwd(*common, None, _hip.stream())
    else:
        rk, yt = _dev(seg["rank"]), _dev(seg.get("ytab") or [None] * len(groups))
        rc = _hip.lib().mmdfn_gru_seq_fwd_seg(*common, _hip.ptr_array(rk),
                                              _hip.int_array(seg["P"]), _hip.int_array(seg["BP"]),
                                              _hip.int_array(seg["tdir"]), _hip.ptr_array(yt), _hip.stream())
    res = _finish(ys + gs)
    assert rc == rc_want, rc
    k = len(groups)
    return [(res[i], res[k + i]) for i in range(k)]


def launch_bwd(groups, seg=None, n=None, rows=None, Ts=None, Hval=H, rc_want=0):
    """groups: [(dy, y, gates, Ws)] -> [(dgi, dgh)] (T, R, 6H), or with seg [(dgi, dgh, dhinit, kout)] (None where not
    asked for: seg["want_init"][g])."""
    dys, yd, gd = _dev([g[0] for g in groups]), _dev([g[1] for g in groups]), _dev([g[2] for g in groups])
    Wd = _dev([w for g in groups for w in g[3]])
    shp = [(g[0].shape[0], g[0].shape[1]) for g in groups]
    dgi = [Guarded((T, R, 6 * H)) for T, R in shp]
    dgh = [Guarded((T, R, 6 * H)) for T, R in shp]
    n = len(groups) if n is None else n
    rows = [R for _, R in shp] if rows is None else rows
    Ts = [T for T, _ in shp] if Ts is None else Ts
    common = (n, _hip.ptr_array(dys), _hip.ptr_array(yd), _hip.ptr_array(gd), _hip.ptr_array(Wd),
              _hip.ptr_array([o.t for o in dgi]), _hip.ptr_array([o.t for o in dgh]), _hip.int_array(rows),
              _hip.int_array(Ts), Hval)
    k = len(groups)
    if seg is None:
        rc = _hip.lib().mmdfn_gru_seq_bwd(*common, None, _hip.stream())
        res = _finish(dgi + dgh)
        assert rc == rc_want, rc
        return [(res[i], res[k + i]) for i in range(k)]
    want = seg.get("want_init") or [False] * k
    wk = seg.get("want_kout", want)
    di = [Guarded((R, H)) if w else None for (T, R), w in zip(shp, want)]
    ko = [Guarded((R,), fill=-7) if w else None for (T, R), w in zip(shp, wk)]
    rk = _dev(seg["rank"])
    rc = _hip.lib().mmdfn_gru_seq_bwd_seg(*common, _hip.ptr_array(rk), _hip.int_array(seg["P"]), _hip.int_array(seg["BP"]),
                                          _hip.int_array(seg["tdir"]), _hip.ptr_array([None if o is None else o.t for o in di]),
                                          _hip.ptr_array([None if o is None else o.t for o in ko]), _hip.stream())
    extra = [o for o in di + ko if o is not None]
    _finish(dgi + dgh + extra)
    assert rc == rc_want, rc
    return [(dgi[i].t.cpu(), dgh[i].t.cpu(), None if di[i] is None else di[i].t.cpu(), None if ko[i] is None else ko[i].t.cpu())
            for i in range(k)]


def _all_nan(*ts):
    return all(bool(torch.isnan(t).all()) for t in ts)


def _none_nan(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _is_mfma(shapes, env=None):
    low = 0 if (env or {}).get("MMDFN_GRU_MFMA_MIN") == "0" else 1024
    return 2 * sum(R for _, R in shapes) > low


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the checks of sections 1-3 on one set of groups, whatever launch form the library picks for it
# ---------------------------------------------------------------------------------------------------------------------
def check_forward(shapes, seed, wscale, mfma, tag, scales=(0.01, 1.0, 1.0, 30.0)):
    groups = []
    for i, (T, R) in enumerate(shapes):
        Ws, bs = make_weights(seed + 10 * i, wscale)
        groups.append((make_gi(seed + 10 * i + 1, T, R, scales), Ws, bs))
    res = launch_fwd(groups)
    worst = {}
    for (gi, Ws, bs), (y, gates) in zip(groups, res):
        assert _none_nan(y, gates), "an element was not written, or is not finite"
        for k, v in forward_ratios(gi, Ws, bs, y, gates, mfma).items():
            worst[k] = max(worst.get(k, 0.0), v)
    _say("fwd %s w=%g" % (tag, wscale), **worst)
    assert max(worst.values()) <= 1.0, worst
    return groups, res


def check_backward_local(shapes, seed, wscale, mfma, tag):
    assert all(T <= 2 for T, _ in shapes)
    groups = []
    for i, (T, R) in enumerate(shapes):
        dy, y, gates = make_saved(seed + 10 * i, T, R)
        groups.append((dy, y, gates, make_weights(seed + 10 * i + 1, wscale)[0]))
    res = launch_bwd(groups)
    worst = {}
    for (dy, y, gates, Ws), (dgi, dgh) in zip(groups, res):
        assert _none_nan(dgi, dgh)
        for k, v in bwd_local_ratios(dy, y, gates, Ws, dgi, dgh, mfma).items():
            worst[k] = max(worst.get(k, 0.0), v)
        # exactly saturated saved gates: every factor r (1-r), z (1-z), 1 - n^2 is exactly 0, and z = 1 passes nothing to dgi
        g4, h4 = dgi.view(*dgi.shape[:2], 2, 3, H), dgh.view(*dgh.shape[:2], 2, 3, H)
        for t4 in (g4, h4):
            assert float(t4[:, :, :, 0, 0:10].abs().max()) == 0.0          # r in {0, 1}
            assert float(t4[:, :, :, 1, 10:30].abs().max()) == 0.0         # z in {0, 1}
            assert float(t4[:, :, :, 2, 30:40].abs().max()) == 0.0         # n = +-1
            assert float(t4[:, :, :, 0, 30:40].abs().max()) == 0.0
            assert float(t4[:, :, :, :, 10:20].abs().max()) == 0.0         # z = 1: dgi = 0
    _say("bwd-local %s w=%g" % (tag, wscale), **{k: v for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    return groups, res


def check_backward_long(fwd_groups, fwd_res, seed, tag):
    """Section 3 on the kernel's own forward outputs."""
    g = torch.Generator().manual_seed(seed)
    groups = [(torch.randn(y.shape, generator=g), y, gates, Ws) for (gi, Ws, bs), (y, gates) in zip(fwd_groups, fwd_res)]
    res = launch_bwd(groups)
    ok, rat = True, {}
    for i, ((dy, y, gates, Ws), (dgi, dgh)) in enumerate(zip(groups, res)):
        for k, (q, passes) in bwd_long_ratios(dy, y, gates, Ws, dgi, dgh).items():
            rat["%s[%d]" % (k, i)] = q
            ok = ok and passes
    _say("bwd-long %s" % tag, **rat)
    assert ok, rat
    return groups, res


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the bounds themselves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", [0.1, 0.3, 1.0, 3.0])
def test_bounds_hold_for_a_float32_restatement(wscale):
    """An honest fp32 evaluation of the contract (numpy, the kernels' gate formulas, 110 steps, tiny / ordinary / saturating
    pre-activations) stays inside every forward bound, and not by orders of magnitude: the bounds are neither violated by
    legitimate rounding nor vacuous.  Measured: <= 0.29 (r, z), 0.35 (n), 0.34 (y), 0.052 (ghn); pinned here at 0.5 with a
    floor of 0.01."""
    Ws, bs = make_weights(3, wscale)
    worst = {}
    for giscale in (0.01, 1.0, 30.0):
        gi = make_gi(5, 110, 6, scales=(giscale,))
        y, gates = fwd32(gi, Ws, bs)
        for k, v in forward_ratios(gi, Ws, bs, y, gates).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if giscale == 30.0:
            sat = ((gates[:, :, :, :2] == 0) | (gates[:, :, :, :2] == 1)).float().mean()
            assert float(sat) > 0.2                                  # exactly saturated gates are really in the sample
    _say("cpu-f32 w=%g" % wscale, **worst)
    assert all(0.01 < v <= 0.5 for v in worst.values()), worst
    # and a wrong step is far outside: b_hn left out of ghn, tanh from exp(x) instead of exp(2x)
    gi = make_gi(5, 9, 3, scales=(1.0,))
    y, gates = fwd32(gi, Ws, bs)
    bad = gates.clone()
    bad[:, :, :, 3] -= torch.stack([bs[0][2 * H:], bs[1][2 * H:]])
    assert forward_ratios(gi, Ws, bs, y, bad)["ghn"] > 100
    bad = gates.clone()
    bad[:, :, :, 2] = torch.tanh(0.5 * torch.atanh(gates[:, :, :, 2].clamp(-0.999, 0.999)))
    assert forward_ratios(gi, Ws, bs, y, bad)["n"] > 100


def test_backward_restatements_agree_and_the_local_bounds_hold_for_float32():
    """The float64 backward recurrence against torch autograd of the float64 forward (the contract's two halves are
    consistent), and its float32 evaluation inside the local T = 1, 2 bounds and the section 3 criterion."""
    Ws, bs = make_weights(7, 0.3)
    T, R = 5, 3
    gi = make_gi(8, T, R, scales=(1.0,), zero_row=False).double().requires_grad_(True)
    Wd = [w.double() for w in Ws]
    ys, saved = [], []
    for d in range(2):
        h = torch.zeros(R, H, dtype=torch.float64)
        outs, gs = [None] * T, [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            want, _ = step64(gi[t].view(R, 2, 3 * H)[:, d], h, Wd[d], bs[d])
            h = want["y"]
            outs[t] = h
            gs[t] = torch.stack([want[k] for k in ("r", "z", "n", "ghn")], 1)
        ys.append(torch.stack(outs))
        saved.append(torch.stack(gs))
    y = torch.cat(ys, -1)
    gates = torch.stack(saved, 2)
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(1)).double()
    (y * dy).sum().backward()
    dgi, _, _ = bwd_ref(dy, y.detach(), gates.detach(), Ws, torch.float64)
    assert float((dgi.view(T, R, 6 * H) - gi.grad).abs().max()) < 1e-12 * float(gi.grad.abs().max())
    for T in (1, 2):
        dy, y, gates = make_saved(11 + T, T, 4)
        g32 = bwd_ref(dy, y, gates, Ws, torch.float32)
        rat = bwd_local_ratios(dy, y, gates, Ws, g32[0], g32[1])
        _say("cpu-f32 bwd-local T=%d" % T, **rat)
        assert max(rat.values()) <= 0.7, rat
        bad = g32[1].clone()
        bad[..., 2 * H:] = g32[0][..., 2 * H:]                          # dgh_n without the factor r
        assert bwd_local_ratios(dy, y, gates, Ws, g32[0], bad)["dgh_n"] > 100


# ---------------------------------------------------------------------------------------------------------------------
# GPU: launch edges of the production library
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R", [1, 2, 3, 128, 129, 512, 513, 529])
def test_forward_steps_at_the_launch_edges(R):
    """Section 1 at every row count where the launch form changes (1-3 rows; 128 | 129: the 5-wave form ends; 512 | 513:
    the first MFMA launch, whose last workgroup holds 1 of 16 rows; 529) and T = 1, 2, 3, 33; W_hh ~ U(-0.3, 0.3)."""
    for T in (1, 2, 3, 33):
        check_forward([(T, R)], 100 + T, 0.3, _is_mfma([(T, R)]), "T=%d R=%d" % (T, R))


@gpu
@pytest.mark.parametrize("R", [1, 2, 3, 128, 129, 512, 513, 529])
def test_backward_local_steps_at_the_launch_edges(R):
    for T in (1, 2):
        for wscale in (0.3, 0.0):
            check_backward_local([(T, R)], 200 + T, wscale, _is_mfma([(T, R)]), "T=%d R=%d" % (T, R))


@gpu
@pytest.mark.parametrize("wscale", [0.1, 0.3])
@pytest.mark.parametrize("T,R", [(33, 1), (33, 2), (33, 3), (33, 128), (33, 129), (33, 512), (33, 513), (33, 529), (110, 16),
                                 (110, 129)])
def test_backward_at_length_against_the_float32_restatement(T, R, wscale):
    """Sections 1 and 3 at length: the forward residuals of a T-step run, then the backward on those saved values."""
    mfma = _is_mfma([(T, R)])
    groups, res = check_forward([(T, R)], 300 + T + R, wscale, mfma, "T=%d R=%d" % (T, R))
    check_backward_long(groups, res, 301, "T=%d R=%d w=%g" % (T, R, wscale))


@gpu
@pytest.mark.parametrize("shapes", [[(7, 3), (110, 16), (1, 5), (33, 40)], [(5, 499), (9, 13)], [(5, 500), (9, 13)],
                                    [(2, 499), (1, 13)], [(2, 500), (1, 13)]])
def test_several_groups_in_one_launch(shapes):
    """Groups of different T and rows in one launch; 1 024 chains over two groups stay scalar, 1 026 take the MFMA form."""
    mfma = _is_mfma(shapes)
    tag = "+".join("%dx%d" % s for s in shapes)
    if all(T <= 2 for T, _ in shapes):
        check_backward_local(shapes, 410, 0.3, mfma, tag)
        return
    groups, res = check_forward(shapes, 400, 0.3, mfma, tag)
    check_backward_long(groups, res, 401, tag)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages()]


ALL_FORMS = ("gru_seq_fwd_io_kernel", "gru_seq_fwd_kernel", "gru_seq_fwd_mfma_kernel", "gru_seq_bwd_kpart_kernel",
             "gru_seq_bwd_kernel", "gru_seq_bwd_mfma_kernel")


@gpu
@pytest.mark.parametrize("shapes,fwd,bwd", [
    ([(2, 128)], "gru_seq_fwd_io_kernel", "gru_seq_bwd_kpart_kernel"),
    ([(2, 129)], "gru_seq_fwd_kernel", "gru_seq_bwd_kernel"),
    ([(2, 512)], "gru_seq_fwd_kernel", "gru_seq_bwd_kernel"),
    ([(2, 513)], "gru_seq_fwd_mfma_kernel", "gru_seq_bwd_mfma_kernel"),
    ([(5, 499), (9, 13)], "gru_seq_fwd_kernel", "gru_seq_bwd_kernel"),
    ([(5, 500), (9, 13)], "gru_seq_fwd_mfma_kernel", "gru_seq_bwd_mfma_kernel")])
def test_the_thresholds_pick_the_kernel_they_are_documented_to(shapes, fwd, bwd):
    fg, bg = [], []
    for i, (T, R) in enumerate(shapes):
        Ws, bs = make_weights(i, 0.3)
        fg.append((make_gi(i, T, R), Ws, bs))
        bg.append(make_saved(i, T, R) + (Ws,))
    names = _kernel_names(lambda: (launch_fwd(fg), launch_bwd(bg)))
    ran = {form for form in ALL_FORMS for nm in names if form in nm}      # (no form's name is a substring of another's)
    assert ran == {fwd, bwd}, (ran, names)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: gate edges (production forms at 5 rows; the forced forms below run the same function)
# ---------------------------------------------------------------------------------------------------------------------
def _gate_edge_gi(T, R, seed):
    """(T, R, 2, 3, H) with, in every direction: units 0-9 z pre-activation +100 / +30 over steps 3..5 (z = 1 exactly over
    a span), 10-19 z at -100 (z = 0), 20-29 r at -100 (r = 0), 30-39 r at +30 / +100 and n at +-30 / +-100, 40-49 z at -30;
    row 1 at step 4: r = 0 and z = 0 for ALL units (the state forgets everything before it)."""
    g = torch.Generator().manual_seed(seed)
    gi = torch.randn(T, R, 2, 3, H, generator=g)
    gi[3:6, :, :, 1, 0:5] = 100.0
    gi[3:6, :, :, 1, 5:10] = 30.0
    gi[:, :, :, 1, 10:20] = -100.0
    gi[:, :, :, 0, 20:30] = -100.0
    gi[:, :, :, 0, 30:35] = 30.0
    gi[:, :, :, 0, 35:40] = 100.0
    gi[:, :, :, 2, 30:32] = 30.0
    gi[:, :, :, 2, 32:35] = -30.0
    gi[:, :, :, 2, 35:37] = 100.0
    gi[:, :, :, 2, 37:40] = -100.0
    gi[:, :, :, 1, 40:50] = -30.0
    gi[4, 1, :, 0] = -100.0
    gi[4, 1, :, 1] = -100.0
    return gi


def check_gate_edges(R, mfma, tag):
    T = 9
    Ws, bs = make_weights(21, 0.1)
    gi5 = _gate_edge_gi(T, R, 22)
    gi = gi5.reshape(T, R, 6 * H)
    (y, gates), = launch_fwd([(gi, Ws, bs)])
    assert _none_nan(y, gates)
    rat = forward_ratios(gi, Ws, bs, y, gates, mfma)
    _say("gate-edges %s" % tag, **rat)
    assert max(rat.values()) <= 1.0, rat
    r, z, n = gates[:, :, :, 0], gates[:, :, :, 1], gates[:, :, :, 2]
    y2 = y.view(T, R, 2, H)
    o = torch.tensor([i for i in range(R) if i != 1])                   # (row 1 is the forgetting row)
    assert bool((z[3:6, o, :, 0:10] == 1.0).all()) and bool((z[:, :, :, 10:20] == 0.0).all())
    assert bool((r[:, :, :, 20:30] == 0.0).all()) and bool((r[:, o, :, 30:40] == 1.0).all())
    assert bool((n[:, :, :, 30:32] == 1.0).all()) and bool((n[:, :, :, 32:35] == -1.0).all())
    assert bool((n[:, :, :, 35:37] == 1.0).all()) and bool((n[:, :, :, 37:40] == -1.0).all())
    assert float(z[:, o, :, 40:50].max()) < 1e-9 and float(z[:, o, :, 40:50].min()) > 0.0        # sig(-30 + a): tiny, not 0
    # z = 1 over steps 3..5: y_t is bit-equal to the previous state of its direction
    assert torch.equal(_bits(y2[3:6, o, 0, 0:10]), _bits(y2[2:5, o, 0, 0:10]))
    assert torch.equal(_bits(y2[3:6, o, 1, 0:10]), _bits(y2[4:7, o, 1, 0:10]))
    # z = 0: y_t is bit-equal to n_t
    assert torch.equal(_bits(y2[:, :, :, 10:20]), _bits(n[:, :, :, 10:20]))
    # r = 0: n = tanh(gi_n) whatever W_hn h + b_hn is
    want = torch.tanh(gi5[:, :, :, 2, 20:30].double())
    assert _ratio(n[:, :, :, 20:30], want, 2 * U * gi5[:, :, :, 2, 20:30].double().abs() + 6 * U) <= 1.0
    # row 1, step 4 forgets: perturbing the gi of the steps before it (in processing order) leaves it and every later y
    # bit-unchanged
    gi_p = gi5.clone()
    gi_p[:4, 1, 0] += 0.5
    gi_p[5:, 1, 1] -= 0.5
    (y_p, _), = launch_fwd([(gi_p.reshape(T, R, 6 * H), Ws, bs)])
    y_p = y_p.view(T, R, 2, H)
    assert torch.equal(_bits(y_p[4:, 1, 0]), _bits(y2[4:, 1, 0])) and torch.equal(_bits(y_p[:5, 1, 1]), _bits(y2[:5, 1, 1]))
    assert not torch.equal(y_p[3, 1, 0], y2[3, 1, 0]) and not torch.equal(y_p[5, 1, 1], y2[5, 1, 1])
    assert torch.equal(_bits(y_p[:, 0]), _bits(y2[:, 0]))                 # and no other row notices
    # backward through these saved values: finite, and the saturated units pass exactly nothing
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(23))
    (dgi, dgh), = launch_bwd([(dy, y, gates, Ws)])
    assert _none_nan(dgi, dgh)
    g4 = dgi.view(T, R, 2, 3, H)
    assert float(g4[3:6, o, :, :, 0:10].abs().max()) == 0.0               # z = 1: dgi is 0 there
    assert float(g4[:, :, :, 1, 10:20].abs().max()) == 0.0                # z = 0: z (1-z) = 0
    assert float(g4[:, :, :, 0, 20:40].abs().max()) == 0.0                # r in {0, 1}
    assert float(g4[:, :, :, 2, 30:40].abs().max()) == 0.0                # n = +-1
    q = bwd_long_ratios(dy, y, gates, Ws, dgi, dgh)
    _say("gate-edges bwd %s" % tag, **{k: v[0] for k, v in q.items()})
    assert all(v[1] for v in q.values()), q


@gpu
def test_gate_edges():
    check_gate_edges(5, False, "production R=5")


def check_zero_weights_and_tiny_arguments(R, mfma, tag):
    """W_hh = 0, b_hh = 0: the pre-activations ARE gi, ghn is exactly 0 and y depends on gi alone.  gi in 1e-6 .. 1e-3 is
    the cancellation region of 1 - 2 / (1 + e^{2x}): only the absolute bound applies; the worst relative error of n is
    printed as a measurement."""
    T = 3
    Ws, bs = make_weights(1, 0.0)
    g = torch.Generator().manual_seed(31)
    mag = 10.0 ** (-6 + 3 * torch.rand(T, R, 6 * H, generator=g))
    gi = mag * torch.where(torch.rand(T, R, 6 * H, generator=g) < 0.5, -1.0, 1.0)
    (y, gates), = launch_fwd([(gi, Ws, bs)])
    rat = forward_ratios(gi, Ws, bs, y, gates, mfma)
    assert float(gates[:, :, :, 3].abs().max()) == 0.0
    n = gates[:, :, :, 2].double()
    want = torch.tanh(gi.view(T, R, 2, 3, H)[:, :, :, 2].double())
    rel = float(((n - want).abs() / want.abs()).max())
    _say("tiny-arguments %s" % tag, worst_relative_error_of_n=rel, **rat)
    assert max(rat.values()) <= 1.0, rat


@gpu
def test_zero_weights_and_tiny_arguments():
    check_zero_weights_and_tiny_arguments(5, False, "production R=5")


@gpu
@pytest.mark.parametrize("R", [5, 129, 513])
def test_weights_scaled_by_three_saturate_the_recurrence(R):
    """W_hh ~ U(-3, 3): |a| reaches 100 and the gates saturate from the recurrence itself."""
    groups, res = check_forward([(33, R)], 500, 3.0, _is_mfma([(33, R)]), "T=33 R=%d" % R, scales=(1.0,))
    r = res[0][1][:, :, :, 0]
    assert float(((r == 0) | (r == 1)).float().mean()) > 0.02


def check_same_signed_products(R, mfma, tag):
    """W_hh >= 0, b_hh = 0 and a state that is positive everywhere (z = 0, n = tanh of a positive argument): every product
    w h of the contraction has the same sign, so neither rounding errors nor dropped bf16 piece products can cancel each
    other.  E_a is a worst-case bound of exactly this situation; a piece product of weight 2^-16 too few misses it."""
    T = 4
    rs = np.random.RandomState(51)
    Ws = [torch.from_numpy(rs.uniform(0, 0.2, size=(3 * H, H)).astype(np.float32)) for _ in range(2)]
    bs = [torch.zeros(3 * H) for _ in range(2)]
    gi = torch.from_numpy(rs.uniform(0.5, 2.0, size=(T, R, 2, 3, H)).astype(np.float32))
    gi[:, :, :, 1] = -100.0
    gi = gi.reshape(T, R, 6 * H)
    (y, gates), = launch_fwd([(gi, Ws, bs)])
    assert float(y.min()) > 0.0
    rat = forward_ratios(gi, Ws, bs, y, gates, mfma)
    _say("same-signed %s" % tag, **rat)
    assert max(rat.values()) <= 1.0, rat


@gpu
@pytest.mark.parametrize("R", [5, 129, 513])
def test_same_signed_products(R):
    check_same_signed_products(R, _is_mfma([(4, R)]), "production R=%d" % R)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: memory contract and refusals
# ---------------------------------------------------------------------------------------------------------------------
def check_row_alone_and_rerun(R, tag, T=9):
    """A row's results are bit-identical alone and inside a batch of the same launch form; two runs are bit-identical."""
    Ws, bs = make_weights(41, 0.3)
    gi = make_gi(42, T, R, zero_row=False)
    (y, gates), = launch_fwd([(gi, Ws, bs)])
    (y2, gates2), = launch_fwd([(gi, Ws, bs)])
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(gates), _bits(gates2))
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(43))
    (dgi, dgh), = launch_bwd([(dy, y, gates, Ws)])
    (dgi2, dgh2), = launch_bwd([(dy, y, gates, Ws)])
    assert torch.equal(_bits(dgi), _bits(dgi2)) and torch.equal(_bits(dgh), _bits(dgh2))
    for j in sorted({0, R // 2, R - 1}):
        (ya, ga), = launch_fwd([(gi[:, j:j + 1], Ws, bs)])
        assert torch.equal(_bits(ya), _bits(y[:, j:j + 1])) and torch.equal(_bits(ga), _bits(gates[:, j:j + 1])), (tag, j)
        (da, ha), = launch_bwd([(dy[:, j:j + 1], y[:, j:j + 1], gates[:, j:j + 1], Ws)])
        assert torch.equal(_bits(da), _bits(dgi[:, j:j + 1])) and torch.equal(_bits(ha), _bits(dgh[:, j:j + 1])), (tag, j)


@gpu
def test_a_row_alone_equals_the_row_in_a_batch_and_runs_repeat():
    check_row_alone_and_rerun(5, "production R=5")
    check_row_alone_and_rerun(128, "production R=128", T=3)


@gpu
@pytest.mark.parametrize("what", ["ngroups0", "ngroups5", "H", "rows0", "rows-1", "T0", "T-1"])
def test_refused_calls_launch_nothing(what):
    Ws, bs = make_weights(1, 0.3)
    T, R = 3, 4
    k = 5 if what == "ngroups5" else 2
    fg = [(make_gi(i, T, R), Ws, bs) for i in range(k)]
    bg = [make_saved(i, T, R) + (Ws,) for i in range(k)]
    kw = dict(rc_want=-1)
    if what == "ngroups0":
        kw["n"] = 0
    elif what == "H":
        kw["Hval"] = 99
    elif what.startswith("rows"):
        kw["rows"] = [R, int(what[4:])]
    elif what.startswith("T"):
        kw["Ts"] = [T, int(what[1:])]
    for y, gates in launch_fwd(fg, **kw):
        assert _all_nan(y, gates)
    for dgi, dgh in launch_bwd(bg, **kw):
        assert _all_nan(dgi, dgh)
    seg = dict(rank=[None] * k, P=[1] * k, BP=[1] * k, tdir=[-1] * k)
    for y, gates in launch_fwd(fg, seg=seg, **kw):
        assert _all_nan(y, gates)
    for dgi, dgh, _, _ in launch_bwd(bg, seg=seg, **kw):
        assert _all_nan(dgi, dgh)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: forced forms (tuning library)
# ---------------------------------------------------------------------------------------------------------------------
FORCED = [{"MMDFN_GRU_R": "2"}, {"MMDFN_GRU_R": "4"}, {"MMDFN_GRU_MFMA_MIN": "0"}, {"MMDFN_GRU_IO": "0"},
          {"MMDFN_GRU_KPART_BWD": "0"}, {"MMDFN_GRU_KPART_BWD": "1"}]
_fid = lambda env: "-".join("%s=%s" % (k[6:], v) for k, v in env.items())


@gpu
@pytest.mark.parametrize("env", FORCED, ids=_fid)
def test_forced_forms(env, kernel_variants):
    """Sections 1-3, the gate edges and the memory contract on every instantiation the production dispatcher cannot reach at
    small sizes: R = 2 / 4 (rows 1, 3, 17, 33: the last workgroup is part-filled), the MFMA form (1 - 3 of 16 rows), the
    4-wave forward, both one-sequence-per-workgroup backward kernels."""
    for k, v in env.items():
        kernel_variants.setenv(k, v)
    tag = _fid(env)
    for R in (1, 3, 17, 33):
        mfma = _is_mfma([(1, R)], env)
        for T in (1, 2, 9):
            groups, res = check_forward([(T, R)], 600 + T, 0.3, mfma, "%s T=%d R=%d" % (tag, T, R))
            if T <= 2:
                check_backward_local([(T, R)], 610 + T, 0.3, mfma, "%s T=%d R=%d" % (tag, T, R))
            else:
                check_backward_long(groups, res, 620, "%s T=%d R=%d" % (tag, T, R))
    mfma = _is_mfma([(1, 3)], env)
    check_gate_edges(3, mfma, tag + " R=3")
    check_gate_edges(17, mfma, tag + " R=17")
    check_zero_weights_and_tiny_arguments(17, mfma, tag + " R=17")
    check_same_signed_products(17, mfma, tag + " R=17")
    check_row_alone_and_rerun(17, tag)
    check_forward([(9, 3), (2, 17), (1, 1)], 630, 0.3, _is_mfma([(9, 21)], env), tag + " groups")


@gpu
@pytest.mark.parametrize("env", [{"MMDFN_GRU_R": "2"}, {"MMDFN_GRU_MFMA_MIN": "0"}], ids=_fid)
def test_forced_forms_really_run(env, kernel_variants):
    for k, v in env.items():
        kernel_variants.setenv(k, v)
    Ws, bs = make_weights(1, 0.3)
    names = _kernel_names(lambda: (launch_fwd([(make_gi(1, 2, 3), Ws, bs)]), launch_bwd([make_saved(1, 2, 3) + (Ws,)])))
    forms = ("mfma_kernel",) if "MMDFN_GRU_MFMA_MIN" in env else ("_kernel<2", "_kernelILi2E")
    assert sum(any(f in nm for f in forms) for nm in names) == 2, names


# ---------------------------------------------------------------------------------------------------------------------
# GPU: segmented entry points
# ---------------------------------------------------------------------------------------------------------------------
def _rank_from_k(T, k):
    """(T, BP) int32 rank array whose row lengths are k: speaker column c talks at its first k[c] steps."""
    t = torch.arange(T).unsqueeze(1)
    kk = torch.as_tensor(k).unsqueeze(0)
    return torch.where(t < kk, t, torch.full_like(t, -1)).to(torch.int32).contiguous()


def _visited(T, R, k, tdir):
    """(T, R, 2) bool: rows with k = 0 run nothing; the truncated direction runs t < k, the other all T steps."""
    kk = torch.as_tensor(k).repeat(R // len(k))
    live = (kk > 0).view(1, R, 1).expand(T, R, 2).clone()
    if tdir >= 0:
        live[:, :, tdir] &= torch.arange(T).unsqueeze(1) < kk.unsqueeze(0)
    return live, kk


def check_segmented(T, P, k, nblocks, tdir, with_tab, seed, tag):
    BP = len(k)
    R = nblocks * BP
    Ws, bs = make_weights(seed, 0.3)
    gi = make_gi(seed + 1, T, R, scales=(0.01, 1.0, 1.0, 10.0), zero_row=False)
    visited, kk = _visited(T, R, k, tdir)
    ytab = None
    if with_tab:
        ytab = torch.rand(T, 1, 2 * H, generator=torch.Generator().manual_seed(seed + 2)) * 2 - 1
    seg = dict(rank=[_rank_from_k(T, k)], P=[P], BP=[BP], tdir=[tdir], ytab=[ytab])
    (y, gates), = launch_fwd([(gi, Ws, bs)], seg=seg)
    assert _none_nan(y)
    y4, g5 = y.view(T, R, 2, H), gates
    # never visited: zeros / table copies in y, the prefill intact in gates
    for d in range(2):
        off = ~visited[:, :, d]
        fill = torch.zeros(T, R, H)
        if with_tab and d == tdir:
            fill = ytab[:, 0, d * H:(d + 1) * H].unsqueeze(1).expand(T, R, H)
        assert torch.equal(_bits(y4[:, :, d][off]), _bits(fill[off])), (tag, d)
        assert _all_nan(g5[:, :, d][off]) and _none_nan(g5[:, :, d][~off]), (tag, d)
    rat = forward_ratios(gi, Ws, bs, y, gates, False, visited)
    _say("seg-fwd %s" % tag, **rat)
    assert max(rat.values()) <= 1.0, rat
    # backward on the kernel's own outputs
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(seed + 3))
    bseg = dict(seg, want_init=[with_tab])
    (dgi, dgh, dhinit, kout), = launch_bwd([(dy, y, gates, Ws)], seg=bseg)
    assert _none_nan(dgi, dgh)
    for t4 in (dgi.view(T, R, 2, 3 * H), dgh.view(T, R, 2, 3 * H)):
        assert float(t4[~visited].abs().max() if bool((~visited).any()) else 0.0) == 0.0
    if with_tab:
        assert torch.equal(kout, kk.to(torch.int32))
        assert _none_nan(dhinit)
    q = bwd_long_ratios(dy, y, gates, Ws, dgi, dgh, visited, dhinit, tdir)
    _say("seg-bwd %s" % tag, **{n: v[0] for n, v in q.items()})
    assert all(v[1] for v in q.values()), q
    if with_tab:
        # rows with k = 1: dh of their one step is dy exactly, so the start-state gradient has the local carry bound
        one = (kk == 1).nonzero().flatten()
        if len(one):
            W = Ws[tdir].double()
            dgk = dgh.view(T, R, 2, 3 * H)[0, one, tdir].double()
            zdh = gates[0, one, tdir, 1].double() * dy[0, one, tdir * H:(tdir + 1) * H].double()
            bound = (3 * H + 4) * U * (dgk.abs() @ W.abs() + zdh.abs()) + TINY
            r1 = _ratio(dhinit[one], dgk @ W + zdh, bound)
            _say("seg-dhinit-k1 %s" % tag, ratio=r1)
            assert r1 <= 1.0
        assert float(dhinit[kk == 0].abs().max() if bool((kk == 0).any()) else 0.0) == 0.0
    return dy, dhinit, kout


SEG_CASES = [
    # T, P, k per (dialogue, speaker) column, blocks of BP rows, truncated direction, start table
    (24, 4, [0, 24, 1, 7, 3, 0, 2, 19], 2, 1, True),
    (24, 4, [0, 24, 1, 7, 3, 0, 2, 19], 2, 0, False),
    (24, 4, [0, 24, 1, 7, 3, 0, 2, 19], 1, 1, False),
    (24, 4, [0, 24, 1, 7, 3, 0, 2, 19], 1, -1, False),
    (9, 1, [9, 0, 1, 4], 3, 1, True),
    (9, 1, [9, 0, 1, 4], 3, 0, False),
    (5, 16, [5, 0, 1, 2, 3, 4, 5, 0, 0, 1, 1, 2, 5, 5, 3, 0], 2, 1, True),
    (5, 16, [5, 0, 1, 2, 3, 4, 5, 0, 0, 1, 1, 2, 5, 5, 3, 0], 2, 0, False),
    (1, 2, [1, 0, 1, 1], 1, 1, True),
]


@gpu
@pytest.mark.parametrize("T,P,k,nblocks,tdir,with_tab", SEG_CASES)
def test_segmented_entry_points(T, P, k, nblocks, tdir, with_tab):
    """mmdfn_gru_seq_fwd_seg / _bwd_seg with hand-built rank arrays: speakers with k = 0 (skipped in both directions),
    k = 1, k = T; P = 1 and P = 16; either direction truncated; the reverse direction started from a table."""
    check_segmented(T, P, k, nblocks, tdir, with_tab, 700 + T + P, "T=%d P=%d tdir=%d tab=%d" % (T, P, tdir, with_tab))


@gpu
@pytest.mark.parametrize("tdir,with_tab", [(1, True), (0, False)])
def test_segmented_entry_points_at_the_schedule_limit(tdir, with_tab):
    """P * T = 2 048, the most the entry points accept: one dialogue whose 16 speakers all run the full 128 steps (a merged
    chain of exactly 2 048 steps) next to one with an ordinary split."""
    k = [128] * 16 + [0, 1, 2, 3, 5, 8, 13, 21, 30, 0, 7, 7, 11, 4, 9, 7]
    check_segmented(128, 16, k, 1, tdir, with_tab, 750, "T=128 P=16 tdir=%d" % tdir)


@gpu
@pytest.mark.parametrize("env", [{"MMDFN_GRU_IO": "0", "MMDFN_GRU_KPART_BWD": "0"}], ids=_fid)
def test_segmented_entry_points_on_the_many_chain_kernels(env, kernel_variants):
    for name, v in env.items():
        kernel_variants.setenv(name, v)
    for T, P, k, nblocks, tdir, with_tab in SEG_CASES[:2] + SEG_CASES[4:5] + SEG_CASES[6:7]:
        check_segmented(T, P, k, nblocks, tdir, with_tab, 760 + T + P, "4wave T=%d P=%d tdir=%d" % (T, P, tdir))


@gpu
@pytest.mark.parametrize("what", ["tab_with_tdir0", "tab_without_rank", "P17", "BP_not_multiple_of_P", "rows_not_multiple_of_BP",
                                  "PT_over_2048", "tdir2", "init_without_kout", "init_with_tdir0"])
def test_segmented_entry_points_refuse(what):
    T, P, BP, R = 4, 2, 4, 8
    k = [1, 2, 0, 4]
    Ws, bs = make_weights(1, 0.3)
    ytab = torch.zeros(T, 1, 2 * H)
    seg = dict(rank=[_rank_from_k(T, k)], P=[P], BP=[BP], tdir=[1], ytab=[None])
    bseg = dict(seg, want_init=[False])
    fwd = bwd = True
    if what == "tab_with_tdir0":
        seg.update(tdir=[0], ytab=[ytab]); bwd = False
    elif what == "tab_without_rank":
        seg.update(rank=[None], ytab=[ytab]); bwd = False
    elif what == "P17":
        T = 4; seg.update(P=[17], BP=[17]); bseg.update(P=[17], BP=[17]); R = 17
        seg["rank"] = bseg["rank"] = [_rank_from_k(T, [1] * 17)]
    elif what == "BP_not_multiple_of_P":
        seg.update(P=[3]); bseg.update(P=[3])
    elif what == "rows_not_multiple_of_BP":
        R = 6
    elif what == "PT_over_2048":
        T, P, BP, R = 129, 16, 16, 16
        seg = dict(rank=[_rank_from_k(T, [1] * 16)], P=[16], BP=[16], tdir=[1], ytab=[None])
        bseg = dict(seg, want_init=[False])
    elif what == "tdir2":
        seg.update(tdir=[2]); bseg.update(tdir=[2])
    elif what == "init_without_kout":
        bseg.update(want_init=[True], want_kout=[False]); fwd = False
    elif what == "init_with_tdir0":
        bseg.update(tdir=[0], want_init=[True]); fwd = False
    if fwd:
        (y, gates), = launch_fwd([(make_gi(1, T, R), Ws, bs)], seg=seg, rc_want=-1)
        assert _all_nan(y, gates)
    if bwd:
        (dgi, dgh, dhinit, kout), = launch_bwd([make_saved(1, T, R) + (Ws,)], seg=bseg, rc_want=-1)
        assert _all_nan(dgi, dgh) and (dhinit is None or _all_nan(dhinit)) and (kout is None or bool((kout == -7).all()))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the table reduction
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("T", [1, 33])
@pytest.mark.parametrize("R", [1, 1023, 1024, 1025])
def test_table_reduction(R, T, d):
    """dyt[t][dir half] = sum_{rows: k <= t} dy[t][row] + sum_{rows: k == t >= 1} dhinit[row], the other half zero; rows at
    the block width, a row with k = 0 and one with k = T; the excluded rows hold NaN (they must be selected, not multiplied)."""
    g = torch.Generator().manual_seed(R + T + d)
    dy = torch.randn(T, R, 2 * H, generator=g)
    dhinit = torch.randn(R, H, generator=g)
    k = torch.randint(0, T + 1, (R,), generator=g)
    k[0] = 0
    k[R - 1] = T
    if R > 2:
        k[1] = min(1, T)
    live = k.view(1, R) <= torch.arange(T).view(T, 1)                 # (T, R): dy[t][row] is part of the sum
    start = (k.view(1, R) == torch.arange(T).view(T, 1)) & (k.view(1, R) >= 1)
    half = dy[:, :, d * H:(d + 1) * H].double()
    want = (half * live.unsqueeze(-1)).sum(1) + (dhinit.double().unsqueeze(0) * start.unsqueeze(-1)).sum(1)
    mag = (half.abs() * live.unsqueeze(-1)).sum(1) + (dhinit.double().abs().unsqueeze(0) * start.unsqueeze(-1)).sum(1)
    dyp = dy.clone()
    dyp.view(T, R, 2, H)[:, :, d][~live] = NAN                          # what the sum excludes may hold anything
    dyp.view(T, R, 2, H)[:, :, 1 - d] = NAN
    dhp = dhinit.clone()
    dhp[~start.any(0)] = NAN
    out = Guarded((T, 1, 2 * H))
    dyd, kd, dhd = dyp.to(DEV), k.to(torch.int32).to(DEV), dhp.to(DEV)
    rc = _hip.lib().mmdfn_gru_tab_reduce(_hip.ptr(dyd), _hip.ptr(kd), _hip.ptr(dhd), _hip.ptr(out.t), R, T, H, d, _hip.stream())
    got, = _finish([out])
    assert rc == 0
    got = got.view(T, 2, H)
    assert float(got[:, 1 - d].abs().max()) == 0.0 and _none_nan(got)
    q = _ratio(got[:, d], want, (R + 2) * U * mag + TINY)
    _say("tab-reduce R=%d T=%d dir=%d" % (R, T, d), ratio=q)
    assert q <= 1.0
    for bad in (dict(R=0), dict(T=0), dict(Hv=99), dict(d=2), dict(d=-1)):
        out = Guarded((T, 1, 2 * H))
        rc = _hip.lib().mmdfn_gru_tab_reduce(_hip.ptr(dyd), _hip.ptr(kd), _hip.ptr(dhd), _hip.ptr(out.t), bad.get("R", R),
                                             bad.get("T", T), bad.get("Hv", H), bad.get("d", d), _hip.stream())
        res, = _finish([out])
        assert rc == -1 and _all_nan(res)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the module-level test of tests/test_gru_gpu.py against the float64 oracle (same shapes, same tolerances)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shapes", [[(7, 3)], [(1, 5)], [(110, 16), (110, 96)], [(33, 40), (33, 700)], [(20, 300)],
                                    [(12, 1), (5, 2), (9, 130)]])
def test_bigru2_forward_backward_against_the_float64_oracle(shapes):
    """test_gru_gpu.test_bigru2_forward_backward with the oracle evaluated in float64: the tolerances no longer have to
    absorb the oracle's own fp32 rounding."""
    import mmdfn_oracle as O
    from mm_dfn_amd import gru as fused
    from mm_dfn_amd import synthetic
    from util import abs_err, rel_err
    rs = np.random.RandomState(len(shapes) * 100 + shapes[0][0])
    grus = []
    for i in range(len(shapes)):
        g = torch.nn.GRU(200, 100, num_layers=2, bidirectional=True)
        g.load_state_dict(synthetic.seeded_state_dict(g.state_dict(), 50 + i, scale=1.5))
        grus.append(g)
    xs = [torch.from_numpy(rs.randn(T, R, 200).astype(np.float32)) for T, R in shapes]
    ws = [torch.from_numpy(rs.randn(T, R, 200).astype(np.float32)) for T, R in shapes]
    want, wgrads, xgrads = [], [], []
    for g, x, w in zip(grus, xs, ws):
        params = {"g." + k: v.detach().double().clone().requires_grad_(True) for k, v in g.state_dict().items()}
        xo = x.double().clone().requires_grad_(True)
        y = O.bigru2(xo, params, "g.", engine="manual")
        (y * w.double()).sum().backward()
        want.append(y.detach())
        wgrads.append({k[2:]: v.grad for k, v in params.items()})
        xgrads.append(xo.grad)
    gd = [g.to(DEV) for g in grus]
    xg = [x.to(DEV).requires_grad_(True) for x in xs]
    ys = fused.bigru2(xg, gd, 0.0, True)
    sum((y * w.to(DEV)).sum() for y, w in zip(ys, ws)).backward()
    for i in range(len(shapes)):
        assert abs_err(ys[i], want[i]) < 2e-6
        assert rel_err(xg[i].grad, xgrads[i]) < 2e-5
        for k, p in gd[i].named_parameters():
            assert rel_err(p.grad, wgrads[i][k]) < 5e-5, k
