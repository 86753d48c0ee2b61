"""The fused LSTM recurrence (K16: csrc/lstm_seq.hip) against a float64 restatement, step by step.

The C entry points are called directly (mmdfn_lstm_seq_fwd / _bwd); the reference is the contract of include/mmdfn_hip.h
restated here in float64 on the CPU, independent of oracle/ and of torch's LSTM:

    a = W_hh h + b_hh + gi;  i, f, o = sig(a_i, a_f, a_o);  g = tanh(a_g);  c' = f c + i g;  y = h' = o tanh(c')
    tc = tanh(c');  do = dh tc o (1-o);  dc = dc_carry + dh o (1 - tc^2);  di = dc g i (1-i);  df = dc c_prev f (1-f);
    dg = dc i (1 - g^2);  dc_carry' = dc f;  dh_prev = dy_prev + dgate W_hh

Nothing below is fitted to what the kernels return.  u = 2^-24 is the fp32 unit roundoff, K = H = 100.  The method and the
first two bounds are tests/test_gru_recurrence_kernels_gpu.py's.

FORWARD: ONE-STEP RESIDUALS.  For every (t, row, direction) the kernel's OWN previous h (from y) and c (from state) are
taken as float64, one float64 step is evaluated, and the kernel's i, f, g, o, c, y are compared element by element.  With
S = |W_hh| |h| + |b_hh| (per gate row):

  E_a   a K-term fp32 dot product in any order (FMA or not) is within K u sum|w h| of the exact one, the bias adds one
        rounding, one u is slack: (K + 2) u S.
  E_x   the pre-activation x = a + gi adds one rounding u |x| <= u (|gi| + S):   E_x = E_a + u (|gi| + S).
  E_s   (i, f, o)  |sig'| <= 1/4; the evaluation rcp(1 + exp(-x)): exp's argument scaling and its ulp move e = exp(-x) by
        (|x| + 2) u relative, i.e. sig by sig (1 - sig)(|x| + 2) u <= 0.73 u; rounding 1 + e moves sig by <= u; rcp's ulp is
        <= u of a result in (0, 1]: 2.73 u, stated as 4 u.                        E_s = E_x / 4 + 4 u.
  E_g   |tanh'| <= 1.  The evaluation 1 - 2 rcp(1 + exp(2x)) with t = 2 / (1 + e) in [0, 2]: e's relative error moves t by
        t (1 - t/2)(|2x| + 2) u <= 1.45 u (the maximum over all x), rounding 1 + e by <= 2 u, rcp's ulp by <= 2 u, the final
        subtraction by u / 2: 5.95 u, stated as 6 u, for ANY argument.             E_g = E_x + 6 u.
  E_c   c' = f c + i g from the kernel's own rounded f, i, g (c is exact: it is the kernel's saved value): the first-order
        terms E_f |c| + E_i |g| + E_g |i|, the cross term E_i E_g, and two products and a sum (or one product and an
        FMA), each at most one rounding of a magnitude <= |f c| + |i g|:
                                                   E_c = E_f |c| + E_i |g| + E_g |i| + E_i E_g + 3 u (|f c| + |i g|).
  E_y   tc = tanh(c') evaluated at the kernel's c': E_tc = E_c (|tanh'| <= 1) + 6 u (the evaluation, as for g); then one
        product:                                   E_y = E_o |tc| + E_tc |o| + E_o E_tc + 2 u |o tc|.
  E_s and E_g are derived for the cheapest honest evaluation (hardware exp / rcp, the GRU kernels' forms).  K16 itself uses
  libm's expf with a true division and libm's tanhf (csrc/lstm_seq.hip), which sit inside them: expf within 1 ulp moves sig by
  sig (1 - sig) 2 u <= u / 2, rounding 1 + e and the correctly rounded quotient by <= u each: 2.5 u <= 4 u; tanhf within 2 ulp
  of a result in [-1, 1]: 4 u <= 6 u.  The bounds are not tightened to the implementation.
Every bound also carries 2^-126 (results below the smallest normal fp32 may be flushed).
A float32 numpy restatement of the same formulas stays inside these bounds and above zero
(test_bounds_hold_for_a_float32_restatement: no device needed), so they are neither violated by honest fp32 nor vacuous.

BACKWARD, LOCAL (T = 1, 2; state and dy are plain inputs, so they are synthetic here).  The first step processed has
dh = dy exactly and dc_carry = 0 (E_dh = E_cc = 0).  The kernel recomputes tc = tanh(c) (E_tc = 6 u, absolute, as above).
B = 1 - tc^2: tc's error moves it by (2 |tc| + E_tc) E_tc, and forming it (tc^2 rounded, then subtracted, or one FMA) by
u (tc^2 + |B|) -- the absolute form, NOT small next to B when |tc| -> 1.  G = 1 - g^2 from the saved g: u (g^2 + |G|).
    E_do = E_dh |tc o (1-o)| + E_tc |dh o (1-o)| + 6 u |do|                       (five roundings, all relative)
    E_dc = E_cc + E_dh |o B| + |dh o| E_B + 4 u (|dc_carry| + |dh o B|)           (two products, one sum)
    E_di = E_dc |g i (1-i)| + 6 u |di|
    E_df = E_dc |c_prev f (1-f)| + 6 u |df|
    E_dg = E_dc |i G| + |dc i| E_G + 6 u |dg|
At T = 2 the second step sees dh = dy + dgate_1 W_hh: one 4H = 400-term contraction of the kernel's OWN dgate of the first
step (read back, so its error does not compound) and the sum with dy:
    E_dh = (4H + 4) u (|dgate_1| |W_hh|) + u (|dy| + |dgate_1| |W_hh|),
and dc_carry = dc_1 f_1, where dc_1 is not an output: the float64 dc_1 with its own bound E_dc (above, first step) is used,
    E_cc = E_dc1 |f_1| + u |dc_1 f_1|.
Every bound also carries 2^-126.

BACKWARD AT LENGTH (T = 33, 110).  No local bound exists (dh and dc of an inner step are not outputs), so the kernel is
calibrated against honest fp32: both the kernel and a float32 CPU restatement of the same recurrence run on the kernel's own
saved forward values and are compared with float64, max-norm per tensor; the kernel's error must be
<= 4 e_ref + 8 u max|want| (the project's precedent in tests/test_gru_recurrence_kernels_gpu.py).

Saturation: sig is exactly 1 at pre-activations of +30 and +100 and exactly 0 at -100 (exp overflows to inf, rcp(inf) = 0);
at -30 the exact value is 9.4e-14, which fp32 represents, so there the tests assert the E_s bound and 0 < sig < 1e-9, not
an exact zero.  tanh is exactly +-1 at all four.  tanh(c) is exactly 1 once 2 / (1 + e^{2c}) < 2^-25, i.e. from c = 10 on.

Measured ratios of every check: profiles/lstm_recurrence_parity.md (the tests print them: pytest -s).
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
GATES = ("i", "f", "g", "o")


def _say(tag, **kv):
    print("LSTM-PARITY %s %s" % (tag, " ".join("%s=%.3g" % (k, v) for k, v in kv.items())), flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement and bounds (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _shift(x, d):
    """The value of the step processed before, for every step of direction d, from x (T, R, H): zero at the start."""
    z = torch.zeros_like(x[:1])
    return torch.cat([z, x[:-1]]) if d == 0 else torch.cat([x[1:], z])


def step64(gi, h, c, W, b):
    """One float64 step for gi (..., 4H), h, c (..., H): ({i, f, g, o, c, y}, the per-element bounds of the docstring)."""
    gi, h, c, W, b = gi.double(), h.double(), c.double(), W.double(), b.double()
    a = h @ W.t() + b
    S = h.abs() @ W.abs().t() + b.abs()
    Ex = (H + 2) * U * S + U * (gi.abs() + S)
    x = a + gi
    k = lambda t, j: t[..., j * H:(j + 1) * H]
    i, f, g, o = torch.sigmoid(k(x, 0)), torch.sigmoid(k(x, 1)), torch.tanh(k(x, 2)), torch.sigmoid(k(x, 3))
    Ei, Ef, Eo = (0.25 * k(Ex, j) + 4 * U + TINY for j in (0, 1, 3))
    Eg = k(Ex, 2) + 6 * U + TINY
    cn = f * c + i * g
    Ec = Ef * c.abs() + Ei * g.abs() + Eg * i.abs() + Ei * Eg + 3 * U * ((f * c).abs() + (i * g).abs()) + TINY
    tc = torch.tanh(cn)
    Etc = Ec + 6 * U
    y = o * tc
    Ey = Eo * tc.abs() + Etc * o.abs() + Eo * Etc + 2 * U * y.abs() + TINY
    return dict(i=i, f=f, g=g, o=o, c=cn, y=y), dict(i=Ei, f=Ef, g=Eg, o=Eo, c=Ec, y=Ey)


def _ratio(got, want, bound):
    """max over the elements of |got - want| / bound; 0 / 0 counts as 0, a non-finite value as inf."""
    got = got.double()
    err = (got - want).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    q = torch.where(torch.isfinite(got), q, torch.full_like(q, float("inf")))
    return float(q.max()) if q.numel() else 0.0


def forward_ratios(gi, Ws, bs, y, state):
    """Teacher-forced residuals: {quantity: worst |kernel - float64 step| / bound} over both directions."""
    T, R = gi.shape[:2]
    gi4 = gi.reshape(T, R, 2, 4 * H)
    out = {}
    for d in range(2):
        yd, cd = y[..., d * H:(d + 1) * H], state[:, :, d, 4]
        want, bound = step64(gi4[:, :, d], _shift(yd, d), _shift(cd, d), Ws[d], bs[d])
        got = dict(i=state[:, :, d, 0], f=state[:, :, d, 1], g=state[:, :, d, 2], o=state[:, :, d, 3], c=cd, y=yd)
        for k in want:
            out[k] = max(out.get(k, 0.0), _ratio(got[k], want[k], bound[k]))
    return out


def fwd32(gi, Ws, bs):
    """float32 numpy restatement of the forward recurrence with the kernels' gate formulas: (y, state)."""
    gi = gi.numpy()
    T, R = gi.shape[:2]
    gi4 = gi.reshape(T, R, 2, 4 * H)
    y = np.zeros((T, R, 2 * H), np.float32)
    state = np.zeros((T, R, 2, 5, H), np.float32)
    one, two = np.float32(1), np.float32(2)
    sig = lambda x: one / (one + np.exp(-x))
    tanh = lambda x: one - two / (one + np.exp(two * x))
    with np.errstate(over="ignore"):
        for d in range(2):
            W, b = Ws[d].numpy(), bs[d].numpy()
            h = np.zeros((R, H), np.float32)
            c = np.zeros((R, H), np.float32)
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                x = (h @ W.T + b) + gi4[t, :, d]
                i, f, g, o = sig(x[:, :H]), sig(x[:, H:2 * H]), tanh(x[:, 2 * H:3 * H]), sig(x[:, 3 * H:])
                c = f * c + i * g
                h = o * tanh(c)
                y[t, :, d * H:(d + 1) * H] = h
                for k, v in enumerate((i, f, g, o, c)):
                    state[t, :, d, k] = v
    return torch.from_numpy(y), torch.from_numpy(state)


def _tanh_like_kernel(c):
    """tanh in c's dtype; in float32 by the plain formula 1 - 2 / (1 + exp(2c)) (honest fp32, not the kernels' libm call)."""
    if c.dtype == torch.float64:
        return torch.tanh(c)
    return 1.0 - 2.0 / (1.0 + torch.exp(2.0 * c))


def _bwd_step(dh, dcc, i, f, g, o, c, cp):
    tc = _tanh_like_kernel(c)
    d_o = dh * tc * o * (1 - o)
    dc = dcc + dh * o * (1 - tc * tc)
    return dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), d_o, dc


def bwd_ref(dy, state, Ws, dtype):
    """The backward recurrence in ``dtype`` on the given saved values: dgate (T, R, 2, 4H)."""
    T, R = dy.shape[:2]
    dgate = torch.zeros(T, R, 2, 4 * H, dtype=dtype)
    st = state.to(dtype)
    for d in range(2):
        W = Ws[d].to(dtype)
        cprev = _shift(st[:, :, d, 4], d)
        rec = torch.zeros(R, H, dtype=dtype)
        dcc = torch.zeros(R, H, dtype=dtype)
        for t in (range(T - 1, -1, -1) if d == 0 else range(T)):
            dh = dy[t, :, d * H:(d + 1) * H].to(dtype) + rec
            i, f, g, o, c = (st[t, :, d, k] for k in range(5))
            di, df, dg, d_o, dc = _bwd_step(dh, dcc, i, f, g, o, c, cprev[t])
            dgt = torch.cat([di, df, dg, d_o], -1)
            dgate[t, :, d] = dgt
            rec = dgt @ W
            dcc = dc * f
    return dgate


def bwd_local_ratios(dy, state, Ws, dgate):
    """T <= 2: every element of dgate against the float64 step under the local bounds of the module docstring."""
    T, R = dy.shape[:2]
    assert T <= 2
    dy, st = dy.double(), state.double()
    dgate = dgate.reshape(T, R, 2, 4 * H)
    out = {}
    for d in range(2):
        W = Ws[d].double()
        cprev = _shift(st[:, :, d, 4], d)
        order = list(range(T - 1, -1, -1)) if d == 0 else list(range(T))
        zero = torch.zeros(R, H, dtype=torch.float64)
        dh, Edh, dcc, Ecc = dy[order[0], :, d * H:(d + 1) * H], zero, zero, zero
        for n, t in enumerate(order):
            if n == 1:
                dg1 = dgate[order[0], :, d].double()
                mag = dg1.abs() @ W.abs()
                dyt = dy[t, :, d * H:(d + 1) * H]
                Edh = (4 * H + 4) * U * mag + U * (dyt.abs() + mag)
                dh = dyt + dg1 @ W
                f1 = st[order[0], :, d, 1]
                dcc = dc * f1
                Ecc = Edc * f1.abs() + U * dcc.abs()
            i, f, g, o, c = (st[t, :, d, k] for k in range(5))
            cp = cprev[t]
            tc = torch.tanh(c)
            Etc = 6 * U
            B, G = 1 - tc * tc, 1 - g * g
            EB = (2 * tc.abs() + Etc) * Etc + U * (tc * tc + B.abs())
            EG = U * (g * g + G.abs())
            di, df, dg, d_o, dc = _bwd_step(dh, dcc, i, f, g, o, c, cp)
            Edo = Edh * (tc * o * (1 - o)).abs() + Etc * (dh * o * (1 - o)).abs() + 6 * U * d_o.abs() + TINY
            Edc = Ecc + Edh * (o * B).abs() + (dh * o).abs() * EB + 4 * U * (dcc.abs() + (dh * o * B).abs()) + TINY
            Edi = Edc * (g * i * (1 - i)).abs() + 6 * U * di.abs() + TINY
            Edf = Edc * (cp * f * (1 - f)).abs() + 6 * U * df.abs() + TINY
            Edg = Edc * (i * G).abs() + (dc * i).abs() * EG + 6 * U * dg.abs() + TINY
            got = dgate[t, :, d]
            for j, (name, want, bound) in enumerate((("di", di, Edi), ("df", df, Edf), ("dg", dg, Edg), ("do", d_o, Edo))):
                key = name if n == 0 else name + "@2"
                out[key] = max(out.get(key, 0.0), _ratio(got[:, j * H:(j + 1) * H], want, bound))
    return out


def bwd_long_ratios(dy, state, Ws, dgate):
    """(kernel error / e_ref, e_ref, passes): e_ref = the error of the float32 CPU restatement against float64 on the same
    inputs; passes: kernel error <= 4 e_ref + 8 u max|want|."""
    T, R = dy.shape[:2]
    want = bwd_ref(dy, state, Ws, torch.float64)
    ref = bwd_ref(dy, state, Ws, torch.float32)
    got = dgate.reshape(T, R, 2, 4 * H)
    assert bool(torch.isfinite(got).all())
    ek, er, top = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max()), float(want.abs().max())
    return (ek / er if er > 0 else (0.0 if ek == 0 else float("inf"))), er, ek <= 4 * er + 8 * U * top


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_weights(seed, wscale, bscale=None):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.uniform(-1, 1, size=s).astype(np.float32))
    return [f(4 * H, H) * wscale for _ in range(2)], [f(4 * H) * (wscale if bscale is None else bscale) for _ in range(2)]


def make_gi(seed, T, R, scales=(0.01, 1.0, 1.0, 30.0), zero_row=True):
    """randn times a per-element scale drawn from ``scales`` (tiny, ordinary and saturating pre-activations side by side);
    one row of all zeros next to the ordinary ones."""
    g = torch.Generator().manual_seed(seed)
    gi = torch.randn(T, R, 8 * H, generator=g)
    sc = torch.tensor(scales)[torch.randint(len(scales), (T, R, 8 * H), generator=g)]
    gi = gi * sc
    if zero_row and R >= 2:
        gi[:, R // 2] = 0.0
    return gi


def make_saved(seed, T, R, edges=True):
    """Synthetic (dy, state) for the backward: i, f, o in [0, 1], g in [-1, 1], c ~ 2 N(0, 1); with ``edges`` the exactly
    saturated values in fixed unit ranges and one row of all zeros."""
    gen = torch.Generator().manual_seed(seed)
    dy = torch.randn(T, R, 2 * H, generator=gen)
    state = torch.rand(T, R, 2, 5, H, generator=gen)
    state[:, :, :, 2] = state[:, :, :, 2] * 2 - 1
    state[:, :, :, 4] = 2 * torch.randn(T, R, 2, H, generator=gen)
    if edges:
        state[:, :, :, 0, 0:5] = 0.0            # i = 0
        state[:, :, :, 0, 5:10] = 1.0           # i = 1
        state[:, :, :, 1, 10:15] = 1.0          # f = 1
        state[:, :, :, 1, 15:20] = 0.0          # f = 0
        state[:, :, :, 2, 20:25] = 1.0          # g = +-1
        state[:, :, :, 2, 25:30] = -1.0
        state[:, :, :, 2, 30:35] = 1.0 - 2.0 ** -24          # 1 - g^2 is all cancellation
        state[:, :, :, 3, 35:40] = 0.0          # o = 0
        state[:, :, :, 3, 40:45] = 1.0          # o = 1
        state[:, :, :, 4, 45:50] = 12.0         # tanh(c) = 1 exactly: 1 - tc^2 = 0
        state[:, :, :, 4, 50:55] = -15.0
        state[:, :, :, 4, 55:60] = 1e-4         # tanh in its cancellation region
        if R >= 2:
            dy[:, R // 2] = 0.0
            state[:, R // 2] = 0.0
    return dy, state


# ---------------------------------------------------------------------------------------------------------------------
# launches: every output is prefilled with NaN and sits in a larger buffer -- 256 floats in front, one extra row block
# (what one timestep writes) behind -- whose margins hold a fixed bit pattern that must be untouched afterwards
# ---------------------------------------------------------------------------------------------------------------------
PATTERN = 0x5A5AA5A5
LEAD = 256


class Guarded:
    def __init__(self, shape):
        n = int(np.prod(shape))
        self.n, self.tail = n, max(256, (n // shape[0] + 3) & ~3)
        self.buf = torch.full((LEAD + n + self.tail,), PATTERN, dtype=torch.int32, device=DEV)
        self.t = self.buf[LEAD:LEAD + n].view(torch.float32).view(shape)
        self.t.fill_(NAN)

    def margins_intact(self):
        return bool((self.buf[:LEAD] == PATTERN).all()) and bool((self.buf[LEAD + self.n:] == PATTERN).all())


def _dev(ts):
    return [t.to(DEV).contiguous() for t in ts]


def _finish(outs):
    torch.cuda.synchronize()
    for o in outs:
        assert o.margins_intact(), "a kernel wrote outside its output"
    return [o.t.cpu() for o in outs]


def launch_fwd(gi, Ws, bs):
    T, R = gi.shape[:2]
    gid, Wd, bd = _dev([gi])[0], _dev(Ws), _dev(bs)
    y, st = Guarded((T, R, 2 * H)), Guarded((T, R, 2, 5, H))
    _hip.call("mmdfn_lstm_seq_fwd", _hip.ptr(gid), _hip.ptr_array(Wd), _hip.ptr_array(bd), _hip.ptr(y.t), _hip.ptr(st.t),
              R, T, H, _hip.stream())
    return _finish([y, st])


def launch_bwd(dy, y, state, Ws):
    T, R = dy.shape[:2]
    dyd, yd, sd = _dev([dy, y, state])
    Wd = _dev(Ws)
    dg = Guarded((T, R, 8 * H))
    _hip.call("mmdfn_lstm_seq_bwd", _hip.ptr(dyd), _hip.ptr(yd), _hip.ptr(sd), _hip.ptr_array(Wd), _hip.ptr(dg.t),
              R, T, H, _hip.stream())
    return _finish([dg])[0]


def _finite(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _bits(t):
    return t.contiguous().view(torch.int32)


def check_forward(T, R, seed, wscale, tag, scales=(0.01, 1.0, 1.0, 30.0)):
    Ws, bs = make_weights(seed, wscale)
    gi = make_gi(seed + 1, T, R, scales)
    y, state = launch_fwd(gi, Ws, bs)
    assert _finite(y, state), "an element was not written, or is not finite"
    rat = forward_ratios(gi, Ws, bs, y, state)
    _say("fwd %s w=%g" % (tag, wscale), **rat)
    assert max(rat.values()) <= 1.0, rat
    return gi, Ws, bs, y, state


def check_backward_local(T, R, seed, wscale, tag):
    assert T <= 2
    dy, state = make_saved(seed, T, R)
    Ws = make_weights(seed + 1, wscale)[0]
    y = torch.rand(T, R, 2 * H, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    dgate = launch_bwd(dy, y, state, Ws)
    assert _finite(dgate)
    rat = bwd_local_ratios(dy, state, Ws, dgate)
    _say("bwd-local %s w=%g" % (tag, wscale), **rat)
    assert max(rat.values()) <= 1.0, rat
    # exactly saturated saved values pass exactly nothing through their own factor
    d5 = dgate.view(T, R, 2, 4, H)
    assert float(d5[:, :, :, 0, 0:10].abs().max()) == 0.0            # i in {0, 1}: i (1-i) = 0
    assert float(d5[:, :, :, 2, 0:5].abs().max()) == 0.0             # i = 0: dg = dc i (1 - g^2) = 0
    assert float(d5[:, :, :, 1, 10:20].abs().max()) == 0.0           # f in {0, 1}
    assert float(d5[:, :, :, 2, 20:30].abs().max()) == 0.0           # g = +-1: 1 - g^2 = 0
    assert float(d5[:, :, :, 3, 35:45].abs().max()) == 0.0           # o in {0, 1}
    # tanh(c) = +-1 exactly, so 1 - tc^2 = 0: the first step processed (dc_carry = 0) has dc = 0, its do does not vanish
    for d, t0 in ((0, T - 1), (1, 0)):
        assert float(d5[t0, :, d, :3, 45:55].abs().max()) == 0.0
        live = [r for r in range(R) if R < 2 or r != R // 2]
        assert float(d5[t0, live, d, 3, 45:55].abs().min()) > 0.0
    return dy, state, Ws, dgate


def check_backward_long(T, R, seed, wscale, tag):
    gi, Ws, bs, y, state = check_forward(T, R, seed, wscale, tag)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 2))
    dgate = launch_bwd(dy, y, state, Ws)
    q, er, ok = bwd_long_ratios(dy, state, Ws, dgate)
    _say("bwd-long %s w=%g" % (tag, wscale), kernel_over_ref=q, e_ref=er)
    assert ok, (q, er)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the bounds themselves
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wscale", [0.1, 0.3, 1.0])
def test_bounds_hold_for_a_float32_restatement(wscale):
    """An honest fp32 evaluation of the contract (numpy, the kernels' gate formulas, 110 steps, tiny / ordinary / saturating
    pre-activations) stays inside every forward bound and above zero: the bounds are neither violated by legitimate rounding
    nor vacuous; a wrong step is far outside."""
    Ws, bs = make_weights(3, wscale)
    worst = {}
    for giscale in (0.01, 1.0, 30.0):
        gi = make_gi(5, 110, 6, scales=(giscale,))
        y, state = fwd32(gi, Ws, bs)
        for k, v in forward_ratios(gi, Ws, bs, y, state).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if giscale == 30.0:
            s = state[:, :, :, (0, 1, 3)]
            assert float(((s == 0) | (s == 1)).float().mean()) > 0.2       # exactly saturated gates are really in the sample
    _say("cpu-f32 w=%g" % wscale, **worst)
    assert all(0.0 < v <= 1.0 for v in worst.values()), worst
    gi = make_gi(5, 9, 3, scales=(1.0,))
    y, state = fwd32(gi, Ws, bs)
    bad = state.clone()                                                    # b_hh left out of the o gate
    x = torch.logit(state[:, :, :, 3].double().clamp(1e-6, 1 - 1e-6)) - torch.stack([bs[0][3 * H:], bs[1][3 * H:]]).double()
    bad[:, :, :, 3] = torch.sigmoid(x).float()
    assert forward_ratios(gi, Ws, bs, y, bad)["o"] > 100
    bad = state.clone()                                                    # a cell state off by 0.01
    bad[:, :, :, 4] = state[:, :, :, 4] + 0.01
    assert forward_ratios(gi, Ws, bs, y, bad)["c"] > 100


def test_backward_restatements_agree_and_the_local_bounds_hold_for_float32():
    """The float64 backward recurrence against torch autograd of the float64 forward (the contract's two halves are
    consistent), and its float32 evaluation inside the local T = 1, 2 bounds and the at-length criterion."""
    Ws, bs = make_weights(7, 0.3)
    T, R = 5, 3
    gi = make_gi(8, T, R, scales=(1.0,), zero_row=False).double().requires_grad_(True)
    Wd = [w.double() for w in Ws]
    ys, saved = [], []
    for d in range(2):
        h = torch.zeros(R, H, dtype=torch.float64)
        c = torch.zeros(R, H, dtype=torch.float64)
        outs, gs = [None] * T, [None] * T
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            want, _ = step64(gi[t].view(R, 2, 4 * H)[:, d], h, c, Wd[d], bs[d])
            h, c = want["y"], want["c"]
            outs[t] = h
            gs[t] = torch.stack([want[k] for k in ("i", "f", "g", "o", "c")], 1)
        ys.append(torch.stack(outs))
        saved.append(torch.stack(gs))
    y = torch.cat(ys, -1)
    state = torch.stack(saved, 2)
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(1)).double()
    (y * dy).sum().backward()
    dgate = bwd_ref(dy, state.detach(), Ws, torch.float64)
    assert float((dgate.view(T, R, 8 * H) - gi.grad).abs().max()) < 1e-12 * float(gi.grad.abs().max())
    for T in (1, 2):
        dy, state = make_saved(11 + T, T, 4)
        g32 = bwd_ref(dy, state, Ws, torch.float32)
        rat = bwd_local_ratios(dy, state, Ws, g32)
        _say("cpu-f32 bwd-local T=%d" % T, **rat)
        assert 0.0 < max(rat.values()) <= 1.0, rat
        bad = g32.clone()
        bad[..., 2 * H:3 * H] = g32[..., 2 * H:3 * H] * 1.001            # dg off by a part in a thousand
        assert bwd_local_ratios(dy, state, Ws, bad)["dg"] > 100
    dy, state = make_saved(21, 33, 2, edges=False)
    q, er, ok = bwd_long_ratios(dy, state, Ws, bwd_ref(dy, state, Ws, torch.float32))
    assert ok and q == 1.0 and er > 0


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 1), (2, 3), (7, 2), (8, 1), (9, 5), (17, 3)]


@gpu
@pytest.mark.parametrize("T,R", SHAPES)
def test_forward_steps(T, R):
    for wscale in (0.3, 0.0):
        check_forward(T, R, 100 + T, wscale, "T=%d R=%d" % (T, R))


@gpu
def test_forward_and_backward_at_the_staging_block_edges():
    """T = TB-1, TB, TB+1, 2TB+1 for the kernels' own block length (mmdfn_lstm_seq_block_steps), 3 rows."""
    TB = int(_hip.query("mmdfn_lstm_seq_block_steps"))
    assert TB >= 1
    for T in sorted({max(1, TB - 1), TB, TB + 1, 2 * TB + 1}):
        check_backward_long(T, 3, 150 + T, 0.3, "block-edge T=%d R=3" % T)


@gpu
@pytest.mark.parametrize("T,R", [(1, 1), (2, 1), (1, 3), (2, 3), (2, 5)])
def test_backward_local_steps(T, R):
    for wscale in (0.3, 0.0):
        check_backward_local(T, R, 200 + T, wscale, "T=%d R=%d" % (T, R))


@gpu
@pytest.mark.parametrize("wscale", [0.1, 0.3])
@pytest.mark.parametrize("T,R", [(33, 2), (110, 3)] + SHAPES[2:])
def test_backward_at_length_against_the_float32_restatement(T, R, wscale):
    check_backward_long(T, R, 300 + T + R, wscale, "T=%d R=%d" % (T, R))


@gpu
def test_large_weights_saturate_the_recurrence():
    """W_hh ~ U(-10, 10): the gates saturate from the recurrence itself.  |h| = |o tanh(c)| is about 1/2 where the gates are not
    yet saturated, so a pre-activation is a sum of 100 terms of variance ~ (100 / 3) / 4: a standard deviation of ~ 29, and fp32
    rounds sig to exactly 1 from 17.4 on (e^-x < 2^-25) -- a quarter of the i, f, o values; the sample must hold > 2 %."""
    gi, Ws, bs, y, state = check_forward(33, 3, 500, 10.0, "T=33 R=3", scales=(1.0,))
    s = state[:, :, :, (0, 1, 3)]
    assert float(((s == 0) | (s == 1)).float().mean()) > 0.02


@gpu
def test_runs_repeat_rows_are_independent_and_the_directions_are_one_code_path():
    T, R = 11, 5
    Ws, bs = make_weights(41, 0.3)
    gi = make_gi(42, T, R, zero_row=False)
    y, st = launch_fwd(gi, Ws, bs)
    y2, st2 = launch_fwd(gi, Ws, bs)
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(st), _bits(st2))
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(43))
    dg = launch_bwd(dy, y, st, Ws)
    assert torch.equal(_bits(dg), _bits(launch_bwd(dy, y, st, Ws)))
    for j in (0, R // 2, R - 1):
        ya, sa = launch_fwd(gi[:, j:j + 1], Ws, bs)
        assert torch.equal(_bits(ya), _bits(y[:, j:j + 1])) and torch.equal(_bits(sa), _bits(st[:, j:j + 1])), j
        da = launch_bwd(dy[:, j:j + 1], y[:, j:j + 1], st[:, j:j + 1], Ws)
        assert torch.equal(_bits(da), _bits(dg[:, j:j + 1])), j
    # the reverse direction on time-flipped operands with the forward weights IS the forward direction, time-flipped
    gif = gi.clone()
    gif[:, :, 4 * H:] = gi.flip(0)[:, :, :4 * H]
    yf, sf = launch_fwd(gif, [Ws[0], Ws[0]], [bs[0], bs[0]])
    assert torch.equal(_bits(yf[:, :, :H]), _bits(y[:, :, :H]))
    assert torch.equal(_bits(yf[:, :, H:]), _bits(yf[:, :, :H].flip(0)))
    assert torch.equal(_bits(sf[:, :, 1]), _bits(sf[:, :, 0].flip(0)))
    dyf = dy.clone()
    dyf[:, :, H:] = dy.flip(0)[:, :, :H]
    df = launch_bwd(dyf, yf, sf, [Ws[0], Ws[0]])
    assert torch.equal(_bits(df[:, :, 4 * H:]), _bits(df[:, :, :4 * H].flip(0)))
    assert not torch.equal(df[:, :, :4 * H], torch.zeros_like(df[:, :, :4 * H]))


@gpu
def test_saturated_pre_activations():
    """W_hh = 0, b_hh = 0: the pre-activations ARE gi.  Units 0-9 at +100, 10-19 at +30, 20-29 at -100, 30-39 at -30 in every
    gate; the rest ordinary."""
    T, R = 4, 3
    Ws, bs = make_weights(1, 0.0)
    gi5 = torch.randn(T, R, 2, 4, H, generator=torch.Generator().manual_seed(61))
    gi5[..., 0:10] = 100.0
    gi5[..., 10:20] = 30.0
    gi5[..., 20:30] = -100.0
    gi5[..., 30:40] = -30.0
    gi = gi5.reshape(T, R, 8 * H)
    y, st = launch_fwd(gi, Ws, bs)
    assert _finite(y, st)
    rat = forward_ratios(gi, Ws, bs, y, st)
    _say("saturated", **rat)
    assert max(rat.values()) <= 1.0, rat
    for k in (0, 1, 3):
        s = st[:, :, :, k]
        assert bool((s[..., 0:20] == 1.0).all()) and bool((s[..., 20:30] == 0.0).all())
        assert float(s[..., 30:40].max()) < 1e-9 and float(s[..., 30:40].min()) > 0.0          # sig(-30): tiny, not 0
    g = st[:, :, :, 2]
    assert bool((g[..., 0:20] == 1.0).all()) and bool((g[..., 20:40] == -1.0).all())
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(62))
    dg = launch_bwd(dy, y, st, Ws)
    assert _finite(dg)
    assert float(dg.view(T, R, 2, 4, H)[..., 0:30].abs().max()) == 0.0                         # every factor is exactly 0


@gpu
def test_a_cell_that_counts():
    """i = f = 1 and g = 1 exactly (pre-activations of +100, W_hh = 0) for 40 steps: c_t is the step count, exactly; from
    c = 10 on tanh(c) is exactly 1, so y is bit-equal to o; nothing is non-finite, forward or backward, and with
    1 - tc^2 = 0 and i (1-i) = f (1-f) = 1 - g^2 = 0 the backward pass writes exact zeros for di, df, dg."""
    T, R = 40, 2
    Ws, bs = make_weights(1, 0.0)
    gi5 = torch.randn(T, R, 2, 4, H, generator=torch.Generator().manual_seed(71))
    gi5[:, :, :, :3] = 100.0
    gi = gi5.reshape(T, R, 8 * H)
    y, st = launch_fwd(gi, Ws, bs)
    assert _finite(y, st)
    count = torch.arange(1, T + 1, dtype=torch.float32).view(T, 1, 1).expand(T, R, H)
    assert torch.equal(st[:, :, 0, 4], count) and torch.equal(st[:, :, 1, 4], count.flip(0))
    for k in range(3):
        assert bool((st[:, :, :, k] == 1.0).all())
    assert torch.equal(_bits(y[9:, :, :H]), _bits(st[9:, :, 0, 3]))              # forward: c >= 10 from t = 9
    assert torch.equal(_bits(y[:T - 9, :, H:]), _bits(st[:T - 9, :, 1, 3]))      # reverse: c >= 10 up to t = T - 10
    rat = forward_ratios(gi, Ws, bs, y, st)
    assert max(rat.values()) <= 1.0, rat
    dy = torch.randn(T, R, 2 * H, generator=torch.Generator().manual_seed(72))
    dg = launch_bwd(dy, y, st, Ws)
    assert _finite(dg)
    d5 = dg.view(T, R, 2, 4, H)
    assert float(d5[:, :, :, :3].abs().max()) == 0.0 and float(d5[:, :, :, 3].abs().max()) > 0.0


@gpu
def test_refused_calls_write_nothing():
    T, R = 3, 2
    Ws, bs = make_weights(1, 0.3)
    gid, Wd, bd = _dev([make_gi(1, T, R)])[0], _dev(Ws), _dev(bs)
    y, st, dg = Guarded((T, R, 2 * H)), Guarded((T, R, 2, 5, H)), Guarded((T, R, 8 * H))
    for rows, t, h in ((R, T, 99), (0, T, H), (R, 0, H)):
        assert _hip.call("mmdfn_lstm_seq_fwd", _hip.ptr(gid), _hip.ptr_array(Wd), _hip.ptr_array(bd), _hip.ptr(y.t),
                         _hip.ptr(st.t), rows, t, h, _hip.stream(), allow=(-1,)) == -1
        assert _hip.call("mmdfn_lstm_seq_bwd", _hip.ptr(y.t), _hip.ptr(y.t), _hip.ptr(st.t), _hip.ptr_array(Wd), _hip.ptr(dg.t),
                         rows, t, h, _hip.stream(), allow=(-1,)) == -1
    for o in _finish([y, st, dg]):
        assert bool(torch.isnan(o).all())
