"""The direct form of the plain eight-wave GRU backward recurrence (csrc/gru.hip gru_bwd_direct_body): every lane requests
its six operands of step s + D straight from global memory into a register ring and stores its two results itself; the
staged form it replaces (time blocks through LDS) stays selectable in the tuning library (MMDFN_GRU_BWD_STAGED=1) and is the
bit-for-bit reference here.

The shapes sit at the ring's edges (D = BWD_RING_D: the ring has D + 1 slots; T < D never enters the loop, T = D + 1 is one
whole trip with no tail, T = 8, 9, 17 leave tails of 3, 4 and 2 steps) with 1 and 3 rows.  Every operand sits inside a
NaN-filled buffer -- a request that left its array would bring a NaN into a finite result -- and every output inside a
buffer whose margins hold a bit pattern.  The float64 checks are those of test_gru_recurrence_kernels_gpu with its bounds."""
import re

import pytest
import torch

import test_gru_recurrence_kernels_gpu as K
from mm_dfn_amd import _hip

pytestmark = pytest.mark.gpu
H = K.H
D = 4                     # BWD_RING_D of csrc/gru.hip
SHAPES = [(T, R) for T in sorted({1, 2, 3, D - 1, D, D + 1, 8, 9, 17}) for R in (1, 3)]
GROUPS = [[(9, 3), (2, 17), (1, 1)], [(7, 3), (33, 5)]]
_sid = lambda s: "+".join("%dx%d" % tr for tr in s) if isinstance(s, list) else "%dx%d" % s


def _in_arena(t):
    """``t`` on the device, inside a NaN-filled buffer (MARGIN floats on either side: the alignment is kept)."""
    n = t.numel()
    buf = torch.full((n + 2 * K.MARGIN,), K.NAN, device=K.DEV)
    v = buf[K.MARGIN:K.MARGIN + n].view(t.shape)
    v.copy_(t)
    return v


def _saved(shapes, seed):
    return [K.make_saved(seed + 10 * i, T, R) + (K.make_weights(seed + 10 * i + 1, 0.3)[0],) for i, (T, R) in enumerate(shapes)]


def _bwd(groups, riders=None):
    """[(dy, y, gates, Ws)] on the CPU -> [(dgi, dgh)] on the CPU; operands in NaN arenas, outputs guarded."""
    dys, ys, gs = ([_in_arena(g[j]) for g in groups] for j in range(3))
    Wd = [_in_arena(w) for g in groups for w in g[3]]
    shp = [(g[0].shape[0], g[0].shape[1]) for g in groups]
    dgi = [K.Guarded((T, R, 6 * H)) for T, R in shp]
    dgh = [K.Guarded((T, R, 6 * H)) for T, R in shp]
    rc = _hip.lib().mmdfn_gru_seq_bwd(len(groups), _hip.ptr_array(dys), _hip.ptr_array(ys), _hip.ptr_array(gs), _hip.ptr_array(Wd),
                                      _hip.ptr_array([o.t for o in dgi]), _hip.ptr_array([o.t for o in dgh]),
                                      _hip.int_array([R for _, R in shp]), _hip.int_array([T for T, _ in shp]), H, riders,
                                      _hip.stream())
    res = K._finish(dgi + dgh)          # (synchronises; the margins around dgi and dgh are untouched)
    assert rc == 0, rc
    k = len(groups)
    return [(res[i], res[k + i]) for i in range(k)]


def _same_bits(a, b):
    for (gi_a, gh_a), (gi_b, gh_b) in zip(a, b):
        assert K._none_nan(gi_a, gh_a, gi_b, gh_b), "an element was not written, or is not finite"
        assert torch.equal(K._bits(gi_a), K._bits(gi_b)) and torch.equal(K._bits(gh_a), K._bits(gh_b))


def _both_forms(groups, env):
    env.delenv("MMDFN_GRU_BWD_STAGED", raising=False)
    direct = _bwd(groups)
    env.setenv("MMDFN_GRU_BWD_STAGED", "1")
    staged = _bwd(groups)
    env.delenv("MMDFN_GRU_BWD_STAGED")
    return direct, staged


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_direct_and_staged_forms_agree_bit_for_bit(shape, kernel_variants):
    direct, staged = _both_forms(_saved([shape], 700 + shape[0]), kernel_variants)
    _same_bits(direct, staged)


@pytest.mark.parametrize("shapes", GROUPS, ids=_sid)
def test_direct_and_staged_forms_agree_on_groups_of_different_length(shapes, kernel_variants):
    direct, staged = _both_forms(_saved(shapes, 720), kernel_variants)
    _same_bits(direct, staged)


def test_the_switch_selects_the_body(kernel_variants):
    """Default: the direct instantiation <8, 4, 0, 1>; MMDFN_GRU_BWD_STAGED=1: the staged one <8, 4, 0, 0>."""
    groups = _saved([(3, 2)], 730)
    kernel_variants.delenv("MMDFN_GRU_BWD_STAGED", raising=False)
    names = K._kernel_names(lambda: _bwd(groups))
    assert any(re.search(r"gru_seq_bwd_kpart_kernel<8, ?4, ?0, ?1>", n) for n in names), names
    kernel_variants.setenv("MMDFN_GRU_BWD_STAGED", "1")
    names = K._kernel_names(lambda: _bwd(groups))
    assert any(re.search(r"gru_seq_bwd_kpart_kernel<8, ?4, ?0, ?0>", n) for n in names), names


@pytest.mark.parametrize("shapes", [[s] for s in SHAPES] + GROUPS, ids=_sid)
def test_direct_form_against_float64(shapes):
    """The production library's default form: one- and two-step runs against the local bounds, longer ones on the kernel's own
    forward outputs against the accumulated bound (the bounds of test_gru_recurrence_kernels_gpu)."""
    tag = "direct " + _sid(shapes)
    if all(T <= 2 for T, _ in shapes):
        K.check_backward_local(shapes, 740, 0.3, False, tag)
        return
    groups, res = K.check_forward(shapes, 750, 0.3, False, tag)
    K.check_backward_long(groups, res, 751, tag)


@pytest.mark.parametrize("rows,T", [(3, 17), (5, 9)])
def test_rider_launch_gives_the_recurrence_bits_of_the_plain_launch(rows, T):
    """A staged weight-gradient batch makes the launch gru_seq_bwd_riders_kernel: same body, same bits."""
    from test_wgrad_riders_gpu import _batch_call
    lib = _hip.lib()
    groups = _saved([(T, rows)], 760)
    plain = _bwd(groups)
    ctx = _hip.riders_context()
    g = torch.Generator(device=K.DEV).manual_seed(3)
    A, Bm = torch.randn(4100, 300, device=K.DEV, generator=g), torch.randn(4100, 200, device=K.DEV, generator=g)
    C, cs = torch.empty(300, 200, device=K.DEV), torch.empty(300, device=K.DEV)
    call = _batch_call(A, Bm, C, cs, ctx, True)
    call(_hip.stream())
    assert lib.mmdfn_wgrad_riders_staged(ctx) == 1
    names = K._kernel_names(lambda: _same_bits(_bwd(groups, ctx), plain))
    assert any("gru_seq_bwd_riders_kernel" in n for n in names), names
    assert lib.mmdfn_wgrad_riders_staged(ctx) == 0          # the launch took the batch
    _hip.check(lib.mmdfn_wgrad_riders_drain(ctx, _hip.stream(), 0), "mmdfn_wgrad_riders_drain")
    torch.cuda.synchronize()
    ref = A.double().t() @ Bm.double()
    assert float((C.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_two_runs_are_bit_equal_and_a_row_alone_equals_the_row_in_a_batch():
    (dy, y, gates, Ws), = _saved([(9, 3)], 770)
    first = _bwd([(dy, y, gates, Ws)])
    _same_bits(first, _bwd([(dy, y, gates, Ws)]))
    for j in range(3):
        (da, ha), = _bwd([(dy[:, j:j + 1], y[:, j:j + 1], gates[:, j:j + 1], Ws)])
        assert torch.equal(K._bits(da), K._bits(first[0][0][:, j:j + 1])), j
        assert torch.equal(K._bits(ha), K._bits(first[0][1][:, j:j + 1])), j
