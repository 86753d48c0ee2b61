"""The direct form of the plain one-sequence-per-CU GRU forward recurrence (csrc/gru.hip gru_fwd_direct_body): four waves, every
lane requests its three gate pre-activations of step s + D straight from global memory into a register ring and the results go
straight to global memory; the five-wave form it replaces (an I/O wave staging 4-step blocks through LDS) stays selectable in the
tuning library (MMDFN_GRU_FWD_STAGED=1) and is the bit-for-bit reference here.

The shapes sit at the ring's edges (D = FWD_RING_D: the ring has D + 1 slots; T < D never enters the loop, T = 5, 10 are whole
trips with no tail -- 5 the first trip alone, 10 one more --, T = 6, 9, 11, 17 leave tails of 1, 4, 1 and 2 steps) with 1 and 3
rows.  gi sits inside a NaN-filled buffer -- a request that left its array would bring a NaN into a finite result -- and every
output inside a buffer whose margins hold a bit pattern.  The float64 checks are those of test_gru_recurrence_kernels_gpu with
its bounds."""
import re

import pytest
import torch

import test_gru_recurrence_kernels_gpu as K
from mm_dfn_amd import _hip

pytestmark = pytest.mark.gpu
H = K.H
D = 4                     # FWD_RING_D of csrc/gru.hip
SHAPES = [(T, R) for T in (1, 2, 3, 4, 5, 6, 9, 10, 11, 17) for R in (1, 3)]
GROUPS = [[(7, 2), (12, 1)]]
_sid = lambda s: "+".join("%dx%d" % tr for tr in s) if isinstance(s, list) else "%dx%d" % s


def _in_arena(t):
    """``t`` on the device, inside a NaN-filled buffer (MARGIN floats on either side: the alignment is kept)."""
    n = t.numel()
    buf = torch.full((n + 2 * K.MARGIN,), K.NAN, device=K.DEV)
    v = buf[K.MARGIN:K.MARGIN + n].view(t.shape)
    v.copy_(t)
    return v


def _inputs(shapes, seed):
    """[(gi, Ws, bs)] on the CPU: tiny, ordinary and saturating pre-activations side by side, W_hh ~ U(-0.3, 0.3)."""
    out = []
    for i, (T, R) in enumerate(shapes):
        Ws, bs = K.make_weights(seed + 10 * i, 0.3)
        out.append((K.make_gi(seed + 10 * i + 1, T, R), Ws, bs))
    return out


def _fwd(groups, riders=None):
    """[(gi, Ws, bs)] on the CPU -> [(y, gates)] on the CPU; operands in NaN arenas, outputs guarded."""
    gis = [_in_arena(g[0]) for g in groups]
    Wd = [_in_arena(w) for g in groups for w in g[1]]
    bd = [_in_arena(b) for g in groups for b in g[2]]
    shp = [(g[0].shape[0], g[0].shape[1]) for g in groups]
    ys = [K.Guarded((T, R, 2 * H)) for T, R in shp]
    gs = [K.Guarded((T, R, 2, 4, H)) for T, R in shp]
    rc = _hip.lib().mmdfn_gru_seq_fwd(len(groups), _hip.ptr_array(gis), _hip.ptr_array(Wd), _hip.ptr_array(bd),
                                      _hip.ptr_array([o.t for o in ys]), _hip.ptr_array([o.t for o in gs]),
                                      _hip.int_array([R for _, R in shp]), _hip.int_array([T for T, _ in shp]), H, riders,
                                      _hip.stream())
    res = K._finish(ys + gs)            # (synchronises; the margins around y and gates are untouched)
    assert rc == 0, rc
    k = len(groups)
    return [(res[i], res[k + i]) for i in range(k)]


def _same_bits(a, b):
    for (y_a, g_a), (y_b, g_b) in zip(a, b):
        assert K._none_nan(y_a, g_a, y_b, g_b), "an element was not written, or is not finite"
        assert torch.equal(K._bits(y_a), K._bits(y_b)), "y"
        for k, name in enumerate(("r", "z", "n", "ghn")):
            assert torch.equal(K._bits(g_a[:, :, :, k]), K._bits(g_b[:, :, :, k])), name


def _both_forms(groups, env):
    env.delenv("MMDFN_GRU_FWD_STAGED", raising=False)
    direct = _fwd(groups)
    env.setenv("MMDFN_GRU_FWD_STAGED", "1")
    staged = _fwd(groups)
    env.delenv("MMDFN_GRU_FWD_STAGED")
    return direct, staged


@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_direct_and_staged_forms_agree_bit_for_bit(shape, kernel_variants):
    direct, staged = _both_forms(_inputs([shape], 800 + shape[0]), kernel_variants)
    _same_bits(direct, staged)


@pytest.mark.parametrize("shapes", GROUPS, ids=_sid)
def test_direct_and_staged_forms_agree_on_groups_of_different_length(shapes, kernel_variants):
    direct, staged = _both_forms(_inputs(shapes, 820), kernel_variants)
    _same_bits(direct, staged)


def test_the_switch_selects_the_body(kernel_variants):
    """Default: the direct instantiation <0, 0, 0, 1>; MMDFN_GRU_FWD_STAGED=1: the five-wave one <0, 0, 0, 0>."""
    groups = _inputs([(3, 2)], 830)
    kernel_variants.delenv("MMDFN_GRU_FWD_STAGED", raising=False)
    names = K._kernel_names(lambda: _fwd(groups))
    assert any(re.search(r"gru_seq_fwd_io_kernel<0, ?0, ?0, ?1>", n) for n in names), names
    kernel_variants.setenv("MMDFN_GRU_FWD_STAGED", "1")
    names = K._kernel_names(lambda: _fwd(groups))
    assert any(re.search(r"gru_seq_fwd_io_kernel<0, ?0, ?0, ?0>", n) for n in names), names


def test_the_production_library_runs_the_direct_body():
    names = K._kernel_names(lambda: _fwd(_inputs([(3, 2)], 831)))
    assert any(re.search(r"gru_seq_fwd_io_kernel<0, ?0, ?0, ?1>", n) for n in names), names


@pytest.mark.parametrize("shapes", [[s] for s in SHAPES] + GROUPS, ids=_sid)
def test_direct_form_against_float64(shapes):
    """The production library's default form, step by step against the float64 restatement under the forward bounds of
    test_gru_recurrence_kernels_gpu."""
    K.check_forward(shapes, 840, 0.3, False, "direct " + _sid(shapes))


@pytest.mark.parametrize("rows,T", [(3, 17), (5, 9)])
def test_flag_rider_launch_gives_the_recurrence_bits_of_the_plain_launch_and_the_generator_launch_its_flags(rows, T):
    """A staged dropout-flag draw makes the launch gru_seq_fwd_io_flags_kernel: the same body next to rider workgroups of 256
    threads.  y and the gates are those of the plain launch; the flags and the generator state are those of keep_flags_kernel
    (which counter yields which flag depends on neither the grid nor the block size)."""
    lib = _hip.lib()
    n, keep = 1 << 16, 0.6
    groups = _inputs([(T, rows)], 860)
    plain = _fwd(groups)
    fresh_state = lambda: torch.tensor([1234, 40, 0, 0], dtype=torch.int64, device=K.DEV)
    want, st0 = torch.empty(n, device=K.DEV), fresh_state()
    _hip.check(lib.mmdfn_keep_flags(_hip.ptr(want), n, keep, _hip.ptr(st0), _hip.stream()), "mmdfn_keep_flags")
    assert lib.mmdfn_gru_seq_fwd_takes_flags(1, _hip.int_array([rows])) == 1
    ctx = _hip.riders_context()
    got, st1 = torch.full((n,), K.NAN, device=K.DEV), fresh_state()
    _hip.check(lib.mmdfn_keep_flags_stage(_hip.ptr(got), n, keep, _hip.ptr(st1), ctx, _hip.stream()), "mmdfn_keep_flags_stage")
    names = K._kernel_names(lambda: _same_bits(_fwd(groups, ctx), plain))
    assert any("gru_seq_fwd_io_flags_kernel" in nm for nm in names), names
    assert not any("keep_flags_kernel" in nm for nm in names), names
    torch.cuda.synchronize()
    assert torch.equal(K._bits(got), K._bits(want)) and torch.equal(st1, st0)
    _hip.check(lib.mmdfn_keep_flags_flush(ctx, _hip.stream()), "mmdfn_keep_flags_flush")       # (nothing left to launch)
    torch.cuda.synchronize()
    assert torch.equal(K._bits(got), K._bits(want)) and torch.equal(st1, st0)


def test_two_runs_are_bit_equal_and_a_row_alone_equals_the_row_in_a_batch():
    (gi, Ws, bs), = _inputs([(9, 3)], 870)
    first = _fwd([(gi, Ws, bs)])
    _same_bits(first, _fwd([(gi, Ws, bs)]))
    for j in range(3):
        (ya, ga), = _fwd([(gi[:, j:j + 1], Ws, bs)])
        assert torch.equal(K._bits(ya), K._bits(first[0][0][:, j:j + 1])), j
        assert torch.equal(K._bits(ga), K._bits(first[0][1][:, j:j + 1])), j
