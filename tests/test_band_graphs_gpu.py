"""The window and speaker-chain graphs of new_graph=True on the device: K5b (csrc/adjacency_band.hip) through the C entry point
and through ops.build_band_adjacency, GCNII(new_graph=True) and GCNII_lyc(adj=message_passing_relation_graph(...)) on top.

What is compared against what (the convention of test_arccos_graph_gpu.py).  The restatements of band_graph_ref.py are evaluated
on the CPU in float64 (the reference value) and in float32 (the yardstick); errors are max |x - x64| / max |x64|.  A device
result passes at <= 4 x the float32 evaluation's error on the same inputs, which counts as at least 2^-24 (half an ulp of the
largest value).  For the module goldens the float32 run is the reference's own (tests/golden/band_graphs.npz).  acos of an
unshrunk cosine has unbounded slope at +-1 -- in the reference too -- so the random inputs are drawn such that every
off-diagonal float64 cosine inside a dialogue has |c| <= 0.9, and every case asserts that.  The parallel-rows test is the one
that goes to +-1, against a derived bound instead.  Every case prints its figures before it asserts; the measured ratios are in
profiles/r10_band_graph_parity.md.
"""
import math

import pytest
import torch

from band_graph_ref import (WINDOW_WIDTH, band_graph, case, check, load_gold, pack_keys, run_stack,
                            speaker_keys_loop, tiles_of, window_keys_loop)
from mm_dfn_amd import GCNII, GCNII_lyc, _hip, ops
from mm_dfn_amd.graphs import CapturedStep
from mm_dfn_amd.layout import DialogueLayout
from mm_dfn_amd.ops_pad import _lay_args

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(nfeat=40, nlayers=2, nhidden=20, nclass=6, dropout=0.0, lamda=0.5, alpha=0.2, variant=True, return_feature=True,
           use_residue=True)


def draw(N, D, seed):
    return torch.randn(N, D, generator=torch.Generator().manual_seed(seed))


def qmask_of(dialogues, P):
    """(dialogue, position, speaker) one-hot rows; non-zero garbage (ones in column 0 included) behind every dialogue's end."""
    qmask = torch.empty(len(dialogues), max(len(d) for d in dialogues), P)
    qmask[:, :, 0] = 1.0
    qmask[:, :, 1:] = 7.0
    for i, d in enumerate(dialogues):
        qmask[i, :len(d)] = torch.nn.functional.one_hot(torch.tensor(d), P).float()
    return [len(d) for d in dialogues], qmask


def speaker_cases():
    g = torch.Generator().manual_seed(3)
    rnd = torch.randint(0, 3, (64,), generator=g).tolist()
    # P = 2: alternating, only speaker 0, speaker 0 never speaks, length 1;  P = 3: random (1 and 2 share a chain), never, 1
    return [qmask_of([[j % 2 for j in range(65)], [0] * 33, [1] * 20, [1]], 2), qmask_of([rnd, [2, 1, 2, 2, 1], [0]], 3)]


def run_entry(x, keys, lay, width, D=None, M=1):
    """mmdfn_adj_build_band on NaN-filled outputs -> (tiles, rdeg, rc)."""
    N = x.shape[0]
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    deg, rdeg, tiles = nan(N), nan(N), nan(lay.tile_elems)
    rc = _hip.lib().mmdfn_adj_build_band(_hip.ptr(x), _hip.ptr(keys), _hip.ptr(deg), _hip.ptr(rdeg), _hip.ptr(tiles),
                                         *_lay_args(lay), lay.B, M, N, x.shape[1] if D is None else D, lay.max_len, width,
                                         _hip.stream())
    torch.cuda.synchronize()
    return tiles, rdeg, rc


def builder_case(tag, x, lengths, pairs, width, ops_keys):
    """Both ways into the builder against the float64 restatement; exact zeros off the band and in the pad columns."""
    lay = DialogueLayout.get(lengths, 1, torch.device(DEV))
    r64, r32 = band_graph(x.double(), lengths, pairs, width), band_graph(x, lengths, pairs, width)
    if r64["offdiag_cos"].numel():
        assert float(r64["offdiag_cos"].abs().max()) <= 0.9
    want64, written = tiles_of(lay, r64["adj"])
    want32, _ = tiles_of(lay, r32["adj"])
    tiles, rdeg, rc = run_entry(x.to(DEV), pack_keys(pairs).to(DEV), lay, width)
    assert rc == 0
    adj = ops.build_band_adjacency(x.to(DEV), lengths, ops_keys, width)
    assert adj.symmetric and not adj.requires_grad and tuple(adj.cross.shape) == (0, sum(lengths))
    assert torch.equal(adj.tiles[written.to(DEV)], tiles[written.to(DEV)]) and torch.equal(adj.rdeg, rdeg)
    tiles, rdeg = tiles.cpu(), rdeg.cpu()
    assert not torch.isnan(tiles[written]).any() and bool(torch.isfinite(rdeg).all())
    check(tag + " tiles", tiles[written], want64[written], want32[written])
    check(tag + " rdeg", rdeg, r64["rdeg"], r32["rdeg"])
    zero = want64[written] == 0                       # no edge, or a pad column (an edge's weight is never 0 at |c| <= 0.9)
    assert int((tiles[written][zero].view(torch.int32) != 0).sum()) == 0
    assert int((tiles[written][~zero] == 0).sum()) == 0
    check(tag + " to_dense", adj.to_dense(), r64["adj"], r32["adj"])


@pytest.mark.parametrize("D", [200, 40])
@pytest.mark.parametrize("lengths", [[1], [1, 2, 3], [21, 22, 23], [63, 64, 65], [127, 128, 5], [129, 4]])
def test_window_builder_against_float64(lengths, D):
    x = draw(sum(lengths), D, 17 + sum(lengths) + D)
    keys = ops.window_keys(lengths, torch.device(DEV))
    assert torch.equal(keys.cpu(), pack_keys(window_keys_loop(lengths)))
    builder_case("window %s D=%d" % (lengths, D), x, lengths, window_keys_loop(lengths), WINDOW_WIDTH, keys)


@pytest.mark.parametrize("D", [200, 40])
@pytest.mark.parametrize("batch", [0, 1])
def test_speaker_builder_against_float64(batch, D):
    lengths, qmask = speaker_cases()[batch]
    pairs = speaker_keys_loop(qmask, lengths)
    keys = ops.speaker_keys(qmask.to(DEV), lengths)
    assert torch.equal(keys.cpu(), pack_keys(pairs))
    clean = qmask.clone()
    for i, L in enumerate(lengths):
        clean[i, L:] = 0.0
    assert torch.equal(ops.speaker_keys(clean.to(DEV), lengths), keys)          # the padded positions are ignored
    builder_case("speaker P=%d %s D=%d" % (qmask.shape[2], lengths, D), draw(sum(lengths), D, 5 + batch + D), lengths, pairs, 1, keys)


def test_wide_features_take_the_streaming_form():
    """D = 520 > 512: the form that re-reads the row's own features instead of holding them in registers."""
    lengths = [23, 2]
    builder_case("window %s D=520" % lengths, draw(25, 520, 4), lengths, window_keys_loop(lengths), WINDOW_WIDTH,
                 ops.window_keys(lengths, torch.device(DEV)))


def test_zero_norm_row():
    """cos = 0 with a zero row (cossim's `if b == 0: return 0`): weight 0.5 to every band neighbour, nothing non-finite."""
    lengths, z = [30, 3], 7
    x = draw(33, 40, 21)
    x[z] = 0.0
    x[31] = 0.0
    lay = DialogueLayout.get(lengths, 1, torch.device(DEV))
    tiles, rdeg, rc = run_entry(x.to(DEV), ops.window_keys(lengths, torch.device(DEV)), lay, WINDOW_WIDTH)
    assert rc == 0
    _, written = tiles_of(lay, torch.zeros(33, 33))
    tiles, rdeg = tiles.cpu(), rdeg.cpu()
    assert bool(torch.isfinite(tiles[written]).all()) and bool(torch.isfinite(rdeg).all())
    T = tiles[:30 * 32].view(30, 32)
    seen = 0
    for q in range(30):
        if q != z and abs(q - z) <= WINDOW_WIDTH:
            want = (rdeg[z] * 0.5) * rdeg[q]
            assert float(T[z, q]) == float(want) and float(T[q, z]) == float(want), q
            seen += 1
        elif q != z:
            assert float(T[z, q]) == 0.0 and float(T[q, z]) == 0.0
    assert seen == 27
    r64 = band_graph(x.double(), lengths, window_keys_loop(lengths), WINDOW_WIDTH)
    r32 = band_graph(x, lengths, window_keys_loop(lengths), WINDOW_WIDTH)
    assert float(r64["S"][z, z + 1]) == 0.5 and float(r64["S"][31, 30]) == 0.5
    check("zero-norm row tiles", tiles[written], tiles_of(lay, r64["adj"])[0][written], tiles_of(lay, r32["adj"])[0][written])


def test_parallel_rows():
    """64 rows that are x, 2x, 0.5x and -x of 16 base vectors, neighbours in one window: the float32 cosines of the parallel
    pairs round to either side of +-1.  Everything is finite, every raw weight lies in [0, 1], and a parallel pair's weight is
    at least 1 - sqrt(2 (D + 2) 2^-23) / pi: a D-term float32 dot product and the two norms are off by at most (D + 2) 2^-23
    of |x| |y| together, and acos(1 - d) <= sqrt(2 d) (1 + d).  The raw weight S is read off the stored T = (r_p S) r_q
    through the monotonicity of float32 rounding: S <= 1 gives T <= (r_p 1) r_q and S >= b gives T >= (r_p b) r_q."""
    D = 40
    base = draw(16, D, 9)
    x = torch.stack([base, 2 * base, 0.5 * base, -base], 1).reshape(64, D)
    lay = DialogueLayout.get([64], 1, torch.device(DEV))
    tiles, rdeg, rc = run_entry(x.to(DEV), ops.window_keys([64], torch.device(DEV)), lay, WINDOW_WIDTH)
    assert rc == 0
    T, r = tiles.cpu().view(64, 64), rdeg.cpu()
    assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(r).all())
    one = r[:, None] * r[None, :]                                  # (r_p * 1) * r_q in float32
    assert bool((T >= 0).all()) and bool((T <= one).all())
    exact = 1.0 - math.sqrt(2 * (D + 2) * 2.0 ** -23) / math.pi
    bound = torch.tensor(exact, dtype=torch.float32)
    if float(bound) > exact:                                       # the float32 bound never above the derived one
        bound = torch.nextafter(bound, torch.tensor(0.0))
    low = (r[:, None] * bound) * r[None, :]
    pairs = anti = 0
    worst = 1.0
    for b in range(16):
        for u in range(3):
            for v in range(3):
                p, q = 4 * b + u, 4 * b + v
                if p != q:
                    assert float(T[p, q]) >= float(low[p, q]), (p, q)
                    worst = min(worst, float(T[p, q].double() / (r[p].double() * r[q].double())))
                    pairs += 1
            p, q = 4 * b + u, 4 * b + 3                            # antiparallel: weight 1 - acos(-1 + d) / pi <= 1 - bound
            assert float(T[p, q]) <= float((r[p] * (1.0 - bound)) * r[q]), (p, q)
            assert float(T[q, p]) <= float((r[q] * (1.0 - bound)) * r[p]), (q, p)
            anti += 1
    print("parallel pairs %d, smallest raw weight %.9f (bound %.9f); antiparallel pairs %d" % (pairs, worst, float(bound), anti))
    assert pairs == 96 and anti == 48


def test_argument_errors_launch_nothing():
    fn = _hip.lib().mmdfn_adj_build_band
    good = (1, 1, 4, 8, 4, 20)                                     # B, M, N, D, max_len, width
    assert fn(*([None] * 8), *good, None) == -1                    # null pointers alone
    for bad in ((1, 1, 4, 8, 4, -1), (1, 2, 4, 8, 4, 20), (1, 1, 4, 6, 4, 20), (1, 0, 4, 8, 4, 20)):
        assert fn(*([None] * 8), *bad, None) == -1, bad
    # real buffers, one bad argument at a time: -1 and not a float written
    lengths = [4]
    lay = DialogueLayout.get(lengths, 1, torch.device(DEV))
    x, keys = draw(4, 8, 1).to(DEV), ops.window_keys(lengths, torch.device(DEV))
    for kw in (dict(width=-1), dict(width=20, M=2), dict(width=20, D=6)):
        tiles, rdeg, rc = run_entry(x, keys, lay, **kw)
        assert rc == -1 and bool(torch.isnan(tiles).all()) and bool(torch.isnan(rdeg).all()), kw
    P = _hip.ptr
    nan = torch.full((lay.tile_elems,), float("nan"), device=DEV)
    ptrs = [P(x), P(keys), P(nan[:4]), P(nan[4:8]), P(nan), *_lay_args(lay)]
    for k in range(8):
        args = list(ptrs)
        args[k] = None
        assert fn(*args, *good[:3], 8, 4, 20, _hip.stream()) == -1, k
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan).all())
    with pytest.raises(ValueError, match="width"):
        ops.build_band_adjacency(x, lengths, keys, -1)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.build_band_adjacency(draw(4, 6, 1).to(DEV), lengths, keys, 1)
    with pytest.raises(ValueError, match="int32"):
        ops.build_band_adjacency(x, lengths, keys.long(), 1)


def test_propagate_on_sparse_tiles():
    """The downstream kernel takes the dense tiles with their zeros unchanged: ops.propagate against the float64 product, at
    the propagate tolerance of this suite (1e-5 relative, test_graph_kernels_gpu.py)."""
    lengths = [63, 64, 65]
    x = draw(192, 40, 8).to(DEV)
    adj = ops.build_band_adjacency(x, lengths, ops.window_keys(lengths, torch.device(DEV)), WINDOW_WIDTH)
    dense = adj.to_dense().double().cpu()
    assert int((dense[:63, :63] == 0).sum()) == 42 * 43           # the band really leaves zeros in the tiles
    for d in (20, 100):
        H = draw(192, d, 30 + d)
        out = ops.propagate(adj, H.to(DEV))
        want = dense @ H.double()
        e = float((out.double().cpu() - want).abs().max() / want.abs().max())
        print("propagate on the window graph %s d=%d: %.3e" % (lengths, d, e))
        assert e < 1e-5


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return load_gold()


def run_module(m, x, call, G):
    m.zero_grad(set_to_none=True)
    x = x.detach().to(DEV).requires_grad_(True)
    out = call(m, x)
    (out * G.to(DEV)).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"grad/" + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    return res


def near_kink(pres, band=1e-5):
    return sum(int((p.abs() < band * p.abs().amax(1, keepdim=True)).sum()) for p in pres)


def module_case(tag, c, got, A64, reason, keys):
    r64, pres = run_stack(c["sd"], c["x"], A64, c["G"], 0.5, 0.2, reason, torch.float64)
    assert near_kink(pres) == 0
    want = {"out": c["out"], "dx": c["dx"]}
    want.update({k: v for k, v in c.items() if k.startswith("grad/")})
    assert sorted(want) == sorted(keys) and sorted(got) == sorted(keys)
    for k in keys:
        check("%s %s" % (tag, k), got[k], r64[k], want[k])


@pytest.mark.parametrize("n", [0, 1, 2])
def test_gcnii_lyc_on_the_window_graph_against_the_reference_golden(gold, n):
    c = case(gold, "win/%d/" % n)
    lengths = c["lengths"]
    m = GCNII_lyc(**CFG, new_graph=True, reason_flag=True).to(DEV).train()
    m.load_state_dict({k: v.to(DEV) for k, v in c["sd"].items()})
    built = []

    def call(m, x):
        built.append(m.message_passing_relation_graph(x, lengths))
        return m(x, lengths, None, adj=built[-1])
    got = run_module(m, c["x"], call, c["G"])
    adj = built[0]
    assert not adj.requires_grad and adj.symmetric
    r64 = band_graph(c["x"].double(), lengths, window_keys_loop(lengths), WINDOW_WIDTH)
    tag = "GCNII_lyc window %s" % lengths
    check(tag + " adj", adj.to_dense(), r64["adj"], c["adj"])
    keys = ["out", "dx"] + ["grad/" + k for k in c["sd"]]
    module_case(tag, c, got, r64["adj"], True, keys)
    # x.grad holds no graph term: the same bits as a run whose adjacency came in as a plain constant
    const = m.message_passing_relation_graph(c["x"].to(DEV), lengths)
    again = run_module(m, c["x"], lambda m, x: m(x, lengths, None, adj=const), c["G"])
    for k in keys:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("n", [0, 1])
def test_gcnii_new_graph_against_the_reference_golden(gold, n):
    c = case(gold, "spk/%d/" % n)
    lengths, qmask = c["lengths"], c["qmask"].to(DEV)
    pairs = speaker_keys_loop(c["qmask"], lengths)
    r64 = band_graph(c["x"].double(), lengths, pairs, 1)
    tag = "GCNII speaker %s" % lengths
    # gradients: reason_flag=False (the reference's own backward fails with the gate on, make_golden_band_graphs.py)
    m = GCNII(**CFG, new_graph=True, reason_flag=False).to(DEV).train()
    m.load_state_dict({k: v.to(DEV) for k, v in c["sd"].items()})
    got = run_module(m, c["x"], lambda m, x: m(x, lengths, qmask), c["G"])
    adj = m.message_passing_directed_speaker(c["x"].to(DEV), lengths, qmask)
    assert not adj.requires_grad
    check(tag + " adj", adj.to_dense(), r64["adj"], c["adj"])
    keys = ["out", "dx"] + ["grad/" + k for k in c["sd"] if not k.startswith("rnn.")]
    module_case(tag, c, got, r64["adj"], False, keys)
    again = run_module(m, c["x"], lambda m, x: m._forward_fused(x, adj), c["G"])
    for k in keys:
        assert torch.equal(got[k], again[k]), k
    # forward with the gate on
    g = GCNII(**CFG, new_graph=True, reason_flag=True).to(DEV).train()
    g.load_state_dict({k: v.to(DEV) for k, v in c["sd"].items()})
    with torch.no_grad():
        out = g(c["x"].to(DEV), lengths, qmask)
    o64, _ = run_stack(c["sd"], c["x"], r64["adj"], c["G"], 0.5, 0.2, True, torch.float64)
    check(tag + " out (gate on)", out, o64["out"], c["out_gate"])


def test_captured_step_follows_the_qmask():
    """graphs.CapturedStep over GCNII(new_graph=True) forward + backward: the keys are computed inside the graph from the
    static qmask tensor, so a replay follows its contents.  Both replays equal the eager runs bit for bit."""
    lengths = [9, 1, 14]
    N = sum(lengths)
    torch.manual_seed(4)
    m = GCNII(**CFG, new_graph=True, reason_flag=True).to(DEV).train()
    x = draw(N, 40, 12).to(DEV).requires_grad_(True)
    G = draw(N, 60, 13).to(DEV)
    g = torch.Generator().manual_seed(6)
    qa = qmask_of([torch.randint(0, 2, (L,), generator=g).tolist() for L in lengths], 2)[1]
    qb = qmask_of([torch.randint(0, 2, (L,), generator=g).tolist() for L in lengths], 2)[1]
    assert speaker_keys_loop(qa, lengths) != speaker_keys_loop(qb, lengths)
    qmask = qa.to(DEV)
    held = {}

    def step():
        x.grad = None
        out = m(x, lengths, qmask)
        # (only a detached alias outlives the pass: an output kept with its autograd graph would keep the AccumulateGrad nodes
        # of an earlier pass alive, bound to the stream of THAT pass, and a capture must not touch another stream)
        held["out"] = out.detach()
        loss = (out * G).sum()
        loss.backward()
        return loss

    def result():
        torch.cuda.synchronize()
        return [held["out"].clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    want = []
    for q in (qa, qb):
        qmask.copy_(q)
        m.zero_grad(set_to_none=True)
        step()
        want.append(result())
    assert not torch.equal(want[0][0], want[1][0])
    cap = CapturedStep(m, step, warmup=2)
    try:
        for q, w in zip((qb, qa, qb), (want[1], want[0], want[1])):
            qmask.copy_(q)
            cap.replay()
            got = result()
            assert len(got) == len(w) == 2 + 8
            for i, (a, b) in enumerate(zip(got, w)):
                assert torch.equal(a, b), i
    finally:
        cap.close()
