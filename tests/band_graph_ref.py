"""Restatements shared by test_band_graphs.py and test_band_graphs_gpu.py: the two sparse graphs of new_graph=True and the layer
stacks on top of them, written once, generic in the dtype, evaluated on the CPU (float64 = the reference value, float32 = the
yardstick).  Nothing here imports the package's builders."""
import math
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS_HALF = 2.0 ** -24
WINDOW_WIDTH = 20          # 2 * window_size: the union of the reference's [k - 10, k + 10] cliques
WINDOW_CASES = [[1, 2, 5], [21, 22, 23], [45]]


def load_gold():
    g = np.load(os.path.join(GOLD, "band_graphs.npz"), allow_pickle=False)
    return {k: torch.from_numpy(g[k]) for k in g.files}


def case(gold, prefix):
    c = {k[len(prefix):]: v for k, v in gold.items() if k.startswith(prefix)}
    c["lengths"] = [int(n) for n in c["dia_len"]]
    c["sd"] = {k[3:]: v for k, v in c.items() if k.startswith("sd/")}
    return c


# ---- keys: plain Python loops, the way the reference walks its dialogues ---------------------------------------------------------
def window_keys_loop(lengths):
    """[(chain, rank)] per row: chain 0, rank = position."""
    return [(0, j) for L in lengths for j in range(L)]


def speaker_keys_loop(qmask, lengths):
    """message_passing_directed_speaker's two lists (model_GCN.py:355-361): rank = index in speaker0 / speaker1."""
    keys = []
    for i, L in enumerate(lengths):
        n0 = n1 = 0
        for speaker in qmask[i][0:L]:
            if speaker[0] == 1:
                keys.append((0, n0))
                n0 += 1
            else:
                keys.append((1, n1))
                n1 += 1
    return keys


def pack_keys(pairs):
    return torch.tensor([(c << 24) | r for c, r in pairs], dtype=torch.int32)


# ---- the graph ---------------------------------------------------------------------------------------------------------------------
def band_graph(x, lengths, pairs, width):
    """Dense normalised adjacency (N, N), raw weights S, degree^-1/2 and every off-diagonal cosine inside a dialogue, in x's dtype.
    Edge between rows p != q of one dialogue iff chains equal and |rank_p - rank_q| <= width."""
    N = x.shape[0]
    chain = torch.tensor([c for c, _ in pairs])
    rank = torch.tensor([r for _, r in pairs])
    S = x.new_zeros(N, N)
    offdiag = []
    s = 0
    for L in lengths:
        xs = x[s:s + L]
        norm = (xs * xs).sum(-1).sqrt()
        den = norm[:, None] * norm[None, :]
        cos = torch.where(den == 0, torch.zeros_like(den), (xs @ xs.t()) / torch.where(den == 0, torch.ones_like(den), den))
        cos = cos.clamp(-1.0, 1.0)
        c, r = chain[s:s + L], rank[s:s + L]
        eye = torch.eye(L, dtype=torch.bool)
        edge = (c[:, None] == c[None, :]) & ((r[:, None] - r[None, :]).abs() <= width) & ~eye
        w = 1.0 - torch.acos(cos) / math.pi
        S[s:s + L, s:s + L] = torch.where(edge, w, torch.zeros_like(w)) + eye.to(x.dtype)
        offdiag.append(cos[~eye])
        s += L
    rdeg = S.sum(1).pow(-0.5)
    return dict(adj=rdeg[:, None] * S * rdeg[None, :], S=S, rdeg=rdeg, offdiag_cos=torch.cat(offdiag))


def tiles_of(lay, dense):
    """Dense (N, N) -> the flat block-tile array of an M = 1 layout (pad columns 0), and the mask of the written floats."""
    flat = dense.new_zeros(lay.tile_elems)
    written = torch.zeros(lay.tile_elems, dtype=torch.bool)
    for i, L in enumerate(lay.lengths):
        ld, base, rs = int(lay.ld_host[i]), int(lay.tile_base_host[i]), int(lay.row_start_host[i])
        blk = dense.new_zeros(L, ld)
        blk[:, :L] = dense[rs:rs + L, rs:rs + L]
        flat[base:base + L * ld] = blk.reshape(-1)
        written[base:base + L * ld] = True
    return flat, written


# ---- the layer stacks on a given (constant) adjacency -----------------------------------------------------------------------------
def gconv(cur, A, h0, W, lamda, alpha, l):
    theta = math.log(lamda / l + 1)
    hi = A @ cur
    return theta * (torch.cat([hi, h0], 1) @ W) + (1 - theta) * ((1 - alpha) * hi + alpha * h0)


def stack(sd, x, A, lamda, alpha, reason):
    """GCNII_lyc.forward / GCNII.forward (model_GCN.py:444-488, :256-286) without dropout, variant=True, use_residue=True,
    return_feature=True, on the constant adjacency A; returns (out, ReLU pre-activations)."""
    nl = len([k for k in sd if k.startswith("convs.")])
    pres = [x @ sd["fcs.0.weight"].t() + sd["fcs.0.bias"]]
    h0 = torch.relu(pres[0])
    cur, h, c = h0, torch.zeros_like(h0), torch.zeros_like(h0)
    for i in range(nl):
        q = cur
        if reason:
            g = q @ sd["rnn.weight_ih_l0"].t() + sd["rnn.bias_ih_l0"] + h @ sd["rnn.weight_hh_l0"].t() + sd["rnn.bias_hh_l0"]
            gi, gf, gg, go = g.chunk(4, 1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
            h = torch.sigmoid(go) * torch.tanh(c)
            cur = h
        pres.append(gconv(cur, A, h0, sd["convs.%d.weight" % i], lamda, alpha, i + 1))
        cur = torch.relu(pres[-1])
        if reason:
            cur = cur + q
    return torch.cat([x, cur], -1), pres


def run_stack(sd, x, A, G, lamda, alpha, reason, dtype):
    """out, dx and the parameter gradients of (out * G).sum() in ``dtype``; A is a constant."""
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = x.detach().cpu().to(dtype).requires_grad_(True)
    out, pres = stack(sd, x, A.detach().cpu().to(dtype), lamda, alpha, reason)
    (out * G.cpu().to(dtype)).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"grad/" + k: v.grad for k, v in sd.items() if v.grad is not None})
    return res, pres


def err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max())


def check(name, got, want64, want32, lines=None):
    """Device result against float64: at most 4 x the float32 evaluation's error (floor: half an ulp of the largest value)."""
    e, e32 = err(got, want64), err(want32, want64)
    ratio = e / max(e32, EPS_HALF)
    msg = "%-44s kernel %.3e  float32 CPU %.3e  ratio %.2f" % (name, e, e32, ratio)
    print(msg)
    if lines is not None:
        lines.append(msg)
    assert e <= 4 * max(e32, EPS_HALF), msg
    return ratio
