"""Shared helpers for the parity tests (oracle = checker, HIP path = thing checked)."""
import numpy as np
import torch

import mmdfn_oracle as O
from mm_dfn_amd import synthetic
from mm_dfn_amd.layout import BlockTileAdjacency, DialogueLayout, pair_list


def rel_err(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def abs_err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def random_block_adjacency(seed, lengths, M, device):
    """Random NON-symmetric tiles + cross diagonals; returns (BlockTileAdjacency on device, dense CPU matrix)."""
    rs = np.random.RandomState(seed)
    lay = DialogueLayout.get(lengths, M, device)
    tiles = [torch.from_numpy(rs.uniform(-1, 1, size=(L, L)).astype(np.float32)) for L in lengths for _ in range(M)]
    cross = torch.from_numpy(rs.uniform(-1, 1, size=(lay.npairs, lay.N)).astype(np.float32))
    adj = BlockTileAdjacency.from_parts(lay, tiles, cross, device=device)
    N = lay.N
    dense = torch.zeros(M * N, M * N)
    it = iter(tiles)
    start = 0
    for L in lengths:
        for m in range(M):
            dense[m * N + start:m * N + start + L, m * N + start:m * N + start + L] = next(it)
        start += L
    ar = torch.arange(N)
    for k, (m, n) in enumerate(pair_list(M)):
        dense[m * N + ar, n * N + ar] = cross[k]
        dense[n * N + ar, m * N + ar] = cross[k]
    return adj, dense, tiles, cross


def party_qmask(lengths, L, P, seed, pad_flag=False):
    """(L, B, P) float32 speaker mask with every row kind the party kernels meet, as far as the shape allows: one-hot rows;
    in every dialogue of at least 4 utterances one zero-hot valid utterance, one multi-hot row with 2 flags and (3 speakers
    to choose from) one with 3 flags; speaker P-1 silent in the last dialogue (when P >= 3, or P = 2 with another dialogue
    left for the multi-hot rows); with ``pad_flag`` one flag on a padding row of every dialogue shorter than L."""
    rs = np.random.RandomState(seed)
    B = len(lengths)
    q = np.zeros((L, B, P), np.float32)
    silent = (B - 1, P - 1) if P >= 3 or (P == 2 and B >= 2) else None
    for b, n in enumerate(lengths):
        spk = [p for p in range(P) if (b, p) != silent]
        q[np.arange(n), b, rs.choice(spk, size=n)] = 1.0
        if n >= 4:
            for t, nf in zip(rs.permutation(n), (0, 2, 3)):
                if nf <= len(spk):
                    q[t, b] = 0.0
                    q[t, b, rs.choice(spk, size=nf, replace=False)] = 1.0
        if pad_flag and n < L:
            q[rs.randint(n, L), b, rs.choice(spk)] = 1.0
    return torch.from_numpy(q)


def oracle_params(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def model_and_batch(cfg, seed, ragged, device, lengths=None, dropout=0.0):
    model = synthetic.build_model(dropout=dropout, **cfg)
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), seed))
    batch = synthetic.make_batch(seed + 1, ragged=ragged, lengths=lengths, **cfg)
    return model.to(device), batch


def dropout_tape_from_tap(draws, model, lengths, L, prefix="graph_model.graph_net."):
    """The oracle's DropoutTape for ONE forward of ``model`` (a DialogueGNNModel in train mode, graph_type 'GDF', 'DeepGCN' or 'None')
    from the keep flags the device drew for it: ``draws`` = what mm_dfn_amd.ops_flags.TAP collected during that forward,
    (n, p, flags, site) per ``keep_flags`` call.  The flags are read from the tapped tensors NOW, so for a captured step
    call this after every replay (the replay rewrites the same tensors).

    Layouts (mm_dfn_amd/gru.py bigru2, graph_conv.py _forward_stack, ops_head.py head):
      * one draw per bigru2 group, (T, rows_g, 200) of the group's layer-0 output: the context group's rows are the B
        dialogues; the party group's rows are (modality, dialogue, speaker) in the order of the gather's S, modalities =
        those with a non-zero speaker weight, and its time index is the speaker's packed rank -- the compacted position of
        the oracle's party_encode;
      * the stack's one flat draw [R nfeat | R H | nl R H], R = M N rows stacked modality-major (the oracle's cat(feats, 0));
      * the head's (N, M W).
    The oracle also encodes party modalities whose speaker weight is 0 (model.py:1090,1121,1154) and so has dropout sites
    the device does not: their output is multiplied by 0, neither a value nor a gradient depends on their mask, and they are
    left off the tape (identity).

    Strict: the number of draws, every draw's size, rate and site label must be what this model's forward implies, no two
    draws may overlap in memory (two sites sharing flags would still "match" the oracle fed the same flags), and every
    draw must be mapped -- a dropout site added to the product later fails here instead of being ignored.
    Returns (O.DropoutTape, {ReLU site: bool keep mask} for relu_flips_from_tap)."""
    assert model.training and model.dropout > 0 and not model.av_using_lstm and 'l' in model.present
    B, N, M = len(lengths), int(sum(lengths)), len(model.present)
    P = model.n_speakers
    p = float(model.dropout)
    wts = dict(zip('avl', model.speaker_weights))
    act = [m for m in model.present if model.use_crn_speaker and wts[m] != 0.0]
    expect = [("gru", L * B * 200)] + ([("gru", L * len(act) * B * P * 200)] if act else [])
    if model.graph_type == 'GDF':
        net = model.graph_model.graph_net
        nl, H, F = len(net.convs), net.convs[0].out_features, net.fcs[0].in_features
        R = M * N
        expect.append(("stack", R * F + (1 + nl) * R * H))
        W = (F + H) if model.use_residue else H
    elif model.graph_type == 'DeepGCN':
        # (the unimodal GCNII nets apply torch's own dropout, not keep flags: their masks are the caller's to add to the tape)
        assert model.att_type == 'concat_subsequently' and model.use_residue
        W = 300
    else:
        assert model.graph_type == 'None' and model.att_type in ('concat_subsequently', 'concat_only')
        W = 300
    expect.append(("head", N * M * W))
    assert len(draws) == len(expect), "%d keep-flag draws, expected %d (%s)" % (len(draws), len(expect), [d[3] for d in draws])
    flags = []
    for (n, dp, t, site), (want_site, want_n) in zip(draws, expect):
        assert site == want_site and n == want_n and t.numel() == want_n, "draw %r of %d flags where %r of %d belongs" % (
            site, n, want_site, want_n)
        assert abs(dp - p) < 1e-12, (dp, p)
        f = t.detach().float().cpu().reshape(-1)
        assert bool(((f == 0) | (f == 1)).all()), "%s: keep flags must be 0 / 1" % site
        flags.append(f)
    # no two sites share flags: the draws are disjoint pieces of memory (slices of the step's pool, or buffers of their own)
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel(), site) for _, _, t, site in draws)
    for (_, end, a), (start, _, b) in zip(spans, spans[1:]):
        assert end <= start, "the %s and %s draws overlap in memory" % (a, b)
    it = iter(flags)
    masks, keep = {}, {}
    masks["lstm_l"] = next(it).view(L, B, 200)
    if act:
        party = next(it).view(L, len(act), B, P, 200)
        for i, m in enumerate(act):
            for spk in range(P):
                masks["party.%s.%d" % (m, spk)] = party[:, i, :, spk, :]
    if model.graph_type == 'GDF':
        st = next(it)
        masks[prefix + "x"] = st[:R * F].view(R, F)
        masks[prefix + "h0"] = st[R * F:R * (F + H)].view(R, H)
        for i in range(nl):
            masks[prefix + "conv%d" % i] = st[R * (F + H) + i * R * H:R * (F + H) + (i + 1) * R * H].view(R, H)
            keep[prefix + "conv%d" % i] = masks[prefix + "conv%d" % i] > 0
    masks["head"] = next(it).view(N, M * W)
    keep["head"] = masks["head"] > 0
    assert next(it, None) is None
    return O.DropoutTape(masks), keep


def check_tape_consumed(tape):
    """Every mask on the tape was asked for by exactly one site of the oracle's forward, with the mask's shape."""
    seen = [s for s, _ in tape.seen]
    assert len(seen) == len(set(seen)), seen
    unused = sorted(set(tape.masks) - set(seen))
    assert not unused, "masks no oracle site asked for: %s" % unused
    for s, shape in tape.seen:
        if tape.masks.get(s) is not None:
            assert tuple(tape.masks[s].shape) == shape, (s, shape)


def relu_flips_from_tap(tap, probe, prefix, M, N, limit=16, band=1e-5, keep=None):
    """ReLU units on which the device and the oracle sit on different sides of the kink.  ``tap``: one entry of
    mm_dfn_amd.gcn_stack.TAP (the fused node's h0, per-layer gate masks and output); ``probe``: the oracle's ReluProbe of
    the same forward.  Every disagreement must be a pre-activation within ``band`` of zero (anything larger is a real
    error and fails here) and there may be at most ``limit`` of them.  ``keep`` (dropout on): {site: bool mask} of the units
    the site's dropout kept -- a dropped unit has gate mask 0 on the device whatever its ReLU decided, and the head's
    pre-activation in the oracle is the dropped feature, so only kept units are compared there (a dropped unit passes no
    gradient on either side).  Returns {site: LongTensor (k, 2)} for O.ReluProbe(flips=...)."""
    flips, total = {}, 0
    keep = keep or {}

    def site(name, dev_on, pre):
        nonlocal total
        differ = dev_on.cpu() != (pre > 0)
        if keep.get(name) is not None:
            differ = differ & keep[name]
        diff = differ.nonzero()
        if len(diff):
            worst = float(pre[diff[:, 0], diff[:, 1]].abs().max())
            assert worst < band, "%s: device and oracle disagree on a ReLU whose pre-activation is %.3g" % (name, worst)
            flips[name] = diff
            total += len(diff)

    site(prefix + "fcs0", tap["h0"] > 0, probe.pre[prefix + "fcs0"])
    for i, g in enumerate(tap["gmask"]):
        site(prefix + "conv%d" % i, g > 0, probe.pre[prefix + "conv%d" % i])
    out = tap["out"]                                   # (M N, W) stacked -> the head's (N, M W) input
    W = out.shape[1]
    head_on = (out > 0).view(M, N, W).permute(1, 0, 2).reshape(N, M * W)
    site("head", head_on, probe.pre["head"])
    assert total <= limit, "%d ReLU units differ between device and oracle" % total
    return flips
