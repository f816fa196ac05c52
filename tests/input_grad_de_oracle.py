"""Support of the NISQA_DE input-gradient tests (not a test module): autograd through the oracle's double-ended chain, pair by pair
-- oracle.net.adapt_cnn -> self_attention on each side, a torch restatement of de_oracle.scores with the masked softmax or the
argmax and the fusion (reference NISQA_lib.py:1264-1294, 1359-1378, 1405-1417), self_attention(pfx='time_dependency_2.model.'),
pool_att_ff -- in float64 (the yardstick) or float32 (what fp32 arithmetic alone is off by), and the seeded cases the CPU tests, the
GPU tests and the fixtures share.

Hard alignment: the argmax carries no gradient, so the gradient depends on WHICH reference row was gathered.  Where the float64
top-2 score gap of a degraded token is <= TIE an fp32 evaluation may choose the other row legitimately (tests/test_gpu_de.py's
rule): with ``idx`` given the oracle gathers the given row there, and float64's own everywhere else; the caller asserts that the
given indices equal float64's wherever the gap is larger."""
import numpy as np
import torch

import de_oracle as DO
import input_grad_oracle as IG
import lstm_train_oracle as LT
from oracle import net as onet

TIE = 1e-5
TD2 = 'time_dependency_2.model.'
CONFIGS = [('cosine', 'hard', 'x/y/-'), ('dot', 'soft', '+/-'), ('cosine', 'soft', 'x/y')]       # as tests/test_de_host.py
NAMES = {CONFIGS[0]: 'cos_hard', CONFIGS[1]: 'dot_soft', CONFIGS[2]: 'cos_soft'}

# pairs (degraded, reference) segments; clips lstm_train_oracle.batch(seed_batch, 15 + 4 (n - 1) frames), the reference side
# from seed_batch + 1000; weights de_oracle.random_de_state_dict(seed_sd, fuse)
SMALL = dict(seed_sd=41, seed_batch=541, pairs=[(1, 3), (3, 1), (2, 2)], L=4, seed_g=42)
EDGE = dict(seed_sd=41, seed_batch=541, pairs=[(65, 3), (1, 65), (64, 64)], L=None, seed_g=42)


def case(config, spec=SMALL, fill=0.0):
    """-> (state_dict, args, x float32 [B, L, 2, 48, 15] with ``fill`` in the padding rows, n_wins int64 [B, 2], g float32 [B, 1])"""
    align, apply, fuse = config
    args = DO.de_args(align, apply, fuse)
    sd = DO.random_de_state_dict(spec['seed_sd'], fuse)
    frames = lambda side: [15 + 4 * (p[side] - 1) for p in spec['pairs']]
    specs_d, _ = LT.batch(spec['seed_batch'], frames(0))
    specs_r, _ = LT.batch(spec['seed_batch'] + 1000, frames(1))
    L = spec['L'] or max(max(p) for p in spec['pairs'])
    xd, nd = IG.segment_tensor(specs_d, args, L, fill)
    xr, nr = IG.segment_tensor(specs_r, args, L, fill)
    x = np.concatenate([xd, xr], 2)
    n_wins = np.stack([nd, nr], 1).astype(np.int64)
    assert n_wins.tolist() == [list(p) for p in spec['pairs']]
    g = np.random.default_rng(spec['seed_g']).standard_normal((len(n_wins), 1)).astype(np.float32)
    return sd, args, x, n_wins, g


def scores(xd, xr, align):
    """de_oracle.scores in torch: att[i, j] between degraded token i and reference token j"""
    if align == 'cosine':
        xd = xd / xd.norm(dim=1, keepdim=True).clamp(min=1e-8)
        xr = xr / xr.norm(dim=1, keepdim=True).clamp(min=1e-8)
    return xd @ xr.T


def fuse_rows(x, y, fuse):
    if fuse == 'x/y/-':
        return torch.cat([x, y, x - y], 1)
    if fuse == '+/-':
        return torch.cat([x + y, x - y], 1)
    return torch.cat([x, y], 1)


def align_fuse(xd, xr, align, apply, fuse, idx=None):
    """-> (fused [n_x, F], the gathered indices [n_x] or None, float top-2 score gap [n_x], this evaluation's own argmax or None)"""
    att = scores(xd, xr, align)
    top = att.detach().topk(min(2, att.shape[1]), dim=1)[0]
    gap = (top[:, 0] - top[:, 1]) if att.shape[1] > 1 else torch.full((att.shape[0],), float('inf'), dtype=att.dtype)
    if apply == 'hard':
        own = att.detach().argmax(1)
        k = own
        if idx is not None:
            k = torch.where(gap <= TIE, torch.as_tensor(np.asarray(idx), dtype=torch.int64), own)
        return fuse_rows(xd, xr[k], fuse), k.numpy(), gap.numpy(), own.numpy()
    return fuse_rows(xd, torch.softmax(att, 1) @ xr, fuse), None, gap.numpy(), None


def oracle(sd, args, x, n_wins, gs, idx=None, dtype=torch.float64, margins=True):
    """x [B, L, 2, 48, 15] (padding rows are never read), n_wins [B, 2], gs: list of g [B, 1]; idx: per pair the hard indices
    to gather at near-ties (see the module docstring) ->
    dict(y [B, 1], dx: one [B, L, 2, 48, 15] per g with zero padding rows, margin [B, L, 2]: the CNN tie margin of every segment
    (input_grad_oracle.cnn_margins; inf at the padding rows), gap: per pair the top-2 score gap of every degraded token, idx:
    per pair the gathered indices, own: per pair this evaluation's argmax (hard; else None)) in ``dtype``'s arithmetic"""
    sd = {k: onet._t(v).to(dtype) for k, v in sd.items() if k.split('.')[-1] != 'num_batches_tracked'}
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    B, L = x.shape[:2]
    y = np.zeros((B, 1))
    dx = [np.zeros(tuple(x.shape)) for _ in gs]
    margin = np.full((B, L, 2), np.inf)
    gaps, idxs, owns = [], [], []
    cnn = lambda v: onet.adapt_cnn(sd, v, args['cnn_pool_1'], args['cnn_pool_2'], args['cnn_pool_3'])
    for b in range(B):
        nd, nr = int(n_wins[b][0]), int(n_wins[b][1])
        xd = x[b, :nd, 0:1].clone().requires_grad_(True)
        xr = x[b, :nr, 1:2].clone().requires_grad_(True)
        td_x = onet.self_attention(sd, cnn(xd), args['td_sa_num_layers'])
        td_y = onet.self_attention(sd, cnn(xr), args['td_sa_num_layers'])
        fused, k, gap, own = align_fuse(td_x, td_y, args['de_align'], args['de_align_apply'], args['de_fuse'],
                                        None if idx is None else idx[b])
        x2 = onet.self_attention(sd, fused, args['td_2_sa_num_layers'], pfx=TD2)
        yb = onet.pool_att_ff(sd, x2, 'pool.model.')
        y[b] = yb.detach().numpy()
        for j, g in enumerate(gs):
            gb = torch.as_tensor(np.asarray(g[b], dtype=np.float64)).to(dtype)
            dd, dr = torch.autograd.grad((yb * gb).sum(), (xd, xr), retain_graph=True)
            dx[j][b, :nd, 0:1] = dd.numpy()
            dx[j][b, :nr, 1:2] = dr.numpy()
        if margins:
            with torch.no_grad():
                margin[b, :nd, 0] = IG.cnn_margins(sd, args, xd.detach()).numpy()
                margin[b, :nr, 1] = IG.cnn_margins(sd, args, xr.detach()).numpy()
        gaps.append(gap)
        idxs.append(k)
        owns.append(own)
    return {'y': y, 'dx': dx, 'margin': margin, 'gap': gaps, 'idx': idxs, 'own': owns}


def channel_error(got, want, keep=None):
    """max |got - want| / max |want| per clip and channel over the rows ``keep`` [B, L, 2] (default: all) -> [B, 2]; 0 where
    no row of a channel is kept (a one-segment clip whose segment is left out)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    B = want.shape[0]
    out = np.zeros((B, 2))
    for b in range(B):
        for c in range(2):
            rows = slice(None) if keep is None else keep[b, :, c]
            w, g = want[b, :, c][rows], got[b, :, c][rows]
            if w.size:
                out[b, c] = np.abs(g - w).max() / np.abs(w).max()
    return out
