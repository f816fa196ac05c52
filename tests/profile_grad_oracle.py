"""Support of the profile-gradient tests (not a test module): a float64 autograd restatement of the per-segment profile as a function
of what it is computed from.  Per clip the oracle network's rows (oracle.net: adapt_cnn -> self_attention; for NISQA_DE
input_grad_de_oracle's alignment + fusion and the second self_attention behind them) go through profile_oracle.att_profile head by
head, and the scalar

    sum c_w * weights + sum c_l * local + sum c_e * embed (+ sum g * score)

is differentiated -- in the segment tensor x (``oracle``), or in the rows the pooling read (``pool_grad``: what the kernel
nisqa_pool_profile_bwd is held to).  The score is oracle.net.pool_att_ff's, not the profile's own sum.

The identity the CPU and the GPU tests use: score = sum_t weights_t local_t, so with c_w = g * local and c_l = g * weights (both taken
as constants at the point) the profile's gradient is the score's for the cotangent g (``identity_cotangents``).

Cotangents come as dicts with any of the keys 'w', 'l' [B, L, heads], 'e' [B, L, 64], 'g' [B, heads]; rows l >= n_wins[b] are never
read."""
import numpy as np
import torch

import audio_grad_oracle as AG
import input_grad_de_oracle as IGD
import input_grad_oracle as IG
import profile_oracle as PO
from oracle import net as onet


def _profile(sd, td, heads):
    """td [n, 64] -> (weights [n, H], local [n, H], score [H]) in td's dtype, differentiable"""
    parts = [PO.att_profile(sd, td, p) for p in heads]
    return (torch.stack([p[0] for p in parts], 1), torch.stack([p[1] for p in parts], 1),
            torch.cat([onet.pool_att_ff(sd, td, p) for p in heads]))


def _scalar(w, l, td, score, cot, b, n):
    """the scalar of one clip for one cotangent dict (see the module docstring)"""
    f = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(td.dtype)
    s = td.sum() * 0.0
    for key, t in (('w', w), ('l', l), ('e', td)):
        if cot.get(key) is not None:
            s = s + (f(cot[key][b][:n]) * t).sum()
    if cot.get('g') is not None:
        s = s + (f(cot['g'][b]) * score).sum()
    return s


def pool_grad(sd, rows, heads, cw=None, cl=None, ce=None, dtype=torch.float64):
    """rows [n, 64]: one clip's valid rows; cw, cl [n, H], ce [n, 64] or None -> d (sum cw * weights + sum cl * local + sum ce * rows)
    / d rows as a numpy array of ``dtype``, every operator evaluated in that dtype (float64: the yardstick; float32: what sets the
    kernel test's bar, as profile_oracle.bars does for the forward)"""
    s = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith('pool') and 'num_batches' not in k}
    x = torch.from_numpy(np.ascontiguousarray(rows)).to(dtype).requires_grad_(True)
    w, l, score = _profile(s, x, heads)
    cot = {k: None if v is None else np.asarray(v)[None] for k, v in (('w', cw), ('l', cl), ('e', ce))}
    return torch.autograd.grad(_scalar(w, l, x, score, cot, 0, x.shape[0]), x)[0].numpy()


def oracle(sd, args, x, n_wins, cots, idx=None, dtype=torch.float64):
    """x [B, L, 1, 48, 15] with n_wins [B] (NISQA, NISQA_DIM) or [B, L, 2, 48, 15] with n_wins [B, 2] (NISQA_DE; idx: the hard indices
    to gather at near-ties, input_grad_de_oracle's rule), cots: a list of cotangent dicts ->
    dict(y [B, H], weights / local [B, L, H], embed [B, L, 64] with zero padding rows, dx: one array of x's shape per cotangent dict,
    margin: the CNN tie margins as input_grad_oracle.oracle / input_grad_de_oracle.oracle report them, and for NISQA_DE gap, idx, own)"""
    de = np.asarray(x).shape[2] == 2
    sd = {k: onet._t(v).to(dtype) for k, v in sd.items() if k.split('.')[-1] != 'num_batches_tracked'}
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    B, L = x.shape[:2]
    heads = ['pool.model.'] if de else IG.heads_of(args['model'])
    H = len(heads)
    out = {'y': np.zeros((B, H)), 'weights': np.zeros((B, L, H)), 'local': np.zeros((B, L, H)), 'embed': np.zeros((B, L, 64)),
           'dx': [np.zeros(tuple(x.shape)) for _ in cots], 'margin': np.full((B, L, 2) if de else (B, L), np.inf),
           'gap': [], 'idx': [], 'own': []}
    cnn = lambda v: onet.adapt_cnn(sd, v, args['cnn_pool_1'], args['cnn_pool_2'], args['cnn_pool_3'])
    for b in range(B):
        if de:
            counts = [int(n_wins[b][0]), int(n_wins[b][1])]
            leaves = [x[b, :counts[c], c:c + 1].clone().requires_grad_(True) for c in range(2)]
            td_x, td_y = [onet.self_attention(sd, cnn(v), args['td_sa_num_layers']) for v in leaves]
            fused, k, gap, own = IGD.align_fuse(td_x, td_y, args['de_align'], args['de_align_apply'], args['de_fuse'],
                                                None if idx is None else idx[b])
            td = onet.self_attention(sd, fused, args['td_2_sa_num_layers'], pfx=IGD.TD2)
            out['gap'].append(gap)
            out['idx'].append(k)
            out['own'].append(own)
        else:
            counts = [int(n_wins[b])]
            leaves = [x[b, :counts[0]].clone().requires_grad_(True)]
            td = onet.self_attention(sd, cnn(leaves[0]), args['td_sa_num_layers'])
        n = counts[0]
        w, l, score = _profile(sd, td, heads)
        out['y'][b], out['weights'][b, :n], out['local'][b, :n] = score.detach().numpy(), w.detach().numpy(), l.detach().numpy()
        out['embed'][b, :n] = td.detach().numpy()
        for j, cot in enumerate(cots):
            grads = torch.autograd.grad(_scalar(w, l, td, score, cot, b, n), leaves, retain_graph=True)
            for c, d in enumerate(grads):
                if de:
                    out['dx'][j][b, :counts[c], c:c + 1] = d.numpy()
                else:
                    out['dx'][j][b, :n] = d.numpy()
        with torch.no_grad():
            for c, v in enumerate(leaves):
                m = IG.cnn_margins(sd, args, v.detach()).numpy()
                if de:
                    out['margin'][b, :counts[c], c] = m
                else:
                    out['margin'][b, :n] = m
    return out


def identity_cotangents(weights, local, g):
    """weights, local [B, L, H] at the point, g [B, H] -> the cotangent dict whose profile gradient is the score's for g"""
    g = np.asarray(g, dtype=np.float64)[:, None, :]
    return {'w': g * np.asarray(local, dtype=np.float64), 'l': g * np.asarray(weights, dtype=np.float64)}


def random_cotangents(seed, B, L, H, keys='wleg'):
    """standard-normal cotangents for the keys named, float32"""
    rng = np.random.default_rng(seed)
    shapes = {'w': (B, L, H), 'l': (B, L, H), 'e': (B, L, 64), 'g': (B, H)}
    return {k: rng.standard_normal(shapes[k]).astype(np.float32) for k in 'wleg' if k in keys}


def compose_de(sd, args, rows_deg, rows_ref, ys_deg, ys_ref, sr, cots, idx=None):
    """de_audio_grad_oracle.compose_de with this module's oracle in the place of input_grad_de_oracle's: the wanted d / d y_deg and
    d / d y_ref of the profile's scalar for each cotangent dict (over the degraded clips' segments), at the segment tensor cut from the
    given clamped rows -> its dict (dy_deg, dy_ref per cotangent dict, mel_margin [B, 2], n_wins [B, 2]) beside ``oracle``'s"""
    seg_hop = args['ms_seg_hop_length']
    B = len(rows_deg)
    segs = [[AG.segments_of(np.asarray(r), seg_hop) for r in rows] for rows in (rows_deg, rows_ref)]
    n_wins = np.array([[len(segs[0][b]), len(segs[1][b])] for b in range(B)], dtype=np.int64)
    x = np.zeros((B, int(n_wins.max()), 2, 48, 15), dtype=np.float32)
    for c in range(2):
        for b, s in enumerate(segs[c]):
            x[b, :len(s), c:c + 1] = s
    net = oracle(sd, args, x, n_wins, cots, idx=idx)
    dy = [[[] for _ in cots], [[] for _ in cots]]
    mm = np.zeros((B, 2))
    for c, (rows, ys) in enumerate(((rows_deg, ys_deg), (rows_ref, ys_ref))):
        for b, yb in enumerate(ys):
            for k in range(len(cots)):
                grow = AG.segments_adjoint(net['dx'][k][b, :n_wins[b, c], c:c + 1], rows[b].shape[0], seg_hop)
                d, _, _, mm[b, c], _ = AG.mel_vjp(yb, sr, grow, args['ms_fmax'])
                dy[c][k].append(d)
    return dict(net, dy_deg=dy[0], dy_ref=dy[1], mel_margin=mm, n_wins=n_wins, x=x)
