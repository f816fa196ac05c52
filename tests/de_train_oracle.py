"""NISQA_DE training test support (not a test module): a float64 CPU restatement of ONE train-mode step of the double-ended model
-- ``model.train(); y_hat = model(x, n_wins); loss = biasLoss.get_loss(...); loss.backward()`` (reference nisqa/NISQA_model.py:
131-152 around NISQA_DE.forward, nisqa/NISQA_lib.py:406-424) -- as a torch-autograd function of an unchanged state_dict, built from
the oracle's operators (oracle/train.py, oracle/net.py) and the alignment / fusion restatement of tests/de_oracle.py.  Dropout masks
and the bias mapping are inputs, in the layout HipTrainerDE documents (nisqa_amd/train_de.py).

Restated: two calls of the shared AdaptCNN in train mode, the degraded clips first (each call normalises by its own batch
statistics and updates the running buffers: two updates per step); the shared first self-attention per clip; hard alignment (the
argmax of the dot / cosine scores over the reference clip's tokens carries no gradient; the gather does) and fusion; the second
self-attention on the fused rows; PoolAttFF; the NaN-aware MSE through the optional cubic bias map.
``pooled_bn=True`` is the WRONG model on purpose: one CNN pass over all 2B clips with pooled statistics -- what a trainer that took
that shortcut would compute (tests/test_gpu_train_de.py shows the step is far from it).
tests/test_de_train_host.py pins this against the reference's own modules.
"""
import numpy as np
import torch

import de_oracle as DO
from oracle import net as onet
from oracle.train import adapt_cnn_train, nan_mse_loss, param_keys, self_attention_train

CNN_SITES = (('cnn_d1', 32), ('cnn_d2', 64), ('cnn_d3', 64), ('cnn_d4', 64))
TD2 = 'time_dependency_2.model.'
FRAMES_DEG, FRAMES_REF = [15, 40, 97, 300, 260], [40, 15, 97, 260, 300]       # n_wins (1,7) (7,1) (21,21) (72,62) (62,72) at hop 4


def de_train_args(align='cosine', fuse='x/y/-', **kw):
    """the shipped double-ended recipe with the reference's dropout probabilities switched off unless given"""
    base = dict(cnn_dropout=0.0, td_sa_dropout=0.0, td_2_sa_dropout=0.0, pool_att_dropout=0.0)
    base.update(kw)
    return DO.de_args(align, 'hard', fuse, **base)


def segments(specs, args):
    """[48, T] spectrograms -> (valid segments [S, 1, 48, 15] clip after clip, n_wins [B])"""
    xs, nw = zip(*[onet.segment_specs(s, args['ms_seg_length'], args['ms_seg_hop_length'], None) for s in specs])
    return torch.cat([torch.as_tensor(x)[:n] for x, n in zip(xs, nw)], 0), np.asarray(nw, dtype=np.int64)


def random_masks(seed, Lx, Ly, n1, n2, p):
    """Dropout multipliers (0 or 1 / (1 - p)) for every site of a step, in HipTrainerDE's layout; every mask is its own draw."""
    rng = np.random.default_rng(seed)
    Lx, Ly = np.asarray(Lx, np.int64), np.asarray(Ly, np.int64)
    L12 = np.concatenate([Lx, Ly])
    draw = lambda *shape: ((rng.random(shape) >= p) / (1.0 - p)).astype(np.float32)
    m = {}
    for pfx, S in (('', int(Lx.sum())), ('ref_', int(Ly.sum()))):
        for k, c in CNN_SITES:
            m[pfx + k] = draw(S, c)
    for fmt, L, n in (('td%d_%s', L12, n1), ('td2_%d_%s', Lx, n2)):
        for l in range(n):
            m[fmt % (l, 'p')] = draw(int((L * L).sum()))
            for t in ('1', 'f', '2'):
                m[fmt % (l, t)] = draw(int(L.sum()), 64)
    return m


def _cnn_masks(masks, pfx, dtype):
    if masks is None:
        return None
    return {k: torch.as_tensor(masks[pfx + k]).to(dtype)[:, :, None, None] for k, _ in CNN_SITES if pfx + k in masks}


def _clip_masks(masks, fmt, L, n_layers, dtype):
    """the packed per-site masks of one self-attention -> {(clip, 'td<l>_<site>'): tensor}, the form oracle.train takes"""
    out = {}
    if masks is None:
        return out
    L = np.asarray(L, np.int64)
    tok = np.concatenate(([0], np.cumsum(L)))
    sq = np.concatenate(([0], np.cumsum(L * L)))
    for l in range(n_layers):
        for t in ('p', '1', 'f', '2'):
            k = fmt % (l, t)
            if k not in masks:
                continue
            v = torch.as_tensor(np.asarray(masks[k])).to(dtype)
            for b, n in enumerate(L):
                out[(b, 'td%d_%s' % (l, t))] = (v.reshape(-1)[sq[b]:sq[b + 1]].reshape(n, n) if t == 'p'
                                                 else v.reshape(-1, 64)[tok[b]:tok[b + 1]])
    return out


def _fuse(x, y, fuse):
    if fuse == 'x/y/-':
        return torch.cat([x, y, x - y], 1)
    if fuse == '+/-':
        return torch.cat([x + y, x - y], 1)
    return torch.cat([x, y], 1)


def train_step(sd, args, segs_d, nw_d, segs_r, nw_r, y, masks=None, bias=None, dtype=torch.float64, pooled_bn=False):
    """-> dict(loss, y_hat [B, 1], grads {key: array}, idx [per pair: hard indices], gap (smallest top-2 score gap over the degraded
    tokens with at least two reference tokens), bufs (BatchNorm running buffers after the step's two updates))."""
    sd = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in sd.items()}
    keys = param_keys(sd)
    for k in keys:
        sd[k] = sd[k].to(dtype).requires_grad_(True)
    nw_d, nw_r = np.asarray(nw_d, np.int64), np.asarray(nw_r, np.int64)
    B, Sx = len(nw_d), int(nw_d.sum())
    pools = (args['cnn_pool_1'], args['cnn_pool_2'], args['cnn_pool_3'])
    xd, xr = torch.as_tensor(segs_d).to(dtype), torch.as_tensor(segs_r).to(dtype)
    md, mr = _cnn_masks(masks, '', dtype), _cnn_masks(masks, 'ref_', dtype)
    stats = [{}, {}]
    if pooled_bn:
        mm = None if masks is None else {k: torch.cat([md[k], mr[k]], 0) for k in md}
        feat = adapt_cnn_train(sd, torch.cat([xd, xr], 0), pools, mm, stats[0])
        fd, fr = feat[:Sx], feat[Sx:]
    else:
        fd = adapt_cnn_train(sd, xd, pools, md, stats[0])
        fr = adapt_cnn_train(sd, xr, pools, mr, stats[1])
    n1, n2 = args['td_sa_num_layers'], args['td_2_sa_num_layers']
    m1 = _clip_masks(masks, 'td%d_%s', np.concatenate([nw_d, nw_r]), n1, dtype)
    m2 = _clip_masks(masks, 'td2_%d_%s', nw_d, n2, dtype)
    out, idxs, gap = [], [], np.inf
    ox = oy = 0
    for b in range(B):
        nx, ny = int(nw_d[b]), int(nw_r[b])
        tx = self_attention_train(sd, fd[ox:ox + nx], n1, m1, b)
        ty = self_attention_train(sd, fr[oy:oy + ny], n1, m1, B + b)
        att = DO.scores(tx.detach().numpy(), ty.detach().numpy(), args['de_align'])
        idx = att.argmax(1)
        if ny > 1:
            srt = np.sort(att, 1)
            gap = min(gap, float((srt[:, -1] - srt[:, -2]).min()))
        idxs.append(idx)
        fused = _fuse(tx, ty[torch.from_numpy(idx)], args['de_fuse'])
        x2 = self_attention_train(sd, fused, n2, m2, b, pfx=TD2)
        out.append(onet.pool_att_ff(sd, x2, 'pool.model.'))
        ox, oy = ox + nx, oy + ny
    y_hat = torch.stack(out).reshape(B, 1)
    loss = nan_mse_loss(y_hat, torch.as_tensor(np.asarray(y)).to(dtype).reshape(B, 1),
                        None if bias is None else torch.as_tensor(np.asarray(bias)).to(dtype).reshape(B, 4))
    grads = dict(zip(keys, torch.autograd.grad(loss, [sd[k] for k in keys])))
    bufs = {}
    for i in range(1, 7):
        p = 'cnn.model.bn%d.' % i
        rm, rv = sd[p + 'running_mean'].to(dtype), sd[p + 'running_var'].to(dtype)
        for st in (stats[:1] if pooled_bn else stats):                 # one update per CNN call, the degraded clips' first
            mean, var, cnt = st['bn%d' % i]
            rm = 0.9 * rm + 0.1 * mean
            rv = 0.9 * rv + 0.1 * var * (cnt / (cnt - 1))
        bufs[p + 'running_mean'], bufs[p + 'running_var'] = rm.numpy(), rv.numpy()
    return {'loss': float(loss.detach()), 'y_hat': y_hat.detach().numpy(), 'grads': {k: g.numpy() for k, g in grads.items()},
            'idx': idxs, 'gap': gap, 'bufs': bufs}
