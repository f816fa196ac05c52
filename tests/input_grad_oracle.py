"""Support of the input-gradient tests (not a test module): the float64 autograd gradient of the oracle network (oracle/net.py:
adapt_cnn -> self_attention -> pool_att_ff, plain torch, eval-mode semantics) with respect to the segment tensor, clip by clip,
the per-segment TIE MARGIN of that evaluation, and the seeded cases the CPU tests, the GPU tests and the fixtures share.

Tie margin of a segment: the smaller of (a) the smallest gap between the two largest values of a pooling window whose maximum is
positive, over the three pooled layers, and (b) the smallest |BatchNorm output| over the six layers.  Below it an fp32 evaluation
may legitimately pick another argmax or the other side of a ReLU than float64 does, and the gradient of THAT segment jumps; the
other segments are unaffected (the values are continuous and the CNN works per segment).
"""
import numpy as np
import torch
import torch.nn.functional as F

import lstm_train_oracle as LT
from nisqa_amd import synth
from oracle import net as onet

ARGS = {'NISQA_DIM': synth.DIM_ARGS, 'NISQA': synth.MOS_ARGS}
POOLED = {1: 'cnn_pool_1', 2: 'cnn_pool_2', 4: 'cnn_pool_3'}


def heads_of(model):
    return ['pool_layers.%d.model.' % h for h in range(5)] if model == 'NISQA_DIM' else ['pool.model.']


def _win(i, n_in, n_out):
    return (i * n_in) // n_out, -(-((i + 1) * n_in) // n_out)


def cnn_margins(sd, args, x):
    """x [N, 1, 48, 15] float64 -> tie margin [N] of adapt_cnn's evaluation (see the module docstring)"""
    margin = torch.full((x.shape[0],), float('inf'), dtype=x.dtype)
    pfx = 'cnn.model.'
    for i in range(1, 7):
        x = F.conv2d(x, sd[pfx + 'conv%d.weight' % i], sd[pfx + 'conv%d.bias' % i], padding=(1, 0) if i == 6 else (1, 1))
        x = F.batch_norm(x, sd[pfx + 'bn%d.running_mean' % i], sd[pfx + 'bn%d.running_var' % i], sd[pfx + 'bn%d.weight' % i],
                         sd[pfx + 'bn%d.bias' % i], False, 0.0, onet.BN_EPS)
        margin = torch.minimum(margin, x.abs().flatten(1).min(1)[0])
        x = F.relu(x)
        if i in POOLED:
            ho, wo = args[POOLED[i]]
            h, w = x.shape[2:]
            for oy in range(ho):
                y0, y1 = _win(oy, h, ho)
                for ox in range(wo):
                    x0, x1 = _win(ox, w, wo)
                    top = x[:, :, y0:y1, x0:x1].flatten(2).topk(2, dim=2)[0]
                    gap = torch.where(top[..., 0] > 0, top[..., 0] - top[..., 1], torch.full_like(top[..., 0], float('inf')))
                    margin = torch.minimum(margin, gap.min(1)[0])
            x = F.adaptive_max_pool2d(x, (ho, wo))
    return margin


def oracle(sd, args, x, n_wins, gs):
    """sd: state_dict, x [B, L, 1, 48, 15] (padding rows are never read), n_wins [B], gs: list of g [B, heads] ->
    dict(y [B, heads], dx: one [B, L, 1, 48, 15] per g with zero padding rows, margin [B, L] with inf at the padding rows), float64"""
    sd = {k: onet._t(v).double() for k, v in sd.items() if k.split('.')[-1] != 'num_batches_tracked'}
    x = torch.as_tensor(np.asarray(x)).double()
    B, L = x.shape[:2]
    heads = heads_of(args['model'])
    y = np.zeros((B, len(heads)))
    dx = [np.zeros(tuple(x.shape)) for _ in gs]
    margin = np.full((B, L), np.inf)
    for b in range(B):
        n = int(n_wins[b])
        xb = x[b, :n].clone().requires_grad_(True)
        feat = onet.adapt_cnn(sd, xb, args['cnn_pool_1'], args['cnn_pool_2'], args['cnn_pool_3'])
        td = onet.self_attention(sd, feat, args['td_sa_num_layers'])
        yb = torch.cat([onet.pool_att_ff(sd, td, hp) for hp in heads])
        y[b] = yb.detach().numpy()
        for k, g in enumerate(gs):
            gb = torch.as_tensor(np.asarray(g[b], dtype=np.float64))
            dx[k][b, :n] = torch.autograd.grad((yb * gb).sum(), xb, retain_graph=True)[0].numpy()
        with torch.no_grad():
            margin[b, :n] = cnn_margins(sd, args, xb.detach()).numpy()
    return {'y': y, 'dx': dx, 'margin': margin}


def segment_tensor(specs, args, L=None, fill=0.0):
    """[48, T] spectrograms -> (x [B, L, 1, 48, 15] float32 with ``fill`` in the padding rows, n_wins [B])"""
    segs = [onet.segment_specs(s, args['ms_seg_length'], args['ms_seg_hop_length'], None) for s in specs]
    n_wins = np.array([n for _, n in segs], dtype=np.int64)
    L = int(n_wins.max()) if L is None else L
    x = np.full((len(specs), L, 1, 48, 15), fill, dtype=np.float32)
    for b, (xs, n) in enumerate(segs):
        x[b, :n] = xs.numpy()
    return x, n_wins


def one_hot(B, H, h):
    g = np.zeros((B, H), dtype=np.float32)
    g[:, h] = 1.0
    return g


# the small case: three clips of 1, 3 and 2 segments padded to L = 4; the tile-edge case: 65, 1 and 32 segments
SMALL = dict(seed_sd=30, seed_batch=530, frames=[15, 23, 19], L=4, n_wins=[1, 3, 2], seed_g=31)
EDGE = dict(seed_sd=0, seed_batch=700, frames=[271, 15, 140], L=None, n_wins=[65, 1, 32], seed_g=701)


def case(model, spec=SMALL, fill=0.0):
    """-> (state_dict, args, x float32 [B, L, 1, 48, 15], n_wins, g float32 [B, heads]) of a seeded case"""
    args = dict(ARGS[model])
    sd = synth.random_state_dict(spec['seed_sd'], model)
    specs, _ = LT.batch(spec['seed_batch'], spec['frames'])
    x, n_wins = segment_tensor(specs, args, spec['L'], fill)
    assert n_wins.tolist() == spec['n_wins']
    g = np.random.default_rng(spec['seed_g']).standard_normal((len(n_wins), len(heads_of(model)))).astype(np.float32)
    return sd, args, x, n_wins, g


def clip_error(got, want):
    """max |got - want| / max |want| per clip -> [B]"""
    B = want.shape[0]
    d = np.abs(np.asarray(got, dtype=np.float64) - want).reshape(B, -1).max(1)
    return d / np.abs(want).reshape(B, -1).max(1)
