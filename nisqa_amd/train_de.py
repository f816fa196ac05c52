"""One optimiser step of the double-ended model NISQA_DE on the GPU (config/train_nisqa_double_ended.yaml) -- DESIGN.md 4.8.1.

What the reference does per batch at nisqa/NISQA_model.py:131-152 with ``model`` = NISQA_DE (NISQA_lib.py:406-424), every
operator a HIP kernel:
  * ``self.cnn(x, n_wins_x)`` then ``self.cnn(y, n_wins_y)``: TWO calls of the shared AdaptCNN in train mode -- train._FlatTrainer.
    _cnn_fwd on the degraded clips, then on the reference clips.  Every BatchNorm normalises a side by that side's batch statistics,
    the running buffers are updated twice (degraded first; num_batches_tracked + 2 per step), Dropout2d draws per call, and the
    shared parameters' gradients are the sum of the two calls' (the second backward pass writes a buffer of its own, which is
    then added);
  * ``self.time_dependency`` on each side: one token batch of the 2B clips, degraded first (nothing couples clips);
  * Alignment (dot / cosine, hard) + Fusion: nisqa_de_align_fuse_packed, which also writes the chosen reference index of every
    degraded token; backward: nisqa_de_align_fuse_bwd (the adjoint of the fusion and of the gather; the argmax has no gradient);
  * ``self.time_dependency_2`` on the B degraded clips at input width 192 / 128 (its linear.weight [64][F] in natural column
    order), the PoolAttFF head, biasLoss.get_loss, Adam.
The attention blocks run operator by operator (train._AttTrainer); only conv2..6 depend on ``precision``.

Dropout masks (``masks=`` of the step entry points; absent: drawn by nisqa_dropout_mask), each 0 or 1 / (1 - p):
  'cnn_d1' .. 'cnn_d4'          [S_deg][C]   Dropout2d sites of the CNN call on the degraded clips (C = 32, 64, 64, 64)
  'ref_cnn_d1' .. 'ref_cnn_d4'  [S_ref][C]   the same sites of the call on the reference clips
  'td<l>_p'                     [sum L^2]    first self-attention, layer l: attention probabilities, the 2B clips packed (degraded
                                             clips first, then the reference clips)
  'td<l>_1', '_f', '_2'         [S_deg + S_ref][64]   its dropout1, FFN dropout, dropout2
  'td2_<l>_p', '_1', '_f', '_2' the same four sites of the second self-attention, over the B degraded clips.
"""
import os

import numpy as np
import torch

from .engine import HipNisqa, check_de_args, DE_ALIGN, DE_FUSE, DE_FUSE_WIDTH
from .train import _AttTrainer, _ClipSet, _ptr, bias_rows, step_tables

PRECISIONS = ('f32', 'mixed', 'bf16x3', 'bf16x6', 'f16x4')
_CNN_SITES = (('cnn_d1', 32), ('cnn_d2', 64), ('cnn_d3', 64), ('cnn_d4', 64))
_TD1, _TD2 = 'time_dependency.model.', 'time_dependency_2.model.'


def check_de_train_args(args, precision=None):
    """The NISQA_DE configurations HipTrainerDE trains -> precision; everything else raises NotImplementedError naming the option,
    before any GPU work.  Trained: what engine.check_de_args runs (cnn_model=adapt with the nisqa.tar geometry, td = td_2 = self_att
    with d_model 64, one head, h 64, pool=att, de_align dot / cosine, the three de_fuse, de_fuse_dim null) with
    de_align_apply=hard and pool_att_dropout 0."""
    g = lambda k, d=None: args.get(k, d)
    if g('model') != 'NISQA_DE':
        raise NotImplementedError('HIP double-ended training step covers model=NISQA_DE, got model={}'.format(g('model')))
    check_de_args(args)                                                    # de_align bahd / luong / distance / none, de_fuse_dim, td_2=lstm, ...
    if g('de_align_apply', 'hard') != 'hard':
        raise NotImplementedError('NISQA_DE training: de_align_apply={} is not built (hard only: soft alignment needs the backward of '
                                  'the scores, the softmax and the cosine normalisation)'.format(g('de_align_apply')))
    if float(g('pool_att_dropout') or 0):
        raise NotImplementedError('NISQA_DE training: pool_att_dropout > 0 is not built (0 in every shipped config)')
    prec = precision or os.environ.get('NISQA_HIP_TRAIN_PRECISION', 'bf16x6')
    if prec not in PRECISIONS:
        raise ValueError('precision must be f32, mixed, bf16x3, bf16x6 or f16x4, got {}'.format(prec))
    return prec


class HipTrainerDE(_AttTrainer):
    LAYOUT = 'nisqa_amd flat buffer (HipTrainerDE.keys / kshape order)'
    FEAT_W = _TD1 + 'linear.weight'            # the only Linear on the flattened CNN output; time_dependency_2's keeps its columns

    def __init__(self, args, state_dict, device=None, lr=1e-3, precision=None):
        """args / state_dict: a NISQA_DE model (check_de_train_args); precision of conv2..6 as HipTrainer's (default 'bf16x6'),
        everything else fp32 in every mode."""
        self.precision = check_de_train_args(args, precision)
        a = args
        single = dict(a, model='NISQA', td_2='skip')                      # mel front end + geometry checks: the single-ended engine
        self.eng = HipNisqa(single, state_dict, device, precision='f32')
        self.lib, self.device, self.args = self.eng.lib, self.eng.device, args
        self.lr = float(lr)
        self.n_layers, self.n_layers2 = int(a['td_sa_num_layers']), int(a['td_2_sa_num_layers'])
        self.align, self.fuse = DE_ALIGN[a.get('de_align', 'dot')], DE_FUSE[a.get('de_fuse', 'x/y/-')]
        self.fuse_width = DE_FUSE_WIDTH[a.get('de_fuse', 'x/y/-')]
        self.heads = ['pool.model.']
        self.p_cnn, self.p_td, self.p_td2 = float(a['cnn_dropout']), float(a['td_sa_dropout']), float(a['td_2_sa_dropout'])
        w2 = state_dict[_TD2 + 'linear.weight']
        if tuple(w2.shape) != (64, self.fuse_width):
            raise ValueError('{}linear.weight is {}, de_fuse={} needs [64, {}]'.format(_TD2, tuple(w2.shape), a.get('de_fuse'),
                                                                                    self.fuse_width))
        self._init_params(state_dict, 64 + 8 * (self.n_layers + self.n_layers2))
        # the second CNN backward pass of a step writes here (train._FlatTrainer._cnn_bwd overwrites some gradients)
        self.gflat2 = torch.zeros_like(self.gflat)
        self.G2 = {k: self.gflat2[self.off[k]:self.off[k] + int(np.prod(self.kshape[k]))].view(self.kshape[k])
                   for k in self.keys if k.startswith('cnn.')}
        self._cnn_lo = min(self.off[k] for k in self.G2)
        self._cnn_hi = max(self.off[k] + int(np.prod(self.kshape[k])) for k in self.G2)
        pools = [tuple(a['cnn_pool_1']), tuple(a['cnn_pool_2']), tuple(a['cnn_pool_3'])]
        geo = [(48, 15, pools[0]), (24, 7, pools[1]), (12, 5, (12, 5)), (12, 5, pools[2]), (6, 3, (6, 3)), (6, 1, (6, 1))]
        self._init_cnn(geo, 0, self.lib.nisqa_conv1_bn_act_pool_fwd, self.lib.nisqa_conv1_bn_act_pool_bwd)
        self._prep_key = None
        self.last_idx = None

    # ---- batch bookkeeping ---------------------------------------------------------------------------------
    def _prepare(self, nw_deg, nw_ref):
        Lx, Ly = np.asarray(nw_deg, dtype=np.int64).reshape(-1), np.asarray(nw_ref, dtype=np.int64).reshape(-1)
        if len(Lx) == 0 or len(Lx) != len(Ly) or (Lx < 1).any() or (Ly < 1).any():
            raise ValueError('a step needs as many reference clips as degraded clips, each of at least one segment; got n_wins '
                             '{} and {}'.format(Lx.tolist(), Ly.tolist()))
        B = len(Lx)
        L12 = np.concatenate([Lx, Ly])
        key = L12.tobytes()
        if key != self._prep_key:
            # index tables of the step, one upload: the 2B clips of the first self-attention ('a_'), the B degraded clips of the
            # second one and of the pooling, the reference side's segment offsets for its CNN call, the alignment's vectors
            pa, tiles_a = step_tables(L12)
            pd, tiles_d = step_tables(Lx)
            parts = [('a_' + k, v) for k, v in pa] + pd
            parts += [('r_seg_off', np.concatenate(([0], np.cumsum(Ly))).astype(np.int32)), ('n_wins', L12.astype(np.int32)),
                      ('tile_off', np.concatenate(([0], np.cumsum((Lx + 63) // 64))).astype(np.int32))]
            host, buf, tv = self._upload_tables(parts)
            self._prep_key, self._prep_host, self._prep_buf = key, host, buf       # host stays alive until the copy has run
            self._prep_tables = (tv, tiles_a, tiles_d)
        tv, tiles_a, tiles_d = self._prep_tables
        self._tv = tv
        self.B, self.Lx, self.Ly = B, Lx, Ly
        self._cs_all, self._cs_deg = _ClipSet(L12, tv, tiles_a, 'a_'), _ClipSet(Lx, tv, tiles_d)
        self.Sx, self.Sy = int(Lx.sum()), int(Ly.sum())
        self._n_tiles = int(((Lx + 63) // 64).sum())
        self._sums.zero_()
        self._sum_i = 0
        self._casts = []
        # every dropout mask of the step in one buffer: the two CNN calls' sites, then the two self-attentions'
        self._mask_buf, self._mask_pos = None, {}
        sizes = [(pfx + k, S * c) for pfx, S in (('', self.Sx), ('ref_', self.Sy)) for k, c in _CNN_SITES]
        marks = [len(sizes)]
        for fmt, cs, n in (('td%d_%s', self._cs_all, self.n_layers), ('td2_%d_%s', self._cs_deg, self.n_layers2)):
            for l in range(n):
                sizes += [(fmt % (l, 'p'), cs.n_sq)] + [(fmt % (l, t), cs.S * 64) for t in ('1', 'f', '2')]
            marks.append(len(sizes))
        o, starts = 0, []
        for k, n in sizes:
            starts.append(o)
            self._mask_pos[k] = (o, n)
            o += (n + 3) // 4 * 4
        starts.append(o)
        self._mask_total = o
        self._mask_marks = (0, starts[marks[0]], starts[marks[1]], o)

    def _mask_draws(self):
        m = self._mask_marks
        return ((m[0], m[1], self.p_cnn), (m[1], m[2], self.p_td), (m[2], m[3], self.p_td2))

    def _side(self, ref):
        """the clip set _cnn_fwd / _cnn_bwd work on: the degraded clips or the reference clips"""
        self.S = self.Sy if ref else self.Sx
        self.seg_off = self._tv['r_seg_off'] if ref else self._cs_deg.seg_off

    # ---- entry points ----------------------------------------------------------------------------------------
    def step_spec(self, specs_deg, specs_ref, y, masks=None, bias=None):
        """specs_deg / specs_ref: the pairs' [48, T] dB spectrograms, row by row -- used by the parity tests."""
        return self._step(self._spec_batch(specs_deg), self._spec_batch(specs_ref), y, masks, bias)

    def step_pcm(self, deg, ref, y, masks=None, bias=None):
        """deg / ref: (pcm, plan, sr) of the degraded and of the reference clips (float32 device tensor, clips back to back)."""
        return self.step_groups([deg], [ref], y, masks, bias)

    def step_mel(self, deg, ref, y, masks=None, bias=None):
        """deg / ref: (mel [frames][48], frame offsets on the device, n_wins, clip floors) of the degraded and of the reference
        clips, row k of one the pair of row k of the other -- what _mel_groups returns per side and what melstore.MelStore.batch
        serves from the two resident stores."""
        return self._step(tuple(deg), tuple(ref), y, masks, bias)

    def step_groups(self, groups_deg, groups_ref, y, masks=None, bias=None):
        """One step on pairs whose clips are staged as groups, [(pcm, plan, sr), ...] per side -- one group per run of one
        sample rate, as train.concat_groups lays them out.  The two sides are grouped independently (a pair's files may differ in
        rate), but clip k of the degraded side, counted through its groups, and clip k of the reference side are one pair; ``y``,
        ``bias`` and the returned ``y_hat`` follow that order."""
        return self._step(self._mel_groups(groups_deg), self._mel_groups(groups_ref), y, masks, bias)

    # ---- the step ------------------------------------------------------------------------------------------
    def _step(self, deg, ref, y, masks, bias):
        self._prepare(deg[2], ref[2])
        B, Sx, Sy, F, st = self.B, self.Sx, self.Sy, self.fuse_width, self._st()
        tv, cs_all, cs_deg = self._tv, self._cs_all, self._cs_deg
        self.gflat.zero_()
        self.gflat2.zero_()
        y_dev = self._upload(y, 1)
        bias_dev = None if bias is None else self._upload(bias_rows(bias, B, 1)[0], 4)

        # ================= forward =================
        feat = self._new(Sx + Sy, 384)                                         # [token][6][64]: degraded clips, then reference clips
        self._side(False)
        cnn_d, _ = self._cnn_fwd(deg[0], deg[1], deg[3], masks, feat[:Sx])
        self._side(True)
        cnn_r, _ = self._cnn_fwd(ref[0], ref[1], ref[3], masks, feat[Sx:], mask_pfx='ref_', pack=False)
        x1, rec1 = self._sa_fwd(cs_all, feat, 384, _TD1, self.n_layers, masks, 'td%d_%s', self.p_td)
        fused, idx = self._new(Sx, F), self._new(Sx, dtype=torch.int32)
        off, nw = tv['a_seg_off'], tv['n_wins']
        self._ck(self.lib.nisqa_de_align_fuse_packed(_ptr(x1), _ptr(off), _ptr(nw), _ptr(off, B), _ptr(nw, B), _ptr(tv['tile_off']), B,
                                                     self._n_tiles, self.align, self.fuse, F, _ptr(fused), _ptr(idx), st),
                 'nisqa_de_align_fuse_packed')
        x2, rec2 = self._sa_fwd(cs_deg, fused, F, _TD2, self.n_layers2, masks, 'td2_%d_%s', self.p_td2)
        y_hat, loss, dx2 = self._heads_loss(cs_deg, x2, y, y_dev, bias_dev, False)

        # ================= backward =================
        dfused = self._sa_bwd(rec2, dx2)                                       # [Sx][F]
        dx1 = self._new(Sx + Sy, 64)                                           # every row is written: no clearing
        self._ck(self.lib.nisqa_de_align_fuse_bwd(_ptr(dfused), F, _ptr(idx), _ptr(off), _ptr(nw), _ptr(off, B), _ptr(nw, B), B,
                                                  int(max(self.Lx.max(), self.Ly.max())), self.fuse, _ptr(dx1), _ptr(dx1), st),
                 'nisqa_de_align_fuse_bwd')
        dfeat = self._sa_bwd(rec1, dx1)                                        # [Sx + Sy][384]
        rec1 = rec2 = None
        self._side(False)
        self._cnn_bwd(cnn_d, [dfeat[:Sx]])
        self._side(True)
        own = self.G
        self.G = dict(own, **self.G2)                                          # the second call's CNN gradients: their own buffer
        try:
            self._cnn_bwd(cnn_r, [dfeat[Sx:]])
        finally:
            self.G = own
        lo, n = self._cnn_lo, self._cnn_hi - self._cnn_lo
        self._ew(4, self.gflat[lo:lo + n], aux=self.gflat2[lo:lo + n], rows=1, cols=n)
        self.last_idx = idx
        return self._finish_step(y_hat, loss)
