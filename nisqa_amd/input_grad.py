"""d model(x, n_wins) / d x for the CNN-SA-AP checkpoints (NISQA / NISQA_DIM), the StandardCNN + BiLSTM ones and the double-ended
NISQA_DE ones, on the GPU.

After ``model.eval()`` the reference's modules are differentiable functions of the segment tensor x [B, L, 1, 48, 15]
(nisqa/NISQA_lib.py:137-142, 260-268): people use NISQA as a perceptual loss, for saliency maps and for adversarial probing.
``InputGrad(engine, state_dict)(x, n_wins, grad_out)`` is the backward of that function: BatchNorm on the running statistics, no
dropout, the key mask over n_wins, rows l >= n_wins[b] of the result exactly zero.

Nothing is kept from the forward call (HipNisqa.forward_segments runs the fused inference kernels, which keep no activation): the
backward RECOMPUTES the network operator by operator with its activations in HBM -- a backward call costs a second forward --
and walks back through it:
  CNN        eval-mode layers of csrc/input_grad.hip (conv1 on the segment rows, frozen-statistics BatchNorm + ReLU + adaptive
             max-pool forward and backward, conv1's input gradient) around the segment-resident convolutions of the training
             step (csrc/train_conv.hip: forward and input gradient of conv2..6, exact fp32 for precision 'f32', three bf16 terms
             and six products for 'bf16x6');
  attention  _AttTrainer._sa_fwd / _sa_bwd without dropout masks: the eval-mode function;
  heads      attention pooling forward and the input half of its backward, fed with the caller's grad_out; and / or the backward
             of the score's per-segment profile (nisqa_pool_profile_bwd), fed with cotangents per token.
Parameters get no gradient here (that is the trainers' business): the weight-gradient GEMMs and column sums of the borrowed
operators are not run.

``InputGradLSTM`` is the same for the StandardCNN + BiLSTM models (nisqa_tts.tar, pool=last_step_bi; the CNN-LSTM-AVG recipe,
pool=avg or max), whose grad_out is [B, 1]:
  CNN        the same eval-mode layers, with the StandardCNN's pools -- pool_first = MaxPool2d(2, 2, padding (0, 1)), which no
             adaptive window expresses, and the 2 x 2 pools after conv2 and conv4 -- by nisqa_bn_eval_act_maxpool2_fwd / _bwd, and
             conv2..6 by the exact fp32 implicit GEMM (nisqa_conv3x3_gemm modes 0 and 1), whatever the engine's precision;
  BiLSTM     fc_out, nisqa_lstm_train_fwd (gates and cell states kept) and nisqa_lstm_train_bptt without the bias sums, then
             dx20 = dgates w_ih and dfeat = dx20 fc_out.weight;
  pooling    PoolLastStepBi / PoolAvg / PoolMax inside the two LSTM entries; dpooled = grad_out pool.model.linear.weight.

``InputGradDE`` is the same for NISQA_DE (x [B, L, 2, 48, 15], n_wins [B, 2], grad_out [B, 1]): InputGrad's operators around the
alignment + fusion kernels of csrc/de_align.hip, hard (nisqa_de_align_fuse_packed / _bwd) or soft (nisqa_de_align_soft_packed /
nisqa_de_align_soft_bwd) -- DESIGN.md 4.8.2.  Its ``packed`` entry takes and returns the 2B-clip layout the engine's audio path
holds (degraded clips, then reference clips) and can leave out one side's CNN backward -- DESIGN.md 4.8.3.
"""
import numpy as np
import torch

from .engine import check_segments, LSTM_POOL_MODE
from .train import _AttTrainer, _ClipSet, _CONV, _FlatTrainer, _ptr, step_tables
from .train_lstm import FC_W, GEO, HipTrainerLSTM, LSTM_KEYS, POOL_KEYS

_TD1, _TD2 = 'time_dependency.model.', 'time_dependency_2.model.'

PRECISIONS = ('f32', 'bf16x6')          # the engine precisions whose operands are the reference's fp32 values


def check_precision(precision):
    """A gradient is built for the engine precisions that carry fp32 operands exactly; the fast ones refuse, naming themselves.
    No GPU is touched."""
    if precision not in PRECISIONS:
        raise NotImplementedError('the gradient of model(x, n_wins) with respect to x is built for the engine precisions {}, '
                                  'not for {}'.format(' and '.join(PRECISIONS), precision))
    return precision


class _EvalCNN(object):
    """The eval-mode CNN with its activations kept and the walk back to x, for a trainer's parameter layout (self.P, self.bn,
    self._geo): conv1 on the segment rows, six frozen-statistics BatchNorm + ReLU (+ pool) layers, conv2..6 through the subclass's
    ``_conv_eval``.  MAXPOOL2[i] = the pad_w of a MaxPool2d(2, stride 2, padding (0, pad_w)) behind layer i (the StandardCNN);
    every other layer pools by the adaptive windows of its geometry (the AdaptCNN), the identity among them."""
    MAXPOOL2 = {}

    def _bn_ptrs(self, i):
        P = self.P
        return (_ptr(P['cnn.model.bn%d.weight' % i]), _ptr(P['cnn.model.bn%d.bias' % i]), _ptr(self.bn[i]['mean']),
                _ptr(self.bn[i]['var']))

    def _cnn_fwd_eval(self, x, seg_off, B, S):
        """x [B, L, 1, 48, 15] -> (per layer (z, arg), the features [S][pixels * 64] in (pixel, c) order)"""
        L_, P, st = self.lib, self.P, self._st()
        recs, act = [], None
        for i in range(1, 7):
            co = _CONV[i - 1][1]
            h, w, (ho, wo) = self._geo[i - 1]
            bias = P['cnn.model.conv%d.bias' % i]
            z = self._new(S * h * w, co)
            if i == 1:
                self._ck(L_.nisqa_conv1_segments_fwd(_ptr(x), x.shape[1], _ptr(seg_off), B, S, _ptr(P['cnn.model.conv1.weight']),
                                                     _ptr(bias), _ptr(z), st), 'nisqa_conv1_segments_fwd')
            else:
                self._conv_eval(0, i, act, z, S, bias)
            arg = None if (h, w) == (ho, wo) else self._new(S, ho * wo, co, dtype=torch.int32)
            act = self._new(S, ho * wo, co)
            if i in self.MAXPOOL2:
                self._ck(L_.nisqa_bn_eval_act_maxpool2_fwd(_ptr(z), *self._bn_ptrs(i), S, h, w, co, self.MAXPOOL2[i], _ptr(act),
                                                           arg.data_ptr(), st), 'nisqa_bn_eval_act_maxpool2_fwd')
            else:
                self._ck(L_.nisqa_bn_eval_act_pool_fwd(_ptr(z), *self._bn_ptrs(i), S, h, w, co, ho, wo, _ptr(act),
                                                       arg.data_ptr() if arg is not None else None, st), 'nisqa_bn_eval_act_pool_fwd')
            recs.append((z, arg))
        return recs, act.view(S, -1)

    def _cnn_bwd_eval(self, recs, da, seg_off, B, S, L, dx=None):
        """d / d features [S][pixels * 64] -> d / d x [B, L, 1, 48, 15] (written into ``dx`` where one is given); recs is emptied,
        layer by layer"""
        L_, st = self.lib, self._st()
        for i in range(6, 0, -1):
            ci, co = _CONV[i - 1]
            h, w, (ho, wo) = self._geo[i - 1]
            z, arg = recs.pop()
            dz = self._new(S * h * w, co)
            if i in self.MAXPOOL2:
                self._ck(L_.nisqa_bn_eval_act_maxpool2_bwd(_ptr(da), arg.data_ptr(), _ptr(z), *self._bn_ptrs(i), S, h, w, co,
                                                           self.MAXPOOL2[i], _ptr(dz), st), 'nisqa_bn_eval_act_maxpool2_bwd')
            else:
                self._ck(L_.nisqa_bn_eval_act_pool_bwd(_ptr(da), arg.data_ptr() if arg is not None else None, _ptr(z),
                                                       *self._bn_ptrs(i), S, h, w, co, ho, wo, _ptr(dz), st),
                         'nisqa_bn_eval_act_pool_bwd')
            if i == 1:
                break
            hi, wi = self._geo[i - 2][2]
            da = self._new(S, hi * wi, ci)
            self._conv_eval(1, i, dz, da, S)
        dx = self._new(B, L, 1, 48, 15) if dx is None else dx
        self._ck(L_.nisqa_conv1_segments_dgrad(_ptr(dz), _ptr(seg_off), B, L, _ptr(self.P['cnn.model.conv1.weight']), _ptr(dx), st),
                 'nisqa_conv1_segments_dgrad')
        return dx


def _check_grad_out(grad_out, B, H):
    if not torch.is_tensor(grad_out) or tuple(grad_out.shape) != (B, H):
        raise ValueError('expected grad_out of shape [{}, {}], got {}'.format(
            B, H, tuple(grad_out.shape) if torch.is_tensor(grad_out) else type(grad_out).__name__))


def _grad_out(grad_out, B, H, device, profile_cot=None):
    """grad_out checked and as float32 on the device; None is accepted (and returned) only beside a token-level cotangent"""
    if grad_out is None and profile_cot is not None and any(t is not None for t in profile_cot):
        return None
    _check_grad_out(grad_out, B, H)
    return grad_out.detach().to(device, dtype=torch.float32).contiguous()


class InputGrad(_EvalCNN, _AttTrainer):
    FEAT_W = 'time_dependency.model.linear.weight'

    def __init__(self, eng, state_dict):
        if eng.arch != 0:
            raise NotImplementedError('the gradient with respect to x is built for the CNN-SA-AP models (NISQA, NISQA_DIM)')
        self.precision = check_precision(eng.precision)
        self.eng, self.lib, self.device, self.args = eng, eng.lib, eng.device, eng.args
        self._pool_eng = eng                                # the HipNisqa that owns the pooling heads' profile blob
        self.n_layers = eng.n_layers
        self.heads = ['pool_layers.%d.model.' % h for h in range(5)] if eng.dim else ['pool.model.']
        self.p_cnn = self.p_td = 0.0
        state_dict = {k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in state_dict.items()}
        self._layout(state_dict)
        self.load_state_dict(state_dict)
        a = self.args
        pools = [tuple(a['cnn_pool_1']), tuple(a['cnn_pool_2']), tuple(a['cnn_pool_3'])]
        self._init_cnn([(48, 15, pools[0]), (24, 7, pools[1]), (12, 5, (12, 5)), (12, 5, pools[2]), (6, 3, (6, 3)), (6, 1, (6, 1))],
                       0, None, None)
        self.segconv = self.precision != 'f32'              # always segment-resident: 16-bit fragments unless exact fp32
        self._packed = False
        self._tab_key = None

    # the borrowed backward operators, input half only
    def _linear_bwd(self, dY, X, wk, bk, rows, n_in, n_out, need_dx=True):
        dX = self._new(rows, n_in)
        self._gemm(dY, self.P[wk], dX, rows, n_in, n_out, n_out, n_in, n_in)
        return dX

    def _ln_bwd(self, dY, xh, rs, gk, bk, rows):
        dX = self._new(rows, 64)
        self._ck(self.lib.nisqa_layernorm_bwd(_ptr(dY), _ptr(xh), _ptr(rs), _ptr(self.P[gk]), rows, _ptr(dX), self._st()),
                 'nisqa_layernorm_bwd')
        return dX

    def _tables(self, n):
        """The index tables of step_tables for clips of n[b] segments, kept while the counts repeat."""
        key = n.tobytes()
        if key != self._tab_key:
            parts, tiles = step_tables(n)
            host, buf, tv = self._upload_tables(parts)
            self._tab_key, self._tab = key, (host, buf, _ClipSet(n, tv, tiles))
        return self._tab[2]

    def _conv_eval(self, mode, i, src, dst, S, bias=None):
        """conv i forward (mode 0) or its input gradient (mode 1): the segment-resident convolutions of the training step, their
        weight fragments packed at the first call (the weights never change here)"""
        if not self._packed:
            self._pack_frags()
            if any(self._convs[k][0] is None or self._convs[k][1] is None for k in range(2, 7)):
                raise NotImplementedError('no segment-resident convolution for this CNN geometry')
            self._packed = True
        ci, co = _CONV[i - 1]
        hi, wi = self._geo[i - 2][2]
        fn, frags = self._convs[i][mode]
        self._ck(fn(mode, _ptr(src), _ptr(frags), _ptr(dst), S, hi, wi, ci, co, self._pad6 if i == 6 else 1,
                    _ptr(bias) if bias is not None else None, None, self._st()), fn.__name__)

    def _heads_bwd(self, cs, x, g):
        """Attention pooling (NISQA_lib.py:1171-1183) on x [S][64], forward, then d (sum_bh g[b][h] y[b][h]) / d x: the input half
        of _heads_loss's backward with g [B][heads] in the place of the loss gradient."""
        L_ = self.lib
        B, S, H, st = cs.B, cs.S, len(self.heads), self._st()
        dx = torch.zeros((S, 64), dtype=torch.float32, device=self.device)
        tmp = self._new(S, 64)
        for hi_, hp in enumerate(self.heads):
            u = self._linear_fwd(x, hp + 'linear1.weight', hp + 'linear1.bias', S, 64, 128, relu=True)
            sc = self._linear_fwd(u, hp + 'linear2.weight', hp + 'linear2.bias', S, 128, 1)
            att = self._new(S)
            self._ck(L_.nisqa_softmax_rows_fwd(_ptr(sc), cs.pool_off.data_ptr(), cs.pool_len.data_ptr(), B, 1.0, _ptr(att), st),
                     'nisqa_softmax_rows_fwd')
            dpooled = self._new(B, 64)
            self._gemm(g, self.P[hp + 'linear3.weight'], dpooled, B, 64, 1, H, 64, 64, ao=hi_)
            datt = self._new(S)
            self._ggemm(cs, 'datt', dpooled, x, datt, tb=1)
            self._ggemm(cs, 'outer', att, dpooled, tmp, ta=1)
            self._ew(4, dx, aux=tmp)
            self._ck(L_.nisqa_softmax_rows_bwd(_ptr(att), _ptr(datt), cs.pool_off.data_ptr(), cs.pool_len.data_ptr(), B, 1.0,
                                               _ptr(datt), st), 'nisqa_softmax_rows_bwd')
            du = self._linear_bwd(datt, u, hp + 'linear2.weight', hp + 'linear2.bias', S, 128, 1)
            self._ew(2, du, aux=u)
            self._ew(4, dx, aux=self._linear_bwd(du, x, hp + 'linear1.weight', hp + 'linear1.bias', S, 64, 128))
        return dx

    def _profile_bwd(self, cs, x, cot):
        """The backward of the per-segment profile on x [S][64]: cot = (d_weights [S][heads], d_local [S][heads],
        d_embed [S][64]) in the clip set's token layout, float32 on the device, None for zero -> d (sum d_weights * weights +
        sum d_local * local + sum d_embed * x) / d x [S][64]: ONE nisqa_pool_profile_bwd launch, which recomputes the logits."""
        H = len(self.heads)
        ptrs = []
        for t, width in zip(cot, (H, H, 64)):
            assert t is None or (t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()
                                 and tuple(t.shape) == (cs.S, width)), 'a profile cotangent is [S, heads] / [S, 64] float32'
            ptrs.append(_ptr(t) if t is not None else None)
        dx = self._new(cs.S, 64)                            # every row is written: no clearing
        self._ck(self.lib.nisqa_pool_profile_bwd(_ptr(x), 64, _ptr(cs.seg_off), _ptr(cs.pool_len), cs.B, cs.S, H, 0,
                                                 _ptr(self._pool_eng.profile_weights()), *ptrs, _ptr(dx), self._st()),
                 'nisqa_pool_profile_bwd')
        return dx

    def _seed(self, cs, x, g, cot):
        """What the walk back starts from, d / d x [S][64]: _heads_bwd of the score cotangent g [B][heads], _profile_bwd of the
        token-level cotangents cot, or their sum; either may be None (not both).  Without cot: the launches of _heads_bwd alone."""
        if cot is None or all(t is None for t in cot):
            return self._heads_bwd(cs, x, g)
        dx = self._profile_bwd(cs, x, cot)
        return dx if g is None else self._ew(4, dx, aux=self._heads_bwd(cs, x, g))

    def __call__(self, x, n_wins, grad_out, profile_cot=None):
        """x [B, L, 1, 48, 15], n_wins [B], grad_out [B, heads] -> d (sum grad_out * model(x, n_wins)) / d x, float32 on the
        engine's device, in x's shape.  profile_cot = (d_weights, d_local, d_embed), see _profile_bwd: cotangents of the score's
        per-segment profile over the S = sum n_wins valid tokens, clip by clip; with them grad_out may be None."""
        n = check_segments(x, n_wins, 1)
        B, L, H = x.shape[0], x.shape[1], len(self.heads)
        g = _grad_out(grad_out, B, H, self.device, profile_cot)
        x = x.detach().to(self.device, dtype=torch.float32).contiguous()
        cs = self._tables(np.asarray(n, dtype=np.int64))
        recs, feat = self._cnn_fwd_eval(x, cs.seg_off, cs.B, cs.S)
        xs, rec = self._sa_fwd(cs, feat, 384, 'time_dependency.model.', self.n_layers, None, 'td%d_%s', 0.0)
        dfeat = self._sa_bwd(rec, self._seed(cs, xs, g, profile_cot))
        del rec, xs, feat
        return self._cnn_bwd_eval(recs, dfeat, cs.seg_off, B, cs.S, L)


class InputGradDE(InputGrad):
    """The same for the double-ended NISQA_DE checkpoints (NISQA_lib.py:406-424 after model.eval()): x [B, L, 2, 48, 15] with the
    degraded clip's segments in channel 0 and the reference clip's in channel 1, n_wins [B, 2], grad_out [B, 1].  The channels
    are copied into one [2B, L, 1, 48, 15] tensor, degraded clips first, and the chain is HipTrainerDE's on the eval-mode
    operators: ONE _cnn_fwd_eval over the 2B clips (BatchNorm on the running statistics couples nothing, so one pass is the
    reference's two calls), time_dependency over the 2B clips, alignment + fusion, time_dependency_2 and the pooling head over
    the B degraded clips -- and back: _heads_bwd, _sa_bwd, the alignment's backward, _sa_bwd, _cnn_bwd_eval, and the two halves
    of the result side by side again.
      hard  nisqa_de_align_fuse_packed / nisqa_de_align_fuse_bwd, as the training step runs them.  ``last_idx`` keeps the indices
            the recomputation chose: the argmax over the RAW scores of the recomputed first self-attention (operator by operator,
            fp32).  At a near-tie of two scores it may differ from the choice of the fused inference chain that produced y
            (DESIGN.md 4.8 "argmax deviation"); the gradient is then that of the recomputed choice.
      soft  nisqa_de_align_soft_packed, which keeps lse and the aligned rows, and nisqa_de_align_soft_bwd (csrc/de_align.hip)."""

    def __init__(self, eng, state_dict):
        InputGrad.__init__(self, eng.base, state_dict)          # eng: engine.HipNisqaDE; its base runs the CNN-SA-AP half
        self.eng, self.args = eng, eng.args                     # (_pool_eng stays eng.base: pool.model is the single-ended engine's)
        self.n_layers2 = eng.n_layers2
        self.align, self.soft, self.fuse, self.fuse_width = eng.align, eng.apply, eng.fuse, eng.fuse_width
        w2 = state_dict[_TD2 + 'linear.weight']
        if tuple(w2.shape) != (64, self.fuse_width):
            raise ValueError('{}linear.weight is {}, de_fuse={} needs [64, {}]'.format(_TD2, tuple(w2.shape), self.args.get('de_fuse'),
                                                                                    self.fuse_width))
        self.last_idx = None

    def _tables(self, n):
        """The tables of HipTrainerDE._prepare for pairs of n[b] = (degraded, reference) segments, kept while the counts repeat:
        -> ({name: device view}, the clip set of the 2B clips, the clip set of the B degraded clips)"""
        Lx, Ly = n[:, 0], n[:, 1]
        L12 = np.concatenate([Lx, Ly])
        key = L12.tobytes()
        if key != self._tab_key:
            pa, tiles_a = step_tables(L12)
            pd, tiles_d = step_tables(Lx)
            parts = [('a_' + k, v) for k, v in pa] + pd
            parts += [('n_wins', L12.astype(np.int32)), ('tile_off', np.concatenate(([0], np.cumsum((Lx + 63) // 64))).astype(np.int32)),
                      ('r_seg_off', np.concatenate(([0], np.cumsum(Ly))).astype(np.int32))]
            host, buf, tv = self._upload_tables(parts)
            self._tab_key, self._tab = key, (host, buf, tv, _ClipSet(L12, tv, tiles_a, 'a_'), _ClipSet(Lx, tv, tiles_d))
        return self._tab[2:]

    def __call__(self, x, n_wins, grad_out, profile_cot=None):
        """x [B, L, 2, 48, 15], n_wins [B, 2], grad_out [B, 1] -> d (sum grad_out * model(x, n_wins)) / d x, float32 on the
        engine's device, in x's shape; rows l >= n_wins[b, c] of channel c exactly zero.  The channels are copied into the
        2B-clip layout, ``packed`` does the work, and the two halves of its result go side by side again.  profile_cot: see
        ``packed``."""
        n = check_segments(x, n_wins, 2)
        B = x.shape[0]
        g = _grad_out(grad_out, B, 1, self.device, profile_cot)
        x = x.detach().to(self.device, dtype=torch.float32)
        x2 = torch.cat([x[:, :, 0:1], x[:, :, 1:2]], 0).contiguous()             # [2B, L, 1, 48, 15], degraded clips first
        dx = self.packed(x2, np.asarray(n, dtype=np.int64), g, profile_cot=profile_cot)
        return torch.cat([dx[:B], dx[B:]], 2)

    def packed(self, x2, n, g, need=(True, True), profile_cot=None):
        """The same in the 2B-clip layout, for callers that hold it (engine.HipNisqaDE.grad_audio): x2 [2B, L, 1, 48, 15] float32,
        contiguous, on the engine's device, the B degraded clips first, then their B reference clips; n int64 [B, 2] (checked by
        the caller); g [B, 1] float32 on the device -> dx2 in x2's layout.  need = (degraded, reference): the CNN backward runs
        over the segments of the sides named -- the degraded segments are the leading Sx rows of every kept activation, the
        reference segments the rest, so one side is a view -- and the half of dx2 of a side not named is exact zeros.  The
        recomputation and the self-attention backward over both sides stay whole: either side's gradient needs them.
        profile_cot: InputGrad._profile_bwd's cotangents over the Sx valid tokens of the degraded clips (the second
        self-attention's rows); beside them g may be None."""
        B, L, F = n.shape[0], x2.shape[1], self.fuse_width
        assert tuple(x2.shape) == (2 * B, L, 1, 48, 15) and x2.dtype == torch.float32 and x2.is_contiguous() and any(need)
        tv, cs_all, cs_deg = self._tables(n)
        L_, st, Sx = self.lib, self._st(), cs_deg.S
        off, nw = tv['a_seg_off'], tv['n_wins']
        pair = (_ptr(off), _ptr(nw), _ptr(off, B), _ptr(nw, B))                  # offsets and counts: degraded side, reference side
        n_tiles, n_max = int(((n[:, 0] + 63) // 64).sum()), int(n.max())
        # recompute, activations kept
        recs, feat = self._cnn_fwd_eval(x2, cs_all.seg_off, 2 * B, cs_all.S)
        del x2
        x1, rec1 = self._sa_fwd(cs_all, feat, 384, _TD1, self.n_layers, None, 'td%d_%s', 0.0)
        fused = self._new(Sx, F)
        if self.soft:
            lse, aligned = self._new(Sx), self._new(Sx, 64)
            self._ck(L_.nisqa_de_align_soft_packed(_ptr(x1), *pair, _ptr(tv['tile_off']), B, n_tiles, self.align, self.fuse, F,
                                                   _ptr(fused), _ptr(lse), _ptr(aligned), st), 'nisqa_de_align_soft_packed')
        else:
            idx = self._new(Sx, dtype=torch.int32)
            self._ck(L_.nisqa_de_align_fuse_packed(_ptr(x1), *pair, _ptr(tv['tile_off']), B, n_tiles, self.align, self.fuse, F,
                                                   _ptr(fused), _ptr(idx), st), 'nisqa_de_align_fuse_packed')
            self.last_idx = idx
        xs, rec2 = self._sa_fwd(cs_deg, fused, F, _TD2, self.n_layers2, None, 'td2_%d_%s', 0.0)
        # backward, input halves only
        dfused = self._sa_bwd(rec2, self._seed(cs_deg, xs, g, profile_cot))      # [Sx][F]
        del rec2, xs, fused
        dx1 = self._new(cs_all.S, 64)                                            # every row is written: no clearing
        if self.soft:
            self._ck(L_.nisqa_de_align_soft_bwd(_ptr(x1), _ptr(dfused), F, _ptr(lse), _ptr(aligned), *pair, B, n_max, self.align,
                                                self.fuse, _ptr(dx1), _ptr(dx1), st), 'nisqa_de_align_soft_bwd')
        else:
            self._ck(L_.nisqa_de_align_fuse_bwd(_ptr(dfused), F, _ptr(idx), *pair, B, n_max, self.fuse, _ptr(dx1), _ptr(dx1), st),
                     'nisqa_de_align_fuse_bwd')
        dfeat = self._sa_bwd(rec1, dx1)                                          # [Sx + Sy][384]
        del rec1, x1, feat, dfused, dx1
        if all(need):
            return self._cnn_bwd_eval(recs, dfeat, cs_all.seg_off, 2 * B, cs_all.S, L)   # [2B, L, 1, 48, 15]
        # one side: its segments' rows of every activation, its clips' offsets counted from its first segment
        lo, hi, c0, seg_off = (0, Sx, 0, cs_deg.seg_off) if need[0] else (Sx, cs_all.S, B, tv['r_seg_off'])
        recs = [(z.view(cs_all.S, -1)[lo:hi], arg[lo:hi] if arg is not None else None) for z, arg in recs]
        dx2 = torch.zeros((2 * B, L, 1, 48, 15), dtype=torch.float32, device=self.device)
        self._cnn_bwd_eval(recs, dfeat[lo:hi], seg_off, B, hi - lo, L, dx=dx2[c0:c0 + B])
        return dx2


class InputGradLSTM(_EvalCNN, _FlatTrainer):
    """The same for the StandardCNN + BiLSTM models (nisqa_tts.tar and the CNN-LSTM-AVG / -MAX recipe), on HipTrainerLSTM's
    parameter layout and operators: the StandardCNN's 2 x 2 pools by nisqa_bn_eval_act_maxpool2_fwd / _bwd, conv2..6 by the exact
    fp32 implicit GEMM (nisqa_conv3x3_gemm modes 0 and 1: what the LSTM trainer runs at these shapes), fc_out, the BiLSTM with
    its gates kept and the backward through time, fed with grad_out through the pooling's linear layer.  The arithmetic is exact
    fp32 under either accepted engine precision: this family has no split-bf16 training convolutions."""
    FEAT_W = FC_W
    MAXPOOL2 = {1: 1, 2: 0, 4: 0}                     # pool_first = MaxPool2d(2, 2, padding (0, 1)), MaxPool2d(2) after conv2 and conv4
    _param_order = HipTrainerLSTM._param_order

    def __init__(self, eng, state_dict):
        if eng.arch not in LSTM_POOL_MODE:
            raise NotImplementedError('InputGradLSTM is built for the StandardCNN + BiLSTM models')
        self.precision = check_precision(eng.precision)
        self.eng, self.lib, self.device, self.args = eng, eng.lib, eng.device, eng.args
        self.pool_mode = LSTM_POOL_MODE[eng.arch]
        state_dict = {k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in state_dict.items()}
        self._layout(state_dict)
        self.load_state_dict(state_dict)
        for a_, b_ in zip(LSTM_KEYS[0::2], LSTM_KEYS[1::2]):       # both directions back to back: one pointer per tensor kind
            assert self.off[b_] == self.off[a_] + int(np.prod(self.kshape[a_])), 'LSTM directions must be adjacent'
        self._geo, self._pad6 = GEO, 1
        self._tab_key = None

    def _tables(self, n):
        """seg_off [B + 1] on the device, kept while the counts repeat"""
        key = n.tobytes()
        if key != self._tab_key:
            seg_off = torch.from_numpy(np.concatenate(([0], np.cumsum(n))).astype(np.int32)).to(self.device)
            self._tab_key, self._tab = key, seg_off
        return self._tab

    def _conv_eval(self, mode, i, src, dst, S, bias=None):
        ci, co = _CONV[i - 1]
        hi, wi = self._geo[i - 2][2]
        self._ck(self.lib.nisqa_conv3x3_gemm(mode, _ptr(src), _ptr(self.P['cnn.model.conv%d.weight' % i]), _ptr(dst), S, hi, wi, ci,
                                             co, self._pad6 if i == 6 else 1, _ptr(bias) if bias is not None else None, 1,
                                             self._st()), 'nisqa_conv3x3_gemm mode %d' % mode)

    def __call__(self, x, n_wins, grad_out):
        """x [B, L, 1, 48, 15], n_wins [B], grad_out [B, 1] -> d (sum grad_out * model(x, n_wins)) / d x, float32 on the engine's
        device, in x's shape."""
        n = check_segments(x, n_wins, 1)
        B, L, S = x.shape[0], x.shape[1], int(n.sum())
        _check_grad_out(grad_out, B, 1)
        x = x.detach().to(self.device, dtype=torch.float32).contiguous()
        g = grad_out.detach().to(self.device, dtype=torch.float32).contiguous()
        seg_off = self._tables(np.asarray(n, dtype=np.int64))
        L_, P, st = self.lib, self.P, self._st()
        # recompute, activations kept
        recs, feat = self._cnn_fwd_eval(x, seg_off, B, S)                     # [S][12 pixels][64]
        x20 = self._linear_fwd(feat, FC_W, 'cnn.model.fc_out.bias', S, 768, 20)
        del feat
        save, hprev = self._new(S, 2, 640), self._new(S, 2, 128)              # hprev: written by the entry, not read here
        pooled, argmax = self._new(B, 256), self._new(B, 256, dtype=torch.int32)
        wih, whh = P[LSTM_KEYS[0]], P[LSTM_KEYS[2]]
        self._ck(L_.nisqa_lstm_train_fwd(_ptr(x20), _ptr(seg_off), B, _ptr(wih), _ptr(whh), _ptr(P[LSTM_KEYS[4]]),
                                         _ptr(P[LSTM_KEYS[6]]), self.pool_mode, _ptr(save), _ptr(hprev), _ptr(pooled),
                                         argmax.data_ptr(), st), 'nisqa_lstm_train_fwd')
        del x20, hprev, pooled
        # backward, input halves only
        dpooled = self._new(B, 256)
        self._gemm(g, P[POOL_KEYS[0]], dpooled, B, 256, 1, 1, 256, 256)
        dgates = self._new(S, 1024)                                           # [token][direction][4 gates x 128]
        self._ck(L_.nisqa_lstm_train_bptt(_ptr(seg_off), B, _ptr(whh), _ptr(save), self.pool_mode, _ptr(dpooled),
                                          argmax.data_ptr(), _ptr(dgates), None, st), 'nisqa_lstm_train_bptt')
        del save
        dx20 = self._new(S, 20)                                               # sum over both directions: K = 1024
        self._gemm(dgates, wih, dx20, S, 20, 1024, 1024, 20, 20)
        dfeat = self._new(S, 768)
        self._gemm(dx20, P[FC_W], dfeat, S, 768, 20, 20, 768, 768)
        del dgates
        return self._cnn_bwd_eval(recs, dfeat, seg_off, B, S, L)
