"""d model(x, n_wins) / d x for the CNN-SA-AP checkpoints (NISQA / NISQA_DIM), on the GPU.

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
  heads      attention pooling forward and the input half of its backward, fed with the caller's grad_out.
Parameters get no gradient here (that is the trainers' business): the weight-gradient GEMMs and column sums of the borrowed
operators are not run.
"""
import numpy as np
import torch

from .engine import check_segments
from .train import _AttTrainer, _ClipSet, _CONV, _ptr, step_tables

PRECISIONS = ('f32', 'bf16x6')          # the engine precisions whose operands are the reference's fp32 values


def check_precision(precision):
    """A gradient is built for the engine precisions that carry fp32 operands exactly; the fast ones refuse, naming themselves.
    No GPU is touched."""
    if precision not in PRECISIONS:
        raise NotImplementedError('the gradient of model(x, n_wins) with respect to x is built for the engine precisions {}, '
                                  'not for {}'.format(' and '.join(PRECISIONS), precision))
    return precision


class InputGrad(_AttTrainer):
    FEAT_W = 'time_dependency.model.linear.weight'

    def __init__(self, eng, state_dict):
        if eng.arch != 0:
            raise NotImplementedError('the gradient with respect to x is built for the CNN-SA-AP models (NISQA, NISQA_DIM)')
        self.precision = check_precision(eng.precision)
        self.eng, self.lib, self.device, self.args = eng, eng.lib, eng.device, eng.args
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

    def _cnn_fwd_eval(self, x, cs):
        """x [B, L, 1, 48, 15] -> (per layer (z, arg), the features [S][384] in (y, c) order)"""
        L_, P, S, st = self.lib, self.P, cs.S, self._st()
        if not self._packed:
            self._pack_frags()
            if any(self._convs[i][0] is None or self._convs[i][1] is None for i in range(2, 7)):
                raise NotImplementedError('no segment-resident convolution for this CNN geometry')
            self._packed = True
        recs, act = [], None
        for i in range(1, 7):
            ci, co = _CONV[i - 1]
            h, w, (ho, wo) = self._geo[i - 1]
            bk = 'cnn.model.conv%d.bias' % i
            z = self._new(S * h * w, co)
            if i == 1:
                self._ck(L_.nisqa_conv1_segments_fwd(_ptr(x), x.shape[1], _ptr(cs.seg_off), cs.B, S, _ptr(P['cnn.model.conv1.weight']),
                                                     _ptr(P[bk]), _ptr(z), st), 'nisqa_conv1_segments_fwd')
            else:
                hi, wi = self._geo[i - 2][2]
                fwd = self._convs[i][0]
                self._ck(fwd[0](0, _ptr(act), _ptr(fwd[1]), _ptr(z), S, hi, wi, ci, co, self._pad6 if i == 6 else 1, _ptr(P[bk]), None,
                                st), fwd[0].__name__)
            arg = None if (h, w) == (ho, wo) else self._new(S, ho * wo, co, dtype=torch.int32)
            act = self._new(S, ho * wo, co)
            self._ck(L_.nisqa_bn_eval_act_pool_fwd(_ptr(z), *self._bn_ptrs(i), S, h, w, co, ho, wo, _ptr(act),
                                                   arg.data_ptr() if arg is not None else None, st), 'nisqa_bn_eval_act_pool_fwd')
            recs.append((z, arg))
        return recs, act.view(S, 384)

    def _bn_ptrs(self, i):
        P = self.P
        return (_ptr(P['cnn.model.bn%d.weight' % i]), _ptr(P['cnn.model.bn%d.bias' % i]), _ptr(self.bn[i]['mean']),
                _ptr(self.bn[i]['var']))

    def _cnn_bwd_eval(self, recs, da, cs, B, L):
        """d / d features [S][384] -> d / d x [B, L, 1, 48, 15]"""
        L_, S, st = self.lib, cs.S, self._st()
        for i in range(6, 0, -1):
            ci, co = _CONV[i - 1]
            h, w, (ho, wo) = self._geo[i - 1]
            z, arg = recs.pop()
            dz = self._new(S * h * w, co)
            self._ck(L_.nisqa_bn_eval_act_pool_bwd(_ptr(da), arg.data_ptr() if arg is not None else None, _ptr(z), *self._bn_ptrs(i),
                                                   S, h, w, co, ho, wo, _ptr(dz), st), 'nisqa_bn_eval_act_pool_bwd')
            if i == 1:
                break
            hi, wi = self._geo[i - 2][2]
            dgrad = self._convs[i][1]
            da = self._new(S, hi * wi, ci)
            self._ck(dgrad[0](1, _ptr(dz), _ptr(dgrad[1]), _ptr(da), S, hi, wi, ci, co, self._pad6 if i == 6 else 1, None, None, st),
                     dgrad[0].__name__)
        dx = self._new(B, L, 1, 48, 15)
        self._ck(L_.nisqa_conv1_segments_dgrad(_ptr(dz), _ptr(cs.seg_off), B, L, _ptr(self.P['cnn.model.conv1.weight']), _ptr(dx), st),
                 'nisqa_conv1_segments_dgrad')
        return dx

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

    def __call__(self, x, n_wins, grad_out):
        """x [B, L, 1, 48, 15], n_wins [B], grad_out [B, heads] -> d (sum grad_out * model(x, n_wins)) / d x, float32 on the
        engine's device, in x's shape."""
        n = check_segments(x, n_wins, 1)
        B, L, H = x.shape[0], x.shape[1], len(self.heads)
        if not torch.is_tensor(grad_out) or tuple(grad_out.shape) != (B, H):
            raise ValueError('expected grad_out of shape [{}, {}], got {}'.format(
                B, H, tuple(grad_out.shape) if torch.is_tensor(grad_out) else type(grad_out).__name__))
        x = x.detach().to(self.device, dtype=torch.float32).contiguous()
        g = grad_out.detach().to(self.device, dtype=torch.float32).contiguous()
        cs = self._tables(np.asarray(n, dtype=np.int64))
        recs, feat = self._cnn_fwd_eval(x, cs)
        xs, rec = self._sa_fwd(cs, feat, 384, 'time_dependency.model.', self.n_layers, None, 'td%d_%s', 0.0)
        dfeat = self._sa_bwd(rec, self._heads_bwd(cs, xs, g))
        del rec, xs, feat
        return self._cnn_bwd_eval(recs, dfeat, cs, B, L)
