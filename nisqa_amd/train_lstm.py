"""One optimiser step of the StandardCNN + BiLSTM models on the GPU: nisqa_tts.tar (pool=last_step_bi) and the CNN-LSTM-AVG
recipe (config/train_nisqa_cnn_lstm_avg.yaml, pool=avg, or pool=max) -- DESIGN.md 4.9.

What the reference does per batch at nisqa/NISQA_model.py:131-152 for ``model`` = NISQA with cnn_model=standard, td=lstm:
StandardCNN in train mode (NISQA_lib.py:712-836: batch-statistics BatchNorm over the valid segments, ReLU, pool_first =
MaxPool2d(2, 2, padding (0, 1)), 2 x 2 pools, Dropout2d at four sites, fc_out 768 -> 20), the BiLSTM over each clip's n_wins
segments (NL:897-943), PoolLastStepBi / PoolAvg / PoolMax and the linear layer (NL:1099-1115, 1185-1224), biasLoss.get_loss,
backward and Adam -- with every operator a HIP kernel:
  * layer 1: nisqa_conv1_moments + nisqa_conv1_bn_act_pool_std_fwd / _bwd (conv1 from the spectrogram, never written);
  * layers 2..6: nisqa_conv3x3_fwd_stats / nisqa_conv3x3_gemm (exact fp32 MFMA, padding (1, 1)) and nisqa_bn_act_pool_fwd /
    nisqa_bn_act_pool_bwd (2 x 2 pools after conv2 and conv4: the adaptive windows of 24 x 8 -> 12 x 4 and 12 x 4 -> 6 x 2 are
    exactly the 2 x 2 windows, tests/test_gpu_train_lstm.py);
  * fc_out, the pooling's linear layer and every weight / input gradient of the LSTM: nisqa_gemm_f32_one;
  * the BiLSTM: nisqa_lstm_train_fwd (saves gates and cell states) and nisqa_lstm_train_bptt (csrc/train_lstm.hip);
  * loss, Adam, dropout masks: nisqa_mse_loss, nisqa_adam_step, nisqa_dropout_mask.
Precision: 'f32' only (exact fp32 MFMA convolutions, fp32 VALU recurrence): the reference's arithmetic.

Flat-buffer layout (``keys`` order, the checkpoint's optimizer_state_dict['layout']): the CNN in state_dict order (conv
weights as [C_out][3*3*C_in], fc_out's 768 columns in [pixel][channel] order instead of the reference's [channel][pixel]),
then the LSTM with both directions of each tensor back to back (weight_ih, weight_hh, bias_ih, bias_hh), then the pooling's
linear layer.  ``state_dict()`` returns the reference's keys and shapes.
"""
import os

import numpy as np
import torch

from . import dist as _dist
from .engine import HipNisqa, check_lstm_args, LSTM_POOL_MODE
from .train import _FlatTrainer, _ptr

_CONV = [(1, 16), (16, 32), (32, 64), (64, 64), (64, 64), (64, 64)]      # (C_in, C_out) of conv1..conv6
_DROP_AFTER = {2: 'cnn_d1', 3: 'cnn_d2', 4: 'cnn_d3', 5: 'cnn_d4'}       # Dropout2d sites (NISQA_lib.py:820-828)
# conv output (H, W) and the pool after it: pool_first 48 x 15 -> 24 x 8, pool after conv2 and conv4, identity elsewhere
GEO = [(48, 15, (24, 8)), (24, 8, (12, 4)), (12, 4, (12, 4)), (12, 4, (6, 2)), (6, 2, (6, 2)), (6, 2, (6, 2))]
LSTM_PFX = 'time_dependency.model.lstm.'
LSTM_KEYS = [LSTM_PFX + k for k in ('weight_ih_l0', 'weight_ih_l0_reverse', 'weight_hh_l0', 'weight_hh_l0_reverse',
                                    'bias_ih_l0', 'bias_ih_l0_reverse', 'bias_hh_l0', 'bias_hh_l0_reverse')]
POOL_KEYS = ['pool.model.linear.weight', 'pool.model.linear.bias']
FC_W = 'cnn.model.fc_out.weight'


def fc_to_kernel(w):
    """fc_out.weight [20][768] with columns c * 12 + pixel (the reference's flatten of [64][6][2]) -> columns pixel * 64 + c"""
    return w.reshape(w.shape[0], 64, 12).permute(0, 2, 1).reshape(w.shape[0], 768)


def fc_from_kernel(w):
    return w.reshape(w.shape[0], 12, 64).permute(0, 2, 1).reshape(w.shape[0], 768)


def check_train_lstm_args(args, precision=None):
    """The configurations HipTrainerLSTM trains -> (pool mode, precision); everything else raises NotImplementedError naming the
    option, before any GPU work."""
    if args.get('cnn_model') != 'standard' or args.get('td') != 'lstm':
        raise NotImplementedError('HIP LSTM training step covers cnn_model=standard, td=lstm, got cnn_model={}, td={}'.format(
            args.get('cnn_model'), args.get('td')))
    arch = check_lstm_args(args)
    prec = precision or os.environ.get('NISQA_HIP_TRAIN_PRECISION') or 'f32'
    if prec != 'f32':
        raise NotImplementedError("HIP LSTM training step: precision '{}' is not built for StandardCNN + BiLSTM ('f32' only)".format(prec))
    return LSTM_POOL_MODE[arch], prec


class HipTrainerLSTM(_FlatTrainer):
    LAYOUT = 'nisqa_amd flat buffer (HipTrainerLSTM.keys / kshape order)'

    def __init__(self, args, state_dict, device=None, lr=1e-3, precision=None):
        """args / state_dict: a NISQA model with cnn_model=standard, td=lstm (engine.check_lstm_args); precision: 'f32' only."""
        self.pool_mode, self.precision = check_train_lstm_args(args, precision)
        self.pool = args.get('pool')
        missing = [k for k in LSTM_KEYS + POOL_KEYS + [FC_W] if k not in state_dict]
        if missing:
            raise NotImplementedError('HIP LSTM training step: state_dict lacks {}'.format(missing))
        self.eng = HipNisqa(args, state_dict, device, precision='f32')       # mel front end + geometry checks
        self.lib, self.device, self.args = self.eng.lib, self.eng.device, args
        self.lr = float(lr)
        self.p_cnn, self.p_td = float(args.get('cnn_dropout') or 0.0), 0.0
        self._kchunk = int(os.environ.get('NISQA_HIP_TRAIN_KCHUNK', '128'))      # split-K chunk of the weight gradients
        self.t = 0
        self._layout(state_dict)
        for a_, b_ in zip(LSTM_KEYS[0::2], LSTM_KEYS[1::2]):       # both directions back to back: one pointer per tensor kind
            assert self.off[b_] == self.off[a_] + int(np.prod(self.kshape[a_])), 'LSTM directions must be adjacent'
        self.load_state_dict(state_dict)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self._sums = torch.zeros((24, 512), dtype=torch.float64, device=self.device)
        self._cast_table, self._cast_key = None, None
        self._rng_seed, self._rng_off = int(torch.initial_seed()) & (2 ** 64 - 1), 0     # torch.manual_seed governs the masks
        self._prep_key = None

    # ---- parameters ------------------------------------------------------------------------------------
    def _param_order(self, sd):
        cnn = [k for k in sd if k.startswith('cnn.model.') and k.split('.')[-1] not in ('running_mean', 'running_var',
                                                                                         'num_batches_tracked')]
        keys = cnn + LSTM_KEYS + POOL_KEYS
        extra = [k for k in sd if k not in keys and k.split('.')[-1] not in ('running_mean', 'running_var', 'num_batches_tracked')]
        if extra:
            raise NotImplementedError('HIP LSTM training step: unexpected parameters {}'.format(extra))
        return keys

    @staticmethod
    def _to_kernel(k, v):
        if k.startswith('cnn.model.conv') and k.endswith('.weight'):
            return v.permute(0, 2, 3, 1).reshape(v.shape[0], -1)
        if k == FC_W:
            return fc_to_kernel(v)
        return v

    @staticmethod
    def _from_kernel(k, v, ref_shape):
        if k.startswith('cnn.model.conv') and k.endswith('.weight'):
            co, ci = ref_shape[0], ref_shape[1]
            return v.reshape(co, 3, 3, ci).permute(0, 3, 1, 2)
        if k == FC_W:
            return fc_from_kernel(v)
        return v

    # ---- batch bookkeeping ---------------------------------------------------------------------------------
    def _prepare(self, n_wins):
        L = np.asarray(n_wins, dtype=np.int64)
        if len(L) == 0 or (L < 1).any():
            raise ValueError('every clip needs at least one segment, got n_wins={}'.format(L.tolist()))
        self.B, self.S, self.L = len(L), int(L.sum()), L
        key = L.tobytes()
        if key != self._prep_key:
            self.seg_off = torch.from_numpy(np.concatenate(([0], np.cumsum(L))).astype(np.int32)).to(self.device)
            self._prep_key = key
        self._sums.zero_()
        self._sum_i = 0
        self._casts = []
        self._mask_buf, self._mask_pos = None, {}
        o = 0
        for k, c in (('cnn_d1', 32), ('cnn_d2', 64), ('cnn_d3', 64), ('cnn_d4', 64)):
            self._mask_pos[k] = (o, self.S * c)
            o += (self.S * c + 3) // 4 * 4
        self._mask_total = self._mask_split = o

    def _sum_rows(self, n=1):
        s = self._sums[self._sum_i:self._sum_i + n].view(-1)
        self._sum_i += n
        return s

    def _upload(self, a, cols):
        a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(self.B, cols))
        if self.device.type != 'cuda':
            return torch.from_numpy(a).to(self.device)
        h = torch.empty(a.shape, dtype=torch.float32, pin_memory=True)
        h.numpy()[...] = a
        return h.to(self.device, non_blocking=True)

    # ---- the step ------------------------------------------------------------------------------------------
    def _step(self, mel, frame_off, n_wins, floor, y, masks, bias):
        L_ = self.lib
        self._prepare(n_wins)
        B, S, st = self.B, self.S, self._st()
        hop = int(self.args['ms_seg_hop_length'])
        P, G = self.P, self.G
        self.gflat.zero_()
        y_dev = self._upload(y, 1)
        bias_dev = None if bias is None else self._upload(bias, 4)

        # ================= forward: StandardCNN in train mode =================
        cnn = []
        act = None
        for i in range(1, 7):
            ci, co = _CONV[i - 1]
            h, w, (ho, wo) = GEO[i - 1]
            rows = S * h * w
            wk, bk = 'cnn.model.conv%d.weight' % i, 'cnn.model.conv%d.bias' % i
            gk, bek = 'cnn.model.bn%d.weight' % i, 'cnn.model.bn%d.bias' % i
            drop = self._mask(masks, _DROP_AFTER[i], (S, co), self.p_cnn) if i in _DROP_AFTER else None
            out = self._new(S, ho * wo, co)
            arg = self._new(S, ho * wo, co, dtype=torch.int32)
            mr = self._new(2 * co)
            dp = _ptr(drop) if drop is not None else None
            if i == 1:
                mom, sums = self._sum_rows()[:54], self._sum_rows()[:32]
                self._ck(L_.nisqa_conv1_moments(_ptr(mel), _ptr(frame_off), _ptr(self.seg_off), _ptr(floor), B, S, hop,
                                                mom.data_ptr(), st), 'nisqa_conv1_moments')
                self._ck(L_.nisqa_conv1_bn_act_pool_std_fwd(_ptr(mel), _ptr(frame_off), _ptr(self.seg_off), _ptr(floor), B, S, hop,
                                                            _ptr(P[wk]), _ptr(P[bk]), mom.data_ptr(), _ptr(P[gk]), _ptr(P[bek]),
                                                            _ptr(self.bn[1]['mean']), _ptr(self.bn[1]['var']), sums.data_ptr(),
                                                            _ptr(mr), dp, _ptr(out), arg.data_ptr(), st),
                         'nisqa_conv1_bn_act_pool_std_fwd')
                cnn.append(dict(z=None, x=None, arg=arg, mr=mr, drop=drop, mom=mom))
            else:
                hi, wi = GEO[i - 2][2]
                z = self._new(rows, co)
                sums = self._sum_rows()
                self._ck(L_.nisqa_conv3x3_fwd_stats(0, _ptr(act), _ptr(P[wk]), _ptr(z), S, hi, wi, ci, co, 1, _ptr(P[bk]),
                                                    sums.data_ptr(), st), 'nisqa_conv3x3_fwd_stats')
                self._ck(L_.nisqa_bn_act_pool_fwd(_ptr(z), sums.data_ptr(), _ptr(P[gk]), _ptr(P[bek]), _ptr(self.bn[i]['mean']),
                                                  _ptr(self.bn[i]['var']), _ptr(mr), S, h, w, co, ho, wo, dp, _ptr(out),
                                                  arg.data_ptr(), st), 'nisqa_bn_act_pool_fwd')
                cnn.append(dict(z=z, x=act, arg=arg, mr=mr, drop=drop))
            self.bn[i]['n'] += 1
            act = out
        feat = act.view(S, 768)                                               # [S][12 pixels][64] in (pixel, c) order
        x20 = self._linear_fwd(feat, FC_W, 'cnn.model.fc_out.bias', S, 768, 20)

        # ================= forward: BiLSTM + pooling + linear, loss =================
        save, hprev = self._new(S, 2, 640), self._new(S, 2, 128)
        pooled = self._new(B, 256)
        argmax = self._new(B, 256, dtype=torch.int32)
        wih, whh = P[LSTM_KEYS[0]], P[LSTM_KEYS[2]]
        self._ck(L_.nisqa_lstm_train_fwd(_ptr(x20), _ptr(self.seg_off), B, _ptr(wih), _ptr(whh), _ptr(P[LSTM_KEYS[4]]),
                                         _ptr(P[LSTM_KEYS[6]]), self.pool_mode, _ptr(save), _ptr(hprev), _ptr(pooled),
                                         argmax.data_ptr(), st), 'nisqa_lstm_train_fwd')
        y_hat = self._new(B, 1)
        self._gemm(pooled, P[POOL_KEYS[0]], y_hat, B, 1, 256, 256, 256, 1, tb=1, bias=P[POOL_KEYS[1]])
        loss_v, dyh = self._new(2), self._new(B, 1)
        self._ck(L_.nisqa_mse_loss(_ptr(y_hat), _ptr(y_dev), _ptr(bias_dev) if bias_dev is not None else None, B, 1,
                                   _ptr(loss_v), _ptr(dyh), st), 'nisqa_mse_loss')
        loss = loss_v[:1]
        if _dist.world()[1] > 1:
            # the loss is a mean over the labelled clips of the WHOLE batch: rescale this rank's share
            cnt = torch.as_tensor((~np.isnan(np.asarray(y, np.float32).reshape(B, 1))).sum(0), dtype=torch.float32)
            tot = _dist.all_reduce_sum_(cnt.clone())
            share = torch.where(tot > 0, cnt / tot.clamp(min=1), torch.zeros_like(cnt)).to(self.device)
            self._ck(L_.nisqa_elementwise(5, _ptr(dyh), None, _ptr(share), B, 1, _ptr(dyh), st), 'nisqa_elementwise')
            loss = _dist.all_reduce_sum_((loss_v[1:] * share).sum().reshape(1))

        # ================= backward: linear, pooling, BiLSTM, fc_out =================
        s = self._coldot(dyh, dyh, B, 1)
        self._defer_cast(s, 0, 1, G[POOL_KEYS[1]])
        self._gemm(dyh, pooled, G[POOL_KEYS[0]], 1, 256, B, 1, 256, 256, ta=1)
        dpooled = self._new(B, 256)
        self._gemm(dyh, P[POOL_KEYS[0]], dpooled, B, 256, 1, 1, 256, 256)
        dgates = self._new(S, 1024)                                           # [token][direction][4 gates x 128]
        dbias = self._sum_rows(2)                                             # float64 [2][512]
        self._ck(L_.nisqa_lstm_train_bptt(_ptr(self.seg_off), B, _ptr(whh), _ptr(save), self.pool_mode, _ptr(dpooled),
                                          argmax.data_ptr(), _ptr(dgates), dbias.data_ptr(), st), 'nisqa_lstm_train_bptt')
        for d in range(2):
            self._defer_cast(dbias, 512 * d, 512, G[LSTM_KEYS[4 + d]])
            self._defer_cast(dbias, 512 * d, 512, G[LSTM_KEYS[6 + d]])
        # dW_ih of both directions in one product (their rows are adjacent): [1024][20] = dgates^T x20
        self._gemm(dgates, x20, G[LSTM_KEYS[0]], 1024, 20, S, 1024, 20, 20, ta=1, ksplit=self._ksplit(S, 1024, 20))
        for d in range(2):                                                    # dW_hh = dgates_d^T h_prev_d
            self._gemm(dgates, hprev, G[LSTM_KEYS[2 + d]], 512, 128, S, 1024, 256, 128, ta=1, ao=512 * d, bo=128 * d,
                       ksplit=self._ksplit(S, 512, 128))
        dx20 = self._new(S, 20)                                               # sum over both directions: K = 1024
        self._gemm(dgates, wih, dx20, S, 20, 1024, 1024, 20, 20)
        da = self._linear_bwd(dx20, feat, FC_W, 'cnn.model.fc_out.bias', S, 768, 20).view(S, 12, 64)

        # ================= backward: StandardCNN =================
        for i in range(6, 0, -1):
            c = cnn[i - 1]
            ci, co = _CONV[i - 1]
            h, w, (ho, wo) = GEO[i - 1]
            g, b_ = P['cnn.model.bn%d.weight' % i], P['cnn.model.bn%d.bias' % i]
            dg, db = G['cnn.model.bn%d.weight' % i], G['cnn.model.bn%d.bias' % i]
            dp = _ptr(c['drop']) if c['drop'] is not None else None
            if i == 1:
                acc = self._sum_rows()[:176]
                self._ck(L_.nisqa_conv1_bn_act_pool_std_bwd(_ptr(mel), _ptr(frame_off), _ptr(self.seg_off), _ptr(floor), B, S, hop,
                                                            _ptr(P['cnn.model.conv1.weight']), _ptr(P['cnn.model.conv1.bias']),
                                                            c['mom'].data_ptr(), _ptr(g), _ptr(b_), _ptr(c['mr']), dp, _ptr(da),
                                                            c['arg'].data_ptr(), acc.data_ptr(), _ptr(dg), _ptr(db),
                                                            _ptr(G['cnn.model.conv1.weight']), st), 'nisqa_conv1_bn_act_pool_std_bwd')
                break                                                         # conv biases: exactly zero (gflat was cleared)
            rows = S * h * w
            hi, wi = GEO[i - 2][2]
            dz = self._new(rows, co)
            s2 = self._sum_rows()
            self._ck(L_.nisqa_bn_act_pool_bwd(_ptr(da), c['arg'].data_ptr(), dp, _ptr(c['z']), _ptr(c['mr']), _ptr(g), _ptr(b_), S,
                                              h, w, co, ho, wo, s2.data_ptr(), _ptr(dz), _ptr(dg), _ptr(db), st),
                     'nisqa_bn_act_pool_bwd')
            wk = 'cnn.model.conv%d.weight' % i
            self._ck(L_.nisqa_conv3x3_gemm(2, _ptr(c['x']), _ptr(dz), _ptr(G[wk]), S, hi, wi, ci, co, 1, None,
                                           self._ksplit(rows, co, 9 * ci), st), 'nisqa_conv3x3_gemm wgrad')
            da = self._new(S, hi * wi, ci)
            self._ck(L_.nisqa_conv3x3_gemm(1, _ptr(dz), _ptr(P[wk]), _ptr(da), S, hi, wi, ci, co, 1, None, 1, st),
                     'nisqa_conv3x3_gemm dgrad')
            c['x'] = None
        return self._finish_step(y_hat, loss)
