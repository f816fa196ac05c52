"""One optimiser step of the StandardCNN + BiLSTM models on the GPU: nisqa_tts.tar (pool=last_step_bi) and the CNN-LSTM-AVG
recipe (config/train_nisqa_cnn_lstm_avg.yaml, pool=avg, or pool=max) -- DESIGN.md 4.9.

What the reference does per batch at nisqa/NISQA_model.py:131-152 for ``model`` = NISQA with cnn_model=standard, td=lstm:
StandardCNN in train mode (NISQA_lib.py:712-836: batch-statistics BatchNorm over the valid segments, ReLU, pool_first =
MaxPool2d(2, 2, padding (0, 1)), 2 x 2 pools, Dropout2d at four sites, fc_out 768 -> 20), the BiLSTM over each clip's n_wins
segments (NL:897-943), PoolLastStepBi / PoolAvg / PoolMax and the linear layer (NL:1099-1115, 1185-1224), biasLoss.get_loss,
backward and Adam -- with every operator a HIP kernel; the CNN runs through train._FlatTrainer's loop (_cnn_fwd / _cnn_bwd)
with the geometry GEO, conv6 padded like conv1..5 and the _std_ layer-1 entry points:
  * layer 1: nisqa_conv1_moments + nisqa_conv1_bn_act_pool_std_fwd / _bwd (conv1 from the spectrogram, never written);
  * layers 2..6: nisqa_conv3x3_fwd_stats / nisqa_conv3x3_gemm (exact fp32 MFMA, padding (1, 1): what the loop picks for 'f32'
    at shapes nisqa_segconv_supported refuses) and nisqa_bn_act_pool_fwd /
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
from .train import _FlatTrainer, _BN_BUFFERS, _ptr, bias_rows, feat_to_kernel, feat_from_kernel

# conv output (H, W) and the pool after it: pool_first 48 x 15 -> 24 x 8, pool after conv2 and conv4, identity elsewhere
GEO = [(48, 15, (24, 8)), (24, 8, (12, 4)), (12, 4, (12, 4)), (12, 4, (6, 2)), (6, 2, (6, 2)), (6, 2, (6, 2))]
LSTM_PFX = 'time_dependency.model.lstm.'
LSTM_KEYS = [LSTM_PFX + k for k in ('weight_ih_l0', 'weight_ih_l0_reverse', 'weight_hh_l0', 'weight_hh_l0_reverse',
                                    'bias_ih_l0', 'bias_ih_l0_reverse', 'bias_hh_l0', 'bias_hh_l0_reverse')]
POOL_KEYS = ['pool.model.linear.weight', 'pool.model.linear.bias']
FC_W = 'cnn.model.fc_out.weight'


# fc_out.weight [20][768]: columns c * 12 + pixel (the reference's flatten of [64][6][2]) <-> columns pixel * 64 + c
fc_to_kernel, fc_from_kernel = feat_to_kernel, feat_from_kernel


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
    FEAT_W = FC_W

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
        self._init_params(state_dict, 24)
        for a_, b_ in zip(LSTM_KEYS[0::2], LSTM_KEYS[1::2]):       # both directions back to back: one pointer per tensor kind
            assert self.off[b_] == self.off[a_] + int(np.prod(self.kshape[a_])), 'LSTM directions must be adjacent'
        self._init_cnn(GEO, 1, self.lib.nisqa_conv1_bn_act_pool_std_fwd, self.lib.nisqa_conv1_bn_act_pool_std_bwd)
        self._prep_key = None

    # ---- parameters ------------------------------------------------------------------------------------
    def _param_order(self, sd):
        cnn = [k for k in sd if k.startswith('cnn.model.') and k.split('.')[-1] not in _BN_BUFFERS]
        keys = cnn + LSTM_KEYS + POOL_KEYS
        extra = [k for k in sd if k not in keys and k.split('.')[-1] not in _BN_BUFFERS]
        if extra:
            raise NotImplementedError('HIP LSTM training step: unexpected parameters {}'.format(extra))
        return keys

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

    # ---- the step ------------------------------------------------------------------------------------------
    def _step(self, mel, frame_off, n_wins, floor, y, masks, bias):
        L_ = self.lib
        self._prepare(n_wins)
        B, S, st = self.B, self.S, self._st()
        P, G = self.P, self.G
        self.gflat.zero_()
        y_dev = self._upload(y, 1)
        bias_dev = None if bias is None else self._upload(bias_rows(bias, B, 1)[0], 4)      # [B,4] or [B,1,4]: one head
        cnn, act = self._cnn_fwd(mel, frame_off, floor, masks)
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
        self._cnn_bwd(cnn, [self._linear_bwd(dx20, feat, FC_W, 'cnn.model.fc_out.bias', S, 768, 20)])     # [S][12][64]
        return self._finish_step(y_hat, loss)
