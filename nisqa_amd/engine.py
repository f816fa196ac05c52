"""Device engine: owns the packed weights / tables on one GPU and drives libnisqa_hip.so.

PyTorch is used only for device memory, streams and H2D/D2H copies; all arithmetic of the hot
path (mel front end, AdaptCNN, self-attention, attention pooling) runs in the HIP kernels behind
the C ABI (include/nisqa_hip.h).  No fallback: constructing the engine without a GPU or without
the built library raises.
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import lib as _lib
from . import weights as _w
from .melbank import KAISER_BEST_PRECISION, MelTables, kaiser_best_table, resampled_lengths

SEG_LEN = 15
TOK_PAD = 64          # tokens of a clip are padded to whole 64-token workgroups (csrc/td16_bf16x6.hip); the other kernels need 32
# The precision every GEMM of the path runs in unless the caller (or NISQA_HIP_PRECISION) says otherwise.  'bf16x6' carries the
# reference's fp32 operands EXACTLY (three bf16 terms, six MFMA products per term pair, fp32 accumulation): reference-grade
# arithmetic, as far from a float64 evaluation as the exact-fp32 kernels and the reference's own CPU float32
# (tests/test_gpu_parity.py::test_rounding_error_of_the_precision_modes_against_float64).  'bf16x3' (16 of the 24 operand mantissa
# bits, |dMOS| <= 5e-5, 1.5 x faster) was the default until round 4 and stays selectable; 'f32' is the exact fp32-MFMA path.
#
# Round 5 added 'f16x4' / 'f16x3': the AdaptCNN with every fp32 operand as TWO f16 terms of the power-of-two-scaled tensor (11 + 11
# significand bits and the low term's sign: the fp32 value itself for ~75 % of the values, one fp32 ulp off for the rest) and all four /
# three term products; self-attention and pooling run as in 'bf16x6'.  Measured against float64 they are as close as 'f32' and 'bf16x6'
# (the same test), at 4 / 3 instead of 6 MFMA products -- but an operand may lose its last bit, so they are opt-in, not the default.
DEFAULT_PRECISION = 'bf16x6'


def _pack_bf16(terms):
    return lambda sd: _w.pack_adapt_cnn_bf16(sd, conv1_pairs=True, terms=terms)


# What a precision IS, stated once: nisqa_model_dev.cnn_mode; the operand format of self-attention and pooling (a key of TD: the f16 CNN
# modes pair with the three-term kernels); how cnn_wb is packed (None: no 16-bit blob); and per CNN stage -- frame-fed AdaptCNN,
# segment-fed AdaptCNN, StandardCNN, segment-fed StandardCNN -- the entry point and what it takes between cnn_w and the stream (`terms`:
# the digit the precision's name ends in; the f16 entries serve both counts).
Precision = collections.namedtuple('Precision', 'cnn_mode td pack_cnn adapt segments standard standard_segments')
_WB, _F16 = 'cnn_wb feat', 'cnn_wb terms feat'
PRECISION = {
    'f32': Precision(0, 'f32', None, ('nisqa_cnn_adapt', 'p3 feat'), ('nisqa_cnn_adapt_segments', 'p3 feat'), ('nisqa_cnn_standard', 'p3 feat'),
                     ('nisqa_cnn_standard_segments', 'p3 feat')),
    'bf16x3': Precision(1, 'bf16x3', _pack_bf16(2), ('nisqa_cnn_adapt_bf16', 'cnn_wb p3 feat'), ('nisqa_cnn_adapt_segments_bf16', _WB),
                        ('nisqa_cnn_standard_bf16', _WB), ('nisqa_cnn_standard_segments_bf16', _WB)),
    'bf16x6': Precision(2, 'bf16x6', _pack_bf16(3), ('nisqa_cnn_adapt_bf16x6', _WB), ('nisqa_cnn_adapt_segments_bf16x6', _WB),
                        ('nisqa_cnn_standard_bf16x6', _WB), ('nisqa_cnn_standard_segments_bf16x6', _WB)),
    'f16x3': Precision(3, 'bf16x6', _w.pack_adapt_cnn_f16, ('nisqa_cnn_adapt_f16', _F16), ('nisqa_cnn_adapt_segments_f16', _F16),
                       ('nisqa_cnn_standard_f16', _F16), ('nisqa_cnn_standard_segments_f16', _F16)),
    'f16x4': Precision(4, 'bf16x6', _w.pack_adapt_cnn_f16, ('nisqa_cnn_adapt_f16', _F16), ('nisqa_cnn_adapt_segments_f16', _F16),
                       ('nisqa_cnn_standard_f16', _F16), ('nisqa_cnn_standard_segments_f16', _F16)),
}
PRECISIONS = tuple(PRECISION)
CNN_MODE = {p: row.cnn_mode for p, row in PRECISION.items()}
# Self-attention and pooling per operand format: the two entries (they take the 16-bit blob behind the fp32 one where `terms` is set), the
# fused self-attention + pooling entry where one exists, and the terms per fragment of td_wb / pool_wb (None: no blob).
TdFormat = collections.namedtuple('TdFormat', 'selfatt pool fused terms')
TD = {
    'f32': TdFormat('nisqa_td_selfatt', 'nisqa_pool_att', None, None),
    'bf16x3': TdFormat('nisqa_td_selfatt_bf16', 'nisqa_pool_att_bf16', None, 2),
    'bf16x6': TdFormat('nisqa_td_selfatt_bf16x6', 'nisqa_pool_att_bf16x6', 'nisqa_td_pool_bf16x6', 3),
}
# the name a failing entry is reported under, where that is not its own
WHAT = {'nisqa_cnn_adapt_segments_bf16': 'nisqa_cnn_adapt_segments_bf16x3', 'nisqa_cnn_standard_bf16': 'nisqa_cnn_standard_bf16x3',
        'nisqa_cnn_standard_segments_bf16': 'nisqa_cnn_standard_segments_bf16x3',
        'nisqa_td_selfatt_bf16': 'nisqa_td_selfatt_bf16x3', 'nisqa_pool_att_bf16': 'nisqa_pool_att_bf16x3'}


def cnn_call(precision, stage, head, cnn_wb, p3, feat, stream):
    """stage: 'adapt' | 'segments' | 'standard' | 'standard_segments'; head: the entry's arguments up to and including cnn_w
    -> (entry name, the name _lib.check reports, the entry's whole argument list)"""
    name, tail = getattr(PRECISION[precision], stage)
    vals = {'cnn_wb': cnn_wb, 'p3': p3, 'feat': feat, 'terms': int(precision[-1])}
    return name, WHAT.get(name, name), list(head) + [vals[k] for k in tail.split()] + [stream]


def td_call(td_precision, stage, head, wb, tail):
    """stage: 'selfatt' | 'pool'; head: the arguments up to and including the fp32 blob, wb: the 16-bit blob, tail: those behind it
    -> (entry name, the name _lib.check reports, the entry's whole argument list)"""
    fmt = TD[td_precision]
    name = getattr(fmt, stage)
    return name, WHAT.get(name, name), list(head) + ([wb] if fmt.terms else []) + list(tail)


class BatchPlan(object):
    """Host-side shape metadata of one batch (the only thing the host computes per batch)."""

    def __init__(self, lengths, hop, seg_hop, max_segments, names=None):
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        self.n_clips = int(len(lengths))
        if self.n_clips == 0:
            raise ValueError('empty batch')
        self.lengths = lengths
        self.T = (1 + lengths // hop).astype(np.int64)             # librosa centre framing
        n_full = self.T - (SEG_LEN - 1)                              # NISQA_lib.py:2256
        for i in np.nonzero(n_full < 1)[0]:
            raise ValueError(
                'Sample too short. Only {} windows available but seg_length={}. '
                'Consider zero padding the audio sample. File: {}'.format(
                    int(self.T[i]), SEG_LEN, names[i] if names is not None else i))
        n = -(-n_full // seg_hop) if seg_hop > 1 else n_full        # NISQA_lib.py:2271-2273
        if max_segments is not None:
            for i in np.nonzero(n > max_segments)[0]:
                raise ValueError('n_wins {} > max_length {} --- {}. Increase max window length ms_max_segments!'.format(
                    int(n[i]), max_segments, names[i] if names is not None else i))
        self.n_wins = n.astype(np.int32)
        self.clip_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        self.frame_off = np.concatenate([[0], np.cumsum(self.T)]).astype(np.int32)
        npad = (n + TOK_PAD - 1) // TOK_PAD * TOK_PAD
        self.tok_off = np.concatenate([[0], np.cumsum(npad)]).astype(np.int32)
        self.total_samples = int(self.clip_off[-1])
        self.total_frames = int(self.frame_off[-1])
        self.total_tok = int(self.tok_off[-1])
        self.dev = None

    @classmethod
    def from_n_wins(cls, n_wins):
        """Plan for callers that already hold segments (model.forward): only the token layout is needed."""
        self = cls.__new__(cls)
        n = np.asarray(n_wins, dtype=np.int64).reshape(-1)
        self.n_clips = int(len(n))
        self.lengths = np.zeros(self.n_clips, np.int64)
        self.T = np.zeros(self.n_clips, np.int64)
        self.n_wins = n.astype(np.int32)
        self.clip_off = np.zeros(self.n_clips + 1, np.int64)
        self.frame_off = np.zeros(self.n_clips + 1, np.int32)
        npad = (n + TOK_PAD - 1) // TOK_PAD * TOK_PAD
        self.tok_off = np.concatenate([[0], np.cumsum(npad)]).astype(np.int32)
        self.total_samples, self.total_frames, self.total_tok = 0, 0, int(self.tok_off[-1])
        self.dev = None
        return self

    def to(self, device):
        """The four index tables on ``device``: packed into ONE page-locked buffer and sent with one asynchronous copy.
        (Four pageable ``.to(device)`` calls each block the host until everything queued before them on the stream has
        run -- behind a batch's 245 MB PCM copy that is 4 ms of the predict loop.)"""
        if self.dev is None or self.dev['device'] != device:
            parts = (('clip_off', self.clip_off), ('frame_off', self.frame_off), ('tok_off', self.tok_off), ('n_wins', self.n_wins))
            offs, total = [], 0
            for _, a in parts:
                offs.append(total)
                total += (a.nbytes + 15) // 16 * 16
            pin = torch.device(device).type == 'cuda'
            host = torch.empty(max(total, 16), dtype=torch.uint8, pin_memory=pin)
            hv = host.numpy()
            for (_, a), o in zip(parts, offs):
                hv[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            buf = host.to(device, non_blocking=pin)
            self.dev = {'device': device, '_buf': buf, '_host': host}
            for (k, a), o in zip(parts, offs):
                self.dev[k] = buf[o:o + a.nbytes].view(torch.from_numpy(a[:0]).dtype)
        return self.dev

    def token_index(self):
        """Indices (into the padded token axis) of the valid tokens, clip by clip."""
        return np.concatenate([self.tok_off[b] + np.arange(self.n_wins[b]) for b in range(self.n_clips)])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _or(value, default):
    return default if value is None else value


def check_segments(x, n_wins, channels):
    """The arguments of the reference's inner operator model(x, n_wins): x [B, L, channels, 48, 15] (1 channel: NL:137-142; 2, degraded
    and reference: NL:399-404), n_wins one count in [1, L] per clip and channel -> the counts as int64 [B] (channels == 1) or
    [B, channels].  Raises ValueError; no device is touched here beyond reading n_wins."""
    if not torch.is_tensor(x) or x.dim() != 5 or tuple(x.shape[2:]) != (channels, 48, SEG_LEN):
        raise ValueError('expected x of shape [B, L, {}, 48, 15], got {}'.format(
            channels, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    n = np.asarray(n_wins.detach().cpu().numpy() if torch.is_tensor(n_wins) else n_wins)
    B, L = x.shape[0], x.shape[1]
    if channels == 1:
        if n.size != B or B == 0:
            raise ValueError('n_wins must hold one count in [1, L] per clip')
        n = n.reshape(-1)
    elif n.shape != (B, channels) or B == 0:
        raise ValueError('n_wins must be of shape [B, {}], got {}'.format(channels, tuple(n.shape)))
    if not np.issubdtype(n.dtype, np.integer) and not (np.isfinite(n).all() and (n == np.floor(n)).all()):
        raise ValueError('n_wins must hold whole numbers')
    n = n.astype(np.int64)
    if (n < 1).any() or (n > L).any():
        raise ValueError('n_wins must hold one count in [1, L] per clip' + ('' if channels == 1 else ' and channel'))
    return n


# pool option of a StandardCNN + BiLSTM model -> nisqa_model_dev.arch / nisqa_lstm_pool's pool_mode
LSTM_ARCH = {'last_step_bi': 1, 'avg': 2, 'max': 3}
LSTM_POOL_MODE = {1: _lib.LSTM_POOL_LAST_STEP_BI, 2: _lib.LSTM_POOL_AVG, 3: _lib.LSTM_POOL_MAX}


def check_lstm_args(args, n_heads=1):
    """The StandardCNN + BiLSTM configurations the HIP engine runs: nisqa_tts.tar (pool=last_step_bi) and the CNN-LSTM-AVG recipe
    (config/train_nisqa_cnn_lstm_avg.yaml, pool=avg, or pool=max) -- fc 20, one bidirectional layer of 128, td_2=skip, one head.
    Returns the nisqa_model_dev.arch (1, 2, 3); anything else raises NotImplementedError naming the option, before any GPU work.
    Missing keys take the reference NISQA's defaults (NISQA_lib.py:36-73)."""
    g = lambda k, d=None: args.get(k, d)
    if g('td_2', 'skip') not in (None, 'skip'):
        raise NotImplementedError('HIP engine: td=lstm needs td_2=skip, got td_2={}'.format(g('td_2')))
    if n_heads != 1 or g('model', 'NISQA') != 'NISQA':
        raise NotImplementedError('HIP engine: td=lstm is built for model=NISQA (one MOS head), got model={}'.format(
            g('model', 'NISQA_DIM' if n_heads == 5 else 'NISQA')))
    if not g('td_lstm_bidirectional', True):
        raise NotImplementedError('HIP engine: a unidirectional LSTM (td_lstm_bidirectional=False) is not supported; the BiLSTM is')
    pool = g('pool')
    if pool not in LSTM_ARCH:
        raise NotImplementedError('HIP engine: pool={} on the LSTM is not supported (last_step_bi, avg, max)'.format(pool))
    if g('td_lstm_num_layers', 1) != 1:
        raise NotImplementedError('HIP engine: td_lstm_num_layers={} is not supported (1)'.format(g('td_lstm_num_layers')))
    if g('td_lstm_h', 128) != 128:
        raise NotImplementedError('HIP engine: td_lstm_h={} is not supported (128)'.format(g('td_lstm_h')))
    if g('cnn_fc_out_h', 20) != 20:
        raise NotImplementedError('HIP engine: cnn_fc_out_h={} is not supported with td=lstm (20)'.format(g('cnn_fc_out_h')))
    return LSTM_ARCH[pool]


# What profile_pcm / profile_segments return (HipNisqa, HipNisqaDE): device tensors in the plan's token layout.  aligned_to: NISQA_DE
# with hard alignment only -- int32 [NP], the reference token each degraded token was aligned to (-1 on padding rows) --, else None.
PoolProfile = collections.namedtuple('PoolProfile', 'scores embed weights local aligned_to')


def check_profile_args(args):
    """A score splits into per-segment weights and local scores where the pooling is a weighted mean followed by a linear layer:
    PoolAttFF and PoolAvg.  The last LSTM step (last_step_bi) and the maximum over time (max) are no such mean: NotImplementedError
    naming the pool, before any GPU work (no device is touched here)."""
    if args.get('td') == 'lstm' and args.get('pool') != 'avg':
        raise NotImplementedError('a score has no per-segment profile with pool={} (pool=att and pool=avg have one)'.format(
            args.get('pool')))


def check_profile_grad_args(args):
    """The profile is differentiable where its backward can enter the existing chain per token: behind self-attention (PoolAttFF).
    The StandardCNN + BiLSTM family's pool=avg profile is refused by name -- nisqa_lstm_train_bptt takes ONE pooled gradient per
    clip, not a dh per step --, and so is what has no profile at all (check_profile_args).  No device is touched here."""
    check_profile_args(args)
    if args.get('td') == 'lstm':
        raise NotImplementedError('the per-segment profile of the StandardCNN + BiLSTM models (pool=avg) has no gradient: the BiLSTM\'s '
                                  'backward through time takes a pooled gradient, not one per step; the plain profile works')


class HipNisqa(object):
    """nisqa.tar / nisqa_mos_only.tar (CNN-SA-AP) on one MI355X."""

    def __init__(self, args, state_dict, device=None, precision=None):
        """precision -- one of PRECISIONS, for every GEMM of the path (AdaptCNN / StandardCNN, self-attention, pooling):
        'bf16x6' (DEFAULT_PRECISION, the bench contract line): fp32 operands as three bf16 terms, an exact split, six MFMA products per
                 term pair -- the reference's operands bit for bit at 1.8 x the rate of 'f32';
        'f32'    exact fp32 MFMA, the reference's own arithmetic;
        'f16x4' / 'f16x3' (opt-in): the CNN on two f16 terms of the power-of-two-scaled tensors, four / three products (one fp32 ulp
                 off for ~25 % of the operands; as close to float64 as 'f32' by measurement); self-attention and pooling as in 'bf16x6';
        'bf16x3' (opt-in): two bf16 terms, three products: 16 of the 24 operand mantissa bits, |dMOS| <= 5e-5, the fast mode.
        The environment variable NISQA_HIP_PRECISION overrides the default."""
        a = args
        lstm = a.get('cnn_model') == 'standard' and a.get('td') == 'lstm'
        lstm_arch = check_lstm_args(a) if lstm else 0           # unsupported LSTM options raise before any GPU work
        if a.get('td') == 'self_att' and a.get('pool') in ('avg', 'max'):
            raise NotImplementedError('HIP engine: pool={} behind self-attention is not supported (pool=att)'.format(a.get('pool')))
        if not torch.cuda.is_available():
            raise RuntimeError('nisqa_amd: no GPU visible (torch.cuda.is_available() is False); '
                               'the HIP engine has no CPU fallback')
        self.lib = _lib.load()
        self.device = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
        self.args = args
        sa = a.get('cnn_model') == 'adapt' and a.get('td') == 'self_att' and a.get('pool') == 'att'
        if not (sa or lstm) or a.get('td_2') not in (None, 'skip') or a.get('td_sa_pos_enc'):
            raise NotImplementedError(
                'HIP engine covers cnn_model=adapt / td=self_att / pool=att (nisqa.tar, nisqa_mos_only.tar) and '
                'cnn_model=standard / td=lstm / pool=last_step_bi, avg or max (nisqa_tts.tar, the CNN-LSTM-AVG recipe); '
                'got cnn_model={} td={} td_2={} pool={}'.format(a.get('cnn_model'), a.get('td'), a.get('td_2'), a.get('pool')))
        if a['ms_seg_length'] != SEG_LEN or a['ms_n_mels'] != 48:
            raise NotImplementedError('HIP engine is built for 15-frame segments of 48 mel bands')
        if sa and (list(a['cnn_pool_1']) != [24, 7] or list(a['cnn_pool_2']) != [12, 5] or list(a['cnn_pool_3']) != [6, 3]
                   or a['td_sa_nhead'] != 1 or a['td_sa_d_model'] != 64 or not a.get('pool_att_h')):
            raise NotImplementedError('HIP engine is built for the nisqa.tar geometry (pools 24x7/12x5/6x3, 1 head, '
                                      'd_model 64, pool_att_h)')
        self.arch = lstm_arch           # 0 CNN-SA-AP; 1 / 2 / 3 StandardCNN + BiLSTM + last-step / average / max pooling
        # ms_sr: lb.load(path, sr=ms_sr) resamples every file to that rate first (NISQA_lib.py:2300, 2304); None in every shipped checkpoint
        self.ms_sr = int(a['ms_sr']) if a.get('ms_sr') is not None else None
        self._resample_tables = {}
        self.seg_hop = int(a['ms_seg_hop_length'])
        self.max_segments = a['ms_max_segments']
        self.dim = a['model'] == 'NISQA_DIM'
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        self.precision = precision or os.environ.get('NISQA_HIP_PRECISION') or DEFAULT_PRECISION
        if self.precision not in PRECISIONS:
            raise ValueError('precision must be one of {}, got {}'.format(', '.join(PRECISIONS), self.precision))
        row = PRECISION[self.precision]
        self.td_precision = row.td              # the operand format of self-attention / pooling
        self.cnn_wb = up(row.pack_cnn(state_dict).view(np.int16)) if row.pack_cnn else None
        self._mel = {}
        self._ws = {}                      # one workspace per stream (batches may be in flight on several)
        self._flac_ws = {}                 # the same for nisqa_flac_decode
        self._state_dict, self._input_grad = state_dict, None     # grad_segments builds its operator chain from them on first use
        self._profile_w = None                                      # pool_profile packs its blob from state_dict on first use
        if self.arch >= 1:
            # StandardCNN (split 16-bit or exact-fp32 MFMA) + BiLSTM + last-step / average / max pooling (fp32 VALU in every mode)
            self.n_layers, self.n_heads = 0, 1
            self.cnn_w = up(_w.pack_standard_cnn(state_dict))
            self.td_w = up(_w.pack_lstm_laststep(state_dict))
            self.pool_w = torch.zeros(4, dtype=torch.float32, device=self.device)
            self.td_wb = self.pool_wb = None
            return
        self.n_layers = int(a['td_sa_num_layers'])
        heads = ['pool_layers.%d.model.' % h for h in range(5)] if self.dim else ['pool.model.']
        self.n_heads = len(heads)
        self.cnn_w = up(_w.pack_adapt_cnn(state_dict))
        self.td_w = up(_w.pack_self_att(state_dict, self.n_layers))
        self.pool_w = up(_w.pack_pool_att(state_dict, heads))
        terms = TD[self.td_precision].terms
        self.td_wb = up(_w.pack_self_att_bf16(state_dict, self.n_layers, terms=terms).view(np.int16)) if terms else None
        self.pool_wb = up(_w.pack_pool_att_bf16(state_dict, heads, terms=terms).view(np.int16)) if terms else None

    # -- tables -----------------------------------------------------------------------------
    def mel_tables(self, sr):
        sr = int(sr)
        if sr not in self._mel:
            a = self.args
            t = MelTables(sr, a['ms_n_fft'], a['ms_hop_length'], a['ms_win_length'], a['ms_n_mels'], a['ms_fmax'])
            up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
            d = {'host': t, 'window': up(t.window), 'twiddle': up(t.twiddle), 'band_start': up(t.band_start),
                 'band_len': up(t.band_len), 'band_woff': up(t.band_woff), 'band_w': up(t.band_w)}
            d['cfg'] = _lib.MelCfg(t.n_fft, t.hop, t.win, t.n_mels, t.n_bins, int(t.band_w.size), 1e-8, 80.0)
            d['model'] = _lib.ModelDev(_ptr(d['window']), _ptr(d['twiddle']), _ptr(d['band_start']), _ptr(d['band_len']),
                                       _ptr(d['band_woff']), _ptr(d['band_w']), _ptr(self.cnn_w), _ptr(self.td_w),
                                       _ptr(self.pool_w), self.n_layers, self.n_heads, self.seg_hop, None,
                                       _ptr(self.cnn_wb) if self.cnn_wb is not None else None,
                                       CNN_MODE[self.precision],
                                       _ptr(self.td_wb) if self.td_wb is not None else None,
                                       _ptr(self.pool_wb) if self.pool_wb is not None else None, self.arch)
            self._mel[sr] = d
        return self._mel[sr]

    def plan(self, lengths, sr, names=None):
        return BatchPlan(lengths, self.mel_tables(sr)['host'].hop, self.seg_hop, self.max_segments, names)

    # -- ms_sr: what the batch looks like after lb.load(path, sr=ms_sr) -------------------------------------
    def rate(self, sr):
        """The rate the spectrogram is computed at for a file of rate ``sr``: ms_sr when the checkpoint sets it."""
        return int(sr) if self.ms_sr is None else self.ms_sr

    def audio_plan(self, lengths, sr, names=None):
        """plan() of a batch of files of rate ``sr`` as the network sees them (resampled to ms_sr when that is set)."""
        if self.ms_sr is None or int(sr) == self.ms_sr:
            return self.plan(lengths, sr, names)
        return self.plan(resampled_lengths(lengths, sr, self.ms_sr)[0], self.ms_sr, names)

    def resample(self, pcm, lengths, sr):
        """pcm: device tensor, the clips of ``lengths`` samples back to back at rate ``sr`` (float32 or int16 PCM) -> float32 device
        tensor, the clips at ms_sr back to back (librosa.resample(..., res_type='kaiser_best') + fix_length: nisqa_resample)."""
        sr = int(sr)
        if self.ms_sr is None or sr == self.ms_sr:
            return pcm
        ratio = float(self.ms_sr) / float(sr)
        if sr not in self._resample_tables:
            # built once per source rate, on the default stream, and complete before any stream of the predict loop reads it (the
            # loop alternates two kernel streams: a table uploaded on one of them would be unordered against the other)
            ds = torch.cuda.default_stream(self.device)
            with torch.cuda.stream(ds):
                t = torch.from_numpy(kaiser_best_table(ratio)).to(self.device)
            ds.synchronize()
            self._resample_tables[sr] = t
        table = self._resample_tables[sr]
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        n_out, valid = resampled_lengths(lengths, sr, self.ms_sr)
        offs = np.concatenate([np.concatenate([[0], np.cumsum(lengths)]), np.concatenate([[0], np.cumsum(n_out)]), valid]).astype(np.int64)
        assert pcm.numel() == int(lengths.sum()) and pcm.dtype in (torch.float32, torch.int16)
        host = torch.empty(offs.shape, dtype=torch.int64, pin_memory=True)       # page-locked + non-blocking: a pageable copy would block the host
        host.numpy()[...] = offs                                                   # until the stream has drained (caching host allocator: reuse is stream-safe)
        dev = host.to(self.device, non_blocking=True)
        b = len(lengths)
        out = torch.empty(int(n_out.sum()), dtype=torch.float32, device=self.device)
        ws = torch.empty(max(8, self.lib.nisqa_resample_workspace_bytes(b, int(n_out.max()))), dtype=torch.uint8, device=self.device)
        rc = self.lib.nisqa_resample(_ptr(pcm), 1 if pcm.dtype == torch.int16 else 0, _ptr(dev[:b + 1]), _ptr(dev[b + 1:2 * b + 2]),
                                     _ptr(dev[2 * b + 2:]), b, int(n_out.max()), ratio, _ptr(table), table.shape[0],
                                     1 << KAISER_BEST_PRECISION, _ptr(ws), ws.numel(), _ptr(out), self._stream())
        _lib.check(rc, 'nisqa_resample')
        return out

    def forward_audio(self, pcm, lengths, sr, plan, stage_events=None):
        """forward_pcm for a batch as the files hold it: resampled to ms_sr first when the checkpoint asks for that (``plan`` from
        audio_plan(lengths, sr))."""
        return self.forward_pcm(self.resample(pcm, lengths, sr), plan, self.rate(sr), stage_events)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # -- whole forward --------------------------------------------------------------------------
    def forward_pcm(self, pcm, plan, sr, stage_events=None):
        """pcm: device tensor [plan.total_samples], float32 samples or int16 PCM (scaled by 1/32768 inside the mel
        kernel, as soundfile does for lb.load) -> device tensor [B, n_heads].

        stage_events: optional list of 6 recorded-once torch.cuda.Event(enable_timing=True); they are
        re-recorded at the stage boundaries (profiling hook of nisqa_model_dev)."""
        assert pcm.dtype in (torch.float32, torch.int16) and pcm.is_cuda and pcm.numel() == plan.total_samples
        mt = self.mel_tables(sr)
        d = plan.to(self.device)
        need = self.lib.nisqa_workspace_bytes(plan.n_clips, plan.total_frames, plan.total_tok)
        skey = torch.cuda.current_stream(self.device).cuda_stream
        ws = self._ws.get(skey)
        if ws is None or ws.numel() < need:
            ws = self._ws[skey] = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=self.device)
        out = torch.empty((plan.n_clips, self.n_heads), dtype=torch.float32, device=self.device)
        model = _lib.ModelDev.from_buffer_copy(mt['model'])
        if stage_events is not None:
            arr = (ctypes.c_void_p * 6)(*[ctypes.c_void_p(e.cuda_event if e is not None else None) for e in stage_events])
            model.stage_events = ctypes.cast(arr, ctypes.c_void_p)
        entry = self.lib.nisqa_predict_batch_pcm16 if pcm.dtype == torch.int16 else self.lib.nisqa_predict_batch
        rc = entry(_ptr(pcm), _ptr(d['clip_off']), _ptr(d['frame_off']), _ptr(d['tok_off']),
                   _ptr(d['n_wins']), plan.n_clips, plan.total_frames, plan.total_tok,
                   ctypes.byref(mt['cfg']), ctypes.byref(model), _ptr(ws),
                   ws.numel(), _ptr(out), self._stream())
        _lib.check(rc, 'nisqa_predict_batch')
        return out

    def decode(self, raw_dev, clips, n_samples, out=None):
        """raw_dev: uint8 device tensor, WAV data chunks as the files hold them; clips: their nisqa_wav_clip table (numpy structured
        array of lib.WavClip's layout, src_off into raw_dev, dst_off into the result) -> float32 device tensor [n_samples], what
        lb.load(path, sr=None) returns for each clip (nisqa_wav_decode).  The table is checked here, on the host: the kernel skips
        an entry it cannot take, it does not report it."""
        t = np.ascontiguousarray(clips, dtype=np.dtype(_lib.WavClip)).reshape(-1)
        n_samples = int(n_samples)
        assert raw_dev.dtype == torch.uint8 and raw_dev.is_cuda and raw_dev.is_contiguous()
        if out is None:
            out = torch.empty(n_samples, dtype=torch.float32, device=self.device)
        assert out.dtype == torch.float32 and out.numel() >= n_samples and out.is_contiguous()
        if len(t) == 0 or int(t['n_frames'].max()) <= 0:
            return out
        ch, cont, enc = t['channels'].astype(np.int64), t['container'].astype(np.int64), t['encoding'] & ~_lib.WAVENC_BIG_ENDIAN
        enc_ok = ((enc == _lib.WAVENC_PCM) & (cont >= 1) & (cont <= 4)) | ((enc == _lib.WAVENC_FLOAT) & ((cont == 4) | (cont == 8))) \
            | (((enc == _lib.WAVENC_ALAW) | (enc == _lib.WAVENC_MULAW)) & (cont == 1))
        ok = enc_ok & (ch >= 1) & (ch * cont <= _lib.WAV_DECODE_MAX_BLOCK) & (t['channel'] >= -1) & (t['channel'] < ch) \
            & ((t['channel'] >= 0) | (ch <= _lib.WAV_DECODE_MAX_MEAN)) & (t['n_frames'] >= 0) \
            & (t['src_off'] >= 0) & (t['src_off'] % 16 == 0) & (t['src_off'] + t['n_frames'] * ch * cont <= raw_dev.numel()) \
            & (t['dst_off'] >= 0) & (t['dst_off'] + t['n_frames'] <= n_samples)
        if not ok.all():
            raise ValueError('nisqa_wav_decode: table entry %d is outside what the kernel takes: %r' % (int(np.flatnonzero(~ok)[0]), t[~ok][0]))
        host = torch.empty(t.nbytes, dtype=torch.uint8, pin_memory=True)         # page-locked + non-blocking, like the tables of resample
        host.numpy()[...] = t.view(np.uint8)
        dev = host.to(self.device, non_blocking=True)
        rc = self.lib.nisqa_wav_decode(_ptr(raw_dev), raw_dev.numel(), _ptr(dev), len(t), max(1, int(t['n_frames'].max())),
                                       _ptr(out), self._stream())
        _lib.check(rc, 'nisqa_wav_decode')
        return out

    def flac_decode(self, raw_dev, clips, frames_off, n_rows, n_samples, out_i16, out=None, ws=None):
        """raw_dev: uint8 device tensor holding FLAC frame regions as the files have them and, from byte ``frames_off`` on, their
        ``n_rows`` nisqa_flac_frame rows (what nisqa_ingest_flac_read writes); clips: the nisqa_flac_clip table (numpy structured array
        of lib.FlacClip's layout; frame0 and md5_off are filled in here) -> (out, status): out an int16 (``out_i16``: mono 16-bit
        streams only) or float32 device tensor [n_samples] with clip i at dst_off, status an int32 device tensor [n_clips + 1], all
        zero when every frame and every MD5 held (nisqa_flac_decode).  Nothing is synchronised: the caller reads ``status`` with the
        batch's results (ingest.check_flac_status).  The clip table is checked here on the host; the frame rows, which native code
        wrote, are checked against it on the device."""
        t = np.ascontiguousarray(clips, dtype=np.dtype(_lib.FlacClip)).reshape(-1).copy()
        n_samples, n_rows, frames_off = int(n_samples), int(n_rows), int(frames_off)
        assert raw_dev.dtype == torch.uint8 and raw_dev.is_cuda and raw_dev.is_contiguous()
        dtype = torch.int16 if out_i16 else torch.float32
        if out is None:
            out = torch.empty(n_samples, dtype=dtype, device=self.device)
        assert out.dtype == dtype and out.numel() >= n_samples and out.is_contiguous()
        ch, bits, nf = t['channels'].astype(np.int64), t['bits'].astype(np.int64), t['n_frames'].astype(np.int64)
        t['frame0'] = np.concatenate(([0], np.cumsum(nf[:-1]))) if len(t) else 0
        ok = (ch >= 1) & (ch <= 2) & (bits >= 4) & (bits <= 24) & (t['channel'] >= -1) & (t['channel'] < ch) \
            & (t['n_samples'] >= 1) & (t['n_samples'] < 2 ** 31) & (t['block_size'] >= 1) & (t['block_size'] <= 65535) \
            & (nf == (t['n_samples'] + t['block_size'] - 1) // np.maximum(t['block_size'], 1)) \
            & (t['src_off'] >= 0) & (t['src_off'] % 16 == 0) & (t['src_bytes'] >= 1) & (t['src_bytes'] < 2 ** 31) \
            & (t['src_off'] + t['src_bytes'] <= raw_dev.numel()) & (t['dst_off'] >= 0) & (t['dst_off'] + t['n_samples'] <= n_samples)
        if out_i16:
            ok &= (bits == 16) & (ch == 1)
        if len(t) == 0 or not ok.all() or int(nf.sum()) != n_rows or frames_off < 0 or frames_off % 4 or frames_off + 16 * n_rows > raw_dev.numel():
            bad = t[~ok][0] if len(t) and not ok.all() else (n_rows, frames_off)
            raise ValueError('nisqa_flac_decode: the tables are outside what the kernel takes: %r' % (bad,))
        need_md5 = (t['md5_set'] != 0) & (not out_i16)
        sizes = np.where(need_md5, (t['n_samples'] * ch * ((bits + 7) // 8) + 3) // 4 * 4, 0)
        t['md5_off'] = np.cumsum(sizes) - sizes
        md5_bytes = int(sizes.sum())
        max_block, max_ch = int(t['block_size'].max()), int(ch.max())
        need = self.lib.nisqa_flac_workspace_bytes(n_rows, max_block, max_ch, md5_bytes)
        if ws is None:
            skey = torch.cuda.current_stream(self.device).cuda_stream
            ws = self._flac_ws.get(skey)
            if ws is None or ws.numel() < need:
                ws = self._flac_ws[skey] = None              # (the old one goes back to the allocator first)
                ws = self._flac_ws[skey] = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=self.device)
        status = torch.zeros(len(t) + 1, dtype=torch.int32, device=self.device)
        host = torch.empty(t.nbytes, dtype=torch.uint8, pin_memory=True)
        host.numpy()[...] = t.view(np.uint8)
        dev = host.to(self.device, non_blocking=True)
        rc = self.lib.nisqa_flac_decode(_ptr(raw_dev), raw_dev.numel(), _ptr(dev), len(t), ctypes.c_void_p(raw_dev.data_ptr() + frames_off),
                                        n_rows, max_block, max_ch, 1 if out_i16 else 0, _ptr(out), n_samples, md5_bytes, _ptr(ws),
                                        ws.numel(), _ptr(status), self._stream())
        _lib.check(rc, 'nisqa_flac_decode')
        return out, status

    def pcm16_to_f32(self, pcm16):
        out = torch.empty(pcm16.numel(), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nisqa_pcm16_to_f32(_ptr(pcm16), _ptr(out), pcm16.numel(), self._stream()), 'nisqa_pcm16_to_f32')
        return out

    # -- stage-by-stage API (parity tests, profiling) ---------------------------------------------
    def mel(self, pcm, plan, sr, clamp=True):
        """-> (mel_tm [TT,48] dB, clip_floor [B]); with clamp the top_db floor is applied in place."""
        mt = self.mel_tables(sr)
        d = plan.to(self.device)
        mel = torch.empty((plan.total_frames, 48), dtype=torch.float32, device=self.device)
        cmax = torch.zeros(plan.n_clips, dtype=torch.int32, device=self.device)
        floor = torch.empty(plan.n_clips, dtype=torch.float32, device=self.device)
        entry = self.lib.nisqa_mel_db_pcm16 if pcm.dtype == torch.int16 else self.lib.nisqa_mel_db
        _lib.check(entry(_ptr(pcm), _ptr(d['clip_off']), _ptr(d['frame_off']), plan.n_clips,
                         plan.total_frames, ctypes.byref(mt['cfg']), _ptr(mt['window']),
                         _ptr(mt['twiddle']), _ptr(mt['band_start']), _ptr(mt['band_len']),
                         _ptr(mt['band_woff']), _ptr(mt['band_w']), _ptr(mel), _ptr(cmax),
                         self._stream()), 'nisqa_mel_db')
        _lib.check(self.lib.nisqa_mel_finalize(_ptr(mel), _ptr(d['frame_off']), plan.n_clips, plan.total_frames,
                                               _ptr(cmax), 80.0, _ptr(floor), 1 if clamp else 0, self._stream()),
                   'nisqa_mel_finalize')
        return mel, floor

    def _cnn_stage(self, stage, head, plan, feat, p3_rows):
        """run the stage's entry of this precision (head: its arguments up to cnn_w) -> the pooled-conv scratch [NP][p3_rows][64] where
        the entry writes one, else None"""
        needs_p3 = 'p3' in getattr(PRECISION[self.precision], stage)[1].split()
        p3 = torch.empty((plan.total_tok, p3_rows, 64), dtype=torch.float32, device=self.device) if needs_p3 else None
        name, what, args = cnn_call(self.precision, stage, head + (_ptr(self.cnn_w),), _ptr(self.cnn_wb) if self.cnn_wb is not None else None,
                                    _ptr(p3) if needs_p3 else None, _ptr(feat), self._stream())
        _lib.check(getattr(self.lib, name)(*args), what)
        return p3

    def _mel_head(self, mel_tm, clip_floor, plan):
        d = plan.to(self.device)
        return (_ptr(mel_tm), _ptr(d['frame_off']), _ptr(d['tok_off']), _ptr(d['n_wins']), _ptr(clip_floor), plan.n_clips, plan.total_tok,
                self.seg_hop)

    def cnn(self, mel_tm, clip_floor, plan):
        """AdaptCNN -> (feat [NP, 384], the pooled conv4 tensor [NP, 18, 64] or None: the one-launch kernels keep it out of memory)"""
        feat = torch.zeros((plan.total_tok, 384), dtype=torch.float32, device=self.device)
        return feat, self._cnn_stage('adapt', self._mel_head(mel_tm, clip_floor, plan), plan, feat, 18)

    def _segments_head(self, x, plan):
        d = plan.to(self.device)
        return (_ptr(x), x.shape[1], _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, plan.total_tok)

    def cnn_segments(self, x, plan):
        """AdaptCNN on the segment tensor x [B, L, 1, 48, 15] (device, float32, contiguous) -> feat [NP, 384]"""
        feat = torch.empty((plan.total_tok, 384), dtype=torch.float32, device=self.device)
        self._cnn_stage('segments', self._segments_head(x, plan), plan, feat, 18)
        return feat

    def cnn_std_segments(self, x, plan):
        """StandardCNN + fc_out on the segment tensor x [B, L, 1, 48, 15] (device, float32, contiguous) -> feat20 [NP, 20]"""
        feat = torch.zeros((plan.total_tok, 20), dtype=torch.float32, device=self.device)
        self._cnn_stage('standard_segments', self._segments_head(x, plan), plan, feat, 12)
        return feat

    def forward_segments(self, x, n_wins):
        """Reference inner operator model(x[B,L,1,48,15], n_wins[B]) -> [B, heads] (NL:137-142, NL:260-268)."""
        n = check_segments(x, n_wins, 1)
        x = x.to(self.device, dtype=torch.float32).contiguous()
        plan = BatchPlan.from_n_wins(n)
        if self.arch >= 1:
            return self.lstm(self.cnn_std_segments(x, plan), plan)[0]
        return self.td_pool(self.cnn_segments(x, plan), plan)

    def grad_segments(self, x, n_wins, grad_out):
        """The backward of forward_segments in precision 'f32' / 'bf16x6', for the CNN-SA-AP models (input_grad.InputGrad) and the
        StandardCNN + BiLSTM ones (input_grad.InputGradLSTM): grad_out [B, heads] -> d (sum grad_out * model(x, n_wins)) / d x,
        float32 [B, L, 1, 48, 15] on the engine's device -- the reference's module in eval mode (BatchNorm on the running
        statistics, no dropout, the key mask / the packed sequence over n_wins); rows l >= n_wins[b] are exactly zero.
        forward_segments keeps no activation, so this call recomputes the network with its activations in HBM: it costs a
        second forward (nisqa_amd/input_grad.py).  NISQA_DE has its own engine class and its own grad_segments
        (HipNisqaDE.grad_segments, input_grad.InputGradDE)."""
        from . import input_grad
        input_grad.check_precision(self.precision)
        if self._input_grad is None:
            self._input_grad = (input_grad.InputGrad if self.arch == 0 else input_grad.InputGradLSTM)(self, self._state_dict)
        return self._input_grad(x, n_wins, grad_out)

    # -- the gradient with respect to the audio samples (csrc/mel_bwd.hip) ----------------------------------
    def segments_from_mel(self, mel_clamped, plan):
        """clamped dB rows [TT, 48] -> the segment tensor x [B, L, 1, 48, 15] the segment-fed CNN reads, L = the largest n_wins:
        segment k of clip b = frames seg_hop k .. seg_hop k + 14 (NISQA_lib.py:2266-2280); rows k >= n_wins[b] are zero.  Device
        indexing, no arithmetic: the values are mel_clamped's bits."""
        L = int(plan.n_wins.max())
        k, j = np.arange(L)[None, :, None], np.arange(SEG_LEN)[None, None, :]
        valid = k < plan.n_wins[:, None, None]
        idx = np.where(valid, plan.frame_off[:-1, None, None].astype(np.int64) + self.seg_hop * k + j, 0)
        rows = mel_clamped[torch.from_numpy(idx).to(self.device)]                           # [B, L, 15, 48]
        rows = rows.masked_fill(~torch.from_numpy(valid[:, :, :1]).to(self.device)[..., None], 0.0)
        return rows.permute(0, 1, 3, 2).unsqueeze(2).contiguous()

    def segments_from_mel_db(self, mel_db, clip_floor, plan, L=None):
        """segments_from_mel(torch.maximum(mel_db, floor of each frame's clip), plan) in one launch (nisqa_mel_segments_fwd): the
        UNCLAMPED dB rows [TT, 48] and clip_floor [B] of mel(..., clamp=False) -> x [B, L, 1, 48, 15], L >= the largest n_wins
        (default: that count); rows k >= n_wins[b] are exact zeros.  The same bits as the indexing path, without its index
        upload, gather, mask and transposing copy."""
        n_max = int(plan.n_wins.max())
        L = n_max if L is None else int(L)
        if L < n_max:
            raise ValueError('L = {} is smaller than the largest segment count {}'.format(L, n_max))
        assert mel_db.dtype == torch.float32 and mel_db.is_cuda and mel_db.is_contiguous() \
            and tuple(mel_db.shape) == (plan.total_frames, 48)
        assert clip_floor.dtype == torch.float32 and clip_floor.is_cuda and clip_floor.is_contiguous() \
            and clip_floor.numel() == plan.n_clips
        d = plan.to(self.device)
        x = torch.empty((plan.n_clips, L, 1, 48, SEG_LEN), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nisqa_mel_segments_fwd(_ptr(mel_db), _ptr(clip_floor), _ptr(d['frame_off']), _ptr(d['n_wins']),
                                                   plan.n_clips, plan.total_frames, self.seg_hop, L, _ptr(x), self._stream()),
                   'nisqa_mel_segments_fwd')
        return x

    def segments_to_mel_bwd(self, dx, plan):
        """The adjoint of segments_from_mel: dx [B, L, 1, 48, 15] (float32, contiguous; rows k >= n_wins[b] are never read)
        -> d / d mel_clamped [TT, 48]; frames no segment holds get 0 (nisqa_segments_to_mel_bwd)."""
        assert dx.dtype == torch.float32 and dx.is_cuda and dx.is_contiguous() and dx.shape[0] == plan.n_clips \
            and tuple(dx.shape[2:]) == (1, 48, SEG_LEN) and dx.shape[1] >= int(plan.n_wins.max())
        d = plan.to(self.device)
        dmel = torch.empty((plan.total_frames, 48), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nisqa_segments_to_mel_bwd(_ptr(dx), dx.shape[1], _ptr(d['n_wins']), _ptr(d['frame_off']), plan.n_clips,
                                                      plan.total_frames, self.seg_hop, _ptr(dmel), self._stream()),
                   'nisqa_segments_to_mel_bwd')
        return dmel

    def mel_bwd(self, pcm, plan, sr, g, mel_db, clip_floor):
        """The backward of mel(pcm, plan, sr, clamp=True): g [TT, 48] = d L / d (clamped dB rows), mel_db / clip_floor what
        mel(..., clamp=False) returned for the same pcm -> d L / d pcm, float32 [plan.total_samples].  Three launches
        (nisqa_mel_db_bwd_gate, nisqa_mel_frame_bwd, nisqa_mel_overlap_add_bwd) around a workspace of total_frames * win floats;
        the spectra are recomputed, nothing of the forward but its dB rows is read.  float32 samples only."""
        assert pcm.dtype == torch.float32 and pcm.is_cuda and pcm.is_contiguous() and pcm.numel() == plan.total_samples
        for t in (g, mel_db):
            assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == (plan.total_frames, 48)
        assert clip_floor.dtype == torch.float32 and clip_floor.numel() == plan.n_clips
        mt = self.mel_tables(sr)
        d = plan.to(self.device)
        cfg, st = ctypes.byref(mt['cfg']), self._stream()
        dm = torch.empty_like(mel_db)
        _lib.check(self.lib.nisqa_mel_db_bwd_gate(_ptr(g), _ptr(mel_db), _ptr(clip_floor), _ptr(d['frame_off']), plan.n_clips,
                                                  plan.total_frames, cfg, _ptr(dm), st), 'nisqa_mel_db_bwd_gate')
        ws = torch.empty(int(self.lib.nisqa_mel_bwd_workspace_bytes(plan.total_frames, mt['cfg'].win)), dtype=torch.uint8,
                         device=self.device)
        _lib.check(self.lib.nisqa_mel_frame_bwd(_ptr(pcm), _ptr(d['clip_off']), _ptr(d['frame_off']), plan.n_clips, plan.total_frames,
                                                cfg, _ptr(mt['window']), _ptr(mt['twiddle']), _ptr(mt['band_start']),
                                                _ptr(mt['band_len']), _ptr(mt['band_woff']), _ptr(mt['band_w']), _ptr(dm), _ptr(ws),
                                                ws.numel(), st), 'nisqa_mel_frame_bwd')
        dpcm = torch.empty(plan.total_samples, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nisqa_mel_overlap_add_bwd(_ptr(ws), _ptr(d['clip_off']), _ptr(d['frame_off']), plan.n_clips,
                                                      plan.total_frames, plan.total_samples, cfg, _ptr(dpcm), st),
                   'nisqa_mel_overlap_add_bwd')
        return dpcm

    def grad_audio(self, pcm, plan, sr, grad_out):
        """The backward of forward_pcm in precision 'f32' / 'bf16x6': pcm float32 [plan.total_samples] at rate ``sr`` (the rate the
        spectrogram is computed at: the resampler of ms_sr has no backward), grad_out [B, heads]
        -> d (sum grad_out * forward_pcm(pcm, plan, sr)) / d pcm, float32 [plan.total_samples].
        Nothing is kept from the forward: the dB rows are recomputed (mel, unclamped, with clip_floor), the clamped segment tensor
        is cut from them on the device, grad_segments (a recomputation of the network) gives d / d x, and the
        segment adjoint and the mel backward carry it to the samples.  The segment-fed and the frame-fed CNN give the same bits
        for the same window, so the gradient belongs to the values forward_pcm returned."""
        return self._audio_bwd(pcm, plan, sr, lambda x: self.grad_segments(x, plan.n_wins, grad_out))

    def _audio_bwd(self, pcm, plan, sr, segments_bwd):
        """grad_audio's chain around ``segments_bwd``: x [B, L, 1, 48, 15] -> d / d x"""
        from . import input_grad
        input_grad.check_precision(self.precision)
        assert pcm.dtype == torch.float32, 'int16 PCM has no gradient'
        pcm = pcm.detach().contiguous()
        mel_db, floor = self.mel(pcm, plan, sr, clamp=False)
        clip_of_frame = torch.from_numpy(np.repeat(np.arange(plan.n_clips), plan.T)).to(self.device)
        x = self.segments_from_mel(torch.maximum(mel_db, floor[clip_of_frame][:, None]), plan)
        dx = segments_bwd(x)
        del x
        return self.mel_bwd(pcm, plan, sr, self.segments_to_mel_bwd(dx, plan), mel_db, floor)

    # -- the gradient of the per-segment profile (nisqa_pool_profile_bwd) ------------------------------------------
    def profile_cotangents(self, plan, d_weights, d_local, d_embed):
        """Cotangents of a PoolProfile in the plan's token layout ([NP, heads], [NP, heads], [NP, 64]; None: zero) -> the same over
        the plan's valid tokens, clip by clip, float32 on the device: what input_grad.InputGrad takes as ``profile_cot``.  Padding
        rows are dropped here, whatever they hold."""
        idx = torch.from_numpy(plan.token_index()).to(self.device)
        out = []
        for name, t, width in (('d_weights', d_weights, self.n_heads), ('d_local', d_local, self.n_heads), ('d_embed', d_embed, 64)):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (plan.total_tok, width)):
                raise ValueError('expected {} of shape [{}, {}], got {}'.format(
                    name, plan.total_tok, width, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
            out.append(None if t is None else t.detach().to(self.device, dtype=torch.float32)[idx].contiguous())
        return tuple(out)

    def grad_profile_segments(self, x, n_wins, d_scores=None, d_weights=None, d_local=None, d_embed=None):
        """The backward of profile_segments in precision 'f32' / 'bf16x6', CNN-SA-AP models: d_scores [B, heads] and d_weights,
        d_local [NP, heads], d_embed [NP, 64] in the token layout of BatchPlan.from_n_wins(n_wins) (padding rows are ignored); None
        means zero -> d (sum d_scores * scores + sum d_weights * weights + sum d_local * local + sum d_embed * embed) / d x, float32
        [B, L, 1, 48, 15], rows l >= n_wins[b] exact zeros.  grad_segments with one more launch: the token-level cotangents become
        d / d (the rows the pooling read) in nisqa_pool_profile_bwd, are added to the pooling heads' backward of d_scores (which
        is skipped when d_scores is None), and ONE walk back through self-attention and the CNN serves all four.  The BiLSTM
        family's pool=avg profile has no backward (its BPTT entry takes a pooled gradient, not one per step)."""
        from . import input_grad
        check_profile_grad_args(self.args)
        input_grad.check_precision(self.precision)
        n = check_segments(x, n_wins, 1)
        cot = self.profile_cotangents(BatchPlan.from_n_wins(n), d_weights, d_local, d_embed)
        if self._input_grad is None:
            self._input_grad = input_grad.InputGrad(self, self._state_dict)
        return self._input_grad(x, n_wins, d_scores, profile_cot=cot)

    def grad_profile_audio(self, pcm, plan, sr, d_scores=None, d_weights=None, d_local=None, d_embed=None):
        """The backward of profile_pcm, built as grad_audio is on grad_segments: pcm float32 [plan.total_samples] at the rate the
        spectrogram is computed at, the cotangents of grad_profile_segments in the plan's token layout
        -> d / d pcm, float32 [plan.total_samples]."""
        check_profile_grad_args(self.args)
        return self._audio_bwd(pcm, plan, sr,
                               lambda x: self.grad_profile_segments(x, plan.n_wins, d_scores, d_weights, d_local, d_embed))

    # -- nisqa_tts.tar stages ------------------------------------------------------------------------
    def cnn_std(self, mel_tm, clip_floor, plan):
        """StandardCNN + fc_out -> feat20 [NP, 20]"""
        feat = torch.zeros((plan.total_tok, 20), dtype=torch.float32, device=self.device)
        self._cnn_stage('standard', self._mel_head(mel_tm, clip_floor, plan), plan, feat, 12)
        return feat

    def lstm(self, feat20, plan, want_seq=False, arch=None, want_pooled=False):
        """BiLSTM + the pooling of ``arch`` (default: the engine's own; 1 PoolLastStepBi, 2 PoolAvg, 3 PoolMax)
        -> (out [B,1], seq [NP,256] or None), and the pooled vector [B,256] as a third item when want_pooled"""
        arch = self.arch if arch is None else arch
        if arch not in LSTM_POOL_MODE:
            raise ValueError('lstm(): arch must be 1, 2 or 3, got {}'.format(arch))
        d = plan.to(self.device)
        hfin = torch.empty((plan.n_clips, 256), dtype=torch.float32, device=self.device)
        seq = torch.zeros((plan.total_tok, 256), dtype=torch.float32, device=self.device) if want_seq else None
        out = torch.empty((plan.n_clips, 1), dtype=torch.float32, device=self.device)
        if arch == 1:
            _lib.check(self.lib.nisqa_lstm_laststep(_ptr(feat20), _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips,
                                                    _ptr(self.td_w), _ptr(hfin), _ptr(seq) if want_seq else None, _ptr(out),
                                                    self._stream()), 'nisqa_lstm_laststep')
        else:
            _lib.check(self.lib.nisqa_lstm_pool(_ptr(feat20), _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, _ptr(self.td_w),
                                                LSTM_POOL_MODE[arch], _ptr(hfin), _ptr(seq) if want_seq else None, _ptr(out),
                                                self._stream()), 'nisqa_lstm_pool')
        return (out, seq, hfin) if want_pooled else (out, seq)

    def td(self, feat, plan, td_w=None, td_wb=None, n_layers=None):
        """self-attention -> x [NP, 64]; the weights default to the engine's own"""
        td_w, td_wb, n_layers = _or(td_w, self.td_w), _or(td_wb, self.td_wb), _or(n_layers, self.n_layers)
        d = plan.to(self.device)
        ws = torch.empty(plan.total_tok * 64 * 9, dtype=torch.float32, device=self.device)
        x = torch.zeros((plan.total_tok, 64), dtype=torch.float32, device=self.device)
        name, what, args = td_call(self.td_precision, 'selfatt',
                                   (_ptr(feat), _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, plan.total_tok, n_layers, _ptr(td_w)),
                                   _ptr(td_wb) if td_wb is not None else None, (_ptr(ws), _ptr(x), self._stream()))
        _lib.check(getattr(self.lib, name)(*args), what)
        return x

    def td_pool(self, feat, plan, td_w=None, td_wb=None, n_layers=None, pool_w=None, pool_wb=None, n_heads=None, want_x=False):
        """self-attention + attention pooling as the whole-batch forward runs them: in the three-term modes ONE chain of
        n_layers + 1 launches (nisqa_td_pool_bf16x6), otherwise td() then pool().  want_x: -> (out, x [NP, 64]), x the rows the
        pooling read (the chain writes them in either form; rows of padding tokens hold whatever the kernels left there)"""
        fused = TD[self.td_precision].fused
        if not fused:
            x = self.td(feat, plan, td_w, td_wb, n_layers)
            out = self.pool(x, plan, pool_w, pool_wb, n_heads)
            return (out, x) if want_x else out
        td_w, td_wb, n_layers = _or(td_w, self.td_w), _or(td_wb, self.td_wb), _or(n_layers, self.n_layers)
        pool_wb, n_heads = _or(pool_wb, self.pool_wb), _or(n_heads, self.n_heads)
        d = plan.to(self.device)
        ws = torch.empty(plan.total_tok * 64 * 9, dtype=torch.float32, device=self.device)
        wsp = torch.empty(plan.total_tok * 16 + plan.n_clips, dtype=torch.float32, device=self.device)
        x = torch.zeros((plan.total_tok, 64), dtype=torch.float32, device=self.device)
        out = torch.empty((plan.n_clips, n_heads), dtype=torch.float32, device=self.device)
        _lib.check(getattr(self.lib, fused)(_ptr(feat), _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, plan.total_tok, n_layers,
                                            _ptr(td_w), _ptr(td_wb), n_heads, _ptr(pool_wb), _ptr(ws), _ptr(x), _ptr(wsp), _ptr(out),
                                            self._stream()), fused)
        return (out, x) if want_x else out

    def pool(self, x, plan, pool_w=None, pool_wb=None, n_heads=None):
        """attention pooling -> [B, n_heads]; the weights default to the engine's own"""
        pool_w, pool_wb, n_heads = _or(pool_w, self.pool_w), _or(pool_wb, self.pool_wb), _or(n_heads, self.n_heads)
        d = plan.to(self.device)
        ws = torch.empty(plan.total_tok * 16, dtype=torch.float32, device=self.device)
        out = torch.empty((plan.n_clips, n_heads), dtype=torch.float32, device=self.device)
        name, what, args = td_call(self.td_precision, 'pool',
                                   (_ptr(x), _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, plan.total_tok, n_heads, _ptr(pool_w)),
                                   _ptr(pool_wb) if pool_wb is not None else None, (_ptr(ws), _ptr(out), self._stream()))
        _lib.check(getattr(self.lib, name)(*args), what)
        return out

    # -- per-segment profile of a score (csrc/pool_profile.hip) ---------------------------------------------------
    def pool_profile(self, x, plan):
        """nisqa_pool_profile on the rows x the pooling read ([NP, 64] behind self-attention, [NP, 256] behind the BiLSTM with
        pool=avg) -> (weights [NP, heads], local [NP, heads]); rows of padding tokens are never read and come back as zeros."""
        check_profile_args(self.args)
        mode, ld = (0, 64) if self.arch == 0 else (1, 256)
        assert x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() and tuple(x.shape) == (plan.total_tok, ld)
        d = plan.to(self.device)
        weights = torch.empty((plan.total_tok, self.n_heads), dtype=torch.float32, device=self.device)
        local = torch.empty((plan.total_tok, self.n_heads), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.nisqa_pool_profile(_ptr(x), ld, _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, plan.total_tok,
                                               self.n_heads, mode, _ptr(self.profile_weights()), _ptr(weights), _ptr(local),
                                               self._stream()), 'nisqa_pool_profile')
        return weights, local

    def profile_weights(self):
        """The natural-order fp32 blob nisqa_pool_profile and nisqa_pool_profile_bwd read, packed from the state_dict on first use"""
        if self._profile_w is None:
            heads = ['pool_layers.%d.model.' % h for h in range(5)] if self.dim else ['pool.model.']
            blob = _w.pack_pool_profile(self._state_dict, heads) if self.arch == 0 else _w.pack_pool_profile_avg(self._state_dict)
            self._profile_w = torch.from_numpy(blob).to(self.device)
        return self._profile_w

    def _profile(self, scores, x, plan, aligned_to=None):
        weights, local = self.pool_profile(x, plan)
        valid = torch.zeros(plan.total_tok, dtype=torch.bool, device=self.device)
        valid[torch.from_numpy(plan.token_index()).to(self.device)] = True
        embed = torch.where(valid[:, None], x, torch.zeros((), dtype=x.dtype, device=self.device))     # padding rows: exact zeros
        return PoolProfile(scores, embed, weights, local, aligned_to)

    def profile_features(self, feat, plan):
        """The CNN rows of a plan -> PoolProfile: the scores from the chain forward_pcm / forward_segments run (bit for bit theirs),
        the rows that chain's pooling read, and nisqa_pool_profile on them."""
        check_profile_args(self.args)
        scores, x = self.td_pool(feat, plan, want_x=True) if self.arch == 0 else self.lstm(feat, plan, want_seq=True)
        return self._profile(scores, x, plan)

    def profile_pcm(self, pcm, plan, sr):
        """forward_pcm with the score taken apart per segment -> PoolProfile(scores [B, heads], embed [NP, D], weights [NP, heads],
        local [NP, heads]) in the plan's token layout (clip b: rows plan.tok_off[b] .. + plan.n_wins[b]; padding rows are exact zeros):
          scores   forward_pcm's, bit for bit (the same kernels in the same order; they do not come from the profile);
          embed    the rows the pooling read: the last self-attention layer's output (D = 64), or the BiLSTM's with pool=avg (256);
          weights  the share a_t of segment t in the score: PoolAttFF's softmax over the clip's segments (one track per head, NISQA_DIM:
                   mos, noi, dis, col, loud), 1 / n_wins for PoolAvg; they sum to 1 per clip and head;
          local    what segment t says on its own, in MOS units: s_t = w3 . x_t + b3 (PoolAvg: w . h_t + b).
        score = sum_t a_t s_t up to float32 rounding.  pool=last_step_bi and pool=max have no such decomposition:
        NotImplementedError, before any GPU work.  Not a throughput path: the stages run one by one with their tensors in HBM."""
        check_profile_args(self.args)
        assert pcm.dtype in (torch.float32, torch.int16) and pcm.is_cuda and pcm.numel() == plan.total_samples
        mel, floor = self.mel(pcm, plan, sr, clamp=False)
        return self.profile_features(self.cnn(mel, floor, plan)[0] if self.arch == 0 else self.cnn_std(mel, floor, plan), plan)

    def profile_audio(self, pcm, lengths, sr, plan):
        """profile_pcm for a batch as the files hold it (resampled to ms_sr first when the checkpoint sets it; see forward_audio)"""
        check_profile_args(self.args)
        return self.profile_pcm(self.resample(pcm, lengths, sr), plan, self.rate(sr))

    def profile_segments(self, x, n_wins):
        """profile_pcm for the reference's inner operator model(x[B,L,1,48,15], n_wins[B]): scores are forward_segments', bit for bit;
        the token layout is BatchPlan.from_n_wins(n_wins)'s."""
        check_profile_args(self.args)
        n = check_segments(x, n_wins, 1)
        x = x.to(self.device, dtype=torch.float32).contiguous()
        plan = BatchPlan.from_n_wins(n)
        return self.profile_features(self.cnn_segments(x, plan) if self.arch == 0 else self.cnn_std_segments(x, plan), plan)


# -- NISQA_DE (double-ended): reference NISQA_lib.py:272-424 ------------------------------------------------------------------
DE_ALIGN = {'dot': 0, 'cosine': 1}                 # AttDot / AttCosine (NISQA_lib.py:1272-1294)
DE_APPLY = {'hard': 0, 'soft': 1}                  # ApplyHardAttention / ApplySoftAttention (:1359-1378)
DE_FUSE = {'x/y/-': 0, '+/-': 1, 'x/y': 2}         # Fusion without lin_fusion (:1380-1417)
DE_FUSE_WIDTH = {'x/y/-': 192, '+/-': 128, 'x/y': 128}
DE_FEAT_LD = 384                                   # row stride of the fused features: the self-attention kernels' projection width


def check_de_args(args, precision=None):
    """The NISQA_DE configurations the HIP engine runs; anything else raises NotImplementedError naming the option -- before any GPU
    work (no device is touched here)."""
    a = args
    g = lambda k, d=None: a.get(k, d)
    if g('cnn_model') != 'adapt':
        raise NotImplementedError('NISQA_DE on the HIP engine needs cnn_model=adapt, got cnn_model={}'.format(g('cnn_model')))
    if list(g('cnn_pool_1') or []) != [24, 7] or list(g('cnn_pool_2') or []) != [12, 5] or list(g('cnn_pool_3') or []) != [6, 3] \
            or g('cnn_fc_out_h') is not None or (g('cnn_c_out_1'), g('cnn_c_out_2'), g('cnn_c_out_3')) != (16, 32, 64):
        raise NotImplementedError('NISQA_DE on the HIP engine needs the nisqa.tar CNN geometry (cnn_c_out 16/32/64, pools 24x7/12x5/6x3, '
                                  'cnn_fc_out_h null)')
    for td in ('td', 'td_2'):
        if g(td) != 'self_att':
            raise NotImplementedError('NISQA_DE on the HIP engine needs {}=self_att, got {}={}'.format(td, td, g(td)))
        if g(td + '_sa_d_model') != 64 or g(td + '_sa_nhead') != 1 or g(td + '_sa_h') != 64 or not g(td + '_sa_num_layers'):
            raise NotImplementedError('NISQA_DE on the HIP engine needs {0}_sa_d_model=64, {0}_sa_nhead=1, {0}_sa_h=64'.format(td))
        if g(td + '_sa_pos_enc'):
            raise NotImplementedError('NISQA_DE on the HIP engine has no positional encoding ({}_sa_pos_enc)'.format(td))
    if g('pool') != 'att' or not g('pool_att_h'):
        raise NotImplementedError('NISQA_DE on the HIP engine needs pool=att, got pool={}'.format(g('pool')))
    if g('de_align', 'dot') not in DE_ALIGN:
        raise NotImplementedError('NISQA_DE on the HIP engine: de_align={} is not supported (dot, cosine)'.format(g('de_align', 'dot')))
    if g('de_align_apply', 'hard') not in DE_APPLY:
        raise NotImplementedError('NISQA_DE on the HIP engine: de_align_apply={} is not supported (hard, soft)'.format(
            g('de_align_apply', 'hard')))
    if g('de_fuse', 'x/y/-') not in DE_FUSE:
        raise NotImplementedError('NISQA_DE on the HIP engine: de_fuse={} is not supported (x/y/-, +/-, x/y)'.format(g('de_fuse', 'x/y/-')))
    if g('de_fuse_dim') is not None:
        raise NotImplementedError('NISQA_DE on the HIP engine: de_fuse_dim={} (lin_fusion) is not supported'.format(g('de_fuse_dim')))
    if precision == 'bf16x3':
        raise NotImplementedError('NISQA_DE on the HIP engine: precision bf16x3 is not supported (f32, bf16x6, f16x4, f16x3)')


class HipNisqaDE(object):
    """NISQA_DE (double-ended: a degraded clip scored against its reference clip, NISQA_lib.py:406-424) on one MI355X.
    A batch of B pairs is ONE plan of 2B clips: the B degraded clips, then their B reference clips.  mel + AdaptCNN and the first
    self-attention run on all 2B clips with the shared weights; nisqa_de_align_fuse aligns and fuses; the second self-attention
    (time_dependency_2) and the attention pooling run on the B degraded clips."""

    def __init__(self, args, state_dict, device=None, precision=None):
        prec = precision or os.environ.get('NISQA_HIP_PRECISION') or DEFAULT_PRECISION
        check_de_args(args, prec)
        self.args = args
        single = dict(args, model='NISQA', td_2='skip')               # mel, CNN, time_dependency, pool.model: the single-ended engine
        self.base = HipNisqa(single, state_dict, device, prec)
        self.lib, self.device, self.precision = self.base.lib, self.base.device, self.base.precision
        self.n_heads = 1
        self.align = DE_ALIGN[args.get('de_align', 'dot')]
        self.apply = DE_APPLY[args.get('de_align_apply', 'hard')]
        self.fuse = DE_FUSE[args.get('de_fuse', 'x/y/-')]
        self.fuse_width = DE_FUSE_WIDTH[args.get('de_fuse', 'x/y/-')]
        self.n_layers2 = int(args['td_2_sa_num_layers'])
        self._input_grad = None                                       # grad_segments builds its operator chain on first use
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        pfx = 'time_dependency_2.model.'
        self.td2_w = up(_w.pack_self_att(state_dict, self.n_layers2, pfx, in_features=self.fuse_width))
        terms = TD[self.base.td_precision].terms
        self.td2_wb = up(_w.pack_self_att_bf16(state_dict, self.n_layers2, pfx, terms=terms, in_features=self.fuse_width).view(np.int16)) \
            if terms else None

    def _stream(self):
        return self.base._stream()

    # -- plans ------------------------------------------------------------------------------------------
    def plan(self, lengths_deg, lengths_ref, sr, names=None):
        """One plan of 2B clips (degraded, then reference) at one rate."""
        return self.base.plan(list(lengths_deg) + list(lengths_ref), sr, names)

    # -- stages -----------------------------------------------------------------------------------------
    def align_fuse(self, x, plan, want_idx=False):
        """x: [NP, 64] first self-attention output of the plan's 2B clips -> (fused [NP_deg, 384] with the fused features in columns
        0 .. F-1 and zeros behind them, hard-mode indices [NP_deg] int32 or None)."""
        B = plan.n_clips // 2
        assert plan.n_clips == 2 * B and x.shape == (plan.total_tok, 64) and x.dtype == torch.float32
        d = plan.to(self.device)
        np_deg = int(plan.tok_off[B])
        out = torch.zeros((np_deg, DE_FEAT_LD), dtype=torch.float32, device=self.device)
        idx = torch.empty(np_deg, dtype=torch.int32, device=self.device) if want_idx else None
        t, n = d['tok_off'], d['n_wins']
        _lib.check(self.lib.nisqa_de_align_fuse(_ptr(x), _ptr(t), _ptr(n), _ptr(t[B:]), _ptr(n[B:]), B, np_deg, self.align, self.apply,
                                                self.fuse, DE_FEAT_LD, _ptr(out), _ptr(idx) if want_idx else None, self._stream()),
                   'nisqa_de_align_fuse')
        return out, idx

    def td2_pool(self, fused, dplan, want_x=False):
        """time_dependency_2 + pool on the fused features of the degraded clips (dplan: their plan) -> [B, 1]; want_x: and the rows
        the pooling read (HipNisqa.td_pool)"""
        b = self.base
        return b.td_pool(fused, dplan, td_w=self.td2_w, td_wb=self.td2_wb, n_layers=self.n_layers2, pool_w=b.pool_w, pool_wb=b.pool_wb,
                         n_heads=1, want_x=want_x)

    def forward_features(self, feat, plan, want_idx=False):
        """feat [NP, 384]: AdaptCNN output of the plan's 2B clips -> ([B, 1], hard-mode indices or None)"""
        x = self.base.td(feat, plan)                   # materialised: the alignment reads every token of both clips
        fused, idx = self.align_fuse(x, plan, want_idx)
        B = plan.n_clips // 2
        out = self.td2_pool(fused, BatchPlan.from_n_wins(plan.n_wins[:B]))
        return (out, idx) if want_idx else out

    def features(self, pcm, plan, sr):
        mel, floor = self.base.mel(pcm, plan, sr, clamp=False)
        return self.base.cnn(mel, floor, plan)[0]

    def forward_segments(self, x, n_wins):
        """Reference inner operator model(x[B,L,2,48,15], n_wins[B,2]) -> [B, 1] (NL:399-424): channel 0 holds the degraded clip's
        segments, channel 1 the reference clip's (torch.chunk(x, 2, dim=2), NL:399-404).  One plan of 2B clips, degraded first;
        each channel is copied into a contiguous [2B, L, 1, 48, 15] tensor for the segment-fed AdaptCNN (not the throughput path:
        predict never materialises segments)."""
        n = check_segments(x, n_wins, 2)
        x = x.to(self.device, dtype=torch.float32)
        x2 = torch.cat([x[:, :, 0:1], x[:, :, 1:2]], 0).contiguous()
        plan = BatchPlan.from_n_wins(np.concatenate([n[:, 0], n[:, 1]]))
        return self.forward_features(self.base.cnn_segments(x2, plan), plan)

    def grad_segments(self, x, n_wins, grad_out):
        """The backward of forward_segments in precision 'f32' / 'bf16x6' (input_grad.InputGradDE): x [B, L, 2, 48, 15], n_wins
        [B, 2], grad_out [B, 1] -> d (sum grad_out * model(x, n_wins)) / d x, float32 [B, L, 2, 48, 15] on the engine's device --
        the reference's module in eval mode, for hard and soft alignment alike (hard: the argmax carries no gradient); rows
        l >= n_wins[b, c] of channel c are exactly zero.  forward_segments keeps no activation, so this call recomputes the
        network operator by operator with its activations in HBM: it costs a second forward.  In hard mode the recomputation
        takes its own argmax (InputGradDE.last_idx), which at a near-tie of two scores may differ from the fused chain's."""
        return self._grad()(x, n_wins, grad_out)

    def _grad(self):
        from . import input_grad
        input_grad.check_precision(self.precision)
        if self._input_grad is None:
            self._input_grad = input_grad.InputGradDE(self, self.base._state_dict)
        return self._input_grad

    def forward_pcm(self, pcm, plan, sr, want_idx=False):
        """pcm: device tensor of the plan's 2B clips back to back (degraded, then reference; float32 or int16 PCM) -> [B, 1]"""
        assert pcm.is_cuda and pcm.numel() == plan.total_samples
        return self.forward_features(self.features(pcm, plan, sr), plan, want_idx)

    # -- per-segment profile of a score (HipNisqa.profile_pcm) ---------------------------------------------------
    def profile_features(self, feat, plan):
        """forward_features with the score taken apart over the DEGRADED clips' tokens -> PoolProfile in the token layout of
        BatchPlan.from_n_wins(plan.n_wins[:B]): scores forward_features', bit for bit; embed the second self-attention's output;
        aligned_to the hard alignment's reference token per degraded token (what want_idx returns), None with soft alignment."""
        hard = self.apply == DE_APPLY['hard']
        fused, idx = self.align_fuse(self.base.td(feat, plan), plan, want_idx=hard)
        dplan = BatchPlan.from_n_wins(plan.n_wins[:plan.n_clips // 2])
        scores, x = self.td2_pool(fused, dplan, want_x=True)
        return self.base._profile(scores, x, dplan, idx)

    def profile_pcm(self, pcm, plan, sr):
        """forward_pcm with the score taken apart per segment of the degraded clip (profile_features)"""
        assert pcm.is_cuda and pcm.numel() == plan.total_samples
        return self.profile_features(self.features(pcm, plan, sr), plan)

    def profile_audio(self, pcm, lengths_deg, lengths_ref, sr, plan):
        """profile_pcm for 2B clips as the caller holds them (resampled to ms_sr first when the checkpoint sets it; forward_audio)"""
        b = self.base
        return self.profile_pcm(b.resample(pcm, list(lengths_deg) + list(lengths_ref), sr), plan, b.rate(sr))

    def audio_plan(self, lengths_deg, lengths_ref, sr, names=None):
        """plan() of 2B clips of rate ``sr`` as the network sees them (resampled to ms_sr when the checkpoint sets it)."""
        return self.base.audio_plan(list(lengths_deg) + list(lengths_ref), sr, names)

    def forward_audio(self, pcm, lengths_deg, lengths_ref, sr, plan):
        """forward_pcm for 2B clips as the caller holds them, degraded clips first: resampled to ms_sr first when the checkpoint
        asks for that, as forward_items does (``plan`` from audio_plan(lengths_deg, lengths_ref, sr))."""
        b = self.base
        return self.forward_pcm(b.resample(pcm, list(lengths_deg) + list(lengths_ref), sr), plan, b.rate(sr))

    # -- the gradient with respect to both audio signals -------------------------------------------------------
    def grad_audio(self, pcm, plan, sr, grad_out, need=(True, True)):
        """The backward of forward_pcm in precision 'f32' / 'bf16x6': pcm float32 [plan.total_samples], the plan's 2B clips back to
        back (degraded, then reference) at the rate ``sr`` the spectrogram is computed at, grad_out [B, 1]
        -> (d_deg, d_ref) = d (sum grad_out * forward_pcm(pcm, plan, sr)) / d pcm split at the first reference sample: float32
        [sum lengths_deg] and [sum lengths_ref]; None for a side that ``need`` = (degraded, reference) does not name.
        The 2B-clip layout is kept end to end: base.mel (unclamped rows + floors), the clamped segment tensor cut on the device
        (nisqa_mel_segments_fwd), InputGradDE.packed -- no channel split, no concatenation --, the segment adjoint and the mel
        backward.  The degraded clips are a prefix of pcm, of the dB rows, of the floors and of d / d mel, the reference clips
        the suffix: with one side named, the CNN backward, the segment adjoint and the mel backward run on that side's view
        under its own plan.  Hard alignment: the argmax carries no gradient, and the backward takes the recomputation's own
        argmax (InputGradDE.last_idx), which at a near-tie of two scores may differ from the choice of the fused inference chain
        that produced the score (DESIGN.md 4.8 "argmax deviation")."""
        return self._audio_bwd(pcm, plan, sr, grad_out, need, None)

    def _deg_cotangents(self, n_deg, d_weights, d_local, d_embed):
        """HipNisqa.profile_cotangents over the degraded clips' tokens (the layout of BatchPlan.from_n_wins(n_deg))"""
        return self.base.profile_cotangents(BatchPlan.from_n_wins(n_deg), d_weights, d_local, d_embed)

    def grad_profile_segments(self, x, n_wins, d_scores=None, d_weights=None, d_local=None, d_embed=None):
        """HipNisqa.grad_profile_segments for x [B, L, 2, 48, 15], n_wins [B, 2]: d_scores [B, 1]; d_weights, d_local [NP, 1] and
        d_embed [NP, 64] over the DEGRADED clips' tokens, in the layout of BatchPlan.from_n_wins(n_wins[:, 0]) -> d / d x, float32
        in x's shape (both channels: the reference clip's segments reach the profile through the alignment)."""
        n = check_segments(x, n_wins, 2)
        return self._grad()(x, n_wins, d_scores, profile_cot=self._deg_cotangents(n[:, 0], d_weights, d_local, d_embed))

    def grad_profile_audio(self, pcm, plan, sr, d_scores=None, d_weights=None, d_local=None, d_embed=None, need=(True, True)):
        """The backward of profile_pcm, built as grad_audio is: the cotangents of grad_profile_segments over the degraded clips'
        tokens -> (d_deg, d_ref) as grad_audio returns them, None for a side ``need`` does not name."""
        self._grad()                                                         # the precision is refused before anything is copied
        cot = self._deg_cotangents(plan.n_wins[:plan.n_clips // 2], d_weights, d_local, d_embed)
        return self._audio_bwd(pcm, plan, sr, d_scores, need, cot)

    def _audio_bwd(self, pcm, plan, sr, grad_out, need, cot):
        """grad_audio's chain; cot: token-level cotangents for InputGradDE.packed (beside them grad_out may be None)"""
        ig = self._grad()
        need = (bool(need[0]), bool(need[1]))
        B, b = plan.n_clips // 2, self.base
        assert plan.n_clips == 2 * B and any(need) and pcm.dtype == torch.float32, 'int16 PCM has no gradient'
        from .input_grad import _grad_out
        g = _grad_out(grad_out, B, 1, self.device, cot)
        pcm = pcm.detach().contiguous()
        mel_db, floor = b.mel(pcm, plan, sr, clamp=False)
        x2 = b.segments_from_mel_db(mel_db, floor, plan)
        n = np.stack([plan.n_wins[:B], plan.n_wins[B:]], 1).astype(np.int64)
        dx2 = ig.packed(x2, n, g, need, cot)
        del x2
        if all(need):
            d = b.mel_bwd(pcm, plan, sr, b.segments_to_mel_bwd(dx2, plan), mel_db, floor)
            return d[:int(plan.clip_off[B])], d[int(plan.clip_off[B]):]
        side = 0 if need[0] else 1
        sub = self._side_plan(plan, sr, side)
        c, s, f = slice(side * B, side * B + B), int(plan.clip_off[B]), int(plan.frame_off[B])
        rows, smp = (slice(0, f), slice(0, s)) if side == 0 else (slice(f, None), slice(s, None))
        d = b.mel_bwd(pcm[smp], sub, sr, b.segments_to_mel_bwd(dx2[c], sub), mel_db[rows], floor[c].contiguous())
        return (d, None) if side == 0 else (None, d)

    def _side_plan(self, plan, sr, side):
        """The plan of the B degraded (side 0) or reference (side 1) clips of a 2B-clip plan, built once per plan."""
        subs = plan.__dict__.setdefault('_de_sides', {})
        if side not in subs:
            B = plan.n_clips // 2
            subs[side] = self.base.plan(plan.lengths[side * B:side * B + B], sr)
        return subs[side]

    def forward_items(self, items, names=None):
        """items: 2B host clips (samples int16 / float32, sr) -- the degraded clips, then the reference clips -> [B, 1] on the device.
        Clips of one (rate, sample type) share one mel + CNN launch; with several such groups the CNN rows are gathered into the
        2B-clip layout (a copy) before the self-attention."""
        names = names if names is not None else [None] * len(items)
        groups = {}
        for c, (y, sr) in enumerate(items):
            groups.setdefault((int(sr), y.dtype == np.int16), []).append(c)
        b = self.base
        n_wins = np.zeros(len(items), np.int64)
        parts = []
        for (sr, _), cs in groups.items():
            lengths = [len(items[c][0]) for c in cs]
            gplan = b.audio_plan(lengths, sr, [names[c] for c in cs])
            pcm = torch.from_numpy(np.concatenate([items[c][0] for c in cs])).to(self.device)
            pcm = b.resample(pcm, lengths, sr)
            parts.append((cs, gplan, self.features(pcm, gplan, b.rate(sr))))
            n_wins[cs] = gplan.n_wins
        plan = BatchPlan.from_n_wins(n_wins)
        if len(parts) == 1 and parts[0][0] == list(range(len(items))):
            feat = parts[0][2]
        else:
            src, base_row = np.zeros(plan.total_tok, np.int64), 0
            for cs, gplan, f in parts:
                for k, c in enumerate(cs):
                    rows = int(plan.tok_off[c + 1] - plan.tok_off[c])
                    src[plan.tok_off[c]:plan.tok_off[c] + rows] = base_row + gplan.tok_off[k] + np.arange(rows)
                base_row += gplan.total_tok
            feat = torch.cat([f for _, _, f in parts])[torch.from_numpy(src).to(self.device)]
        return self.forward_features(feat, plan)
