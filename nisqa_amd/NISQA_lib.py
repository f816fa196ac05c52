"""Host-side mirror of the reference's hot-path interface in nisqa/NISQA_lib.py: same names,
argument meaning and error behaviour, with the arithmetic moved to the HIP engine.

  SpeechQualityDataset  (reference NL:2052-2236)  file table + ms_* parameters; items are read here,
                                                   spectrograms are computed on the GPU
  predict_mos / predict_dim (NL:1420-1467)        batching loop: WAV ingest -> device -> HIP forward
  NISQA / NISQA_DIM     (NL:29-268)                parameter containers with the reference's
                                                   state_dict keys; forward() runs the HIP path
  NISQA_DE              (NL:272-424)               the same for the double-ended model

Evaluation statistics (eval_results and helpers, NL:1469-1852) are re-exported from nisqa_amd/evaluation.py.
Training runs through nisqa_amd/trainloop.py (CNN-SA-AP: nisqa_amd/train.py; StandardCNN + BiLSTM with pool last_step_bi / avg /
max: nisqa_amd/train_lstm.py; NISQA_DE: nisqa_amd/train_de.py).  Out of scope here (raise NotImplementedError): alternative blocks
no shipped checkpoint uses.
"""
import os
import sys
import time
from contextlib import nullcontext as _nullcontext

import numpy as np
import pandas as pd; pd.options.mode.chained_assignment = None
import torch
import torch.nn as nn

from . import dist as _dist
from .evaluation import (calc_eval_metrics, calc_mapped, calc_mapping, calc_rmse, calc_rmse_star, eval_results,  # noqa: F401
                         fit_first_order, fit_monotonic_third_order, fit_second_order, fit_third_order, is_const)
from . import ingest as _ingest
from . import lib as _lib_mod
from .wavio import read_wav


# ---------------------------------------------------------------------------------------------
# Parameter containers: identical module tree / state_dict keys as the reference so that
# nisqa.tar loads with load_state_dict(strict=True) (NISQA_model.py:1023).
# ---------------------------------------------------------------------------------------------
class _Params(nn.Module):
    """Leaf holding named tensors (weights as Parameters, running stats as buffers)."""

    def __init__(self, shapes, buffers=()):
        super().__init__()
        for name, shape in shapes.items():
            self.register_parameter(name, nn.Parameter(torch.zeros(shape), requires_grad=False))
        for name, shape, dtype in buffers:
            self.register_buffer(name, torch.zeros(shape, dtype=dtype))


def _conv(cout, cin, kh, kw):
    return _Params({'weight': (cout, cin, kh, kw), 'bias': (cout,)})


def _bn(c):
    return _Params({'weight': (c,), 'bias': (c,)},
                   [('running_mean', (c,), torch.float32), ('running_var', (c,), torch.float32),
                    ('num_batches_tracked', (), torch.int64)])


def _lin(cout, cin):
    return _Params({'weight': (cout, cin), 'bias': (cout,)})


class _AdaptCNNParams(nn.Module):
    def __init__(self, c1, c2, c3, kernel_size, pool_3):
        super().__init__()
        kh, kw = (kernel_size, kernel_size) if isinstance(kernel_size, int) else tuple(kernel_size)
        chans = [1, c1, c2, c3, c3, c3, c3]
        for i in range(1, 7):
            k_w = pool_3[1] if i == 6 else kw                       # NL:625, NL:672-676
            setattr(self, 'conv%d' % i, _conv(chans[i], chans[i - 1], kh, k_w))
            setattr(self, 'bn%d' % i, _bn(chans[i]))
        self.fan_out = c3 * pool_3[0]


class _SALayerParams(nn.Module):
    def __init__(self, d, h):
        super().__init__()
        self.self_attn = nn.Module()
        self.self_attn.register_parameter('in_proj_weight', nn.Parameter(torch.zeros(3 * d, d), requires_grad=False))
        self.self_attn.register_parameter('in_proj_bias', nn.Parameter(torch.zeros(3 * d), requires_grad=False))
        self.self_attn.out_proj = _lin(d, d)
        self.linear1 = _lin(h, d)
        self.linear2 = _lin(d, h)
        self.norm1 = _Params({'weight': (d,), 'bias': (d,)})
        self.norm2 = _Params({'weight': (d,), 'bias': (d,)})


class _SelfAttentionParams(nn.Module):
    def __init__(self, input_size, d, layers, h):
        super().__init__()
        self.norm1 = _Params({'weight': (d,), 'bias': (d,)})
        self.linear = _lin(d, input_size)
        self.layers = nn.ModuleList([_SALayerParams(d, h) for _ in range(layers)])


class _PoolAttFFParams(nn.Module):
    def __init__(self, d, h):
        super().__init__()
        self.linear1 = _lin(h, d)
        self.linear2 = _lin(1, h)
        self.linear3 = _lin(1, d)


class _StandardCNNParams(nn.Module):
    def __init__(self, c1, c2, c3, fc_out_h):
        super().__init__()
        chans = [1, c1, c2, c3, c3, c3, c3]
        for i in range(1, 7):
            setattr(self, 'conv%d' % i, _conv(chans[i], chans[i - 1], 3, 3))
            setattr(self, 'bn%d' % i, _bn(chans[i]))
        self.fc_out = _lin(fc_out_h, c3 * 6 * 2)                   # NL:803-807
        self.fan_out = fc_out_h


class _LSTMParams(nn.Module):
    def __init__(self, input_size, lstm_h):
        super().__init__()
        # parameter holder with nn.LSTM's own key names (weight_ih_l0, ..., *_reverse); never called
        self.lstm = nn.LSTM(input_size=input_size, hidden_size=lstm_h, num_layers=1, batch_first=True, bidirectional=True)
        for p_ in self.lstm.parameters():
            p_.requires_grad_(False)


class _PoolLastStepBiParams(nn.Module):            # the [256] -> 1 linear layer of PoolLastStepBi, PoolAvg and PoolMax alike
    def __init__(self, d):
        super().__init__()
        self.linear = _lin(1, d)


class _Wrap(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model


class _NisqaBase(nn.Module):
    """Shared by NISQA and NISQA_DIM: builds the parameter tree, owns the (lazy) HIP engine."""

    def __init__(self, n_heads, **kw):
        super().__init__()
        g = lambda k, d=None: kw.get(k, d)
        self._hp = dict(kw)
        self._engine = None
        self._engine_args = None
        if g('cnn_model') == 'standard' and g('td') == 'lstm' and n_heads == 1:
            # nisqa_tts.tar (pool=last_step_bi) and the CNN-LSTM-AVG recipe (pool=avg / max): one parameter tree, the pooling's
            # linear layer is pool.model.linear in all three (NL:712-836, NL:897-943, NL:1099-1115, NL:1185-1224)
            from .engine import check_lstm_args
            check_lstm_args(kw, n_heads)
            self.cnn = _Wrap(_StandardCNNParams(g('cnn_c_out_1', 16), g('cnn_c_out_2', 32), g('cnn_c_out_3', 64),
                                                g('cnn_fc_out_h', 20)))
            self.time_dependency = _Wrap(_LSTMParams(self.cnn.model.fan_out, g('td_lstm_h', 128)))
            self.pool = _Wrap(_PoolLastStepBiParams(2 * g('td_lstm_h', 128)))
            return
        if g('cnn_model', 'adapt') != 'adapt' or g('td', 'self_att') != 'self_att' or g('pool', 'att') != 'att' \
                or g('td_2', 'skip') not in (None, 'skip') or not g('pool_att_h', 128):
            raise NotImplementedError(
                'nisqa_amd accelerates the CNN-SA-AP path (cnn_model=adapt, td=self_att, td_2=skip, pool=att with '
                'pool_att_h) and the StandardCNN + BiLSTM path of nisqa_tts and the CNN-LSTM-AVG recipe (cnn_model=standard, '
                'td=lstm, pool=last_step_bi, avg or max); got '
                'cnn_model={} td={} td_2={} pool={}'.format(g('cnn_model'), g('td'), g('td_2'), g('pool')))
        self.cnn = _Wrap(_AdaptCNNParams(g('cnn_c_out_1', 16), g('cnn_c_out_2', 32), g('cnn_c_out_3', 64),
                                         g('cnn_kernel_size', 3), g('cnn_pool_3', [6, 3])))
        d = g('td_sa_d_model', 64)
        self.time_dependency = _Wrap(_SelfAttentionParams(self.cnn.model.fan_out, d, g('td_sa_num_layers', 2),
                                                          g('td_sa_h', 64)))
        if n_heads == 5:
            self.pool_layers = nn.ModuleList([_Wrap(_PoolAttFFParams(d, g('pool_att_h', 128))) for _ in range(5)])
        else:
            self.pool = _Wrap(_PoolAttFFParams(d, g('pool_att_h', 128)))

    def bind_args(self, args):
        """Give the module the checkpoint's args (ms_* front-end parameters live there, NISQA_model.py:941-942)."""
        self._engine_args = args
        self._engine = None
        return self

    def engine(self, device=None):
        if self._engine is None:
            from .engine import HipNisqa
            if self._engine_args is None:
                raise RuntimeError('bind_args(checkpoint_args) must be called before the HIP engine is built')
            self._engine = HipNisqa(self._engine_args, self.state_dict(), device)
        return self._engine

    def forward(self, x, n_wins):
        """Reference inner operator model(x[B,L,1,48,15], n_wins[B]) -> [B, heads] (NL:137-142, NL:260-268).
        When gradients are enabled and x requires one, the result carries a grad_fn and backward delivers d / d x as the
        reference's module does in eval mode (engine.HipNisqa.grad_segments; precisions 'f32' and 'bf16x6', any other raises
        NotImplementedError here), for the CNN-SA-AP and the StandardCNN + BiLSTM models alike.  The values are those of the plain
        call, bit for bit; there is no double backward, and the parameters get no gradient."""
        from .engine import DEFAULT_PRECISION, check_segments
        n = check_segments(x, n_wins, 1)                           # malformed arguments raise before the engine is built
        dev = x.device if x.is_cuda else None
        if not (torch.is_grad_enabled() and x.requires_grad):
            return self.engine(dev).forward_segments(x, n_wins)
        from .input_grad import check_precision
        check_precision(self._engine.precision if self._engine is not None
                        else os.environ.get('NISQA_HIP_PRECISION') or DEFAULT_PRECISION)        # refused before any GPU work
        eng = self.engine(dev)
        # the Function sees the tensor the kernels read: torch supplies the adjoint of the device / dtype conversion
        return _SegmentsFunction.apply(x.to(eng.device, dtype=torch.float32).contiguous(), eng, n)

    def forward_audio(self, y, sr, lengths=None):
        """Scores of in-memory audio: y a floating tensor on any device, [N] for one clip or [B, N] for a padded batch of clips at
        one integer rate ``sr``, lengths [B] whole numbers in [1, N] (default: N for every clip) -> [B, heads] on the engine's
        device.  Samples at n >= lengths[b] are never read.  The clips are packed back to back and go through the engine's
        forward_pcm (through its resampler first when the checkpoint sets ms_sr): the result is forward_pcm's, bit for bit, in
        every engine precision.
        When gradients are enabled and y requires one, the result carries a grad_fn and backward delivers d / d y in y's shape,
        dtype and device, exact zeros at n >= lengths[b] whatever y holds there (engine.HipNisqa.grad_audio: the backward of the
        mel front end and of the segmenting behind grad_segments; precisions 'f32' and 'bf16x6').  The values are the plain
        call's, bit for bit; there is no double backward and the parameters get no gradient.
        Refused before any GPU work: a y that is not floating or not of rank 1 or 2, an empty batch, lengths out of range
        (ValueError); a clip too short for one segment or with more than ms_max_segments segments (engine.BatchPlan's
        ValueErrors); a gradient in a fast precision, or while the checkpoint's ms_sr differs from sr -- the resampler has no
        backward -- (NotImplementedError; the plain call still works)."""
        y2, n, sr, plan = self._audio_plan(y, sr, lengths)
        dev = y.device if y.is_cuda else None
        if not (torch.is_grad_enabled() and y.requires_grad):
            eng = self.engine(dev)
            return _score_audio(eng, y2.detach().to(eng.device, dtype=torch.float32), n, sr, plan)
        _check_audio_grad(self, sr)
        eng = self.engine(dev)
        # the Function sees the samples the kernels read: torch supplies the adjoint of the device / dtype / rank conversion
        return _AudioFunction.apply(y2.to(eng.device, dtype=torch.float32), eng, n, sr, plan)

    def profile_audio(self, y, sr, lengths=None, differentiable=False):
        """forward_audio with every score taken apart per segment: the same arguments, the same checks and the same refusals
        (forward_audio's, raised before any GPU work) -> SegmentProfile (see there) with
          scores [B, heads]           forward_audio's, bit for bit, in every engine precision;
          weights, local [B, Lmax, heads]   the share a_l of segment l in the score and what the segment says on its own, in MOS
                                      units: score = sum_l weights * local up to float32 rounding (PoolAttFF: the attention
                                      weights and w3 . x_l + b3; PoolAvg: 1 / n_wins and w . h_l + b);
          embed [B, Lmax, D]          the rows the pooling read (D = 64 behind self-attention, 256 behind the BiLSTM);
          n_wins [B], t_start / t_end [Lmax]   the segment counts and each segment's span in seconds.
        Rows l >= n_wins[b] are exact zeros.  pool=last_step_bi and pool=max have no such decomposition: NotImplementedError naming
        the pool, before any GPU work.  Not a throughput path.
        By default the result is detached, whatever y requires.  With ``differentiable=True``, gradients enabled and a y that
        requires one, scores, weights, local and embed are the four outputs of ONE autograd function (values: the plain call's,
        bit for bit) and backward delivers d / d y of whatever was built on them -- min_l local, a distance between embeddings -- in
        y's shape, dtype and device, exact zeros at n >= lengths[b]: the four cotangents (None: zero; rows l >= n_wins[b] are
        ignored whatever they hold) go through ONE recomputation and ONE backward chain (engine.HipNisqa.grad_profile_audio;
        DESIGN.md 4.10).  No double backward, no gradient for the parameters.  Refused before any GPU work, as forward_audio
        refuses a gradient: a fast precision, an ms_sr that differs from sr; and the StandardCNN + BiLSTM family with pool=avg,
        whose backward through time takes no per-step gradient (NotImplementedError; its plain profile works).  With nothing to
        differentiate, differentiable=True is the plain call."""
        from .engine import check_profile_args, check_profile_grad_args
        y2, n, sr, plan = self._audio_plan(y, sr, lengths)
        check_profile_args(self._engine_args)
        dev = y.device if y.is_cuda else None
        if not (differentiable and torch.is_grad_enabled() and y.requires_grad):
            eng = self.engine(dev)
            with torch.no_grad():
                prof = eng.profile_audio(_pack_clips(y2.detach().to(eng.device, dtype=torch.float32), n), n, sr, plan)
            return _segment_profile(prof, plan.n_wins, self._engine_args)
        check_profile_grad_args(self._engine_args)
        _check_audio_grad(self, sr)
        eng = self.engine(dev)
        # the Function sees the samples the kernels read: torch supplies the adjoint of the device / dtype / rank conversion
        return _differentiable_profile(eng, (y2.to(eng.device, dtype=torch.float32),), (n,), sr, plan, self._engine_args)

    def _audio_plan(self, y, sr, lengths):
        """The argument checks of forward_audio and the plan it builds, on the host -> (y as [B, N], lengths, sr, plan)"""
        from .engine import BatchPlan
        from .melbank import resampled_lengths
        y2, n = _audio_args(y, lengths)
        if int(sr) != sr or int(sr) < 1:
            raise ValueError('sr must be one positive integer rate for the batch, got {}'.format(sr))
        sr, args = int(sr), self._engine_args
        if args is None:
            raise RuntimeError('bind_args(checkpoint_args) must be called before the HIP engine is built')
        rate = sr if args.get('ms_sr') is None else int(args['ms_sr'])
        # the engine's audio_plan(n, sr), on the host: too short a clip and too many segments raise here
        plan = BatchPlan(n if rate == sr else resampled_lengths(n, sr, rate)[0], int(rate * args['ms_hop_length']),
                         int(args['ms_seg_hop_length']), args['ms_max_segments'])
        return y2, n, sr, plan


class SegmentProfile(object):
    """What profile_audio returns.  scores [B, heads], weights / local [B, Lmax, heads], embed [B, Lmax, D] and (NISQA_DE)
    aligned_to [B, Lmax] are tensors on the engine's device, Lmax the largest segment count of the batch; n_wins [B]
    (int64) and t_start / t_end [Lmax] (float64, seconds) are host tensors.  heads: the names of the head axis, in order.
    The tensors are detached unless profile_audio(..., differentiable=True) had something to differentiate: then scores, weights,
    local and embed (never aligned_to) share one grad_fn, and a loss built on any of them -- the worst segment's local score,
    res.local[..., 0].masked_fill(pad, inf).amin(1), or the distance between two clips' embed -- backpropagates to the samples.
    Rows l >= n_wins[b] take no part: whatever cotangent reaches them is dropped."""
    __slots__ = ('scores', 'weights', 'local', 'embed', 'n_wins', 't_start', 't_end', 'aligned_to', 'heads')

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def __repr__(self):
        return 'SegmentProfile(B={}, Lmax={}, heads={})'.format(self.scores.shape[0], self.weights.shape[1], list(self.heads))


HEAD_NAMES = {1: ('mos',), 5: ('mos', 'noi', 'dis', 'col', 'loud')}          # the head axis of NISQA / NISQA_DE and of NISQA_DIM


def segment_times(args, n_segments):
    """(t_start, t_end) of segments 0 .. n_segments - 1 in seconds, float64: segment l covers the ms_seg_length frames from frame
    l * ms_seg_hop_length on, a frame being ms_hop_length seconds (NL:2266-2280)."""
    first = np.arange(int(n_segments), dtype=np.float64) * int(args['ms_seg_hop_length'])
    hop = float(args['ms_hop_length'])
    return first * hop, (first + int(args['ms_seg_length'])) * hop


def _segment_profile(prof, n_wins, args):
    """engine.PoolProfile in the plan's token layout (n_wins: the counts of the clips it covers) -> SegmentProfile [B, Lmax, ...]"""
    from .engine import BatchPlan
    n = np.asarray(n_wins, np.int64)
    tok_off, L = BatchPlan.from_n_wins(n).tok_off, int(n.max())
    valid = np.arange(L)[None, :] < n[:, None]
    dev = prof.scores.device
    rows = torch.from_numpy(np.where(valid, tok_off[:-1, None].astype(np.int64) + np.arange(L)[None, :], 0)).to(dev)
    pad = ~torch.from_numpy(valid).to(dev)
    cut = lambda t: t.detach()[rows].masked_fill(pad[..., None], 0.0)
    t0, t1 = segment_times(args, L)
    aligned = None
    if args.get('model') == 'NISQA_DE':                            # hard alignment: the engine's indices; soft: -1 everywhere
        aligned = torch.full((len(n), L), -1, dtype=torch.int64, device=dev) if prof.aligned_to is None else \
            prof.aligned_to.detach().to(torch.int64)[rows].masked_fill(pad, -1)
    return SegmentProfile(scores=prof.scores.detach(), weights=cut(prof.weights), local=cut(prof.local), embed=cut(prof.embed),
                          n_wins=torch.from_numpy(n.copy()), t_start=torch.from_numpy(t0), t_end=torch.from_numpy(t1),
                          aligned_to=aligned, heads=HEAD_NAMES[prof.scores.shape[1]])


def _audio_args(y, lengths, name='y', size='N'):
    """The checks of forward_audio on one batch of clips: y [N] or [B, N] floating, lengths [B] whole numbers in [1, N] or None
    -> (y as [B, N], the lengths as int64 [B]).  Raises ValueError; no device is touched beyond reading lengths."""
    if not torch.is_tensor(y) or not y.is_floating_point() or y.dim() not in (1, 2):
        raise ValueError('expected {} as a floating tensor of shape [{}] or [B, {}], got {}'.format(
            name, size, size, '{} {}'.format(y.dtype, tuple(y.shape)) if torch.is_tensor(y) else type(y).__name__))
    y2 = y if y.dim() == 2 else y.unsqueeze(0)
    B, N = y2.shape
    if B == 0 or N == 0:
        raise ValueError('empty batch')
    if lengths is None:
        return y2, np.full(B, N, dtype=np.int64)
    n = np.asarray(lengths.detach().cpu().numpy() if torch.is_tensor(lengths) else lengths).reshape(-1)
    if n.size != B or not (np.issubdtype(n.dtype, np.integer) or (np.isfinite(n).all() and (n == np.floor(n)).all())):
        raise ValueError('lengths must hold one whole number in [1, {}] per clip'.format(size))
    n = n.astype(np.int64)
    if (n < 1).any() or (n > N).any():
        raise ValueError('lengths must hold one whole number in [1, {}] per clip'.format(size))
    return y2, n


def _pack_clips(y, lengths):
    """y [B, N] on the device, lengths [B] -> the clips back to back [sum lengths] (no sample at n >= lengths[b] is read)"""
    if (lengths == y.shape[1]).all():
        return y.contiguous().reshape(-1)
    return torch.cat([y[b, :int(n)] for b, n in enumerate(lengths)])


def _unpack_clips(d, y, lengths):
    """The adjoint of _pack_clips: d [sum lengths] -> [B, N] in y's shape, exact zeros at n >= lengths[b] whatever y holds there"""
    if (lengths == y.shape[1]).all():
        return d.view_as(y)
    dy, o = torch.zeros_like(y), 0
    for b, n in enumerate(lengths):
        dy[b, :int(n)] = d[o:o + int(n)]
        o += int(n)
    return dy


def _score_audio(eng, y, lengths, sr, plan):
    return eng.forward_audio(_pack_clips(y, lengths), lengths, sr, plan)


class _AudioFunction(torch.autograd.Function):
    """HipNisqa.forward_audio on the packed clips with grad_audio as the backward.  The forward is the inference path untouched; only
    y and the lengths are kept, and the backward recomputes what it needs (the dB rows and the network)."""

    @staticmethod
    def forward(ctx, y, eng, lengths, sr, plan):
        ctx.eng, ctx.lengths, ctx.sr = eng, lengths, sr
        ctx.save_for_backward(y)
        return _score_audio(eng, y, lengths, sr, plan)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        y, = ctx.saved_tensors
        eng, lengths, sr = ctx.eng, ctx.lengths, ctx.sr
        d = eng.grad_audio(_pack_clips(y, lengths), eng.plan(lengths, sr), sr, grad_out)
        return _unpack_clips(d, y, lengths), None, None, None, None


class _AudioFunctionDE(torch.autograd.Function):
    """HipNisqaDE.forward_audio on the 2B packed clips (degraded, then reference) with its grad_audio as the backward.  The forward
    is the inference path untouched; only the two sample tensors are kept (the lengths and the plan, host metadata, ride on
    ctx), and the backward recomputes what it needs.  A side that needs no gradient gets None, and its mel backward is not run."""

    @staticmethod
    def forward(ctx, y_deg, y_ref, eng, n_deg, n_ref, sr, plan):
        ctx.eng, ctx.n_deg, ctx.n_ref, ctx.sr, ctx.plan = eng, n_deg, n_ref, sr, plan
        ctx.save_for_backward(y_deg, y_ref)
        return _score_audio_de(eng, y_deg, y_ref, n_deg, n_ref, sr, plan)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        y_deg, y_ref = ctx.saved_tensors
        pcm = torch.cat([_pack_clips(y_deg, ctx.n_deg), _pack_clips(y_ref, ctx.n_ref)])
        d = ctx.eng.grad_audio(pcm, ctx.plan, ctx.sr, grad_out, ctx.needs_input_grad[:2])
        return tuple(_unpack_clips(dk, y, n) if dk is not None else None
                     for dk, y, n in zip(d, (y_deg, y_ref), (ctx.n_deg, ctx.n_ref))) + (None,) * 5


def _score_audio_de(eng, y_deg, y_ref, n_deg, n_ref, sr, plan):
    return eng.forward_audio(torch.cat([_pack_clips(y_deg, n_deg), _pack_clips(y_ref, n_ref)]), n_deg, n_ref, sr, plan)


def _check_audio_grad(model, sr):
    """What forward_audio and profile_audio refuse when a gradient with respect to the audio is asked for, before any GPU work: an
    engine precision without a gradient (that of the engine, or the one it would be built with) and a checkpoint that resamples."""
    from .engine import DEFAULT_PRECISION
    from .input_grad import check_precision
    check_precision(model._engine.precision if model._engine is not None
                    else os.environ.get('NISQA_HIP_PRECISION') or DEFAULT_PRECISION)
    ms_sr = model._engine_args.get('ms_sr')
    if ms_sr is not None and int(ms_sr) != sr:
        raise NotImplementedError('the gradient with respect to the audio needs sr == ms_sr ({} != {}): the resampler has no '
                                  'backward; the plain call works'.format(sr, int(ms_sr)))


class _ProfileFunction(torch.autograd.Function):
    """An engine's profile_audio (HipNisqa: one sample tensor; HipNisqaDE: the degraded and the reference one) with its
    grad_profile_audio as the backward.  The forward is profile_audio's untouched; its SegmentProfile is handed out through ``box``
    and its scores, weights, local and embed are the outputs.  Only the samples are kept: the backward scatters the four cotangents
    into the token layout (rows l >= n_wins[b] are dropped, None stays None) and runs ONE recomputation and ONE chain for them."""

    @staticmethod
    def forward(ctx, eng, lengths, sr, plan, args, box, *ys):
        ctx.eng, ctx.lengths, ctx.sr, ctx.plan = eng, lengths, sr, plan
        ctx.save_for_backward(*ys)
        ctx.set_materialize_grads(False)
        prof = eng.profile_audio(torch.cat([_pack_clips(y, n) for y, n in zip(ys, lengths)]), *lengths, sr, plan)
        sp = _segment_profile(prof, plan.n_wins[:len(lengths[0])], args)
        box.append(sp)
        return sp.scores, sp.weights, sp.local, sp.embed

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_scores, *d_tokens):
        ys, lengths, plan = ctx.saved_tensors, ctx.lengths, ctx.plan
        if d_scores is None and all(d is None for d in d_tokens):
            return (None,) * (6 + len(ys))
        tok = _to_token_layout(d_tokens, plan.n_wins[:len(lengths[0])])
        pcm = torch.cat([_pack_clips(y, n) for y, n in zip(ys, lengths)])
        if len(ys) == 1:
            ds = (ctx.eng.grad_profile_audio(pcm, plan, ctx.sr, d_scores, *tok),)
        else:
            ds = ctx.eng.grad_profile_audio(pcm, plan, ctx.sr, d_scores, *tok, need=ctx.needs_input_grad[6:])
        return (None,) * 6 + tuple(_unpack_clips(d, y, n) if d is not None else None for d, y, n in zip(ds, ys, lengths))


def _to_token_layout(ds, n_wins):
    """The adjoint of _segment_profile's cut: tensors [B, Lmax, w] (or None) -> [NP, w] in the token layout of clips of n_wins[b]
    segments; rows l >= n_wins[b] are dropped whatever they hold, padding rows of the result are zeros.  The indices come from the
    host: nothing here waits for the device."""
    from .engine import BatchPlan
    n = np.asarray(n_wins, np.int64)
    plan = BatchPlan.from_n_wins(n)
    valid = np.flatnonzero(np.arange(int(n.max()))[None, :] < n[:, None])                  # into the flattened [B * Lmax]
    out, idx = [], None
    for d in ds:
        if d is not None:
            idx = idx or [torch.from_numpy(a.astype(np.int64)).to(d.device) for a in (valid, plan.token_index())]
            d = d.new_zeros((plan.total_tok, d.shape[-1])).index_copy_(0, idx[1], d.reshape(-1, d.shape[-1]).index_select(0, idx[0]))
        out.append(d)
    return out


def _differentiable_profile(eng, ys, lengths, sr, plan, args):
    """_ProfileFunction on the sample tensors ys (on the engine's device, float32) -> the SegmentProfile of the plain call whose
    scores, weights, local and embed carry the function's grad_fn"""
    box = []
    out = _ProfileFunction.apply(eng, lengths, sr, plan, args, box, *ys)
    sp, = box
    sp.scores, sp.weights, sp.local, sp.embed = out
    return sp


class _SegmentsFunction(torch.autograd.Function):
    """An engine's forward_segments (HipNisqa, HipNisqaDE) with its grad_segments as the backward.  The forward is the inference path untouched;
    only x and n_wins are kept, and the backward recomputes what it needs (it costs a second forward)."""

    @staticmethod
    def forward(ctx, x, eng, n_wins):
        ctx.eng, ctx.n_wins = eng, n_wins
        ctx.save_for_backward(x)
        return eng.forward_segments(x, n_wins)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, = ctx.saved_tensors
        return ctx.eng.grad_segments(x, ctx.n_wins, grad_out), None, None


def init_parameters_(model):
    """Random initialisation with the distributions the reference's modules get from PyTorch (for training from
    scratch, pretrained_model: false): Conv2d / Linear kaiming-uniform(a=sqrt 5) weights and U(+-1/sqrt(fan_in)) biases,
    BatchNorm / LayerNorm at identity with fresh running statistics, nn.MultiheadAttention's xavier-uniform in_proj and
    zero attention biases, and SelfAttention._reset_parameters (NL:981-984): xavier-uniform on every matrix of the
    time-dependency block."""
    import math
    for name, mod in model.named_modules():
        if not isinstance(mod, _Params):
            continue
        names = dict(mod.named_parameters(recurse=False))
        bufs = dict(mod.named_buffers(recurse=False))
        w = names.get('weight')
        if 'running_mean' in bufs or (w is not None and w.dim() == 1):         # BatchNorm / LayerNorm
            nn.init.ones_(w)
            nn.init.zeros_(names['bias'])
            if 'running_mean' in bufs:
                bufs['running_mean'].zero_()
                bufs['running_var'].fill_(1.0)
                bufs['num_batches_tracked'].zero_()
        elif w is not None:                                                      # Conv2d / Linear
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))
            fan_in = w[0].numel()
            nn.init.uniform_(names['bias'], -1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in))
    td = getattr(model, 'time_dependency', None)
    if td is not None and isinstance(td.model, _SelfAttentionParams):
        for layer in td.model.layers:
            nn.init.zeros_(layer.self_attn.in_proj_bias)
            nn.init.zeros_(layer.self_attn.out_proj.bias)
        for p_ in td.model.parameters():
            if p_.dim() > 1:
                nn.init.xavier_uniform_(p_)
    return model


class NISQA(_NisqaBase):
    def __init__(self, **kw):
        super().__init__(1, **kw)
        self.name = 'NISQA'


class NISQA_DIM(_NisqaBase):
    def __init__(self, **kw):
        super().__init__(5, **kw)
        self.name = 'NISQA_DIM'


class NISQA_DE(nn.Module):
    """Parameter container of the double-ended model (NL:272-424) with the reference's state_dict keys: cnn.*, time_dependency.*,
    time_dependency_2.* (input width = the fuse width), pool.*.  Alignment / Fusion hold no parameters for de_align dot / cosine and
    de_fuse_dim null -- the configurations the HIP engine runs (engine.check_de_args); anything else raises here, before any GPU work."""

    def __init__(self, **kw):
        super().__init__()
        from .engine import DE_FUSE_WIDTH, check_de_args
        g = lambda k, d=None: kw.get(k, d)
        check_de_args(dict(kw, de_align=g('de_align', 'dot'), de_align_apply=g('de_align_apply', 'hard'), de_fuse=g('de_fuse', 'x/y/-')))
        self.name = 'NISQA_DE'
        self._hp = dict(kw)
        self._engine = None
        self._engine_args = None
        self.cnn = _Wrap(_AdaptCNNParams(g('cnn_c_out_1', 16), g('cnn_c_out_2', 32), g('cnn_c_out_3', 64),
                                         g('cnn_kernel_size', 3), g('cnn_pool_3', [6, 3])))
        d = g('td_sa_d_model', 64)
        self.time_dependency = _Wrap(_SelfAttentionParams(self.cnn.model.fan_out, d, g('td_sa_num_layers', 2), g('td_sa_h', 64)))
        self.time_dependency_2 = _Wrap(_SelfAttentionParams(DE_FUSE_WIDTH[g('de_fuse', 'x/y/-')], g('td_2_sa_d_model', 64),
                                                            g('td_2_sa_num_layers', 2), g('td_2_sa_h', 64)))
        self.pool = _Wrap(_PoolAttFFParams(g('td_2_sa_d_model', 64), g('pool_att_h', 128)))

    def bind_args(self, args):
        self._engine_args = args
        self._engine = None
        return self

    def engine(self, device=None):
        if self._engine is None:
            from .engine import HipNisqaDE
            if self._engine_args is None:
                raise RuntimeError('bind_args(checkpoint_args) must be called before the HIP engine is built')
            self._engine = HipNisqaDE(self._engine_args, self.state_dict(), device)
        return self._engine

    def forward(self, x, n_wins):
        """Reference inner operator model(x[B,L,2,48,15], n_wins[B,2]) -> [B, 1] (NL:399-424): channel 0 of x holds the degraded
        clip's segments, channel 1 the reference clip's.  Malformed arguments raise ValueError before any GPU work.
        When gradients are enabled and x requires one, the result carries a grad_fn and backward delivers d / d x as the
        reference's module does in eval mode, for hard and soft alignment (engine.HipNisqaDE.grad_segments; precisions 'f32' and
        'bf16x6', any other raises NotImplementedError here).  The values are those of the plain call, bit for bit; there is no
        double backward, and the parameters get no gradient."""
        from .engine import DEFAULT_PRECISION, check_segments
        n = check_segments(x, n_wins, 2)
        dev = x.device if x.is_cuda else None
        if not (torch.is_grad_enabled() and x.requires_grad):
            return self.engine(dev).forward_segments(x, n_wins)
        from .input_grad import check_precision
        check_precision(self._engine.precision if self._engine is not None
                        else os.environ.get('NISQA_HIP_PRECISION') or DEFAULT_PRECISION)        # refused before any GPU work
        eng = self.engine(dev)
        return _SegmentsFunction.apply(x.to(eng.device, dtype=torch.float32).contiguous(), eng, n)

    def forward_audio(self, y_deg, y_ref, sr, lengths_deg=None, lengths_ref=None):
        """Full-reference scores of in-memory audio: y_deg [N] or [B, N] the degraded clips, y_ref [M] or [B, M] their clean
        references -- floating tensors of the same rank and the same B on any device (both on one GPU if both are on a GPU), N and
        M independent -- at one integer rate ``sr``; lengths_deg / lengths_ref [B] whole numbers in [1, N] / [1, M] (default: the
        full row) -> [B, 1] on the engine's device.  Samples at n >= lengths[b] are never read.  Both sides are packed back to
        back, the degraded clips first, and go through the engine's forward_pcm (through its resampler first when the checkpoint
        sets ms_sr): the result is HipNisqaDE.forward_pcm's, bit for bit, in every engine precision.
        When gradients are enabled and y_deg or y_ref requires one, the result carries a grad_fn and backward delivers d / d y_deg
        and d / d y_ref, each in its input's shape, dtype and device, exact zeros at n >= lengths[b] whatever the input holds
        there (engine.HipNisqaDE.grad_audio: the mel backward and the segment adjoint behind InputGradDE, in the 2B-clip layout
        end to end; precisions 'f32' and 'bf16x6').  A side that requires no gradient gets none, and its mel backward and CNN
        backward are not run.  The values are the plain call's, bit for bit; there is no double backward and the parameters get
        no gradient.
        Hard alignment (de_align_apply=hard): the argmax carries no gradient.  The backward recomputes the network and takes the
        recomputation's own argmax (InputGradDE.last_idx); at a near-tie of two scores that may differ from the choice of the
        fused inference chain that produced the score (DESIGN.md 4.8 "argmax deviation"), and the gradient is then that of the
        recomputed choice.
        Refused before any GPU work: a side that is not floating or not of rank 1 or 2, sides of different rank or B, on different
        GPUs, an empty batch, lengths out of range (ValueError); a clip of either side too short for one segment or with more
        than ms_max_segments segments (engine.BatchPlan's ValueErrors); a gradient in a fast precision, or while the
        checkpoint's ms_sr differs from sr -- the resampler has no backward -- (NotImplementedError; the plain call still
        works)."""
        d2, r2, n_deg, n_ref, sr, plan = self._audio_plan(y_deg, y_ref, sr, lengths_deg, lengths_ref)
        dev = y_deg.device if y_deg.is_cuda else (y_ref.device if y_ref.is_cuda else None)
        if not (torch.is_grad_enabled() and (y_deg.requires_grad or y_ref.requires_grad)):
            eng = self.engine(dev)
            to = lambda y: y.detach().to(eng.device, dtype=torch.float32)
            return _score_audio_de(eng, to(d2), to(r2), n_deg, n_ref, sr, plan)
        _check_audio_grad(self, sr)
        eng = self.engine(dev)
        # the Function sees the samples the kernels read: torch supplies the adjoint of the device / dtype / rank conversion
        to = lambda y: y.to(eng.device, dtype=torch.float32)
        return _AudioFunctionDE.apply(to(d2), to(r2), eng, n_deg, n_ref, sr, plan)

    def profile_audio(self, y_deg, y_ref, sr, lengths_deg=None, lengths_ref=None, differentiable=False):
        """forward_audio with the score taken apart per segment of the DEGRADED clip: the same arguments, checks and refusals
        (forward_audio's, raised before any GPU work) -> SegmentProfile as _NisqaBase.profile_audio returns it (scores [B, 1]
        forward_audio's, bit for bit; weights, local [B, Lmax, 1]; embed [B, Lmax, 64], the second self-attention's output;
        n_wins [B] of the degraded clips; t_start / t_end [Lmax]) and additionally
          aligned_to [B, Lmax] int64   the reference segment each degraded segment was aligned to with hard alignment
                                       (HipNisqaDE.forward_pcm(..., want_idx=True)); -1 with soft alignment and on padding rows.
        Not a throughput path.  By default the result is detached.  With ``differentiable=True``, gradients enabled and a y_deg or
        y_ref that requires one, scores, weights, local and embed are the four outputs of ONE autograd function, as
        _NisqaBase.profile_audio describes, and backward delivers d / d y_deg and d / d y_ref (engine.HipNisqaDE.grad_profile_audio;
        the refusals, the hard alignment's argmax and the side that requires no gradient are forward_audio's)."""
        d2, r2, n_deg, n_ref, sr, plan = self._audio_plan(y_deg, y_ref, sr, lengths_deg, lengths_ref)
        dev = y_deg.device if y_deg.is_cuda else (y_ref.device if y_ref.is_cuda else None)
        args = dict(self._engine_args, model='NISQA_DE')
        if not (differentiable and torch.is_grad_enabled() and (y_deg.requires_grad or y_ref.requires_grad)):
            eng = self.engine(dev)
            to = lambda y: y.detach().to(eng.device, dtype=torch.float32)
            with torch.no_grad():
                prof = eng.profile_audio(torch.cat([_pack_clips(to(d2), n_deg), _pack_clips(to(r2), n_ref)]), n_deg, n_ref, sr, plan)
            return _segment_profile(prof, plan.n_wins[:len(n_deg)], args)
        _check_audio_grad(self, sr)
        eng = self.engine(dev)
        to = lambda y: y.to(eng.device, dtype=torch.float32)
        return _differentiable_profile(eng, (to(d2), to(r2)), (n_deg, n_ref), sr, plan, args)

    def _audio_plan(self, y_deg, y_ref, sr, lengths_deg, lengths_ref):
        """The argument checks of forward_audio and the 2B-clip plan it builds, on the host
        -> (y_deg as [B, N], y_ref as [B, M], lengths_deg, lengths_ref, sr, plan)"""
        from .engine import BatchPlan
        from .melbank import resampled_lengths
        d2, n_deg = _audio_args(y_deg, lengths_deg, 'y_deg', 'N')
        r2, n_ref = _audio_args(y_ref, lengths_ref, 'y_ref', 'M')
        if y_deg.dim() != y_ref.dim() or d2.shape[0] != r2.shape[0]:
            raise ValueError('y_deg and y_ref must have the same rank and the same number of clips, got {} and {}'.format(
                tuple(y_deg.shape), tuple(y_ref.shape)))
        if y_deg.is_cuda and y_ref.is_cuda and y_deg.device != y_ref.device:
            raise ValueError('y_deg and y_ref are on different GPUs: {} and {}'.format(y_deg.device, y_ref.device))
        if int(sr) != sr or int(sr) < 1:
            raise ValueError('sr must be one positive integer rate for both sides, got {}'.format(sr))
        sr, args = int(sr), self._engine_args
        if args is None:
            raise RuntimeError('bind_args(checkpoint_args) must be called before the HIP engine is built')
        rate = sr if args.get('ms_sr') is None else int(args['ms_sr'])
        # the engine's audio_plan(n_deg, n_ref, sr), on the host: too short a clip and too many segments raise here, on either side
        n2 = np.concatenate([n_deg, n_ref])
        plan = BatchPlan(n2 if rate == sr else resampled_lengths(n2, sr, rate)[0], int(rate * args['ms_hop_length']),
                         int(args['ms_seg_hop_length']), args['ms_max_segments'])
        return d2, r2, n_deg, n_ref, sr, plan


# ---------------------------------------------------------------------------------------------
# Dataset mirror
# ---------------------------------------------------------------------------------------------
class SpeechQualityDataset(object):
    """File table of the reference dataset (NL:2052-2236).  Same constructor arguments; loading a
    waveform replaces ``_load_spec`` (the spectrogram itself is produced on the GPU).

    ``to_memory`` (the recipes' tr_ds_to_memory) is kept as ``self.to_memory``; no work is done at construction, because the
    engine does not exist yet: ``nisqaModel.load_to_memory()`` (called by ``train()``) computes every spectrogram once on the
    GPU and keeps them in device memory (``self.store``, and ``self.ref_store`` over the reference files of a double-ended
    set: melstore.MelStore).  From then on the training loop, the validation pass and ``__getitem__`` read no file; edits to
    the files or to the filename column are not seen, as in the reference (NL:2105-2127).  ``to_memory_workers`` stays accepted
    and unused: the fill is one GPU pass, not a pool of loader processes."""

    def __init__(self, df, df_con=None, data_dir='', folder_column='', filename_column='filename', mos_column='MOS',
                 seg_length=15, max_length=None, to_memory=False, to_memory_workers=0, transform=None,
                 seg_hop_length=1, ms_n_fft=1024, ms_hop_length=80, ms_win_length=170, ms_n_mels=32, ms_sr=48e3,
                 ms_fmax=16e3, ms_channel=None, double_ended=False, filename_column_ref=None, dim=False):
        if double_ended and not filename_column_ref:
            raise ValueError('a double-ended dataset needs filename_column_ref (the csv column of the reference files, csv_ref)')
        if transform is not None:
            raise NotImplementedError('spectrogram transforms are not supported on the HIP path')
        self.df, self.df_con, self.data_dir = df, df_con, data_dir
        self.filename_column, self.mos_column = filename_column, mos_column
        self.seg_length, self.seg_hop_length, self.max_length = seg_length, seg_hop_length, max_length
        self.ms_n_fft, self.ms_hop_length, self.ms_win_length = ms_n_fft, ms_hop_length, ms_win_length
        self.ms_n_mels, self.ms_sr, self.ms_fmax, self.ms_channel = ms_n_mels, ms_sr, ms_fmax, ms_channel
        self.dim = dim
        self.double_ended, self.filename_column_ref = bool(double_ended), filename_column_ref
        self.to_memory = bool(to_memory)
        self.store = self.ref_store = None                         # melstore.MelStore once load_to_memory has run

    def ref_view(self):
        """The same table with the reference files as its file column (double-ended datasets): the readers and the header probe
        take a dataset's file column, so the reference file of item i is item i of this view."""
        v = object.__new__(type(self))
        v.__dict__.update(self.__dict__)
        v.filename_column, v.double_ended = self.filename_column_ref, False
        v.store, v.ref_store = self.ref_store, None
        return v

    def __len__(self):
        return len(self.df)

    def file_path(self, index):
        return os.path.join(self.data_dir, self.df[self.filename_column].iloc[index])   # NL:2132

    def file_paths(self, indices):
        """Paths of many items at once: the filename column is read out once per CALL (a pandas scalar lookup per item
        costs more host time than staging the item's samples; nothing is cached on the dataset, so an in-place edit of
        the column is always seen)."""
        names, d = self.df[self.filename_column].tolist(), self.data_dir
        return [os.path.join(d, names[i]) for i in indices]

    def load_audio(self, index):
        """(samples, sr) of item ``index``; raises ValueError('Could not load file ...') like NL:2305-2306."""
        return read_wav(self.file_path(index), self.ms_channel)

    def bind_engine(self, factory):
        """``factory()`` -> HipNisqa; lets __getitem__ produce spectrogram segments like the reference dataset."""
        self._engine_factory = factory
        return self

    def __getitem__(self, index):
        """(x_spec_seg [max_length,1,n_mels,seg_length], y, (index, n_wins)) like NL:2162-2233.  The spectrogram is
        computed by the HIP front end; the overlapping-window gather (NL:2266-2280) is a host-side view for callers
        that want the reference's item format -- the predict loop never materialises it.
        A double-ended dataset gives (x [max_length,2,n_mels,seg_length], y, (index, [n_wins_deg, n_wins_ref])) like NL:2170-2214:
        channel 0 the degraded file's segments, channel 1 the reference file's, both from the HIP front end."""
        assert isinstance(index, int), 'index must be integer (no slice)'
        if getattr(self, '_engine_factory', None) is None and not (self.store is not None and self.store.filled):
            raise RuntimeError('SpeechQualityDataset item access needs bind_engine(...) (spectrograms are computed on the GPU)')
        if self.double_ended:
            (xd, y, (_, nd)), (xr, _, (_, nr)) = self._item(index), self.ref_view()._item(index)
            if self.max_length is None and int(nd) != int(nr):     # (the reference's torch.cat of unpadded halves fails there too)
                raise ValueError('a double-ended item without max_length needs equal segment counts, got {} and {}'.format(
                    int(nd), int(nr)))
            return torch.cat([xd, xr], 1), y, (index, np.array([int(nd), int(nr)]))
        return self._item(index)

    def _item(self, index):
        """the single-ended item of this dataset's file column"""
        if self.store is not None and self.store.filled:           # resident (to_memory): served from the store, NL:2165
            spec, n_wins = self.store.item(index)
        else:
            eng = self._engine_factory()
            if hasattr(eng, 'base'):                               # HipNisqaDE: mel, resampling and plans are its single-ended engine's
                eng = eng.base
            y, sr = self.load_audio(index)
            plan = eng.audio_plan([len(y)], sr, names=[self.file_path(index)])
            pcm = eng.resample(torch.from_numpy(y).to(eng.device), [len(y)], sr)      # (ms_sr: lb.load resamples first, NL:2300-2304)
            mel, _ = eng.mel(pcm, plan, eng.rate(sr), clamp=True)                     # int16 PCM or float32 samples
            spec = mel.cpu().numpy()                               # [T, n_mels]
            n_wins = int(plan.n_wins[0])
        idx = self.seg_hop_length * np.arange(n_wins)[:, None] + np.arange(self.seg_length)[None, :]
        x = np.transpose(spec[idx], (0, 2, 1))[:, None]           # [n_wins, 1, n_mels, seg_length]
        if self.max_length is not None:
            pad = np.zeros((self.max_length,) + x.shape[1:], np.float32)
            pad[:n_wins] = x
            x = pad
        return torch.from_numpy(np.ascontiguousarray(x)), self.label(index), (index, np.array(n_wins))

    def label(self, index):
        """y of item ``index`` like NL:2217-2231: NaN in predict_only mode, else row ``index`` of the MOS column(s)."""
        if self.mos_column == 'predict_only':
            return np.full(5 if self.dim else 1, np.nan, dtype=np.float32)
        cols = ['mos', 'noi', 'dis', 'col', 'loud'] if self.dim else [self.mos_column]
        return np.array([self.df[c].iloc[index] for c in cols], dtype=np.float32)

    def labels(self, n):
        """Labels of the first n items like NL:2217-2231: NaN rows in predict_only mode, else the csv columns."""
        if self.mos_column == 'predict_only':
            return np.full((n, 5 if self.dim else 1), np.nan, dtype=np.float32)
        cols = ['mos', 'noi', 'dis', 'col', 'loud'] if self.dim else [self.mos_column]
        return np.stack([self.df[c].to_numpy(dtype=np.float32)[:n] for c in cols], 1)


# ---------------------------------------------------------------------------------------------
# Batching loop
# ---------------------------------------------------------------------------------------------
_STREAMS = {}


def _loop_streams(device):
    """(copy stream, [kernel stream, kernel stream]) of the predict loop on ``device``, created once per process.
    The copy stream has high priority = a hardware queue of its own: streams of one priority share a small pool of
    hardware queues round-robin, and a copy stream that lands on the queue of a kernel stream is serialised behind its
    kernels."""
    key = str(device)
    if key not in _STREAMS:
        nk = int(os.environ.get('NISQA_LOOP_KERNEL_STREAMS', '2'))
        ks = [torch.cuda.Stream(device=device) for _ in range(max(1, min(nk, 2)))]
        _STREAMS[key] = (torch.cuda.Stream(device=device, priority=-1), [ks[0], ks[-1]])
    return _STREAMS[key]


LOOP_STATS = {}                 # host seconds of the last _predict call by phase (tools/probe_loop.py)


# work a launch chain should carry before a batch is closed (batch_policy): the AdaptCNN kernel runs 512 four-segment
# workgroups at a time (2 per CU), so 16 k segments are ~8 rounds -- the size of the bs = 64 x 10 s configuration the
# kernels were tuned on; the BiLSTM of the nisqa_tts.tar path runs ONE workgroup per (clip, direction) for as many
# sequential steps as the longest clip has segments: 128 clips x 2 directions fill the 256 CUs
MIN_TOKENS_SA = 16384
MIN_CLIPS_LSTM = 128
BATCH_BYTE_CAP = 256 << 20          # staged PCM per batch (the page-locked ring holds three such slots)


def tokens_of(ds, n_frames, sample_rate):
    """Segments per clip from WAV header fields alone: frames T = 1 + samples // hop (librosa centre framing, NL:2311),
    n_wins = ceil((T - (seg_length - 1)) / seg_hop) (NL:2256-2273).  hop as melbank.MelTables derives it."""
    sr = np.asarray(sample_rate, dtype=np.float64)
    n_frames = np.asarray(n_frames, dtype=np.int64)
    if getattr(ds, 'ms_sr', None) is not None:                     # lb.load(..., sr=ms_sr): ceil(n * ms_sr / sr) samples at ms_sr
        n_frames = np.ceil(n_frames.astype(np.float64) * (float(ds.ms_sr) / np.maximum(sr, 1.0))).astype(np.int64)
        sr = np.full_like(sr, float(ds.ms_sr))
    hop = np.maximum(1, (sr * float(ds.ms_hop_length)).astype(np.int64))
    T = 1 + n_frames // hop
    return np.maximum(1, -(-(T - (int(ds.seg_length) - 1)) // max(1, int(ds.seg_hop_length))))


def batch_policy(eng, ds, indices, bs):
    """Length-aware batches for the predict loop (ingest.LengthAware): --bs is a lower bound, batches are cut by
    segments / clips / staged bytes after sorting a window of items by length."""
    lstm = getattr(eng, 'arch', 0) in (1, 2, 3)           # StandardCNN + BiLSTM with last-step / average / max pooling
    # Large jobs get larger batches: an H2D copy carries ~80 us that does not scale with its size (64 MB copies run at 53 GB/s inside
    # the loop where 245 MB copies run at 56), but a job needs a few hundred batches to keep the pipeline's fill and drain small --
    # so the floor grows with the job, 1 x (<= 25 k items) ... 4 x (>= 100 k items) of MIN_TOKENS_SA.  Measured on a directory of
    # 98 304 ten-second files at --bs 64: 48.5 k clips/s (1 x) / 50.0-50.9 k (2 x) / 50.3-51.2 k (4 x); on 32 768 files 4 x is the
    # slowest (128 batches).  Rows do not depend on the batch composition (tested).
    n_items = len(indices)
    scale = min(4, max(1, n_items // (384 * 66)))
    return _ingest.LengthAware(indices, bs, lambda f, r: tokens_of(ds, f, r),
                               min_tokens=0 if lstm else int(os.environ.get('NISQA_MIN_TOKENS', MIN_TOKENS_SA * scale)),
                               min_clips=int(os.environ.get('NISQA_MIN_CLIPS', MIN_CLIPS_LSTM)) if lstm else 1,
                               byte_cap=int(os.environ.get('NISQA_BATCH_BYTES', BATCH_BYTE_CAP)))


def pair_tokens(ds, indices, num_workers=0):
    """Work of each item of a double-ended dataset: the degraded file's segments plus the reference file's, from the RIFF headers
    alone (an unreadable header counts as one segment; the error itself is raised when the file is loaded)."""
    idx = list(indices)
    tok = np.zeros(len(idx), dtype=np.int64)
    for view in (ds, ds.ref_view()):
        info = _ingest.probe_headers(view, idx, num_workers)
        ok = info['status'] == _lib_mod.WAV_OK
        tok += np.where(ok, tokens_of(view, np.where(ok, info['n_frames'], 0), np.where(ok, info['sample_rate'], 48000)), 1)
    return tok


def _resident(ds):
    """The filled stores of a dataset that keeps its spectrograms in device memory (to_memory) -> (store, ref_store or None), or
    None: the file-fed loops."""
    store = getattr(ds, 'store', None)
    if store is None or not store.filled:
        return None
    ref = getattr(ds, 'ref_store', None) if getattr(ds, 'double_ended', False) else None
    if getattr(ds, 'double_ended', False) and (ref is None or not ref.filled):
        return None
    return store, ref


def _predict_resident(model, ds, stores, bs, dev, on_rows=None):
    """_predict / _predict_de for a resident dataset: no file is opened.  The shard's items are cut into batches by work
    (melstore.work_batches, the floors of batch_policy), every batch is one nisqa_mel_gather per store and the engine's stage API
    from (mel, floor, plan) on: cnn + td_pool, cnn_std + lstm, or -- double-ended, one plan of 2B clips, degraded then reference --
    cnn + forward_features.  Rows do not depend on the batch composition, so they are the file-fed loop's rows."""
    from . import melstore as _ms
    store, ref = stores
    dev = torch.device(dev)
    eng = model.engine(dev if dev.index is not None else None)
    base = getattr(eng, 'base', eng)
    n = len(ds)
    lo, hi = _dist.shard_range(n)
    bounds = None
    rank, world = _dist.world()
    tok = store.n_wins.astype(np.int64) + (ref.n_wins.astype(np.int64) if ref is not None else 0)
    if world > 1 and os.environ.get('NISQA_SHARD_BY_COUNT') != '1':
        bounds = _dist.balanced_bounds(tok, world)                 # every rank holds the whole store: nothing to exchange
        lo, hi = bounds[rank]
    y_local = np.zeros((hi - lo, eng.n_heads), dtype=np.float32)
    loop_err = None
    try:
        bs = max(1, int(bs))
        lstm = getattr(base, 'arch', 0) in (1, 2, 3)
        if os.environ.get('NISQA_EXACT_BS') == '1':
            cuts = [list(range(s, min(s + bs, hi - lo))) for s in range(0, hi - lo, bs)]
        else:
            cuts = _ms.work_batches(tok[lo:hi], bs, 0 if lstm else int(os.environ.get('NISQA_MIN_TOKENS', MIN_TOKENS_SA)),
                                    int(os.environ.get('NISQA_MIN_CLIPS', MIN_CLIPS_LSTM)) if lstm else 1)
        pending = None                                             # (ids, host rows, event): fetched one batch late

        def fetch(p):
            p[2].synchronize()
            y_local[p[0] - lo] = p[1].numpy()
            if on_rows is not None:
                on_rows(p[0].tolist(), p[1].numpy())

        for cut in cuts:
            ids = np.asarray(cut, dtype=np.int64) + lo
            if ref is None:
                mel, _, n_wins, floor = store.batch(ids)
                plan = _ms.batch_plan(n_wins, store.frames[ids])
                out = base.lstm(base.cnn_std(mel, floor, plan), plan)[0] if lstm else base.td_pool(base.cnn(mel, floor, plan)[0], plan)
            else:
                (_, off_d), (_, off_r) = store.offsets(ids), ref.offsets(ids)
                rows_d, B = int(off_d[-1]), len(ids)
                mel = torch.empty((rows_d + int(off_r[-1]), 48), dtype=torch.float32, device=base.device)
                floor = torch.empty(2 * B, dtype=torch.float32, device=base.device)
                store.gather(ids, off_d, mel[:rows_d], floor[:B])
                ref.gather(ids, off_r, mel[rows_d:], floor[B:])
                plan = _ms.batch_plan(np.concatenate([store.n_wins[ids], ref.n_wins[ids]]),
                                      np.concatenate([store.frames[ids], ref.frames[ids]]))
                out = eng.forward_features(base.cnn(mel, floor, plan)[0], plan)
            rows = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
            rows.copy_(out, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            if pending is not None:
                fetch(pending)
            pending = (ids, rows, done)
        if pending is not None:
            fetch(pending)
    except Exception as e:                                          # noqa: BLE001 (raised on every rank below)
        loop_err = e
    _dist.raise_together(loop_err)
    return _dist.gather_rows(y_local, n, lo, hi, dev, bounds)


def _predict_de(model, ds, bs, dev, num_workers, on_rows=None):
    """_predict for a double-ended dataset (NISQA_DE): y_hat [N, 1].  Items are (degraded, reference) file pairs, read with the
    readers of the single-ended loop (WAV / FLAC, ms_channel) and batched in table order: at least ``bs`` pairs and, unless
    NISQA_EXACT_BS=1, at least MIN_TOKENS_SA segments of work; rows do not depend on the batch composition.  Over several ranks the
    shards are work-balanced on pair_tokens."""
    dev = torch.device(dev)
    if model._engine is None and dev.type != 'cuda':
        raise RuntimeError('nisqa_amd has no CPU path: device {} requested but the hot path runs only as HIP kernels '
                           'on an MI355X'.format(dev))
    eng = model.engine(dev if dev.index is not None else None)
    n = len(ds)
    lo, hi = _dist.shard_range(n)
    bounds = None
    rank, world = _dist.world()
    if world > 1 and os.environ.get('NISQA_SHARD_BY_COUNT') != '1':
        tok = np.zeros(n, dtype=np.int64)
        probe_err = None
        try:
            if hi > lo:
                tok[lo:hi] = pair_tokens(ds, range(lo, hi), num_workers)
        except Exception as e:                                      # noqa: BLE001 (re-raised on every rank below)
            probe_err = e
            tok[lo:hi] = 0
        tok = _dist.all_reduce_sum_i64(tok)
        _dist.raise_together(probe_err)
        bounds = _dist.balanced_bounds(tok, world)
        lo, hi = bounds[rank]
    y_local = np.zeros((hi - lo, 1), dtype=np.float32)
    loop_err = None
    try:
        bs = max(1, int(bs))
        min_tok = 0 if os.environ.get('NISQA_EXACT_BS') == '1' else int(os.environ.get('NISQA_MIN_TOKENS', MIN_TOKENS_SA))
        refs = ds.ref_view()
        i = lo
        while i < hi:
            ids, deg, ref, names, work = [], [], [], [], 0
            while i < hi and (len(ids) < bs or work < min_tok):
                d, r = ds.load_audio(i), refs.load_audio(i)
                ids.append(i)
                deg.append(d)
                ref.append(r)
                names.append((ds.file_path(i), refs.file_path(i)))
                work += int(tokens_of(ds, [len(d[0]), len(r[0])], [d[1], r[1]]).sum())
                i += 1
            out = eng.forward_items(deg + ref, [p[0] for p in names] + [p[1] for p in names])
            rows = out.cpu().numpy()
            y_local[np.asarray(ids) - lo] = rows
            if on_rows is not None:
                on_rows(ids, rows)
    except Exception as e:                                          # noqa: BLE001 (raised on every rank below)
        loop_err = e
    _dist.raise_together(loop_err)
    return _dist.gather_rows(y_local, n, lo, hi, dev, bounds)


def _predict(model, ds, bs, dev, num_workers, on_rows=None):
    """Shared body of predict_mos / predict_dim: returns y_hat [N, heads] float32 for ALL items of ds
    (clip-sharded over ranks when torch.distributed is initialised, then gathered).
    on_rows(ids, rows): optional callback with every batch's item indices and [B, heads] float32 rows as they come back from
    the device (nisqaModel.predict formats the table cells there, under the next batches' transfers)."""
    stores = _resident(ds)
    if stores is not None:
        return _predict_resident(model, ds, stores, bs, dev, on_rows)
    if getattr(ds, 'double_ended', False):
        return _predict_de(model, ds, bs, dev, num_workers, on_rows)
    dev = torch.device(dev)
    if model._engine is None and dev.type != 'cuda':
        raise RuntimeError('nisqa_amd has no CPU path: device {} requested but the hot path runs only as HIP kernels '
                           'on an MI355X'.format(dev))
    eng = model.engine(dev if dev.index is not None else None)
    on_gpu = eng.device.type == 'cuda'
    n = len(ds)
    lo, hi = _dist.shard_range(n)
    bounds = None
    rank, world = _dist.world()
    if world > 1 and os.environ.get('NISQA_SHARD_BY_COUNT') != '1':
        # work-balanced contiguous shards: every rank probes the RIFF headers of its count share (native threads, headers
        # only), the per-clip segment counts are summed into one vector on all ranks, and the shard boundaries follow its
        # prefix sum -- a length-sorted list of mixed 3-30 s clips otherwise gives the last rank several times the first
        # one's work.  An unreadable header counts as one segment here; the error itself is raised where the reference
        # raises it, when the file is loaded.
        # A rank whose probe itself fails (ingest library missing, no filename column ...) still enters both collectives:
        # the others would otherwise wait in all_reduce for ever (dist.raise_together).
        tok = np.zeros(n, dtype=np.int64)
        probe_err = None
        try:
            if hi > lo:
                info = _ingest.probe_headers(ds, range(lo, hi), num_workers)
                ok = info['status'] == _lib_mod.WAV_OK
                tok[lo:hi] = np.where(ok, tokens_of(ds, np.where(ok, info['n_frames'], 0), np.where(ok, info['sample_rate'], 48000)), 1)
        except Exception as e:                                      # noqa: BLE001 (re-raised on every rank below)
            probe_err = e
            tok[lo:hi] = 0
        tok = _dist.all_reduce_sum_i64(tok)
        _dist.raise_together(probe_err)
        bounds = _dist.balanced_bounds(tok, world)
        lo, hi = bounds[rank]
    loop_err, ing, copy_events = None, None, []
    # Three Python threads share the interpreter lock here: this one (enqueue, results, table cells), the producer (staging) and the
    # helper that probes and cuts the NEXT window of 16 384 files -- 20 ms of pure Python per window.  With CPython's default 5 ms
    # switch interval the helper holds the lock in 5 ms slices while the other two need it for microseconds every batch: the copy
    # stream ran dry for 2 x 6-8 ms at every window boundary (rocprofv3 --memory-copy-trace: 85 of 1 735 ms on the csv leg, 135 of
    # 1 794 on the directory leg).  A 0.1 ms interval for the duration of the loop hands the lock over before a copy's worth of
    # time has passed.
    switch_interval = sys.getswitchinterval()
    sys.setswitchinterval(min(switch_interval, float(os.environ.get('NISQA_LOOP_SWITCH_INTERVAL', '1e-4'))))
    T = {'queue_wait': 0.0, 'enqueue': 0.0, 'result_wait': 0.0}
    try:
        bs = max(1, int(bs))
        heads = eng.n_heads
        y_local = np.zeros((hi - lo, heads), dtype=np.float32)
        if os.environ.get('NISQA_EXACT_BS') == '1':                     # the reference's batches: index order, exactly bs clips
            batches = [list(range(s, min(s + bs, hi))) for s in range(lo, hi, bs)]
        else:
            batches = batch_policy(eng, ds, range(lo, hi), bs)
        # host side (ingest.py): a producer thread + num_workers readers stage batches two ahead in page-locked buffers;
        # device side: ONE stream carries nothing but the H2D copies (a stream that also carries kernels gets its copies done
        # by a shader blit that competes with them instead of the SDMA engine: copy and kernels of neighbouring batches then
        # do not overlap at all, tools/probe_overlap.py: 7.5 ms per 256-clip batch against 4.5), two streams take the
        # kernels of alternate batches behind an event, a staging slot is recycled as soon as ITS copy is done, and the D2H
        # of batch i's [B, heads] rows is waited for one batch late (no device-wide sync in the loop)
        # three batches staged ahead (four page-locked slots): the consumer below keeps TWO batches in flight, so the copy of
        # batch k + 1 is queued a whole batch time before the link needs it, not 0.8 ms before (kernels 3 ms + enqueue 0.5 ms
        # against a 4.3 ms copy: with one batch in flight any jitter left the link idle, 89 % of its rate over 98 304 rows)
        ing = _ingest.Ingest(ds, batches, pin=on_gpu, num_workers=num_workers, depth=int(os.environ.get('NISQA_LOOP_DEPTH', '3')),
                             device=eng.device if on_gpu else None,
                             # files that are not mono PCM16 travel as raw data chunks and are decoded by nisqa_wav_decode
                             # (ingest.copy_group on the copy stream, ingest.decode_group on a kernel stream: the two halves of
                             # ingest.group_pcm); NISQA_HOST_DECODE=1: the staging thread decodes them, as before
                             device_decode=on_gpu and _ingest.device_decode_default(),
                             # FLAC streams travel as their frame regions and are decoded by nisqa_flac_decode (NISQA_HOST_FLAC=1:
                             # by the reader threads, as before)
                             device_flac=on_gpu and _ingest.device_flac_default())
        copy_stream, streams = _loop_streams(eng.device) if on_gpu else (None, [None, None])
        inflight = []                                                   # (ids, host rows, event behind them)
        keep_inflight = max(1, int(os.environ.get('NISQA_LOOP_INFLIGHT', '2')))
        time_copies = on_gpu and os.environ.get('NISQA_LOOP_TIME_COPIES') == '1'     # tools: HIP events around every batch's H2D copies
        clock = time.perf_counter

        def drain(keep):
            # waits on the EVENT behind a batch's rows, never on its stream: hipStreamSynchronize also waits for whatever was
            # queued on the stream (or on another stream that shares its hardware queue) after that batch, i.e. for the batch
            # just enqueued -- the loop then runs copy and kernels strictly one after the other (8.2 instead of 4.6 ms per
            # 256 clips; which it was depended on the order streams were created in)
            t0 = clock()
            while len(inflight) > keep:
                ids, rows, done, flagged = inflight.pop(0)
                if done is not None:
                    done.synchronize()
                if flagged is not None:                             # (g, the status words nisqa_flac_decode left for it)
                    _ingest.check_flac_status(flagged[0], flagged[1].numpy(), getattr(ds, 'ms_channel', None))
                y_local[np.asarray(ids) - lo] = rows.numpy()
                if on_rows is not None:
                    on_rows(ids, rows.numpy())
            T['result_wait'] += clock() - t0

        t_it = clock()
        for bi, staged in enumerate(ing):
            t_got = clock()
            T['queue_wait'] += t_got - t_it
            st = streams[bi % 2]
            raw = ing.ring.buf[staged.slot]
            sent, ev = [], None
            try:
                with (torch.cuda.stream(copy_stream) if on_gpu else _nullcontext()):
                    if time_copies:
                        e0 = torch.cuda.Event(enable_timing=True)
                        e0.record(copy_stream)
                    for g in staged.groups:                          # files of one rate share the mel tables
                        plan = eng.audio_plan(g.lengths, g.sr, names=g.names)
                        tables = plan.to(eng.device)
                        # PCM16 stays int16, 2 bytes/sample over PCIe; a raw group crosses as its data chunks.  (Round 5 sent the halves of a batch through TWO copy-only
                        # streams so that one engine's set-up would be covered by the other's transfer: 48.6 / 47.7 k clips/s against
                        # 50.4 / 52.3 k with one stream on the same box -- two SDMA queues share the link worse than one fills it.)
                        sent.append((g, plan, tables, _ingest.copy_group(raw, g, eng.device)))
                    if on_gpu:
                        ev = torch.cuda.Event(enable_timing=time_copies)
                        ev.record(copy_stream)
                        if time_copies:
                            copy_events.append((e0, ev))
            finally:
                ing.ring.release_after(staged.slot, ev)
            if on_gpu:
                st.wait_event(ev)
            with (torch.cuda.stream(st) if on_gpu else _nullcontext()):
                for g, plan, tables, sent_pcm in sent:
                    pcm = _ingest.decode_group(sent_pcm, g, eng)     # (a raw group: every WAV encoding -> float32, on this stream)
                    out = eng.forward_audio(pcm, g.lengths, g.sr, plan)      # (resampled to ms_sr first when the checkpoint sets it)
                    if on_gpu:
                        sent_pcm.record_stream(st)                   # allocated on the copy stream, consumed on this one
                        tables['_buf'].record_stream(st)
                        rows = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
                        rows.copy_(out, non_blocking=True)           # [B, heads] floats, behind the kernels
                        flagged = None
                        if g.kind == 'flac':                         # the decoder's status words come back with the rows
                            words = torch.empty(g.status.shape, dtype=g.status.dtype, pin_memory=True)
                            words.copy_(g.status, non_blocking=True)
                            flagged = (g, words)
                        done = torch.cuda.Event()
                        done.record(st)
                        inflight.append((g.ids, rows, done, flagged))
                    else:
                        inflight.append((g.ids, out, None, None))
            T['enqueue'] += clock() - t_got
            drain(keep=keep_inflight * len(staged.groups))           # results of the batch before the previous one
            t_it = clock()
        drain(keep=0)
    except Exception as e:                                          # noqa: BLE001
        # the reference's errors (unreadable file, too short, too many segments: NL:2305-2306, 2259-2263, 2276-2277) are
        # raised on EVERY rank below, not only on the one whose shard holds the file -- the others would block in the
        # closing all_gather
        loop_err = e
    finally:
        sys.setswitchinterval(switch_interval)
        LOOP_STATS.clear()
        LOOP_STATS.update(T)
        if ing is not None:
            ing.close()
            LOOP_STATS.update({'producer_' + k: v for k, v in ing.stats.items()})
            LOOP_STATS['readers'] = ing.workers
        if copy_events:
            torch.cuda.synchronize()
            LOOP_STATS['copy_busy_s'] = sum(a.elapsed_time(b) for a, b in copy_events) * 1e-3
            LOOP_STATS['copy_span_s'] = copy_events[0][0].elapsed_time(copy_events[-1][1]) * 1e-3
    _dist.raise_together(loop_err)
    return _dist.gather_rows(y_local, n, lo, hi, dev, bounds)


def predict_mos(model, ds, bs, dev, num_workers=0, on_rows=None):
    """predict_mos (NL:1420-1439): fills ds.df['mos_pred'] (float64 like NL:1438), returns (y_hat, y)."""
    y_hat = _predict(model, ds, bs, dev, num_workers, on_rows)[:, :1]
    y = ds.labels(len(ds))[:, :1]
    ds.df['mos_pred'] = y_hat.astype(dtype=float)
    return y_hat, y


def predict_dim(model, ds, bs, dev, num_workers=0, on_rows=None):
    """predict_dim (NL:1441-1467): fills mos/noi/dis/col/loud_pred columns, returns (y_hat, y)."""
    y_hat = _predict(model, ds, bs, dev, num_workers, on_rows)
    y = ds.labels(len(ds))
    ds.df['mos_pred'] = y_hat[:, 0].reshape(-1, 1)
    ds.df['noi_pred'] = y_hat[:, 1].reshape(-1, 1)
    ds.df['dis_pred'] = y_hat[:, 2].reshape(-1, 1)
    ds.df['col_pred'] = y_hat[:, 3].reshape(-1, 1)
    ds.df['loud_pred'] = y_hat[:, 4].reshape(-1, 1)
    return y_hat, y
