"""StandardCNN + BiLSTM training test support (not a test module): a float64 CPU restatement of ONE train-mode step of the
models HipTrainerLSTM trains -- ``model.train(); y_hat = model(x, n_wins); loss = biasLoss.get_loss(...); loss.backward()``
(reference nisqa/NISQA_model.py:131-152) -- as a torch-autograd function of an unchanged state_dict, with the dropout masks
as explicit inputs, and the seeded batches of the fixtures (tests/golden/make_golden_train_lstm.py).

Restated (NL = nisqa/NISQA_lib.py): StandardCNN.forward in train mode (NL:712-836; BatchNorm on the statistics of all valid
segments, pool_first = MaxPool2d(2, 2, padding (0, 1)), Dropout2d after pool2, relu3, pool4, relu5, fc_out on the [C][H][W]
flatten), nn.LSTM over each clip's own n_wins segments (NL:897-943 packs the sequence), PoolLastStepBi / PoolAvg / PoolMax
and their linear layer (NL:1099-1115, 1185-1224), the NaN-aware MSE with the optional cubic bias map (NL:1880-1892,
1946-1950).  tests/test_train_lstm_host.py pins this against the fixtures; the GPU tests use it where masks are non-zero.
"""
import numpy as np
import torch
import torch.nn.functional as F

from nisqa_amd import synth
from oracle import net as onet
from oracle.train import nan_mse_loss, param_keys

# recipe arguments: config/train_nisqa_cnn_lstm_avg.yaml (hop 3, 1300-segment cap) and its pool: max variant; nisqa_tts.tar's
# own arguments (hop 1, last_step_bi) come with the checkpoint
AVG_ARGS = dict(synth.TTS_ARGS, name='train_lstm_avg', ms_fmax=20000, ms_seg_hop_length=3, ms_max_segments=1300, pool='avg',
                cnn_kernel_size=(3, 3), cnn_dropout=0.2)
MAX_ARGS = dict(AVG_ARGS, name='train_lstm_max', pool='max')
FRAMES = [15, 40, 97, 260, 1001]          # one single-segment clip, ragged lengths, a 10 s clip (329 steps at hop 3, 987 at hop 1)
MASK_SITES = (('cnn_d1', 32), ('cnn_d2', 64), ('cnn_d3', 64), ('cnn_d4', 64))


def batch(seed, frames=FRAMES):
    """Seeded spectrogram-like clips [48, T] (dB-ish, a slow envelope plus noise) and labels with one NaN."""
    rng = np.random.default_rng(seed)
    specs = []
    for T in frames:
        env = np.clip(-38 + 14 * np.sin(np.linspace(0, rng.uniform(3, 20), T) + rng.uniform(0, 6)), -80, 0)
        s = (env[None, :] + 9 * rng.standard_normal((48, T)) - 0.3 * np.arange(48)[:, None]).astype(np.float32)
        specs.append(np.maximum(s, s.max() - 80))
    y = rng.uniform(1, 5, (len(frames), 1)).astype(np.float32)
    y[1, 0] = np.nan
    return specs, y


def segments(specs, args):
    xs, nw = zip(*[onet.segment_specs(s, args['ms_seg_length'], args['ms_seg_hop_length'], args['ms_max_segments'])
                   for s in specs])
    x = torch.cat([xi[:n] for xi, n in zip(xs, nw)], 0)           # the valid segments only, clip after clip
    return x, np.asarray(nw, dtype=np.int64)


def random_masks(seed, S, p):
    """Dropout2d multipliers per (segment, channel) for the four sites: 0 or 1 / (1 - p)."""
    rng = np.random.default_rng(seed)
    return {k: ((rng.random((S, c)) >= p) / (1.0 - p)).astype(np.float32) for k, c in MASK_SITES}


def _bn_relu(sd, i, z, stats):
    stats['bn%d' % i] = (z.detach().mean((0, 2, 3)), z.detach().var((0, 2, 3), unbiased=False), z.numel() // z.shape[1])
    z = F.batch_norm(z, None, None, sd['cnn.model.bn%d.weight' % i], sd['cnn.model.bn%d.bias' % i], True, 0.0, onet.BN_EPS)
    return F.relu(z)


def standard_cnn_train(sd, x, masks, stats):
    """StandardCNN.forward in train mode: x [S,1,48,15] -> [S,20]; masks 'cnn_d1'..'cnn_d4' [S,C]."""
    def m(k, t):
        if masks is None or k not in masks:
            return t
        return t * torch.as_tensor(masks[k], dtype=t.dtype).reshape(t.shape[0], t.shape[1], 1, 1)

    conv = lambda i, t: F.conv2d(t, sd['cnn.model.conv%d.weight' % i], sd['cnn.model.conv%d.bias' % i], padding=1)
    x = _bn_relu(sd, 1, conv(1, x), stats)
    x = F.max_pool2d(x, 2, stride=2, padding=(0, 1))
    x = F.max_pool2d(_bn_relu(sd, 2, conv(2, x), stats), 2)
    x = m('cnn_d1', x)
    x = m('cnn_d2', _bn_relu(sd, 3, conv(3, x), stats))
    x = F.max_pool2d(_bn_relu(sd, 4, conv(4, x), stats), 2)
    x = m('cnn_d3', x)
    x = m('cnn_d4', _bn_relu(sd, 5, conv(5, x), stats))
    x = _bn_relu(sd, 6, conv(6, x), stats)
    return F.linear(x.reshape(x.shape[0], -1), sd['cnn.model.fc_out.weight'], sd['cnn.model.fc_out.bias'])


def bilstm(sd, x20, pfx='time_dependency.model.lstm.'):
    """nn.LSTM(20, 128, bidirectional) on one clip's rows x20 [n, 20] -> [n, 256] (autograd through the sd tensors)."""
    lstm = torch.nn.LSTM(20, 128, num_layers=1, batch_first=True, bidirectional=True).to(x20.dtype)
    params = {k: sd[pfx + k] for k in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_ih_l0_reverse',
                                       'weight_hh_l0_reverse', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse')}
    return torch.func.functional_call(lstm, params, (x20[None],))[0][0]


def pool_vector(td, pool):
    if pool == 'avg':
        return td.sum(0) / td.shape[0]
    if pool == 'max':
        return td.max(0)[0]
    if pool == 'last_step_bi':
        return torch.cat([td[-1, :128], td[0, 128:]], 0)
    raise NotImplementedError(pool)


def forward_train(sd, args, segs, n_wins, masks=None):
    """-> (y_hat [B, 1], BatchNorm batch statistics)"""
    stats = {}
    x20 = standard_cnn_train(sd, segs, masks, stats)
    out, o = [], 0
    for n in (int(v) for v in n_wins):
        v = pool_vector(bilstm(sd, x20[o:o + n]), args['pool'])
        out.append(F.linear(v, sd['pool.model.linear.weight'], sd['pool.model.linear.bias']))
        o += n
    return torch.stack(out), stats


def train_step(sd, args, segs, n_wins, y, masks=None, bias=None, dtype=torch.float64):
    """Loss, y_hat, every gradient and the BatchNorm buffers after the step, in ``dtype`` (float64 by default)."""
    sd = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in sd.items()}
    keys = param_keys(sd)
    for k in keys:
        sd[k] = sd[k].to(dtype).requires_grad_(True)
    y_hat, stats = forward_train(sd, args, torch.as_tensor(segs).to(dtype), n_wins, masks)
    loss = nan_mse_loss(y_hat, torch.as_tensor(np.asarray(y)).to(dtype), None if bias is None else torch.as_tensor(np.asarray(bias)).to(dtype))
    grads = dict(zip(keys, torch.autograd.grad(loss, [sd[k] for k in keys])))
    bufs = {}
    for i in range(1, 7):
        mean, var, cnt = stats['bn%d' % i]
        p = 'cnn.model.bn%d.' % i
        bufs[p + 'running_mean'] = (0.9 * sd[p + 'running_mean'].to(dtype) + 0.1 * mean).numpy()
        bufs[p + 'running_var'] = (0.9 * sd[p + 'running_var'].to(dtype) + 0.1 * var * (cnt / (cnt - 1))).numpy()
    return {'loss': float(loss.detach()), 'y_hat': y_hat.detach().numpy(), 'grads': {k: g.numpy() for k, g in grads.items()},
            'bufs': bufs}
