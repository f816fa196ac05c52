"""CNN-LSTM-AVG / CNN-LSTM-MAX test support (not a test module): the model's arguments, the seeded clip set of the fixtures, and a
torch restatement of the forward -- oracle.net's StandardCNN and BiLSTM followed by the reference's masked average / max pooling
(nisqa/NISQA_lib.py:1185-1224) and its linear layer.  tests/test_lstm_pool_host.py checks the restatement against the committed
fixtures (tests/golden/net_lstm_{avg,max}_rand.npz, made from the reference's own modules) and against the reference's PoolAvg /
PoolMax where the reference is importable; the GPU tests check the HIP engine against it."""
import numpy as np
import torch
import torch.nn.functional as F

from nisqa_amd import synth
from oracle import mel as omel, net as onet

# config/train_nisqa_cnn_lstm_avg.yaml: StandardCNN (fc 20) + BiLSTM(128, 1 layer) + pool avg on the fullband front end at segment
# hop 3 with the 1300-segment cap; pool: max is the yaml's one-word variant
LSTM_AVG_ARGS = dict(synth.TTS_ARGS, name='rand_lstm_avg', ms_fmax=20000, ms_seg_hop_length=3, ms_max_segments=1300, pool='avg',
                     cnn_kernel_size=(3, 3), cnn_dropout=0.2)
LSTM_MAX_ARGS = dict(LSTM_AVG_ARGS, name='rand_lstm_max', pool='max')
POOL_ARGS = {'avg': LSTM_AVG_ARGS, 'max': LSTM_MAX_ARGS}
SEED = 11                       # synth.random_state_dict(SEED, 'NISQA_TTS'): the tts key set, the recipe's shapes

HOP = 480                       # 10 ms at 48 kHz
CAP_SAMPLES = 3913 * HOP        # T = 3914 frames: ceil((3914 - 14) / 3) = 1300 segments, the ms_max_segments cap
OVER_CAP_SAMPLES = 3914 * HOP   # T = 3915: 1301 segments, refused
# (synth seed, samples): one segment, ragged lengths, 10 s and a clip at the cap
CLIPS = [(40, 7200), (41, 17760), (42, 48000), (43, 113760), (44, 144000), (45, 480000), (46, CAP_SAMPLES)]
STAGE_CLIPS = [0, 2, 5]         # clips whose feat20 the fixtures store


def model_kwargs(args):
    """The constructor arguments nisqaModel._loadModel passes (reference NISQA_model.py:956-1004)."""
    from oracle.ref_shim import MODEL_ARG_KEYS
    return {k: args[k] for k in MODEL_ARG_KEYS}


def state_dict(seed=SEED):
    return synth.random_state_dict(seed, 'NISQA_TTS')


def clip_pcm(i):
    seed, n = CLIPS[i]
    return synth.to_pcm16(synth.synth_clip(seed, n / 48000.0))


def clip_spec(pcm, args):
    return omel.melspec_db_from_audio(pcm.astype(np.float32) / np.float32(32768.0), 48000, fmax=float(args['ms_fmax']))


def pool_vector(td, pool):
    """PoolAvg / PoolMax before the linear layer, on ONE clip's valid rows td [n, 256]: the masked sum over the valid steps divided by
    n (NISQA_lib.py:1195-1200), or the masked maximum (:1215-1219)."""
    if pool == 'avg':
        return td.sum(0) / td.shape[0]
    if pool == 'max':
        return td.max(0)[0]
    if pool == 'last_step_bi':
        H = td.shape[1] // 2
        return torch.cat([td[-1, :H], td[0, H:]], 0)
    raise NotImplementedError(pool)


def pool_linear(sd, v, pfx='pool.model.'):
    w, b = sd[pfx + 'linear.weight'], sd[pfx + 'linear.bias']
    return F.linear(v, torch.as_tensor(w).to(v.dtype), torch.as_tensor(b).to(v.dtype)).reshape(-1)


def predict(sd, args, spec, dtype=torch.float32, return_stages=False):
    """model.forward on one clip's [48, T] dB spectrogram -> float32 [1] (and the stages feat [n,20], td [n,256], pooled [256] in
    ``dtype``)."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if k.split('.')[-1] != 'num_batches_tracked'}
    with torch.no_grad():
        x, n = onet.segment_specs(spec, args['ms_seg_length'], args['ms_seg_hop_length'], None)
        if n > args['ms_max_segments']:
            raise ValueError('n_wins {} > max_length {}'.format(n, args['ms_max_segments']))
        feat = onet.standard_cnn(sd, x.to(dtype))
        td = onet.bilstm(sd, feat)
        v = pool_vector(td, args['pool'])
        out = pool_linear(sd, v)
    res = out.numpy().astype(np.float32)
    return (res, {'feat': feat, 'td': td, 'pooled': v}) if return_stages else res
