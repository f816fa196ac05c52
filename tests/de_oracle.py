"""NISQA_DE test support (not a test module): the model's arguments, seeded weights, and a float64 / float32 restatement of the
double-ended forward (reference nisqa/NISQA_lib.py:406-424) built from the oracle's single-ended operators plus Alignment + Fusion
(:1228-1417) restated in numpy.  tests/test_de_host.py checks the restatement against the reference's own modules; the GPU tests
check the HIP engine against it."""
import zlib

import numpy as np
import torch

from nisqa_amd import synth
from oracle import net as onet

# the shipped double-ended training config (config/train_nisqa_double_ended.yaml) on the nisqa.tar front end
DE_ARGS = dict(synth.MOS_ARGS, model='NISQA_DE', name='rand_de', double_ended=True,
               td_2='self_att', td_2_sa_d_model=64, td_2_sa_nhead=1, td_2_sa_pos_enc=False, td_2_sa_num_layers=2, td_2_sa_h=64,
               td_2_sa_dropout=0.1, de_align='cosine', de_align_apply='hard', de_fuse='x/y/-', de_fuse_dim=None)
ALIGNS, APPLIES, FUSES = ('cosine', 'dot'), ('hard', 'soft'), ('x/y/-', '+/-', 'x/y')
FUSE_WIDTH = {'x/y/-': 192, '+/-': 128, 'x/y': 128}
MODEL_KEYS = ['ms_seg_length', 'ms_n_mels', 'cnn_model', 'cnn_c_out_1', 'cnn_c_out_2', 'cnn_c_out_3', 'cnn_kernel_size',
              'cnn_dropout', 'cnn_pool_1', 'cnn_pool_2', 'cnn_pool_3', 'cnn_fc_out_h', 'td', 'td_sa_d_model', 'td_sa_nhead',
              'td_sa_pos_enc', 'td_sa_num_layers', 'td_sa_h', 'td_sa_dropout', 'td_lstm_h', 'td_lstm_num_layers', 'td_lstm_dropout',
              'td_lstm_bidirectional', 'td_2', 'td_2_sa_d_model', 'td_2_sa_nhead', 'td_2_sa_pos_enc', 'td_2_sa_num_layers',
              'td_2_sa_h', 'td_2_sa_dropout', 'td_2_lstm_h', 'td_2_lstm_num_layers', 'td_2_lstm_dropout', 'td_2_lstm_bidirectional',
              'pool', 'pool_att_h', 'pool_att_dropout', 'de_align', 'de_align_apply', 'de_fuse_dim', 'de_fuse']


def de_args(align='cosine', apply='hard', fuse='x/y/-', **kw):
    return dict(DE_ARGS, de_align=align, de_align_apply=apply, de_fuse=fuse, **kw)


def model_kwargs(args):
    """The constructor arguments nisqaModel._loadModel passes (reference NISQA_model.py:956-1015)."""
    return {k: args[k] for k in MODEL_KEYS}


def random_de_state_dict(seed, fuse='x/y/-', n_layers2=2):
    """Seeded weights with the key set of a NISQA_DE checkpoint: cnn.*, time_dependency.* and pool.* as synth.random_state_dict
    (the nisqa.tar shapes), time_dependency_2.* (input width = the fuse width) from a numpy generator of the same seed."""
    sd = {k: v for k, v in synth.random_state_dict(seed, 'NISQA').items()}
    rng = np.random.RandomState(int(seed) + 7919)
    rn = lambda *shape, std=1.0: torch.from_numpy((rng.standard_normal(shape) * std).astype(np.float32))
    F = FUSE_WIDTH[fuse]
    p = 'time_dependency_2.model.'
    sd[p + 'norm1.weight'] = 1.0 + rn(64, std=0.1)
    sd[p + 'norm1.bias'] = rn(64, std=0.1)
    sd[p + 'linear.weight'] = rn(64, F, std=F ** -0.5)
    sd[p + 'linear.bias'] = rn(64, std=0.1)
    for l in range(n_layers2):
        q = p + 'layers.%d.' % l
        sd[q + 'self_attn.in_proj_weight'] = rn(192, 64, std=0.25)
        sd[q + 'self_attn.in_proj_bias'] = rn(192, std=0.1)
        sd[q + 'self_attn.out_proj.weight'] = rn(64, 64, std=0.125)
        sd[q + 'self_attn.out_proj.bias'] = rn(64, std=0.1)
        sd[q + 'linear1.weight'] = rn(64, 64, std=0.125)
        sd[q + 'linear1.bias'] = rn(64, std=0.1)
        sd[q + 'linear2.weight'] = rn(64, 64, std=0.125)
        sd[q + 'linear2.bias'] = rn(64, std=0.1)
        for n in ('norm1', 'norm2'):
            sd[q + n + '.weight'] = 1.0 + rn(64, std=0.1)
            sd[q + n + '.bias'] = rn(64, std=0.1)
    return sd


def state_dict_crc(sd):
    c = 0
    for k in sorted(sd):
        c = zlib.crc32(k.encode(), c)
        c = zlib.crc32(np.ascontiguousarray(sd[k].detach().cpu().numpy()).tobytes(), c)
    return c


# -- Alignment + Fusion (NISQA_lib.py:1228-1417), one pair -----------------------------------------------------------------------
def scores(xd, xr, align):
    """att[i, j] between degraded token i and reference token j (valid rows only), in the inputs' dtype."""
    if align == 'cosine':       # torch's CosineSimilarity: each operand / max(||.||, 1e-8), then the dot product
        qn = xd / np.maximum(np.sqrt((xd * xd).sum(1, keepdims=True)), 1e-8)
        yn = xr / np.maximum(np.sqrt((xr * xr).sum(1, keepdims=True)), 1e-8)
        return qn @ yn.T
    return xd @ xr.T


def align_fuse(xd, xr, align, apply, fuse):
    """-> (fused [n_x, F], hard indices [n_x] or None, top-2 score gap [n_x]) for one pair's valid rows."""
    att = scores(xd, xr, align)
    srt = np.sort(att, 1)
    gap = srt[:, -1] - srt[:, -2] if att.shape[1] > 1 else np.full(att.shape[0], np.inf)
    if apply == 'hard':
        idx = att.argmax(1)
        y = xr[idx]
    else:
        e = np.exp(att - att.max(1, keepdims=True))
        y = (e / e.sum(1, keepdims=True)) @ xr
        idx = None
    return fuse_rows(xd, y, fuse), idx, gap


def fuse_rows(x, y, fuse):
    if fuse == 'x/y/-':
        return np.concatenate([x, y, x - y], 1)
    if fuse == '+/-':
        return np.concatenate([x + y, x - y], 1)
    return np.concatenate([x, y], 1)


# -- the whole forward, one pair ---------------------------------------------------------------------------------------------
def _sd(sd, dtype):
    return {k: (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype)
            for k, v in sd.items() if k.split('.')[-1] != 'num_batches_tracked'}


def forward_segments(sd, args, xd, xr, dtype=torch.float64, stages=False):
    """NISQA_DE.forward for one pair of VALID segment stacks xd [n_x, 1, 48, 15], xr [n_y, 1, 48, 15] -> MOS (float) [, stages]."""
    s = _sd(sd, dtype)
    with torch.no_grad():
        f = lambda x: onet.adapt_cnn(s, torch.as_tensor(x).to(dtype), args['cnn_pool_1'], args['cnn_pool_2'], args['cnn_pool_3'])
        td_x = onet.self_attention(s, f(xd), args['td_sa_num_layers'])
        td_y = onet.self_attention(s, f(xr), args['td_sa_num_layers'])
        fused, idx, gap = align_fuse(td_x.numpy(), td_y.numpy(), args['de_align'], args['de_align_apply'], args['de_fuse'])
        x2 = onet.self_attention(s, torch.from_numpy(fused), args['td_2_sa_num_layers'], pfx='time_dependency_2.model.')
        mos = float(onet.pool_att_ff(s, x2, 'pool.model.')[0])
    if stages:
        return mos, {'td_x': td_x.numpy(), 'td_y': td_y.numpy(), 'fused': fused, 'idx': idx, 'gap': gap}
    return mos


def forward_spec(sd, args, spec_d, spec_r, dtype=torch.float64, stages=False):
    """The same from the two clips' [48, T] dB spectrograms (segment_specs, NL:2239-2282)."""
    xd, _ = onet.segment_specs(spec_d, args['ms_seg_length'], args['ms_seg_hop_length'], None)
    xr, _ = onet.segment_specs(spec_r, args['ms_seg_length'], args['ms_seg_hop_length'], None)
    return forward_segments(sd, args, xd, xr, dtype, stages)


# -- test pairs ---------------------------------------------------------------------------------------------------------------
def pairs(sr=48000, long_s=50.0):
    """(name, deg int16, ref int16): delayed + noisy, identical, short / long both ways, silent reference, one long pair."""
    rng = np.random.RandomState(11)
    ref = synth.synth_pcm16(0, 10.0, sr)
    d = int(0.03 * sr)
    delayed = np.concatenate([np.zeros(d, np.int16), ref[:-d]]).astype(np.float64) + rng.standard_normal(len(ref)) * 300.0
    out = [('delay_noise', np.clip(delayed, -32768, 32767).astype(np.int16), ref),
           ('identical', ref.copy(), ref),
           ('deg1s_ref10s', synth.synth_pcm16(1, 1.0, sr), ref),
           ('deg10s_ref1s', ref.copy(), synth.synth_pcm16(2, 1.0, sr)),
           ('ref_zero', synth.synth_pcm16(3, 4.0, sr), np.zeros(4 * sr, np.int16))]
    if long_s:
        out.append(('long', synth.synth_pcm16(4, long_s, sr), synth.synth_pcm16(5, long_s + 2.0, sr)))
    return out
