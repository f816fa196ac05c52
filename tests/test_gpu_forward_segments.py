"""The inner operator model(x, n_wins) on the MI355X for the StandardCNN + BiLSTM family (nisqa_tts.tar, the CNN-LSTM-AVG recipe and
its max variant) and for NISQA_DE, and the double-ended dataset item: the segment-fed StandardCNN kernels against the frame-fed ones
(bit for bit), inert padding, the network against the oracle on tensors the test builds itself, and NISQA_DE against the restated
float64 reference (tests/de_oracle.py)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import de_oracle as DO
import helpers
import lstm_pool_oracle as LO
from nisqa_amd import synth
from oracle import mel as omel, net as onet

pytestmark = pytest.mark.gpu
PRECISIONS = ['f32', 'bf16x3', 'bf16x6', 'f16x4', 'f16x3']
# tests/test_gpu_parity.py's TOL[precision][0]: the bound on feat20 against the oracle network
TOL_FEAT = {'f32': 2e-4, 'bf16x3': 1e-3, 'bf16x6': 2e-4, 'f16x4': 2e-4, 'f16x3': 2e-4}
HOP = 480                                           # 10 ms at 48 kHz

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _tts_engine(precision):
    from nisqa_amd.engine import HipNisqa
    return _cached(('tts', precision),
                   lambda: HipNisqa(dict(helpers.TTS_ARGS), helpers.random_state_dict(9, 'NISQA_TTS'), 'cuda:0', precision=precision))


def _clip_of(seed, n_wins, seg_hop):
    """int16 PCM whose spectrogram has exactly n_wins segments at seg_hop"""
    t = 14 + 1 + seg_hop * (n_wins - 1)
    return synth.synth_pcm16(seed, (t - 1) * HOP / 48000.0 + 0.1)[:(t - 1) * HOP]


def _gather(spec_tm, n_wins, seg_hop):
    """SpeechQualityDataset.__getitem__'s index gather: [T, 48] -> [n_wins, 1, 48, 15]"""
    idx = seg_hop * np.arange(n_wins)[:, None] + np.arange(15)[None, :]
    return np.transpose(spec_tm[idx], (0, 2, 1))[:, None]


def _poison_allocator(byte):
    """Hand the caching allocator a large block full of ``byte``: the next torch.empty of the large pool is carved from it."""
    torch.cuda.synchronize()
    junk = torch.empty(1 << 30, dtype=torch.uint8, device='cuda:0')
    junk.fill_(byte)
    del junk


def _fill(shape, fill):
    x = np.empty(shape, np.float32)
    x[...] = 3e38 if fill == 'big' else fill
    if fill == 'big':
        x[..., 1::2] = -3e38
    return x


# -- segment-fed equals frame-fed ---------------------------------------------------------------------------------------------------
N_WINS = [1, 2, 3, 4, 5, 31, 32, 33, 87]             # one workgroup of four segments, partial last groups, the 32-token boundary
L_SEG = 90                                          # one clip has n_wins == L - 3, the rest have padding


def _frame_batch():
    """GPU mel (unclamped) of clips with exactly N_WINS segments -> (mel device, floor device, plan, the valid segments per clip on
    the host, cut from the spectrogram clamped at the clip's floor)"""
    def make():
        eng = _tts_engine('f32')                    # the mel kernel is the same in every mode
        pcm = [_clip_of(700 + i, n, 1) for i, n in enumerate(N_WINS)]
        plan = eng.plan([len(p) for p in pcm], 48000)
        assert list(plan.n_wins) == N_WINS
        mel, floor = eng.mel(torch.from_numpy(np.concatenate(pcm)).to(eng.device), plan, 48000, clamp=False)
        torch.cuda.synchronize()
        mel_h, floor_h = mel.cpu().numpy(), floor.cpu().numpy()
        segs = []
        for b, n in enumerate(N_WINS):
            spec = np.maximum(mel_h[plan.frame_off[b]:plan.frame_off[b + 1]], floor_h[b])
            segs.append(_gather(spec, n, 1))
        return mel, floor, plan, segs
    return _cached('frame_batch', make)


def _segment_tensor(segs, L, fill=0.0):
    x = _fill((len(segs), L, 1, 48, 15), fill)
    for b, s in enumerate(segs):
        x[b, :len(s)] = s
    return torch.from_numpy(x)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_segment_fed_standard_cnn_equals_frame_fed_bit_for_bit(precision):
    """The same window reaches the same LDS planes ahead of an unchanged instruction stream: feat20 of the segment-fed kernel must
    be the frame-fed kernel's, bit for bit, on every valid row; padding rows stay zero."""
    from nisqa_amd.engine import BatchPlan
    eng = _tts_engine(precision)
    mel, floor, plan, segs = _frame_batch()
    feat_a = eng.cnn_std(mel, floor, plan)
    x = _segment_tensor(segs, L_SEG).to(eng.device)
    splan = BatchPlan.from_n_wins(N_WINS)
    assert list(splan.tok_off) == list(plan.tok_off)
    feat_b = eng.cnn_std_segments(x, splan)
    torch.cuda.synchronize()
    valid = torch.from_numpy(plan.token_index()).to(eng.device)
    assert feat_a.shape == feat_b.shape == (plan.total_tok, 20)
    a, b = feat_a[valid], feat_b[valid]
    assert torch.isfinite(a).all() and a.abs().max() > 0
    diff = (a != b).nonzero()
    print(precision, 'rows', a.shape[0], 'differing elements', diff.shape[0], 'max |d|', float((a - b).abs().max()))
    assert torch.equal(a, b), diff[:8]
    pad = torch.ones(plan.total_tok, dtype=torch.bool, device=eng.device)
    pad[valid] = False
    assert (feat_b[pad] == 0).all() and (feat_a[pad] == 0).all()


@pytest.mark.parametrize('precision', PRECISIONS)
def test_padding_segments_and_stale_memory_are_inert(precision):
    """Segments k >= n_wins are never read and every scratch row that is read was written: forward_segments gives identical bits
    with zeros, NaN and +-3e38 in the padding segments, each on a poisoned allocator."""
    eng = _tts_engine(precision)
    _, _, _, segs = _frame_batch()
    res = []
    for fill, byte in ((0.0, 0x00), (float('nan'), 0xFF), ('big', 0xFF)):
        x = _segment_tensor(segs, L_SEG, fill)
        _poison_allocator(byte)
        res.append(eng.forward_segments(x, N_WINS).cpu().numpy())
    assert res[0].shape == (len(N_WINS), 1) and np.isfinite(res[0]).all()
    for r in res[1:]:
        assert np.array_equal(r.view(np.uint32), res[0].view(np.uint32)), (r, res[0])


# -- against the oracle network ---------------------------------------------------------------------------------------------------------
ORACLE_WINS = [1, 329, 40, 100]
L_ORACLE = 330


def _oracle_set(pool, weights):
    """(args, sd, x [B, L, 1, 48, 15], per clip (reference output, reference feat20)) from ORACLE spectrograms"""
    def make():
        if weights == 'real':
            args, sd = helpers.load_checkpoint(helpers.find_weights('nisqa_tts.tar'))
        elif pool == 'last_step_bi':
            args, sd = dict(helpers.TTS_ARGS), helpers.random_state_dict(9, 'NISQA_TTS')
        else:
            args, sd = dict(LO.POOL_ARGS[pool]), LO.state_dict()
        assert args['pool'] == pool
        hop = int(args['ms_seg_hop_length'])
        xs, refs = [], []
        for i, n in enumerate(ORACLE_WINS):
            pcm = _clip_of(800 + i, n, hop)
            spec = omel.melspec_db_from_audio(pcm.astype(np.float32) / np.float32(32768.0), 48000, fmax=float(args['ms_fmax']))
            x, nw = onet.segment_specs(spec, 15, hop, L_ORACLE)
            assert nw == n
            xs.append(x)
            if pool == 'last_step_bi':
                out, st = onet.predict_from_melspec(sd, args, spec, return_stages=True)
            else:
                out, st = LO.predict(sd, args, spec, return_stages=True)
            refs.append((np.asarray(out), np.asarray(st['feat'])))
        return args, sd, torch.stack(xs, 0), refs
    return _cached(('oracle', pool, weights), make)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('pool,weights', [('last_step_bi', 'rand'), ('avg', 'rand'), ('max', 'rand'), ('last_step_bi', 'real')])
def test_model_forward_matches_the_oracle_network(pool, weights, precision, monkeypatch):
    """NISQA(...)(x, n_wins) for the three poolings of the StandardCNN + BiLSTM family on segment tensors cut from ORACLE
    spectrograms (no HIP mel stage involved): feat20 within tests/test_gpu_parity.py's TOL[precision][0], the output within 1e-3."""
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import BatchPlan
    if weights == 'real' and helpers.find_weights('nisqa_tts.tar') is None:
        pytest.skip('real checkpoint not on this machine')
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    args, sd, x, refs = _oracle_set(pool, weights)
    model = NL.NISQA(**LO.model_kwargs(args))
    model.load_state_dict(sd, strict=True)
    model.bind_args(args)
    out = model(x.cuda(), torch.tensor(ORACLE_WINS)).cpu().numpy()
    eng = model.engine()
    assert eng.precision == precision and eng.arch == {'last_step_bi': 1, 'avg': 2, 'max': 3}[pool] and out.shape == (len(ORACLE_WINS), 1)
    plan = BatchPlan.from_n_wins(ORACLE_WINS)
    feat = eng.cnn_std_segments(x.to(eng.device).contiguous(), plan).cpu().numpy()
    worst_feat = worst_out = 0.0
    for b, (ref_out, ref_feat) in enumerate(refs):
        t0 = int(plan.tok_off[b])
        worst_feat = max(worst_feat, float(np.abs(feat[t0:t0 + ORACLE_WINS[b]] - ref_feat).max()))
        worst_out = max(worst_out, float(np.abs(out[b] - ref_out).max()))
    print(pool, weights, precision, 'max |d| feat20 %.3g, output %.3g' % (worst_feat, worst_out))
    assert worst_feat < TOL_FEAT[precision] and worst_out < 1e-3


# -- NISQA_DE ---------------------------------------------------------------------------------------------------------------------------
L_DE = 250


def _de_pairs():
    """DO.pairs(long_s=6.0) as oracle spectrograms and valid segment stacks: [(name, xd [n_x, 1, 48, 15], xr [n_y, ...], spec_d, spec_r)]"""
    def make():
        out = []
        for name, d, r in DO.pairs(long_s=6.0):
            sd_ = omel.melspec_db_from_audio(d.astype(np.float32) / np.float32(32768.0), 48000)
            sr_ = omel.melspec_db_from_audio(r.astype(np.float32) / np.float32(32768.0), 48000)
            xd, _ = onet.segment_specs(sd_, 15, 4, None)
            xr, _ = onet.segment_specs(sr_, 15, 4, None)
            out.append((name, xd.numpy(), xr.numpy(), sd_, sr_))
        assert any(len(p[1]) != len(p[2]) for p in out) and max(max(len(p[1]), len(p[2])) for p in out) < L_DE
        return out
    return _cached('de_pairs', make)


def _de_tensor(ps, fill):
    x = _fill((len(ps), L_DE, 2, 48, 15), fill)
    for b, (_, xd, xr, _, _) in enumerate(ps):
        x[b, :len(xd), 0:1] = xd
        x[b, :len(xr), 1:2] = xr
    return torch.from_numpy(x)


@pytest.mark.parametrize('precision', ['f32', 'bf16x6', 'f16x4'])
@pytest.mark.parametrize('align,apply,fuse', [('cosine', 'hard', 'x/y/-'), ('dot', 'soft', '+/-')])
def test_double_ended_forward_against_the_restated_reference(precision, align, apply, fuse, monkeypatch):
    """NISQA_DE(...)(x [B, L, 2, 48, 15], n_wins [B, 2]) against the float64 restatement of the reference forward, within the 1e-4
    of tests/test_gpu_de.py::test_end_to_end_against_the_restated_reference; the fill of either channel's padding segments is inert."""
    from nisqa_amd import NISQA_lib as NL
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    args, sd = DO.de_args(align, apply, fuse), DO.random_de_state_dict(5, fuse)
    ps = _de_pairs()
    want = _cached(('de_want', align, apply, fuse),
                   lambda: np.array([DO.forward_spec(sd, args, sd_, sr_, torch.float64) for _, _, _, sd_, sr_ in ps]))
    n_wins = np.array([[len(xd), len(xr)] for _, xd, xr, _, _ in ps])
    model = NL.NISQA_DE(**DO.model_kwargs(args))
    model.load_state_dict(sd, strict=True)
    model.bind_args(args)
    res = []
    for fill in (0.0, float('nan'), 'big'):
        res.append(model(_de_tensor(ps, fill).cuda(), torch.from_numpy(n_wins)).cpu().numpy())
    assert model.engine().precision == precision and res[0].shape == (len(ps), 1)
    err = np.abs(res[0].reshape(-1) - want)
    for b, (name, *_r) in enumerate(ps):
        print('%s %s/%s/%s %-13s n_wins %s hip %.6f oracle %.6f |d| %.2g' % (precision, align, apply, fuse, name, n_wins[b], res[0][b, 0],
                                                                          want[b], err[b]))
    assert np.isfinite(res[0]).all() and err.max() <= 1e-4, err
    for r in res[1:]:
        assert np.array_equal(r.view(np.uint32), res[0].view(np.uint32)), (r, res[0])


# -- double-ended dataset item ----------------------------------------------------------------------------------------------------------
def test_double_ended_dataset_item_and_model_forward_equal_predict(tmp_path):
    from nisqa_amd.NISQA_model import nisqaModel
    d = str(tmp_path)
    durs = [(1.3, 2.1), (2.6, 0.7), (0.5, 0.5)]
    rows = []
    for k, (sd_, sr_) in enumerate(durs):
        synth.write_wav(os.path.join(d, 'deg_%d.wav' % k), synth.synth_pcm16(900 + k, sd_))
        synth.write_wav(os.path.join(d, 'ref_%d.wav' % k), synth.synth_pcm16(910 + k, sr_))
        rows.append({'filepath_deg': 'deg_%d.wav' % k, 'filepath_ref': 'ref_%d.wav' % k})
    pd.DataFrame(rows).to_csv(os.path.join(d, 'pairs.csv'), index=False)
    args, sd = DO.de_args(), DO.random_de_state_dict(6)
    ck = os.path.join(d, 'de.tar')
    torch.save({'args': dict(args, pretrained_model=False, csv_ref='filepath_ref'), 'model_state_dict': sd}, ck)
    m = nisqaModel({'mode': 'predict_csv', 'pretrained_model': ck, 'data_dir': d, 'csv_file': 'pairs.csv', 'csv_deg': 'filepath_deg',
                    'output_dir': d, 'tr_bs_val': 2, 'tr_num_workers': 0, 'ms_channel': None})
    pred = m.predict()['mos_pred'].to_numpy()
    ds, max_length = m.ds_val, args['ms_max_segments']
    ref_ds = ds.ref_view()
    assert ds.double_ended and not ref_ds.double_ended
    for i, (sd_, sr_) in enumerate(durs):
        x, y, (index, n_wins) = ds[i]
        assert tuple(x.shape) == (max_length, 2, 48, 15) and x.dtype == torch.float32 and index == i and np.isnan(y).all()
        assert isinstance(n_wins, np.ndarray) and n_wins.shape == (2,)
        want_n = [onet.n_wins_of(1 + int(round(s * 48000)) // HOP) for s in (sd_, sr_)]
        assert list(n_wins) == want_n, (list(n_wins), want_n)
        xr, _, (_, nr) = ref_ds[i]
        assert int(nr) == n_wins[1] and torch.equal(x[:, 1:2], xr)
        assert (x[n_wins[0]:, 0] == 0).all() and (x[n_wins[1]:, 1] == 0).all() and x[:n_wins[0], 0].abs().max() > 0
        out = m.model(x[None], n_wins[None]).cpu().numpy().reshape(-1)
        print('item %d n_wins %s model(x, n_wins) %.7f predict %.7f' % (i, list(n_wins), out[0], pred[i]))
        assert abs(float(out[0]) - float(pred[i])) <= 1e-6
