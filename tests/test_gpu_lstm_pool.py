"""CNN-LSTM-AVG / CNN-LSTM-MAX on the MI355X: the fused average / max pooling of the BiLSTM (nisqa_lstm_pool, arch 2 / 3 of
nisqa_predict_batch) against the committed reference fixtures, the oracle network, the kernel's own sequence and float64; mode 0 against
nisqa_lstm_laststep; the layout contracts; the drop-in surface.  Reads only tests/golden, never the reference tree."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import helpers
import lstm_pool_oracle as LO
from nisqa_amd import synth

pytestmark = pytest.mark.gpu
ROOT = helpers.ROOT
PRECISIONS = ['f32', 'bf16x3', 'bf16x6', 'f16x4', 'f16x3']
POOLS = ['avg', 'max']
MEL_TOL = 1e-3                  # dB, as tests/test_gpu_parity.py
TOL = {'f32': 2e-4, 'bf16x3': 1e-3, 'bf16x6': 2e-4, 'f16x4': 2e-4, 'f16x3': 2e-4}     # feat20 / BiLSTM states, as test_gpu_parity.py
EPS = float(np.finfo(np.float32).eps)


def _engine(args, sd, precision=None):
    from nisqa_amd.engine import HipNisqa
    return HipNisqa(args, sd, precision=precision)


def _upload(eng, pcm):
    plan = eng.plan([len(p) for p in pcm], 48000)
    dev = torch.from_numpy(np.concatenate(pcm).astype(np.float32) / np.float32(32768.0)).to(eng.device)
    return dev, plan


def _run(eng, pcm, arch=None):
    """mel -> StandardCNN -> BiLSTM + pooling as separate stages -> (plan, feat, out, seq, pooled) on the host"""
    dev, plan = _upload(eng, pcm)
    mel, floor = eng.mel(dev, plan, 48000, clamp=False)
    feat = eng.cnn_std(mel, floor, plan)
    out, seq, pooled = eng.lstm(feat, plan, want_seq=True, arch=arch, want_pooled=True)
    torch.cuda.synchronize()
    return plan, feat.cpu().numpy(), out.cpu().numpy(), seq.cpu().numpy(), pooled.cpu().numpy(), (dev, mel, floor, feat)


@pytest.fixture(scope='module')
def clips():
    return [LO.clip_pcm(i) for i in range(len(LO.CLIPS))]


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('pool', POOLS)
def test_stages_and_fixture(pool, precision, clips):
    g = helpers.golden('net_lstm_%s_rand.npz' % pool)
    args, sd = LO.POOL_ARGS[pool], LO.state_dict()
    eng = _engine(args, sd, precision)
    assert eng.arch == {'avg': 2, 'max': 3}[pool] and eng.seg_hop == 3 and eng.precision == precision
    plan, feat, out_st, seq, pooled, (dev, mel, floor, _) = _run(eng, clips)
    assert list(plan.n_wins) == list(g['n_wins']) and int(plan.n_wins[-1]) == 1300
    out = eng.forward_pcm(dev, plan, 48000).cpu().numpy()
    assert np.array_equal(out, out_st)                           # the whole-batch entry point runs the same kernels
    idx = torch.from_numpy(np.repeat(np.arange(plan.n_clips), plan.T)).to(mel.device)
    mel_h = torch.maximum(mel, floor[idx][:, None]).cpu().numpy()
    worst = {'mel': 0.0, 'feat': 0.0, 'td': 0.0, 'pooled': 0.0, 'out': 0.0}
    for n in range(plan.n_clips):
        spec = mel_h[plan.frame_off[n]:plan.frame_off[n + 1]].T
        worst['mel'] = max(worst['mel'], np.abs(spec - LO.clip_spec(clips[n], args)).max())
        ref_out, st = LO.predict(sd, args, spec, return_stages=True)          # GPU mel -> oracle network
        nw, t0 = int(plan.n_wins[n]), int(plan.tok_off[n])
        worst['feat'] = max(worst['feat'], np.abs(feat[t0:t0 + nw] - st['feat'].numpy()).max())
        worst['td'] = max(worst['td'], np.abs(seq[t0:t0 + nw] - st['td'].numpy()).max())
        worst['pooled'] = max(worst['pooled'], np.abs(pooled[n] - st['pooled'].numpy()).max())
        worst['out'] = max(worst['out'], np.abs(out[n] - ref_out).max())
    err_fix = np.abs(out - g['out']).max()
    print(pool, precision, 'stage max|d|', worst, 'vs reference fixture', err_fix)
    assert worst['mel'] < MEL_TOL and worst['feat'] < TOL[precision] and worst['td'] < TOL[precision]
    assert worst['pooled'] < TOL[precision]
    assert worst['out'] < 1e-3 and err_fix < 1e-3


@pytest.mark.parametrize('precision', ['bf16x6', 'f32'])
def test_fused_pooling_against_the_kernels_own_sequence(precision, clips):
    """max: the pooled vector IS the maximum of the valid rows of seq, bit for bit.  avg: against the float64 mean of the same fp32 rows,
    no further off, clip by clip, than CPU torch fp32 seq.sum(0) / n (the reference's arithmetic) -- 1.5 x that floor at most, the
    1300-segment clip included.  out: the float64 linear layer of the pooled vector within a few fp32 ulps."""
    sd = LO.state_dict()
    w = sd['pool.model.linear.weight'].numpy().astype(np.float64).reshape(-1)
    b = float(sd['pool.model.linear.bias'].numpy()[0])
    for pool in POOLS:
        eng = _engine(LO.POOL_ARGS[pool], sd, precision)
        plan, _, out, seq, pooled, _ = _run(eng, clips)
        for n in range(plan.n_clips):
            nw, t0 = int(plan.n_wins[n]), int(plan.tok_off[n])
            rows = seq[t0:t0 + nw]
            if pool == 'max':
                assert np.array_equal(pooled[n].view(np.uint32), rows.max(0).view(np.uint32)), n
            else:
                exact = rows.astype(np.float64).sum(0) / nw
                cpu = (torch.from_numpy(rows).sum(0) / nw).numpy()
                err_gpu = np.abs(pooled[n].astype(np.float64) - exact).max()
                err_cpu = np.abs(cpu.astype(np.float64) - exact).max()
                floor = max(err_cpu, 0.5 * EPS * np.abs(exact).max())       # an exact sum still rounds once
                print('avg clip %d n %d: |gpu - f64| %.3g  |torch fp32 - f64| %.3g' % (n, nw, err_gpu, err_cpu))
                assert err_gpu <= 1.5 * floor, (n, nw, err_gpu, err_cpu)
            ref = float(np.dot(w, pooled[n].astype(np.float64)) + b)
            scale = float(np.dot(np.abs(w), np.abs(pooled[n].astype(np.float64))) + abs(b))
            assert abs(float(out[n, 0]) - ref) <= 6 * EPS * scale, (pool, n, out[n, 0], ref)


def test_negative_control_the_three_poolings_differ(clips):
    """On the fixture weights avg, max and last_step_bi give outputs more than 1e-3 apart: no test here can pass through the wrong
    pooling."""
    eng = _engine(LO.LSTM_AVG_ARGS, LO.state_dict(), 'bf16x6')
    outs = {arch: _run(eng, clips, arch=arch)[2].reshape(-1) for arch in (1, 2, 3)}
    for a, b in ((1, 2), (1, 3), (2, 3)):
        d = np.abs(outs[a] - outs[b]).max()
        print('arch %d vs %d: max|d| %.4g' % (a, b, d))
        assert d > 1e-3, (a, b, d)
    for pool, arch in (('avg', 2), ('max', 3)):
        assert np.abs(outs[arch] - helpers.golden('net_lstm_%s_rand.npz' % pool)['out'].reshape(-1)).max() < 1e-3


def test_mode_0_is_nisqa_lstm_laststep_bit_for_bit():
    from nisqa_amd import lib
    from nisqa_amd.engine import _ptr
    sd = helpers.random_state_dict(9, 'NISQA_TTS')
    eng = _engine(dict(helpers.TTS_ARGS), sd, 'bf16x6')
    assert eng.arch == 1
    pcm = [synth.synth_pcm16(60 + i, s) for i, s in enumerate((0.16, 1.0, 3.7, 0.4, 10.0))]
    dev, plan = _upload(eng, pcm)
    mel, floor = eng.mel(dev, plan, 48000, clamp=False)
    feat = eng.cnn_std(mel, floor, plan)
    d = plan.to(eng.device)
    res = {}
    for name in ('laststep', 'pool0'):
        hfin = torch.full((plan.n_clips, 256), float('nan'), device=eng.device)
        seq = torch.zeros((plan.total_tok, 256), device=eng.device)
        out = torch.full((plan.n_clips, 1), float('nan'), device=eng.device)
        args = (_ptr(feat), _ptr(d['tok_off']), _ptr(d['n_wins']), plan.n_clips, _ptr(eng.td_w))
        tail = (_ptr(hfin), _ptr(seq), _ptr(out), eng._stream())
        rc = eng.lib.nisqa_lstm_laststep(*args, *tail) if name == 'laststep' else \
            eng.lib.nisqa_lstm_pool(*args, lib.LSTM_POOL_LAST_STEP_BI, *tail)
        assert rc == 0
        torch.cuda.synchronize()
        res[name] = [t.cpu().numpy().view(np.uint32) for t in (out, seq, hfin)]
    for a, b in zip(res['laststep'], res['pool0']):
        assert np.array_equal(a, b)


def _same_bits(what, a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


@pytest.mark.parametrize('pool', POOLS)
def test_layout_contracts(pool, clips):
    """Bit-identical outputs: each clip alone vs in the batch; a 0xFF-filled workspace; two batches in flight on two streams; a batch
    of 160 clips, whose 320 (clip, direction) workgroups outnumber the device's CUs."""
    eng = _engine(LO.POOL_ARGS[pool], LO.state_dict(), 'bf16x6')
    pcm = clips[:-1] + [synth.synth_pcm16(80, 0.6)]
    dev, plan = _upload(eng, pcm)
    batch = eng.forward_pcm(dev, plan, 48000).cpu().numpy()
    for n, p in enumerate(pcm):
        d1, p1 = _upload(eng, [p])
        _same_bits('%s clip %d alone' % (pool, n), eng.forward_pcm(d1, p1, 48000).cpu().numpy()[0], batch[n])
    ws = eng._ws[torch.cuda.current_stream(eng.device).cuda_stream]
    ws.fill_(0xFF)
    _same_bits('%s workspace 0xFF' % pool, eng.forward_pcm(dev, plan, 48000).cpu().numpy(), batch)
    pcm2 = [synth.synth_pcm16(90 + i, 0.3 + 0.05 * i) for i in range(12)]
    dev2, plan2 = _upload(eng, pcm2)
    solo2 = eng.forward_pcm(dev2, plan2, 48000).cpu().numpy()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        o1 = eng.forward_pcm(dev, plan, 48000)
    with torch.cuda.stream(s2):
        o2 = eng.forward_pcm(dev2, plan2, 48000)
    torch.cuda.synchronize()
    _same_bits('%s stream 1' % pool, o1.cpu().numpy(), batch)
    _same_bits('%s stream 2' % pool, o2.cpu().numpy(), solo2)
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    many = [synth.synth_pcm16(200 + (i % 16), 0.2 + 0.01 * (i % 16)) for i in range(160)]
    assert 2 * len(many) > cus
    dm, pm = _upload(eng, many)
    big = eng.forward_pcm(dm, pm, 48000).cpu().numpy()
    d16, p16 = _upload(eng, many[:16])
    small = eng.forward_pcm(d16, p16, 48000).cpu().numpy()
    for i in range(160):
        _same_bits('%s clip %d of 160' % (pool, i), big[i], small[i % 16])


@pytest.mark.parametrize('pool', POOLS)
def test_drop_in_run_predict(tmp_path, pool):
    """run_predict.py with a checkpoint of the recipe: predict_file, predict_dir and predict_csv rows equal the engine's outputs;
    nisqaModel.evaluate() runs on the predict_csv result."""
    from nisqa_amd.NISQA_model import nisqaModel
    args, sd = dict(LO.POOL_ARGS[pool], pretrained_model=False), LO.state_dict()
    d = str(tmp_path)
    ck = os.path.join(d, 'lstm_%s.tar' % pool)
    torch.save({'args': args, 'model_state_dict': sd}, ck)
    durs = [0.16, 0.9, 2.3, 4.0, 1.1, 0.5]
    pcm = [synth.synth_pcm16(300 + i, s) for i, s in enumerate(durs)]
    names = ['f%d.wav' % i for i in range(len(pcm))]
    for nm, p in zip(names, pcm):
        synth.write_wav(os.path.join(d, nm), p, 48000)
    eng = _engine(args, sd)
    dev, plan = _upload(eng, pcm)
    want = dict(zip(names, eng.forward_pcm(dev, plan, 48000).cpu().numpy().reshape(-1)))
    rows = []
    for i, nm in enumerate(names):
        rows.append({'deg': nm, 'mos': 1.0 + 0.6 * i, 'db': 'db%d' % (i % 2)})
    pd.DataFrame(rows).to_csv(os.path.join(d, 'files.csv'), index=False)
    run = lambda *a: subprocess.check_call([sys.executable, os.path.join(ROOT, 'run_predict.py'), '--pretrained_model', ck] + list(a),
                                           cwd=ROOT, timeout=600)
    run('--mode', 'predict_dir', '--data_dir', d, '--output_dir', d, '--bs', '4')
    got = pd.read_csv(os.path.join(d, 'NISQA_results.csv'))
    assert sorted(got['deg']) == sorted(names)
    for _, r in got.iterrows():
        assert abs(r['mos_pred'] - want[r['deg']]) <= 1e-6, (r['deg'], r['mos_pred'], want[r['deg']])
    os.remove(os.path.join(d, 'NISQA_results.csv'))
    run('--mode', 'predict_file', '--deg', os.path.join(d, names[2]), '--output_dir', d)
    got = pd.read_csv(os.path.join(d, 'NISQA_results.csv'))
    assert len(got) == 1 and abs(got['mos_pred'][0] - want[names[2]]) <= 1e-6
    os.remove(os.path.join(d, 'NISQA_results.csv'))
    run('--mode', 'predict_csv', '--data_dir', d, '--csv_file', 'files.csv', '--csv_deg', 'deg', '--output_dir', d, '--bs', '2')
    got = pd.read_csv(os.path.join(d, 'NISQA_results.csv'))
    assert list(got['deg']) == names
    for _, r in got.iterrows():
        assert abs(r['mos_pred'] - want[r['deg']]) <= 1e-6
    m = nisqaModel({'mode': 'predict_csv', 'pretrained_model': ck, 'data_dir': d, 'csv_file': 'files.csv', 'csv_deg': 'deg',
                    'output_dir': None, 'tr_bs_val': 2, 'tr_num_workers': 0, 'ms_channel': None})
    df = m.predict()
    assert np.abs(df['mos_pred'].to_numpy() - got['mos_pred'].to_numpy()).max() <= 1e-6
    m.evaluate(do_print=False)
    assert 'r_p_mean_file' in m.r
