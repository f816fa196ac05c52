"""NISQA_DE (double-ended) on the MI355X: the alignment + fusion kernel against a float64 restatement, the narrow-input second
self-attention, the whole forward against the restated reference forward (tests/de_oracle.py, itself checked against the reference's
NISQA_DE in tests/test_de_host.py), the public predict_csv surface, and determinism."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import de_oracle as DO
from nisqa_amd import synth
from oracle import mel as omel, net as onet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(a, p, f) for a in DO.ALIGNS for p in DO.APPLIES for f in DO.FUSES]


def _engine(args, sd, precision):
    from nisqa_amd.engine import HipNisqaDE
    return HipNisqaDE(args, sd, 'cuda:0', precision=precision)


@pytest.mark.parametrize('align,apply,fuse', COMBOS)
def test_align_fuse_kernel_against_float64(align, apply, fuse):
    from nisqa_amd.engine import BatchPlan
    eng = _engine(DO.de_args(align, apply, fuse), DO.random_de_state_dict(1, fuse), 'f32')
    pairs = [(247, 247), (1, 300), (300, 1), (1300, 1300), (64, 65), (130, 2), (50, 70)] + [(400, 250)] * 40
    B = len(pairs)
    plan = BatchPlan.from_n_wins([p[0] for p in pairs] + [p[1] for p in pairs])
    rng = np.random.RandomState(3)
    x = np.full((plan.total_tok, 64), np.nan, np.float32)        # padding rows are NaN: the kernel must never read them
    for c in range(2 * B):
        x[plan.tok_off[c]:plan.tok_off[c] + plan.n_wins[c]] = rng.standard_normal((plan.n_wins[c], 64))
    tie = 6                                                         # pair 6: every reference row the same vector (exact ties)
    x[plan.tok_off[B + tie]:plan.tok_off[B + tie] + 70] = x[plan.tok_off[B + tie]]
    out, idx = eng.align_fuse(torch.from_numpy(x).cuda(), plan, want_idx=apply == 'hard')
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    idx = idx.cpu().numpy() if idx is not None else None
    F = DO.FUSE_WIDTH[fuse]
    assert np.isfinite(out).all()
    assert (out[:, F:] == 0).all()
    worst = 0.0
    for b, (nx, ny) in enumerate(pairs):
        r0, c0 = plan.tok_off[b], plan.tok_off[B + b]
        xd, xr = x[r0:r0 + nx].astype(np.float64), x[c0:c0 + ny].astype(np.float64)
        want, widx, gap = DO.align_fuse(xd, xr, align, apply, fuse)
        if apply == 'hard':
            k = idx[r0:r0 + nx]
            sure = gap > 1e-5
            assert (k[sure] == widx[sure]).all(), (b, np.nonzero(k[sure] != widx[sure]))
            assert ((k >= 0) & (k < ny)).all()
            if b == tie:
                assert (k == 0).all()                               # torch's argmax: the first maximum
            want = DO.fuse_rows(xd, xr[k], fuse)                    # near-ties: the row of the index the kernel chose
            assert (idx[r0 + nx:plan.tok_off[b + 1]] == -1).all()
        err = float(np.abs(out[r0:r0 + nx, :F] - want).max())
        worst = max(worst, err)
        # 1e-5, or twice what an fp32 evaluation of the same operators is off from float64 (dot-product scores of unit rows reach
        # |s| ~ 30, and the soft weights carry their fp32 rounding)
        fp32, _, _ = DO.align_fuse(xd.astype(np.float32), xr.astype(np.float32), align, apply, fuse)
        tol = max(1e-5, 2.0 * float(np.abs(fp32 - want).max())) if apply == 'soft' else 1e-5
        assert err <= tol, (b, err, tol)
        assert (out[r0 + nx:plan.tok_off[b + 1]] == 0).all()       # padding rows: zeros
    print('align_fuse %s/%s/%s: max |d| %.3g over %d pairs' % (align, apply, fuse, worst, B))


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
@pytest.mark.parametrize('fuse', ['x/y/-', 'x/y'])
def test_narrow_second_self_attention_and_pooling_against_float64(precision, fuse):
    from nisqa_amd.engine import BatchPlan, DE_FEAT_LD
    sd = DO.random_de_state_dict(2, fuse)
    eng = _engine(DO.de_args(fuse=fuse), sd, precision)
    F = DO.FUSE_WIDTH[fuse]
    n = [247, 1, 63, 64, 65, 700]
    plan = BatchPlan.from_n_wins(n)
    rng = np.random.RandomState(4)
    feat = np.zeros((plan.total_tok, DE_FEAT_LD), np.float32)
    for c, k in enumerate(n):
        feat[plan.tok_off[c]:plan.tok_off[c] + k, :F] = rng.standard_normal((k, F))
    got = eng.td2_pool(torch.from_numpy(feat).cuda(), plan).cpu().numpy().reshape(-1)
    s = {k: v.double() for k, v in sd.items() if not k.endswith('num_batches_tracked')}
    for c, k in enumerate(n):
        f = torch.from_numpy(feat[plan.tok_off[c]:plan.tok_off[c] + k, :F]).double()
        x2 = onet.self_attention(s, f, 2, pfx='time_dependency_2.model.')
        want = float(onet.pool_att_ff(s, x2, 'pool.model.')[0])
        assert abs(got[c] - want) <= 2e-4, (precision, c, got[c], want)


def _oracle_pairs(long_s):
    out = []
    for name, d, r in DO.pairs(long_s=long_s):
        sd_ = omel.melspec_db_from_audio(d.astype(np.float32) / np.float32(32768.0), 48000)
        sr_ = omel.melspec_db_from_audio(r.astype(np.float32) / np.float32(32768.0), 48000)
        out.append((name, d, r, sd_, sr_))
    return out


_ORACLE = {}


def _oracle(args, sd, key):
    if key not in _ORACLE:
        ps = _oracle_pairs(50.0)
        res = [DO.forward_spec(sd, args, sd_, sr_, torch.float64, stages=True) for _, _, _, sd_, sr_ in ps]
        _ORACLE[key] = (ps, res)
    return _ORACLE[key]


@pytest.mark.parametrize('precision', ['f32', 'bf16x6', 'f16x4'])
@pytest.mark.parametrize('align,apply,fuse', [('cosine', 'hard', 'x/y/-'), ('dot', 'soft', '+/-')])
def test_end_to_end_against_the_restated_reference(precision, align, apply, fuse):
    args = DO.de_args(align, apply, fuse)
    sd = DO.random_de_state_dict(5, fuse)
    eng = _engine(args, sd, precision)
    ps, res = _oracle(args, sd, (align, apply, fuse))
    B = len(ps)
    want = np.array([m for m, _ in res])
    # from PCM: the whole HIP path, through the file-fed entry and through one 2B-clip plan (with the hard-mode indices)
    items = [(d, 48000) for _, d, _, _, _ in ps] + [(r, 48000) for _, _, r, _, _ in ps]
    got = eng.forward_items(items).cpu().numpy().reshape(-1)
    plan = eng.plan([len(d) for _, d, _, _, _ in ps], [len(r) for _, _, r, _, _ in ps], 48000)
    n_wins = list(plan.n_wins)
    pcm = torch.from_numpy(np.concatenate([y for y, _ in items])).cuda()
    got_plan, idx = eng.forward_pcm(pcm, plan, 48000, want_idx=True)
    assert np.array_equal(got_plan.cpu().numpy().reshape(-1), got)
    err_pcm = np.abs(got - want)
    for b, (name, *_r) in enumerate(ps):
        print('%s %s/%s/%s %-13s hip %.6f oracle %.6f |d| %.2g' % (precision, align, apply, fuse, name, got[b], want[b], err_pcm[b]))
        if apply == 'hard':
            k = idx.cpu().numpy()[plan.tok_off[b]:plan.tok_off[b] + n_wins[b]]
            st = res[b][1]
            flips = np.nonzero(k != st['idx'])[0]
            for f in flips:
                print('   hard-index flip at token %d: hip %d oracle %d, oracle top-2 gap %.3g' % (f, k[f], st['idx'][f], st['gap'][f]))
    assert err_pcm.max() <= 1e-4, err_pcm          # (the repo's PCM parity bar is 1e-3; measured <= 1e-6 here)


def _write_table(d, n=6):
    ps = DO.pairs(long_s=0)
    rows = []
    for k in range(n):
        name, deg, ref = ps[k % len(ps)]
        fd, fr = 'deg_%d.wav' % k, 'ref_%d.wav' % k
        synth.write_wav(os.path.join(d, fd), deg)
        synth.write_wav(os.path.join(d, fr), ref)
        rows.append({'filepath_deg': fd, 'filepath_ref': fr, 'mos': 1.0 + 0.5 * k, 'db': 'db%d' % (k % 2), 'pair': name})
    pd.DataFrame(rows).to_csv(os.path.join(d, 'pairs.csv'), index=False)
    return ps


def test_predict_csv_public_surface(tmp_path, monkeypatch):
    from nisqa_amd.NISQA_model import nisqaModel
    d = str(tmp_path)
    ps = _write_table(d)
    args = DO.de_args()
    sd = DO.random_de_state_dict(6)
    ck = os.path.join(d, 'de.tar')
    torch.save({'args': dict(args, pretrained_model=False, csv_ref='filepath_ref'), 'model_state_dict': sd}, ck)

    def run(bs, exact=False):
        monkeypatch.setenv('NISQA_EXACT_BS', '1' if exact else '0')
        m = nisqaModel({'mode': 'predict_csv', 'pretrained_model': ck, 'data_dir': d, 'csv_file': 'pairs.csv',
                        'csv_deg': 'filepath_deg', 'output_dir': d, 'tr_bs_val': bs, 'tr_num_workers': 0, 'ms_channel': None})
        df = m.predict()
        return m, df
    m1, df1 = run(1)
    _, df64 = run(64)
    _, dfx = run(2, exact=True)
    assert list(df1['filepath_deg']) == ['deg_%d.wav' % k for k in range(6)]
    assert np.array_equal(df1['mos_pred'].to_numpy(), df64['mos_pred'].to_numpy())
    assert np.array_equal(df1['mos_pred'].to_numpy(), dfx['mos_pred'].to_numpy())
    eng = _engine(args, sd, None)
    items = [(ps[k % len(ps)][1], 48000) for k in range(6)] + [(ps[k % len(ps)][2], 48000) for k in range(6)]
    direct = eng.forward_items(items).cpu().numpy().reshape(-1)
    assert np.abs(df1['mos_pred'].to_numpy() - direct).max() <= 1e-6
    m1.ds_val.df['mos'] = pd.read_csv(os.path.join(d, 'pairs.csv'))['mos']
    m1.evaluate(do_print=False)
    assert 'r_p_mean_file' in m1.r
    out_csv = os.path.join(d, 'NISQA_results.csv')
    mine = pd.read_csv(out_csv)
    os.remove(out_csv)
    env = dict(os.environ, NISQA_EXACT_BS='0')
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'run_predict.py'), '--mode', 'predict_csv', '--pretrained_model', ck,
                           '--data_dir', d, '--csv_file', 'pairs.csv', '--csv_deg', 'filepath_deg', '--csv_ref', 'filepath_ref',
                           '--output_dir', d, '--bs', '4'], env=env, cwd=ROOT, timeout=600)
    cli = pd.read_csv(out_csv)
    assert np.array_equal(cli['mos_pred'].to_numpy(), mine['mos_pred'].to_numpy())


def test_determinism_same_batch_and_two_streams():
    args = DO.de_args('cosine', 'soft', 'x/y/-')
    eng = _engine(args, DO.random_de_state_dict(8), None)
    ps = DO.pairs(long_s=0)
    items = [(d, 48000) for _, d, _ in ps] + [(r, 48000) for _, _, r in ps]
    a = eng.forward_items(items).cpu().numpy()
    b = eng.forward_items(items).cpu().numpy()
    assert np.array_equal(a, b)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c = eng.forward_items(items)
    with torch.cuda.stream(s2):
        e = eng.forward_items(items)
    torch.cuda.synchronize()
    assert np.array_equal(a, c.cpu().numpy()) and np.array_equal(a, e.cpu().numpy())
