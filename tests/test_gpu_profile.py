"""Per-segment score profile on the MI355X: nisqa_pool_profile against the float64 restatement (tests/profile_oracle.py, itself checked
against the reference's PoolAttFF / PoolAvg in tests/test_profile_host.py) on the engine's own token rows, and the profile's consistency
with the score the existing chain returns -- bit-equal scores, sum_t weights * local within a bar -- for the CNN-SA-AP models in three
precisions, the StandardCNN + BiLSTM model with pool=avg, NISQA_DE, and the nisqaModel.profile() table.

Every bar is max(1e-5, 2 x how far a float32 CPU evaluation of the same restatement is from its float64 evaluation), per clip, the rule
tests/test_gpu_de.py uses for its soft weights; it is computed from the rows the kernel read, never from the kernel's results."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import helpers
import lstm_pool_oracle as LO
import profile_oracle as PO
from nisqa_amd import synth

pytestmark = pytest.mark.gpu


def _engine(args, sd, precision=None):
    from nisqa_amd.engine import HipNisqa
    return HipNisqa(args, sd, 'cuda:0', precision=precision)


def _nan_padding(x, plan):
    """x with every row no clip's token owns set to NaN: the kernel must never read them"""
    keep = torch.zeros(plan.total_tok, dtype=torch.bool, device=x.device)
    keep[torch.from_numpy(plan.token_index()).to(x.device)] = True
    return torch.where(keep[:, None], x, torch.full((), float('nan'), device=x.device)).contiguous()


def _check_kernel(eng, sd, heads, x, plan, what):
    w, loc = eng.pool_profile(x, plan)
    torch.cuda.synchronize()
    w, loc, rows = w.cpu().numpy(), loc.cpu().numpy(), x.cpu().numpy()
    H = 1 if heads == 'avg' else len(heads)
    assert w.shape == loc.shape == (plan.total_tok, H)
    assert np.isfinite(w).all() and np.isfinite(loc).all()
    worst = {'weights': 0.0, 'local': 0.0}
    for c in range(plan.n_clips):
        r0, n, r1 = int(plan.tok_off[c]), int(plan.n_wins[c]), int(plan.tok_off[c + 1])
        assert np.isfinite(rows[r0:r0 + n]).all() and np.isnan(rows[r0 + n:r1]).all()
        w64, l64, bar_w, bar_l, _, _ = PO.bars(sd, rows[r0:r0 + n], heads)
        err_w, err_l = float(np.abs(w[r0:r0 + n] - w64).max()), float(np.abs(loc[r0:r0 + n] - l64).max())
        print('%s clip %d n %4d: weights |d| %.3g (bar %.3g)  local |d| %.3g (bar %.3g)' % (what, c, n, err_w, bar_w, err_l, bar_l))
        worst['weights'], worst['local'] = max(worst['weights'], err_w), max(worst['local'], err_l)
        assert err_w <= bar_w and err_l <= bar_l, (what, c, n, err_w, bar_w, err_l, bar_l)
        assert np.abs(w[r0:r0 + n].astype(np.float64).sum(0) - 1.0).max() <= 1e-5
        assert (w[r0 + n:r1] == 0).all() and (loc[r0 + n:r1] == 0).all()          # padding rows: exact zeros
    print('%s: worst weights |d| %.3g, worst local |d| %.3g' % (what, worst['weights'], worst['local']))
    return w, loc


@pytest.mark.parametrize('model', ['NISQA', 'NISQA_DIM'])
def test_kernel_against_float64_on_the_engines_own_rows(model):
    """Clip lengths at the edges of the 64-token layout and of the 256-thread token loop, one token and the 1300-token cap, one head
    and five; x is the engine's own self-attention output with NaN in every padding row."""
    from nisqa_amd.engine import BatchPlan
    args = dict(synth.DIM_ARGS) if model == 'NISQA_DIM' else dict(synth.MOS_ARGS)
    sd = synth.random_state_dict(7 if model == 'NISQA_DIM' else 8, model)
    eng = _engine(args, sd, 'f32')
    plan = BatchPlan.from_n_wins([1, 63, 64, 65, 130, 1300])
    idx = torch.from_numpy(plan.token_index()).to(eng.device)
    feat = torch.zeros((plan.total_tok, 384), device=eng.device)
    feat[idx] = torch.randn((len(idx), 384), device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
    x = _nan_padding(eng.td(feat, plan), plan)
    heads = PO.DIM_HEADS if model == 'NISQA_DIM' else PO.MOS_HEADS
    w, loc = _check_kernel(eng, sd, heads, x, plan, 'PoolAttFF %d head(s)' % len(heads))
    w2, loc2 = eng.pool_profile(x, plan)                           # no atomics, fixed orders: the same bits again
    assert np.array_equal(w2.cpu().numpy().view(np.uint32), w.view(np.uint32))
    assert np.array_equal(loc2.cpu().numpy().view(np.uint32), loc.view(np.uint32))


def test_kernel_against_float64_pool_avg():
    from nisqa_amd.engine import BatchPlan
    sd = LO.state_dict()
    eng = _engine(LO.LSTM_AVG_ARGS, sd, 'f32')
    plan = BatchPlan.from_n_wins([1, 64, 65, 700])
    idx = torch.from_numpy(plan.token_index()).to(eng.device)
    feat = torch.zeros((plan.total_tok, 20), device=eng.device)
    feat[idx] = torch.randn((len(idx), 20), device=eng.device, generator=torch.Generator(eng.device).manual_seed(4))
    _, seq = eng.lstm(feat, plan, want_seq=True)
    w, _ = _check_kernel(eng, sd, 'avg', _nan_padding(seq, plan), plan, 'PoolAvg')
    for c, n in enumerate(plan.n_wins):
        r0 = int(plan.tok_off[c])
        assert (w[r0:r0 + n, 0] == np.float32(1.0) / np.float32(n)).all()


def _clips():
    return [synth.synth_pcm16(70, 0.4), synth.synth_pcm16(71, 1.0), synth.synth_pcm16(72, 2.37), synth.synth_pcm16(73, 0.15)]


def _check_scores(prof, plan, sd, heads, want_scores, what):
    """scores bit-equal to the plain call's; per clip sum_t weights * local against them within the bar; padding rows exact zeros"""
    torch.cuda.synchronize()
    sc, emb, w, loc = (t.cpu().numpy() for t in (prof.scores, prof.embed, prof.weights, prof.local))
    assert np.array_equal(sc.view(np.uint32), want_scores.cpu().numpy().view(np.uint32)), what
    worst = 0.0
    for c in range(plan.n_clips):
        r0, n, r1 = int(plan.tok_off[c]), int(plan.n_wins[c]), int(plan.tok_off[c + 1])
        assert (emb[r0 + n:r1] == 0).all() and (w[r0 + n:r1] == 0).all() and (loc[r0 + n:r1] == 0).all()
        _, _, _, _, _, bar = PO.bars(sd, emb[r0:r0 + n], heads)
        got = (w[r0:r0 + n].astype(np.float64) * loc[r0:r0 + n].astype(np.float64)).sum(0)
        err = float(np.abs(got - sc[c].astype(np.float64)).max())
        print('%s clip %d n %3d: |sum w * local - score| %.3g (bar %.3g)' % (what, c, n, err, bar))
        worst = max(worst, err)
        assert err <= bar, (what, c, err, bar)
    print('%s: worst |sum w * local - score| %.3g' % (what, worst))
    return sc, emb, w, loc


@pytest.mark.parametrize('precision', ['f32', 'bf16x6', 'f16x4'])
def test_profile_pcm_is_consistent_with_the_score(precision):
    args, sd = dict(synth.DIM_ARGS), synth.random_state_dict(7, 'NISQA_DIM')
    eng = _engine(args, sd, precision)
    pcm = _clips()
    plan = eng.plan([len(p) for p in pcm], 48000)
    dev = torch.from_numpy(np.concatenate(pcm)).to(eng.device)      # int16 PCM, as the predict loop hands it over
    prof = eng.profile_pcm(dev, plan, 48000)
    assert tuple(prof.embed.shape) == (plan.total_tok, 64) and tuple(prof.weights.shape) == (plan.total_tok, 5)
    first = _check_scores(prof, plan, sd, PO.DIM_HEADS, eng.forward_pcm(dev, plan, 48000), 'NISQA_DIM ' + precision)
    again = eng.profile_pcm(dev, plan, 48000)
    for a, b in zip(first, (again.scores, again.embed, again.weights, again.local)):
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().view(np.uint32))       # two calls: identical bits, every output


def test_profile_segments_scores_are_forward_segments():
    args, sd = dict(synth.MOS_ARGS), synth.random_state_dict(8, 'NISQA')
    eng = _engine(args, sd)
    from nisqa_amd.engine import BatchPlan
    x = torch.randn((2, 5, 1, 48, 15), generator=torch.Generator().manual_seed(1)) * 10.0 - 40.0
    n_wins = [5, 3]
    prof = eng.profile_segments(x, n_wins)
    _check_scores(prof, BatchPlan.from_n_wins(n_wins), sd, PO.MOS_HEADS, eng.forward_segments(x, n_wins), 'NISQA segments')


def test_lstm_avg_profile():
    sd = LO.state_dict()
    eng = _engine(LO.LSTM_AVG_ARGS, sd)
    pcm = _clips()
    plan = eng.plan([len(p) for p in pcm], 48000)
    dev = torch.from_numpy(np.concatenate(pcm)).to(eng.device)
    prof = eng.profile_pcm(dev, plan, 48000)
    assert tuple(prof.embed.shape) == (plan.total_tok, 256) and tuple(prof.weights.shape) == (plan.total_tok, 1)
    _, _, w, _ = _check_scores(prof, plan, sd, 'avg', eng.forward_pcm(dev, plan, 48000), 'CNN-LSTM-AVG')
    for c, n in enumerate(plan.n_wins):
        r0 = int(plan.tok_off[c])
        assert (w[r0:r0 + n, 0] == np.float32(1.0) / np.float32(n)).all()          # exactly 1 / n


def test_double_ended_profile_audio():
    import de_oracle as DO
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import BatchPlan
    args, sd = DO.de_args('cosine', 'hard', 'x/y/-'), DO.random_de_state_dict(5)
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    m.load_state_dict(sd, strict=True)
    f32 = lambda p: torch.from_numpy(p.astype(np.float32) / np.float32(32768.0))
    deg, ref = [f32(synth.synth_pcm16(1, 1.0)), f32(synth.synth_pcm16(3, 2.0))], [f32(synth.synth_pcm16(2, 1.7)), f32(synth.synth_pcm16(4, 0.8))]
    pad = lambda ys: torch.stack([torch.cat([y, torch.full((max(map(len, ys)) - len(y),), float('nan'))]) for y in ys])
    ld, lr = [len(y) for y in deg], [len(y) for y in ref]
    res = m.profile_audio(pad(deg), pad(ref), 48000, ld, lr)
    eng = m.engine()
    plan = eng.plan(ld, lr, 48000)
    dplan = BatchPlan.from_n_wins(plan.n_wins[:2])
    scores = m.forward_audio(pad(deg), pad(ref), 48000, ld, lr)
    assert np.array_equal(res.scores.cpu().numpy().view(np.uint32), scores.cpu().numpy().view(np.uint32))
    _, idx = eng.forward_pcm(torch.cat(deg + ref).to(eng.device), plan, 48000, want_idx=True)
    idx = idx.cpu().numpy()
    L = int(plan.n_wins[:2].max())
    assert res.n_wins.tolist() == plan.n_wins[:2].tolist() and tuple(res.aligned_to.shape) == (2, L) and res.heads == ('mos',)
    assert tuple(res.weights.shape) == tuple(res.local.shape) == (2, L, 1) and tuple(res.embed.shape) == (2, L, 64)
    w, loc, emb, al = (t.cpu().numpy() for t in (res.weights, res.local, res.embed, res.aligned_to))
    for b in range(2):
        n, r0 = int(plan.n_wins[b]), int(dplan.tok_off[b])
        assert np.array_equal(al[b, :n], idx[r0:r0 + n]) and (al[b, n:] == -1).all()
        assert ((al[b, :n] >= 0) & (al[b, :n] < plan.n_wins[2 + b])).all()
        assert (w[b, n:] == 0).all() and (loc[b, n:] == 0).all() and (emb[b, n:] == 0).all()
        _, _, _, _, _, bar = PO.bars(sd, emb[b, :n], PO.MOS_HEADS)
        err = abs(float((w[b, :n, 0].astype(np.float64) * loc[b, :n, 0]).sum()) - float(res.scores[b, 0]))
        print('NISQA_DE pair %d n %d: |sum w * local - score| %.3g (bar %.3g)' % (b, n, err, bar))
        assert err <= bar
    assert np.allclose(res.t_start.numpy()[:3], [0.0, 0.04, 0.08]) and np.allclose(res.t_end.numpy()[:2], [0.15, 0.19])
    assert not res.weights.requires_grad and not res.scores.requires_grad


def test_model_profile_table(tmp_path):
    from nisqa_amd.NISQA_model import nisqaModel
    d = str(tmp_path)
    pcm = {'a.wav': synth.synth_pcm16(80, 1.3), 'b.wav': synth.synth_pcm16(81, 0.6)}
    for name, p in pcm.items():
        synth.write_wav(os.path.join(d, name), p, 48000)
    ck = helpers.random_checkpoint('nisqa.tar', d)
    m = nisqaModel({'mode': 'predict_dir', 'pretrained_model': ck, 'data_dir': d, 'output_dir': d, 'tr_bs_val': 2, 'tr_num_workers': 0,
                    'ms_channel': None})
    pred = m.predict().set_index('deg')
    df = m.profile()
    eng = m.model.engine()
    names = list(m.ds_val.df['deg'])
    plan = eng.plan([len(pcm[f]) for f in names], 48000)
    assert len(df) == int(plan.n_wins.sum())
    cols = ['deg', 'seg', 't_start', 't_end'] + [c for h in ('mos', 'noi', 'dis', 'col', 'loud') for c in ('w_' + h, 'local_' + h)]
    assert list(df.columns) == cols
    emb = eng.profile_pcm(torch.from_numpy(np.concatenate([pcm[f] for f in names])).to(eng.device), plan, 48000).embed.cpu().numpy()
    sd = synth.random_state_dict(7, 'NISQA_DIM')
    for k, f in enumerate(names):
        rows = df[df['deg'] == f]
        n, r0 = int(plan.n_wins[k]), int(plan.tok_off[k])
        assert len(rows) == n and list(rows['seg']) == list(range(n))
        assert np.allclose(rows['t_start'], 0.04 * np.arange(n)) and np.allclose(rows['t_end'] - rows['t_start'], 0.15)
        _, _, _, _, _, bar = PO.bars(sd, emb[r0:r0 + n], PO.DIM_HEADS)
        for h in ('mos', 'noi', 'dis', 'col', 'loud'):
            err = abs(float((rows['w_' + h] * rows['local_' + h]).sum()) - float(pred.loc[f, h + '_pred']))
            print('%s %s: |sum w * local - %s_pred| %.3g (bar %.3g)' % (f, h, h, err, bar))
            assert err <= bar
    back = pd.read_csv(os.path.join(d, 'NISQA_profile.csv'))
    assert list(back.columns) == cols and len(back) == len(df) and np.allclose(back['w_mos'], df['w_mos'], rtol=0, atol=1e-12)
