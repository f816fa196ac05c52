"""GPU tests of what NISQA_DIM's bias-aware loss and mixed-rate training batches add to the training step:

* nisqa_mse_loss_heads (one cubic mapping per clip AND head) against float64 autograd, and bit for bit against nisqa_mse_loss
  where every head gets the same row;
* the CNN-SA-AP step with ``bias [B, 5, 4]`` (fused block and operator by operator, 'f32' and the default precision) against
  float64 autograd through the oracle plus the per-head loss restatement of tests/bias_dim_case.py; ``[B, 4]`` against the same
  table broadcast to ``[B, 5, 4]``;
* HipTrainerLSTM with ``bias [B, 1, 4]``;
* a step on a batch of 48 kHz and 16 kHz clips from PCM (``step_groups``), both trainers, against the oracles on the
  spectrograms the mel kernel returns per group;
* ``nisqaModel.train()`` on a corpus that mixes rates, with the bias-aware loss on the five heads."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import bias_dim_case as case
import helpers
import lstm_train_oracle as LT
from nisqa_amd import synth

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

DEV = 'cuda:0'


def _p(t):
    return t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _conv_bias(k):
    return k.startswith('cnn.model.conv') and k.endswith('.bias')


def _worst(grads, want):
    """max over the tensors of max|got - want| / max(1e-3, max|want|); conv biases (zero under train-mode BatchNorm) left out"""
    worst, wk = 0.0, None
    for k, gr in grads.items():
        if _conv_bias(k):
            continue
        w = np.asarray(want[k])
        e = float(np.abs(np.asarray(gr) - w).max()) / max(1e-3, float(np.abs(w).max()))
        if e > worst:
            worst, wk = e, k
    return worst, wk


# ---- 1. the loss operator --------------------------------------------------------------------------------------------------
def _loss_case(B, H, labelled=True):
    g = torch.Generator().manual_seed(100 * B + H)
    y_hat = 3.0 + torch.randn(B, H, generator=g)
    y = 3.0 + torch.randn(B, H, generator=g)
    if B > 1 and H > 1:
        y[:, 3] = float('nan')                               # a head without any label: loss term 0, gradient 0
        y[2, :] = float('nan')                               # a clip without any label
    elif not labelled:
        y[:] = float('nan')
    h, b = torch.arange(H, dtype=torch.float32), torch.arange(B, dtype=torch.float32)
    rows = torch.stack([0.1 * h - 0.2, 1 - 0.05 * h, torch.full((H,), 0.02), -0.001 * h], 1)          # distinct per head
    bias = rows[None] + (0.01 * b[:, None, None] * torch.tensor([1.0, -1.0, 0.5, 0.1]))                # ... and per clip
    return y_hat, y, bias.contiguous()


@pytest.mark.parametrize('B,H,labelled', [(6, 5, True), (1, 1, True), (1, 1, False), (7, 5, True)])
def test_per_head_loss_operator_matches_float64_autograd(B, H, labelled):
    from nisqa_amd import lib
    L = lib.load()
    y_hat, y, bias = _loss_case(B, H, labelled)
    yh64 = y_hat.double().requires_grad_(True)
    want = case.per_head_loss(yh64, y.double(), bias.double())
    dwant = torch.autograd.grad(want, yh64)[0] if want.requires_grad else torch.zeros(B, H, dtype=torch.float64)
    yd, td, bd = y_hat.to(DEV), y.to(DEV), bias.to(DEV)
    loss, dyh = torch.full((1 + H,), 7.0, device=DEV), torch.full((B, H), 7.0, device=DEV)
    lib.check(L.nisqa_mse_loss_heads(_p(yd), _p(td), _p(bd), B, H, _p(loss), _p(dyh), _st()), 'nisqa_mse_loss_heads')
    torch.cuda.synchronize()
    print('per-head loss', (B, H), 'loss', float(loss[0]), 'want', float(want.detach()), 'max|d - want|', float((dyh.cpu().double() - dwant).abs().max()))
    want = want.detach()
    assert abs(float(loss[0]) - float(want)) < 1e-5
    assert float((dyh.cpu().double() - dwant).abs().max()) < 1e-6
    assert float(loss[1:].sum()) == pytest.approx(float(loss[0]), abs=1e-5)
    if B > 1 and H > 1:
        assert float(loss[1 + 3]) == 0 and (dyh[:, 3] == 0).all() and (dyh[2] == 0).all() and (dyh[0, :3] != 0).all()
    if not labelled:
        assert float(loss[0]) == 0 and (dyh == 0).all()
    # the map matters: without it the loss is another number (so the comparison above is about the coefficients)
    if labelled:
        assert abs(float(case.per_head_loss(y_hat.double(), y.double())) - float(want)) > 1e-3


@pytest.mark.parametrize('B,H', [(6, 5), (1, 1), (7, 5)])
def test_per_head_loss_operator_with_one_row_for_all_heads_equals_the_shared_form_bit_for_bit(B, H):
    """nisqa_mse_loss_heads with [B, H, 4] rows that repeat one [B, 4] table over the heads = nisqa_mse_loss with that table: the
    kernel is the same, it sums sequentially, and only the address of the four coefficients differs."""
    from nisqa_amd import lib
    L = lib.load()
    y_hat, y, bias = _loss_case(B, H)
    shared = bias[:, 0].contiguous()                         # differs between clips
    yd, td = y_hat.to(DEV), y.to(DEV)
    out = []
    for entry, rows in ((L.nisqa_mse_loss, shared), (L.nisqa_mse_loss_heads, shared[:, None, :].expand(B, H, 4).contiguous())):
        rd = rows.to(DEV)
        loss, dyh = torch.zeros(1 + H, device=DEV), torch.zeros(B, H, device=DEV)
        lib.check(entry(_p(yd), _p(td), _p(rd), B, H, _p(loss), _p(dyh), _st()), 'mse loss')
        torch.cuda.synchronize()
        out.append((loss.cpu(), dyh.cpu()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert float(out[0][0][0]) > 0


# ---- 2. the CNN-SA-AP step ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dim_case():
    """The 'dim' batch of tests/golden with the explicit dropout masks of the masked oracle test (test_gpu_train.py), bias rows
    that differ between heads and between clips, and the float64 reference: autograd through oracle.train.forward_train and the
    per-head loss.  Computed once, shared, read only."""
    import make_golden_train as mk
    from oracle import net as onet, train as otrain
    g = helpers.golden('train_dim.npz')
    args = dict(synth.DIM_ARGS)
    args.update({'cnn_dropout': 0.0, 'td_sa_dropout': 0.0, 'pool_att_dropout': 0.0})
    sd = synth.random_state_dict(int(g['seed_sd']), 'NISQA_DIM')
    specs, y = mk.batch(int(g['seed_batch']), int(g['n_clips']), 5)
    segs = torch.cat([onet.segment_specs(s, 15, 4, None)[0] for s in specs])
    n_wins = [int(v) for v in g['n_wins']]
    S, B = sum(n_wins), len(n_wins)
    rng = np.random.default_rng(1)
    drop = lambda shape, p: ((rng.random(shape) >= p).astype(np.float32) / (1 - p))
    mk_, mo = {}, {}
    for key, c in (('cnn_d1', 32), ('cnn_d2', 64), ('cnn_d3', 64), ('cnn_d4', 64)):
        mk_[key] = drop((S, c), 0.2)
        mo[key] = torch.as_tensor(mk_[key])[:, :, None, None]
    tok = np.concatenate(([0], np.cumsum(n_wins)))
    for l in range(2):
        pk = []
        for b, n in enumerate(n_wins):
            m = drop((n, n), 0.1)
            mo[(b, 'td%d_p' % l)] = torch.as_tensor(m)
            pk.append(m.reshape(-1))
        mk_['td%d_p' % l] = np.concatenate(pk)
        for t in ('1', 'f', '2'):
            m = drop((S, 64), 0.1)
            mk_['td%d_%s' % (l, t)] = m
            for b in range(B):
                mo[(b, 'td%d_%s' % (l, t))] = torch.as_tensor(m[tok[b]:tok[b + 1]])
    h, b = np.arange(5, dtype=np.float32), np.arange(B, dtype=np.float32)
    rows = np.stack([0.1 * h - 0.2, 1 - 0.05 * h, np.full(5, 0.02, np.float32), -0.001 * h], 1)
    bias = (rows[None] + 0.03 * b[:, None, None] * np.array([1.0, -1.0, 0.5, 0.1], np.float32)).astype(np.float32)
    assert bias.shape == (B, 5, 4) and np.abs(bias[:, 0] - bias[:, 1]).max(-1).min() > 0 and np.abs(bias[0] - bias[1]).max() > 0
    sd64 = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in sd.items()}
    keys = otrain.param_keys(sd64)
    for k in keys:
        sd64[k] = sd64[k].double().requires_grad_(True)
    y_hat = otrain.forward_train(sd64, args, segs.double(), n_wins, mo)[0]
    loss = case.per_head_loss(y_hat, torch.as_tensor(y).double(), torch.as_tensor(bias).double())
    grads = dict(zip(keys, (t.numpy() for t in torch.autograd.grad(loss, [sd64[k] for k in keys]))))
    return dict(args=args, sd=sd, specs=specs, y=y, masks=mk_, bias=bias, loss=float(loss.detach()), y_hat=y_hat.detach().numpy(),
                grads=grads)


@pytest.mark.parametrize('precision', ['f32', None])
@pytest.mark.parametrize('fused', ['1', '0'])
def test_training_step_with_one_bias_mapping_per_head_matches_float64_oracle(fused, precision, monkeypatch):
    from nisqa_amd.train import HipTrainer
    c = _dim_case()
    monkeypatch.setenv('NISQA_HIP_TRAIN_FUSED_TD', fused)
    tr = HipTrainer(c['args'], c['sd'], DEV, lr=1e-3, precision=precision)
    assert tr.fused_td == (fused == '1')
    loss = tr.step_spec(c['specs'], c['y'], masks=c['masks'], bias=c['bias'])
    torch.cuda.synchronize()
    worst, wk = _worst({k: v.numpy() for k, v in tr.grads().items()}, c['grads'])
    dy = float(np.abs(tr.last['y_hat'].cpu().numpy() - c['y_hat']).max())
    print('per-head bias step, fused', fused, tr.precision, ': loss', float(loss), 'want', c['loss'], 'max|d y_hat|', dy,
          'worst relative gradient error', worst, wk)
    assert float(loss) == pytest.approx(c['loss'], rel=1e-4)
    assert worst < 1e-3, (worst, wk)


@pytest.mark.parametrize('fused', ['1', '0'])
def test_training_step_with_shared_rows_equals_the_same_rows_given_per_head(fused, monkeypatch):
    """``bias [B, 4]`` and the same table broadcast to ``[B, 5, 4]`` are the same arithmetic through the two entries; the fused
    block adds its loss and gradients with atomics, so the two runs are held to the project's bound for one arithmetic in two
    summation orders: 2e-4 of a tensor's largest entry (1e-3 at least, as in the segment-resident vs implicit comparison)."""
    from nisqa_amd.train import HipTrainer
    c = _dim_case()
    monkeypatch.setenv('NISQA_HIP_TRAIN_FUSED_TD', fused)
    shared = np.ascontiguousarray(c['bias'][:, 2])
    res = []
    for bias in (shared, np.ascontiguousarray(np.broadcast_to(shared[:, None, :], (len(shared), 5, 4)))):
        tr = HipTrainer(c['args'], c['sd'], DEV, lr=1e-3)
        loss = tr.step_spec(c['specs'], c['y'], masks=c['masks'], bias=bias)
        torch.cuda.synchronize()
        res.append((float(loss), tr.last['y_hat'].cpu().numpy().copy(), {k: v.numpy() for k, v in tr.grads().items()}))
    (l0, y0, g0), (l1, y1, g1) = res
    worst, wk = _worst(g1, g0)
    print('shared rows vs the same rows per head, fused', fused, ': loss', l0, l1, 'max|d y_hat|', float(np.abs(y1 - y0).max()),
          'worst relative gradient difference', worst, wk)
    assert l1 == pytest.approx(l0, rel=2e-4)
    assert np.abs(y1 - y0).max() < 2e-4 * np.abs(y0).max()
    assert worst < 2e-4, (worst, wk)
    assert abs(l0 - c['loss']) > 1e-3 * c['loss']             # (and these rows are not the per-head rows of the test above)


# ---- 3. HipTrainerLSTM: one head ----------------------------------------------------------------------------------------------
def test_lstm_training_step_takes_bias_rows_in_both_forms():
    from nisqa_amd.train_lstm import HipTrainerLSTM
    args = dict(LT.AVG_ARGS)
    sd = synth.random_state_dict(31, 'NISQA_TTS')
    specs, y = LT.batch(71)
    segs, n_wins = LT.segments(specs, args)
    masks = LT.random_masks(72, int(n_wins.sum()), 0.2)
    bias = np.tile(np.array([[0.1, 0.9, 0.02, -0.001]], np.float32), (len(specs), 1))
    bias[:, 0] += 0.05 * np.arange(len(specs), dtype=np.float32)
    ref = LT.train_step(sd, args, segs, n_wins, y, masks=masks, bias=bias)
    got = []
    for form in (bias, bias[:, None, :]):
        tr = HipTrainerLSTM(args, sd, DEV, lr=1e-3)
        loss = tr.step_spec(specs, y, masks=masks, bias=form)
        torch.cuda.synchronize()
        assert float(loss) == pytest.approx(ref['loss'], rel=1e-4)
        assert np.abs(tr.last['y_hat'].cpu().numpy() - ref['y_hat']).max() < 1e-4
        worst, wk = _worst({k: v.numpy() for k, v in tr.grads().items()}, ref['grads'])
        print('LSTM step, bias', form.shape, ': loss', float(loss), 'want', ref['loss'], 'worst relative gradient error', worst, wk)
        assert worst < 1e-3, (worst, wk)
        for k, v in tr.state_dict().items():
            if 'running' in k:
                assert np.abs(v.numpy() - ref['bufs'][k]).max() < 2e-4 * max(1.0, np.abs(ref['bufs'][k]).max()), k
        got.append(float(loss))
    assert got[0] == pytest.approx(got[1], rel=1e-5)
    with pytest.raises(ValueError):
        HipTrainerLSTM(args, sd, DEV, lr=1e-3).step_spec(specs, y, masks=masks, bias=np.zeros((len(specs), 5, 4), np.float32))


# ---- 4. a batch of two sample rates from PCM ----------------------------------------------------------------------------------
GROUPS = ((48000, (0.16, 0.7, 1.3)), (16000, (0.4, 1.0)))        # the 0.16 s clip is ONE segment


def _mixed_rate_step(tr, n_heads):
    """-> (loss, groups' spectrograms [48, T] with the per-clip floor applied on the host, labels): the step runs on the PCM, the
    oracle on what the mel kernel returns for each group alone."""
    groups, specs, seed = [], [], 300
    for sr, secs in GROUPS:
        pcm = [synth.synth_pcm16(seed + i, s, sr=sr) for i, s in enumerate(secs)]
        seed += len(secs)
        plan = tr.eng.plan([len(p) for p in pcm], sr)
        dev = tr.eng.pcm16_to_f32(torch.from_numpy(np.concatenate(pcm)).to(DEV))
        groups.append((dev, plan, sr))
        mel, floor = tr.eng.mel(dev, plan, sr, clamp=False)
        mel, floor = mel.cpu().numpy(), floor.cpu().numpy()
        for b in range(plan.n_clips):
            specs.append(np.maximum(mel[plan.frame_off[b]:plan.frame_off[b + 1]], floor[b]).T.copy())
    y = np.random.default_rng(5).uniform(1, 5, (len(specs), n_heads)).astype(np.float32)
    y[1, 0] = np.nan
    loss = tr.step_groups(groups, y)
    torch.cuda.synchronize()
    return float(loss), specs, y


def test_mixed_rate_step_from_pcm_matches_oracle():
    from nisqa_amd.train import HipTrainer
    from oracle import net as onet, train as otrain
    args = dict(synth.DIM_ARGS)
    args.update({'cnn_dropout': 0.0, 'td_sa_dropout': 0.0, 'pool_att_dropout': 0.0})
    sd = synth.random_state_dict(7, 'NISQA_DIM')
    tr = HipTrainer(args, sd, DEV, lr=1e-3)
    loss, specs, y = _mixed_rate_step(tr, 5)
    segs, n_wins = zip(*[onet.segment_specs(s, 15, 4, None) for s in specs])
    assert [s.shape[1] for s in specs] == [17, 71, 131, 41, 101] and list(n_wins) == [1, 15, 30, 7, 22]
    assert list(tr.L) == list(n_wins)
    ref = otrain.train_step(sd, args, torch.cat(segs), list(n_wins), y)
    worst, wk = _worst({k: v.numpy() for k, v in tr.grads().items()}, ref['grads'])
    dy = float(np.abs(tr.last['y_hat'].cpu().numpy() - ref['y_hat']).max())
    print('mixed-rate step: loss', loss, 'want', ref['loss'], 'max|d y_hat|', dy, 'worst relative gradient error', worst, wk)
    assert loss == pytest.approx(ref['loss'], rel=1e-4)
    assert dy < 1e-4                                          # in clip order: pins the permutation
    assert worst < 1e-3, (worst, wk)
    for k, v in tr.state_dict().items():
        if 'running' in k:
            want = ref['sd'][k].numpy()
            assert np.abs(v.numpy() - want).max() < 2e-4 * max(1.0, np.abs(want).max()), k


def test_mixed_rate_lstm_step_from_pcm_matches_oracle():
    from nisqa_amd.train_lstm import HipTrainerLSTM
    args = dict(LT.AVG_ARGS, cnn_dropout=0.0)
    sd = synth.random_state_dict(31, 'NISQA_TTS')
    tr = HipTrainerLSTM(args, sd, DEV, lr=1e-3)
    loss, specs, y = _mixed_rate_step(tr, 1)
    segs, n_wins = LT.segments(specs, args)
    assert list(n_wins) == [1, 19, 39, 9, 29] and list(tr.L) == list(n_wins)
    ref = LT.train_step(sd, args, segs, n_wins, y)
    worst, wk = _worst({k: v.numpy() for k, v in tr.grads().items()}, ref['grads'])
    dy = float(np.abs(tr.last['y_hat'].cpu().numpy() - ref['y_hat']).max())
    print('mixed-rate LSTM step: loss', loss, 'want', ref['loss'], 'max|d y_hat|', dy, 'worst relative gradient error', worst, wk)
    assert loss == pytest.approx(ref['loss'], rel=1e-4)
    assert dy < 1e-4
    assert worst < 1e-3, (worst, wk)
    for k, v in tr.state_dict().items():
        if 'running' in k:
            assert np.abs(v.numpy() - ref['bufs'][k]).max() < 2e-4 * max(1.0, np.abs(ref['bufs'][k]).max()), k


def test_one_group_takes_the_step_pcm_path(monkeypatch):
    """step_groups with one group is step_pcm itself: the same call with the same arguments, no mel call of its own."""
    from nisqa_amd.train import HipTrainer
    args = dict(synth.DIM_ARGS)
    tr = HipTrainer(args, synth.random_state_dict(7, 'NISQA_DIM'), DEV, lr=1e-3)
    pcm = [synth.synth_pcm16(i, 0.5 + 0.3 * i) for i in range(3)]
    plan = tr.eng.plan([len(p) for p in pcm], 48000)
    dev = tr.eng.pcm16_to_f32(torch.from_numpy(np.concatenate(pcm)).to(DEV))
    y = np.random.default_rng(0).uniform(1, 5, (3, 5)).astype(np.float32)
    seen = []
    real = tr.step_pcm
    monkeypatch.setattr(tr, 'step_pcm', lambda *a, **k: (seen.append((a, k)), real(*a, **k))[1])
    mels = []
    real_mel = tr.eng.mel
    monkeypatch.setattr(tr.eng, 'mel', lambda *a, **k: (mels.append(1), real_mel(*a, **k))[1])
    loss = tr.step_groups([(dev, plan, 48000)], y)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and len(seen) == 1 and len(mels) == 1
    (a, k), = seen
    assert a[0] is dev and a[1] is plan and a[2] == 48000 and a[3] is y and not k


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------------
def test_train_loop_with_mixed_rates_and_per_head_bias_loss(tmp_path, capsys, monkeypatch):
    """nisqaModel(args).train() for NISQA_DIM with tr_bias_mapping: first_order on a tiny corpus of 16 kHz and 48 kHz files in two
    databases, three epochs; tr_bias_min_r = -1 starts the bias update after the first epoch."""
    import pandas as pd
    from nisqa_amd.NISQA_model import nisqaModel
    from nisqa_amd.engine import HipNisqa
    from nisqa_amd.train import HipTrainer
    rng = np.random.default_rng(14)
    d = tmp_path / 'corpus'
    d.mkdir()
    rows, rate_of = [], {}
    for db, n in (('TRAIN_A', 7), ('TRAIN_B', 6), ('VAL_A', 5)):
        for i in range(n):
            name = '%s_%d.wav' % (db, i)
            sr = 16000 if (len(rows) % 3 == 1) else 48000
            rate_of[name] = sr
            synth.write_wav(str(d / name), synth.synth_pcm16(400 + len(rows), float(rng.uniform(0.5, 1.4)), sr=sr), sr)
            rows.append({'db': db, 'filepath_deg': name, **{t: float(rng.uniform(1, 5)) for t in ('mos', 'noi', 'dis', 'col', 'loud')}})
    pd.DataFrame(rows).to_csv(d / 'files.csv', index=False)
    args = dict(synth.DIM_ARGS)
    args.update({'name': 'tiny_bias', 'data_dir': str(d), 'output_dir': str(tmp_path / 'out'), 'pretrained_model': False,
                 'csv_file': 'files.csv', 'csv_con': None, 'csv_deg': 'filepath_deg', 'csv_mos_train': 'mos',
                 'csv_mos_val': 'mos', 'csv_db_train': ['TRAIN_A', 'TRAIN_B'], 'csv_db_val': ['VAL_A'], 'tr_epochs': 3,
                 'tr_early_stop': 20, 'tr_bs': 4, 'tr_bs_val': 4, 'tr_lr': 1e-3, 'tr_lr_patience': 15, 'tr_num_workers': 2,
                 'tr_parallel': False, 'tr_ds_to_memory': False, 'tr_ds_to_memory_workers': 0, 'tr_device': None,
                 'tr_checkpoint': 'every_epoch', 'tr_verbose': 1, 'tr_bias_mapping': 'first_order', 'tr_bias_min_r': -1.0,
                 'tr_bias_anchor_db': None, 'ms_channel': None})
    torch.manual_seed(3)
    nm = nisqaModel(args)
    # the batches of the run, from the seed (trainloop.train draws one permutation per epoch from this generator): at least one
    # batch of every epoch holds both rates
    rates = np.array([rate_of[os.path.basename(f)] for f in nm.ds_train.df['filepath_deg']])
    assert len(rates) == 13 and set(rates) == {16000, 48000}
    perm = np.random.default_rng(int(torch.initial_seed()) & 0xffffffff)
    expect_groups = []
    for _ in range(3):
        order = perm.permutation(13)
        expect_groups += [len(set(rates[order[s:s + 4]])) for s in range(0, 13, 4)]
    assert len(expect_groups) == 12 and all(max(expect_groups[e * 4:e * 4 + 4]) == 2 for e in range(3))
    seen = []
    real = HipTrainer.step_groups

    def spy(self, groups, y, masks=None, bias=None):
        seen.append((len(groups), [sr for _, _, sr in groups], None if bias is None else np.array(bias, copy=True), np.array(y, copy=True)))
        return real(self, groups, y, masks=masks, bias=bias)

    monkeypatch.setattr(HipTrainer, 'step_groups', spy)
    nm.train()
    out = capsys.readouterr().out
    assert '--> start training' in out and '--> Training done.' in out and '--> bias updated' in out
    assert all(out.count('ep %d sec' % e) == 1 for e in (1, 2, 3))
    assert [n for n, _, _, _ in seen] == expect_groups
    assert all(sorted(srs) == [16000, 48000] for n, srs, _, _ in seen if n == 2)
    for step, (n, _, bias, y) in enumerate(seen):
        assert bias.shape == (len(y), 5, 4) and bias.dtype == np.float32 and y.shape == (len(y), 5)
        if step < 4:                                          # first epoch: the identity for every head
            assert (bias == np.array([0, 1, 0, 0], np.float32)).all()
        else:                                                 # then each head's own line per database
            assert np.abs(bias[:, 0] - bias[:, 1]).max() > 0 and np.abs(bias[:, :, :2] - np.array([0, 1], np.float32)).max() > 0
            assert (bias[:, :, 2:] == 0).all()
    run_dir = tmp_path / 'out' / nm.runname
    hist = pd.read_csv(run_dir / (nm.runname + '__results.csv'))
    assert len(hist) == 3 and np.isfinite(hist['loss'].astype(float)).all()
    for e in (1, 2, 3):
        c = torch.load(str(run_dir / (nm.runname + '__ep_%03d.tar' % e)), map_location='cpu', weights_only=False)
        assert c['epoch'] == e and c['model_name'] == 'NISQA_DIM'
        assert int(c['model_state_dict']['cnn.model.bn1.num_batches_tracked']) == 4 * e
        HipNisqa(c['args'], c['model_state_dict'], DEV)
