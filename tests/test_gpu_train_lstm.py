"""StandardCNN + BiLSTM training on the GPU (nisqa_amd/train_lstm.py, csrc/train_lstm.hip, the StandardCNN layer 1 of
csrc/train.hip): operators against float64 autograd, the whole step against the reference's own train-mode fixtures
(tests/golden/make_golden_train_lstm.py), with explicit dropout masks against tests/lstm_train_oracle.py, and the training
loop end to end."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import lstm_train_oracle as LT
from nisqa_amd import synth
from oracle import net as onet

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _L():
    from nisqa_amd import lib
    return lib, lib.load()


def _p(t):
    return t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max()) / max(1e-12, float(np.abs(want).max()))


# ---- layer 1: conv1 + BatchNorm + ReLU + pool_first (+ dropout) ------------------------------------------------------------
def _layer1_inputs(hop=3):
    specs, _ = LT.batch(61, [15, 40, 97])
    T = np.array([s.shape[1] for s in specs])
    n_wins = np.ceil((T - 14) / hop).astype(np.int64)
    mel = _dev(np.concatenate([s.T for s in specs], 0))
    frame_off = _dev(np.concatenate(([0], np.cumsum(T))), torch.int32)
    seg_off = _dev(np.concatenate(([0], np.cumsum(n_wins))), torch.int32)
    floor = torch.full((len(specs),), -3.0e38, dtype=torch.float32, device=DEV)
    segs = torch.cat([onet.segment_specs(s, 15, hop)[0] for s in specs], 0).double()
    return mel, frame_off, seg_off, floor, len(specs), int(n_wins.sum()), hop, segs


@pytest.mark.parametrize('with_drop', [False, True])
def test_layer1_std_pool_matches_autograd(with_drop):
    lib, L = _L()
    mel, frame_off, seg_off, floor, B, S, hop, segs = _layer1_inputs()
    rng = np.random.default_rng(5)
    w = rng.uniform(-0.3, 0.3, (16, 1, 3, 3))
    b = rng.uniform(-0.5, 0.5, 16)
    gamma, beta = rng.uniform(0.5, 1.5, 16), rng.uniform(-0.3, 0.3, 16)
    drop = ((rng.random((S, 16)) >= 0.3) / 0.7) if with_drop else None
    mom = torch.zeros(54, dtype=torch.float64, device=DEV)
    sums = torch.zeros(32, dtype=torch.float64, device=DEV)
    rm, rv = torch.zeros(16, device=DEV), torch.ones(16, device=DEV)
    mr = torch.empty(32, device=DEV)
    y = torch.empty(S, 192, 16, device=DEV)
    arg = torch.empty(S, 192, 16, dtype=torch.int32, device=DEV)
    wd, bd, gd, bed = _dev(w.reshape(16, 9)), _dev(b), _dev(gamma), _dev(beta)
    dd = _dev(drop) if with_drop else None
    lib.check(L.nisqa_conv1_moments(_p(mel), _p(frame_off), _p(seg_off), _p(floor), B, S, hop, _p(mom), _st()), 'moments')
    lib.check(L.nisqa_conv1_bn_act_pool_std_fwd(_p(mel), _p(frame_off), _p(seg_off), _p(floor), B, S, hop, _p(wd), _p(bd), _p(mom),
                                                _p(gd), _p(bed), _p(rm), _p(rv), _p(sums), _p(mr), _p(dd) if with_drop else None,
                                                _p(y), _p(arg), _st()), 'std_fwd')
    # float64 autograd: conv1 -> batch-statistics BatchNorm -> ReLU -> MaxPool2d(2, 2, padding (0, 1)) -> x drop
    W = torch.tensor(w, requires_grad=True)
    G, Be = torch.tensor(gamma, requires_grad=True), torch.tensor(beta, requires_grad=True)
    z = F.conv2d(segs, W, torch.tensor(b), padding=1)
    r = F.relu(F.batch_norm(z, None, None, G, Be, True, 0.0, onet.BN_EPS))
    ref = F.max_pool2d(r, 2, stride=2, padding=(0, 1))
    assert ref.shape[2:] == (24, 8)
    if with_drop:
        ref = ref * torch.tensor(drop)[:, :, None, None]
    got = y.cpu().double().view(S, 24, 8, 16).permute(0, 3, 1, 2)
    assert (got - ref.detach()).abs().max() < 1e-4 * max(1.0, float(ref.detach().abs().max()))
    # backward
    dy = rng.standard_normal((S, 16, 24, 8))
    gw, gg, gb = torch.autograd.grad((ref * torch.tensor(dy)).sum(), [W, G, Be])
    dyd = _dev(dy.transpose(0, 2, 3, 1).reshape(S, 192, 16))
    acc = torch.zeros(176, dtype=torch.float64, device=DEV)
    dgamma, dbeta, dw = torch.empty(16, device=DEV), torch.empty(16, device=DEV), torch.empty(16, 9, device=DEV)
    lib.check(L.nisqa_conv1_bn_act_pool_std_bwd(_p(mel), _p(frame_off), _p(seg_off), _p(floor), B, S, hop, _p(wd), _p(bd), _p(mom),
                                                _p(gd), _p(bed), _p(mr), _p(dd) if with_drop else None, _p(dyd), _p(arg), _p(acc),
                                                _p(dgamma), _p(dbeta), _p(dw), _st()), 'std_bwd')
    torch.cuda.synchronize()
    assert _rel(dgamma.cpu(), gg) < 1e-4
    assert _rel(dbeta.cpu(), gb) < 1e-4
    assert _rel(dw.cpu(), gw.reshape(16, 9)) < 1e-4


@pytest.mark.parametrize('h,w,c,ho,wo', [(24, 8, 32, 12, 4), (12, 4, 64, 6, 2)])
def test_bn_act_pool_at_standard_cnn_shapes_is_max_pool_2x2(h, w, c, ho, wo):
    """The adaptive windows of nisqa_bn_act_pool_* at 24 x 8 -> 12 x 4 and 12 x 4 -> 6 x 2 are MaxPool2d(2)'s windows, with its
    first-maximum tie order (ReLU zeros tie often)."""
    lib, L = _L()
    rng = np.random.default_rng(h * w + c)
    S = 37
    z = rng.standard_normal((S, c, h, w))
    z[:, :, 0, 0] = z[:, :, 0, 1]                                # exact ties inside windows
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.uniform(-0.5, 0.5, c)
    zd = _dev(z.transpose(0, 2, 3, 1).reshape(S * h * w, c))
    sums = torch.zeros(2 * c, dtype=torch.float64, device=DEV)
    lib.check(L.nisqa_col_dot(_p(zd), _p(zd), S * h * w, c, _p(sums), _st()), 'col_dot')
    rm, rv, mr = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.empty(2 * c, device=DEV)
    y = torch.empty(S, ho * wo, c, device=DEV)
    arg = torch.empty(S, ho * wo, c, dtype=torch.int32, device=DEV)
    gd, bd = _dev(gamma), _dev(beta)
    lib.check(L.nisqa_bn_act_pool_fwd(_p(zd), _p(sums), _p(gd), _p(bd), _p(rm), _p(rv), _p(mr), S, h, w, c, ho, wo, None, _p(y),
                                      _p(arg), _st()), 'bn_act_pool_fwd')
    Z = torch.tensor(z.astype(np.float32).astype(np.float64), requires_grad=True)
    G, Be = torch.tensor(gamma.astype(np.float32).astype(np.float64), requires_grad=True), torch.tensor(beta.astype(np.float32).astype(np.float64), requires_grad=True)
    r = F.relu(F.batch_norm(Z, None, None, G, Be, True, 0.0, onet.BN_EPS))
    ref, idx = F.max_pool2d(r, 2, return_indices=True)
    got = y.cpu().double().view(S, ho, wo, c).permute(0, 3, 1, 2)
    assert (got - ref.detach()).abs().max() < 1e-5
    # the same winning pixel wherever the maximum is positive (there the choice matters for the gradient)
    ga = arg.cpu().view(S, ho, wo, c).permute(0, 3, 1, 2).long()
    pos = ref.detach() > 1e-6
    assert (ga[pos] == idx[pos]).all()
    dy = rng.standard_normal((S, c, ho, wo))
    gz, gg, gb = torch.autograd.grad((ref * torch.tensor(dy)).sum(), [Z, G, Be])
    s2 = torch.zeros(2 * c, dtype=torch.float64, device=DEV)
    dz = torch.empty(S * h * w, c, device=DEV)
    dgamma, dbeta = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dyd = _dev(dy.transpose(0, 2, 3, 1).reshape(S, ho * wo, c))
    lib.check(L.nisqa_bn_act_pool_bwd(_p(dyd), _p(arg), None, _p(zd), _p(mr), _p(gd), _p(bd), S, h, w, c, ho, wo, _p(s2), _p(dz),
                                      _p(dgamma), _p(dbeta), _st()), 'bn_act_pool_bwd')
    torch.cuda.synchronize()
    assert _rel(dz.cpu().view(S, h, w, c).permute(0, 3, 1, 2), gz) < 1e-4
    assert _rel(dgamma.cpu(), gg) < 1e-4 and _rel(dbeta.cpu(), gb) < 1e-4


# ---- BiLSTM train forward and BPTT against float64 nn.LSTM -------------------------------------------------------------------
@pytest.mark.parametrize('pool', ['avg', 'max', 'last_step_bi'])
def test_bilstm_train_operators_match_float64_autograd(pool):
    from nisqa_amd.engine import LSTM_ARCH, LSTM_POOL_MODE
    lib, L = _L()
    rng = np.random.default_rng({'avg': 1, 'max': 2, 'last_step_bi': 3}[pool])
    lens = np.array([63, 1, 1300, 2, 329], dtype=np.int64)                 # ragged, unsorted
    S, B = int(lens.sum()), len(lens)
    k = 1.0 / np.sqrt(128)
    wih, whh = rng.uniform(-k, k, (2, 512, 20)), rng.uniform(-k, k, (2, 512, 128))
    bih, bhh = rng.uniform(-k, k, (2, 512)), rng.uniform(-k, k, (2, 512))
    x = rng.standard_normal((S, 20))
    dpool = rng.standard_normal((B, 256))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)                # the kernel's operands, exactly
    wih, whh, bih, bhh, x, dpool = map(f32, (wih, whh, bih, bhh, x, dpool))
    seg_off = _dev(np.concatenate(([0], np.cumsum(lens))), torch.int32)
    save, hprev = torch.empty(S, 2, 640, device=DEV), torch.empty(S, 2, 128, device=DEV)
    pooled, argmax = torch.empty(B, 256, device=DEV), torch.empty(B, 256, dtype=torch.int32, device=DEV)
    W = [_dev(a) for a in (wih, whh, bih, bhh)]
    xd = _dev(x)
    mode = LSTM_POOL_MODE[LSTM_ARCH[pool]]
    lib.check(L.nisqa_lstm_train_fwd(_p(xd), _p(seg_off), B, _p(W[0]), _p(W[1]), _p(W[2]), _p(W[3]), mode, _p(save), _p(hprev),
                                     _p(pooled), _p(argmax), _st()), 'lstm_train_fwd')
    dgates = torch.empty(S, 2, 512, device=DEV)
    dbias = torch.zeros(2, 512, dtype=torch.float64, device=DEV)
    dpd = _dev(dpool)
    lib.check(L.nisqa_lstm_train_bptt(_p(seg_off), B, _p(W[1]), _p(save), mode, _p(dpd), _p(argmax), _p(dgates), _p(dbias), _st()),
              'lstm_train_bptt')
    torch.cuda.synchronize()
    # float64 reference: states, pooled vectors and every gradient
    sd = {'weight_ih_l0': wih[0], 'weight_hh_l0': whh[0], 'bias_ih_l0': bih[0], 'bias_hh_l0': bhh[0],
          'weight_ih_l0_reverse': wih[1], 'weight_hh_l0_reverse': whh[1], 'bias_ih_l0_reverse': bih[1], 'bias_hh_l0_reverse': bhh[1]}
    sd = {'time_dependency.model.lstm.' + kk: torch.tensor(v, requires_grad=True) for kk, v in sd.items()}
    X = torch.tensor(x, requires_grad=True)
    seqs, pv, o = [], [], 0
    for n in lens:
        td = LT.bilstm(sd, X[o:o + n])
        seqs.append(td)
        pv.append(LT.pool_vector(td, pool))
        o += n
    pv = torch.stack(pv)
    assert np.abs(pooled.cpu().double().numpy() - pv.detach().numpy()).max() < 1e-5
    h_all = torch.cat(seqs).detach().numpy()                             # [S][256]
    hp = hprev.cpu().double().numpy()
    sv = save.cpu().double().numpy()
    o = 0
    for n in lens:                                                       # h_prev of every step: the neighbour's state, or 0
        h = h_all[o:o + n]
        want0 = np.vstack([np.zeros((1, 128)), h[:-1, :128]])
        want1 = np.vstack([h[1:, 128:], np.zeros((1, 128))])
        assert np.abs(hp[o:o + n, 0] - want0).max() < 1e-5 and np.abs(hp[o:o + n, 1] - want1).max() < 1e-5
        # h = o * tanh(c) from the saved gate and cell state
        assert np.abs(sv[o:o + n, 0, 384:512] * np.tanh(sv[o:o + n, 0, 512:]) - h[:, :128]).max() < 1e-5
        o += n
    keys = list(sd)
    grads = torch.autograd.grad((pv * torch.tensor(dpool)).sum(), [sd[kk] for kk in keys] + [X])
    want = dict(zip(keys + ['x'], [g.numpy() for g in grads]))
    dg = dgates.cpu().double().numpy()                                   # [S][2][512]
    for d, sfx in enumerate(('', '_reverse')):
        p = 'time_dependency.model.lstm.'
        hd = hp[:, d]
        assert _rel(dg[:, d].T @ x, want[p + 'weight_ih_l0' + sfx]) < 1e-4
        assert _rel(dg[:, d].T @ hd, want[p + 'weight_hh_l0' + sfx]) < 1e-4
        assert _rel(dbias.cpu().numpy()[d], want[p + 'bias_ih_l0' + sfx]) < 1e-4
        assert _rel(dg[:, d].sum(0), want[p + 'bias_hh_l0' + sfx]) < 1e-4
    assert _rel(dg[:, 0] @ wih[0] + dg[:, 1] @ wih[1], want['x']) < 1e-4


# ---- the whole step ----------------------------------------------------------------------------------------------------------
def _fixture(name):
    g = dict(helpers.golden('train_lstm_%s.npz' % name))
    g.update(dict(helpers.golden('train_lstm_%s_cnn.npz' % name)))
    if name == 'last_step_bi':
        path = helpers.find_weights('nisqa_tts.tar')
        if path is None:
            pytest.skip('nisqa_tts.tar not staged (oracle/_ref/weights)')
        args, sd = helpers.load_checkpoint(path)
        args = dict(args)
        sd = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}
    else:
        args = dict(LT.AVG_ARGS if name == 'avg' else LT.MAX_ARGS)
        sd = synth.random_state_dict(int(g['seed_sd']), 'NISQA_TTS')
    args['cnn_dropout'] = 0.0
    specs, y = LT.batch(int(g['seed_batch']))
    return g, args, sd, specs, y


def _adam_expected(sd, grads, lr):
    """torch.optim.Adam's first step from the stored gradients"""
    ps = {k: torch.nn.Parameter(torch.as_tensor(np.asarray(sd[k])).float().clone()) for k in grads}
    opt = torch.optim.Adam(list(ps.values()), lr=lr)
    for k, p in ps.items():
        p.grad = torch.as_tensor(grads[k]).float()
    opt.step()
    return {k: p.detach().numpy() for k, p in ps.items()}


@pytest.mark.parametrize('name', ['avg', 'max', 'last_step_bi'])
def test_lstm_training_step_matches_reference_fixture(name):
    from nisqa_amd.train_lstm import HipTrainerLSTM
    g, args, sd, specs, y = _fixture(name)
    lr = float(g['lr'])
    tr = HipTrainerLSTM(args, sd, DEV, lr=lr)
    loss = tr.step_spec(specs, y)
    torch.cuda.synchronize()
    assert list(tr.L) == list(g['n_wins'])
    assert float(loss) == pytest.approx(float(g['loss1']), rel=1e-4)
    assert np.abs(tr.last['y_hat'].cpu().numpy() - g['y_hat1']).max() < 1e-4
    grads = tr.grads()
    worst, wk = 0.0, None
    for k, gr in grads.items():
        want = g['grad/' + k]
        assert tuple(gr.shape) == want.shape, k
        if k.startswith('cnn.model.conv') and k.endswith('.bias'):
            assert np.abs(gr.numpy()).max() < 1e-4                  # analytically zero under train-mode BatchNorm
            continue
        e = float(np.abs(gr.numpy() - want).max()) / max(1e-3, float(np.abs(want).max()))
        if e > worst:
            worst, wk = e, k
    print(name, 'worst relative gradient error', worst, wk)
    # max pooling sends each unit's gradient through ONE step: at this random initialisation, relative perturbations of 2e-7 (fp32
    # rounding) of the pre-BatchNorm activations move the reference's own float64 gradients by up to 3.8e-3 of a tensor's largest
    # entry (ReLU gates behind train-mode BatchNorm flip); avg and last_step_bi stay below 6e-4 under the same perturbations
    assert worst < (5e-3 if name == 'max' else 1e-3), (worst, wk)
    new = tr.state_dict()
    for k, v in new.items():
        if 'running' in k:
            want = g['sd1/' + k]
            assert np.abs(v.numpy() - want).max() < 2e-4 * max(1.0, np.abs(want).max()), k
        elif k.endswith('num_batches_tracked'):
            assert int(v) == int(g['sd1/' + k])
    exp = _adam_expected(sd, {k: g['grad/' + k] for k in grads}, lr)
    for k, want in exp.items():
        gref = g['grad/' + k]
        conv_b = k.startswith('cnn.model.conv') and k.endswith('.bias')
        solid = (np.abs(gref) > 1e-3 * max(1e-3, np.abs(gref).max())) & (not conv_b)
        d = np.abs(new[k].numpy() - want)
        assert d[solid].max(initial=0) < 1e-4 and d.max() <= 2.002 * lr, k
    if 'loss2' not in g:
        return
    loss2 = tr.step_spec(specs, y)
    torch.cuda.synchronize()
    assert float(loss2) == pytest.approx(float(g['loss2']), rel=2e-2)
    for k, v in tr.state_dict().items():
        if 'running' in k:
            want = g['sd2/' + k]
            assert np.abs(v.numpy() - want).max() < 1e-3 * max(1.0, np.abs(want).max()), k
    from nisqa_amd.engine import HipNisqa
    HipNisqa(args, tr.state_dict(), DEV)


@pytest.mark.parametrize('pool', ['avg', 'max'])
def test_lstm_training_step_with_dropout_masks_matches_oracle(pool):
    """Explicit non-zero Dropout2d masks and a cubic bias map: the step against the float64 oracle."""
    from nisqa_amd.train_lstm import HipTrainerLSTM
    args = dict(LT.AVG_ARGS if pool == 'avg' else LT.MAX_ARGS)
    sd = synth.random_state_dict(31, 'NISQA_TTS')
    specs, y = LT.batch(71)
    segs, n_wins = LT.segments(specs, args)
    masks = LT.random_masks(72, int(n_wins.sum()), 0.2)
    bias = np.tile(np.array([[0.1, 0.9, 0.02, -0.001]], np.float32), (len(specs), 1))
    ref = LT.train_step(sd, args, segs, n_wins, y, masks=masks, bias=bias)
    tr = HipTrainerLSTM(args, sd, DEV, lr=1e-3)
    loss = tr.step_spec(specs, y, masks=masks, bias=bias)
    torch.cuda.synchronize()
    assert float(loss) == pytest.approx(ref['loss'], rel=1e-4)
    assert np.abs(tr.last['y_hat'].cpu().numpy() - ref['y_hat']).max() < 1e-4
    worst, wk = 0.0, None
    for k, gr in tr.grads().items():
        if k.startswith('cnn.model.conv') and k.endswith('.bias'):
            continue
        want = ref['grads'][k]
        e = float(np.abs(gr.numpy() - want).max()) / max(1e-3, float(np.abs(want).max()))
        if e > worst:
            worst, wk = e, k
    assert worst < 1e-3, (worst, wk)
    for k, v in tr.state_dict().items():
        if 'running' in k:
            assert np.abs(v.numpy() - ref['bufs'][k]).max() < 2e-4 * max(1.0, np.abs(ref['bufs'][k]).max()), k


def test_lstm_train_loop_from_recipe_args_writes_loadable_checkpoints(tmp_path, capsys):
    """nisqaModel(args).train() with the CNN-LSTM-AVG recipe's arguments on a tiny synthetic corpus, two epochs."""
    import pandas as pd
    from nisqa_amd.NISQA_model import nisqaModel
    rng = np.random.default_rng(13)
    d = tmp_path / 'corpus'
    d.mkdir()
    rows = []
    for db, n in (('TRAIN_A', 7), ('TRAIN_B', 6), ('VAL_A', 5)):
        for i in range(n):
            name = '%s_%d.wav' % (db, i)
            synth.write_wav(str(d / name), synth.synth_pcm16(200 + len(rows), float(rng.uniform(0.5, 1.6))), 48000)
            rows.append({'db': db, 'filepath_deg': name, 'mos': float(rng.uniform(1, 5))})
    pd.DataFrame(rows).to_csv(d / 'files.csv', index=False)
    args = dict(LT.AVG_ARGS)
    args.update({'name': 'tiny_lstm', 'data_dir': str(d), 'output_dir': str(tmp_path / 'out'), 'pretrained_model': False,
                 'csv_file': 'files.csv', 'csv_con': None, 'csv_deg': 'filepath_deg', 'csv_mos_train': 'mos',
                 'csv_mos_val': 'mos', 'csv_db_train': ['TRAIN_A', 'TRAIN_B'], 'csv_db_val': ['VAL_A'], 'tr_epochs': 2,
                 'tr_early_stop': 20, 'tr_bs': 4, 'tr_bs_val': 4, 'tr_lr': 1e-3, 'tr_lr_patience': 15, 'tr_num_workers': 2,
                 'tr_parallel': False, 'tr_ds_to_memory': False, 'tr_ds_to_memory_workers': 0, 'tr_device': None,
                 'tr_checkpoint': 'every_epoch', 'tr_verbose': 1, 'tr_bias_mapping': 'first_order', 'tr_bias_min_r': 0.7,
                 'tr_bias_anchor_db': None, 'ms_channel': None})
    torch.manual_seed(4)
    nm = nisqaModel(args)
    nm.train()
    out = capsys.readouterr().out
    assert '--> start training' in out and '--> Training done.' in out
    assert out.count('ep 1 sec') == 1 and out.count('ep 2 sec') == 1
    run_dir = tmp_path / 'out' / nm.runname
    ck = run_dir / (nm.runname + '__ep_002.tar')
    assert ck.exists()
    c = torch.load(str(ck), map_location='cpu', weights_only=False)
    assert c['epoch'] == 2 and int(c['model_state_dict']['cnn.model.bn1.num_batches_tracked']) == 8
    assert 'HipTrainerLSTM' in c['optimizer_state_dict']['layout']
    p = nisqaModel({'mode': 'predict_file', 'pretrained_model': str(ck), 'deg': str(d / 'VAL_A_0.wav'), 'output_dir': None,
                    'csv_file': None, 'csv_deg': None, 'data_dir': None, 'num_workers': 0, 'bs': 1, 'ms_channel': None,
                    'tr_bs_val': 1, 'tr_num_workers': 0})
    df = p.predict()
    assert float(df['mos_pred'].iloc[0]) == pytest.approx(float(nm.ds_val.df['mos_pred'].iloc[0]), abs=1e-4)
    from oracle import ref_shim
    if ref_shim.reference_available():
        ref_shim.build_reference_model(c['args'], c['model_state_dict'])            # strict load into the reference's NISQA
