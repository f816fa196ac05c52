"""StandardCNN + BiLSTM training, host side (no GPU needed): refusals before any GPU work, the flat-buffer layout round trip, the
fc_out column permutation, the trainer chosen by the training loop, argument checks of the new C entry points, and the float64
oracle (tests/lstm_train_oracle.py) against the reference's own fixtures (tests/golden/make_golden_train_lstm.py)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import lstm_train_oracle as LT
from nisqa_amd import synth


def _no_gpu_work(monkeypatch):
    """Any attempt to build the engine (the first GPU work of the trainer) fails the test."""
    from nisqa_amd import train_lstm

    def boom(*a, **k):
        raise AssertionError('GPU work started before the refusal')
    monkeypatch.setattr(train_lstm, 'HipNisqa', boom)


@pytest.mark.parametrize('key,value,word', [
    ('td_2', 'lstm', 'td_2'), ('model', 'NISQA_DIM', 'NISQA_DIM'), ('td_lstm_bidirectional', False, 'unidirectional'),
    ('pool', 'att', 'pool=att'), ('td_lstm_num_layers', 2, 'td_lstm_num_layers=2'), ('td_lstm_h', 64, 'td_lstm_h=64'),
    ('cnn_fc_out_h', 32, 'cnn_fc_out_h=32'), ('td', 'self_att', 'td=self_att'), ('cnn_model', 'adapt', 'cnn_model=adapt')])
def test_refused_options_are_named_before_gpu_work(monkeypatch, key, value, word):
    from nisqa_amd.train_lstm import HipTrainerLSTM
    _no_gpu_work(monkeypatch)
    args = dict(LT.AVG_ARGS, **{key: value})
    with pytest.raises(NotImplementedError, match=word):
        HipTrainerLSTM(args, synth.random_state_dict(1, 'NISQA_TTS'), 'cpu')


@pytest.mark.parametrize('prec', ['bf16x6', 'mixed', 'bf16x3', 'f16x4', 'fp8'])
def test_precisions_other_than_f32_are_refused_by_name(monkeypatch, prec):
    from nisqa_amd.train_lstm import HipTrainerLSTM
    _no_gpu_work(monkeypatch)
    sd = synth.random_state_dict(1, 'NISQA_TTS')
    with pytest.raises(NotImplementedError, match=prec):
        HipTrainerLSTM(dict(LT.AVG_ARGS), sd, 'cpu', precision=prec)
    monkeypatch.setenv('NISQA_HIP_TRAIN_PRECISION', prec)
    with pytest.raises(NotImplementedError, match=prec):
        HipTrainerLSTM(dict(LT.AVG_ARGS), sd, 'cpu')


def _cpu_trainer(sd, args=None):
    """A HipTrainerLSTM with its parameter bookkeeping only (no engine, CPU tensors)."""
    from nisqa_amd.train_lstm import HipTrainerLSTM
    tr = HipTrainerLSTM.__new__(HipTrainerLSTM)
    tr.device = torch.device('cpu')
    tr._layout(sd)
    tr.load_state_dict(sd)
    return tr


def test_state_dict_round_trip_through_kernel_layout_is_bit_identical():
    from nisqa_amd.train_lstm import LSTM_KEYS
    sd = {k: torch.as_tensor(np.asarray(v)) for k, v in synth.random_state_dict(3, 'NISQA_TTS').items()}
    sd['cnn.model.bn2.num_batches_tracked'] = torch.tensor(7)
    tr = _cpu_trainer(sd)
    out = tr.state_dict()
    assert list(out) == list(sd)
    for k, v in sd.items():
        assert tuple(out[k].shape) == tuple(v.shape), k
        assert torch.equal(out[k].to(v.dtype), v), k
    # both directions of every LSTM tensor are adjacent in the flat buffer (one pointer per tensor kind for the kernels)
    for a, b in zip(LSTM_KEYS[0::2], LSTM_KEYS[1::2]):
        assert tr.off[b] == tr.off[a] + int(np.prod(tr.kshape[a]))
    assert tr.keys[-2:] == ['pool.model.linear.weight', 'pool.model.linear.bias']


def test_fc_out_column_permutation_matches_numpy():
    from nisqa_amd.train_lstm import fc_to_kernel, fc_from_kernel
    w = np.random.default_rng(0).standard_normal((20, 768)).astype(np.float32)
    k = fc_to_kernel(torch.from_numpy(w)).numpy()
    # activations are [pixel][channel] (pixel = y * 2 + x of the 6 x 2 map); the reference flattens [channel][y][x]
    for j in (0, 7, 19):
        for c in (0, 5, 63):
            for p in range(12):
                assert k[j, p * 64 + c] == w[j, c * 12 + p]
    assert np.array_equal(fc_from_kernel(torch.from_numpy(k)).numpy(), w)
    # and the features / weight pair gives the reference's product
    feat = np.random.default_rng(1).standard_normal((3, 64, 6, 2)).astype(np.float32)
    act = feat.transpose(0, 2, 3, 1).reshape(3, 768)
    np.testing.assert_allclose(act @ k.T, feat.reshape(3, 768) @ w.T, rtol=1e-5, atol=1e-5)


def test_trainloop_picks_the_trainer_from_the_args():
    from nisqa_amd import trainloop
    from nisqa_amd.train import HipTrainer
    from nisqa_amd.train_lstm import HipTrainerLSTM
    assert trainloop.trainer_class(dict(LT.AVG_ARGS)) is HipTrainerLSTM
    assert trainloop.trainer_class(dict(synth.TTS_ARGS)) is HipTrainerLSTM
    assert trainloop.trainer_class(dict(synth.MOS_ARGS)) is HipTrainer
    assert HipTrainerLSTM.LAYOUT != HipTrainer.LAYOUT
    # HipTrainer itself keeps refusing StandardCNN + BiLSTM
    with pytest.raises(NotImplementedError):
        HipTrainer(dict(LT.AVG_ARGS), synth.random_state_dict(1, 'NISQA_TTS'), 'cpu')


def test_new_entry_points_reject_bad_arguments():
    from nisqa_amd import lib
    L = lib.load()
    p = ctypes.c_void_p(16)                     # never dereferenced: the checks return before any HIP call
    ERR = 1
    assert L.nisqa_lstm_train_fwd(None, p, 2, p, p, p, p, 1, p, p, p, p, None) == ERR
    assert L.nisqa_lstm_train_fwd(p, p, 0, p, p, p, p, 1, p, p, p, p, None) == ERR
    assert L.nisqa_lstm_train_fwd(p, p, 2, p, p, p, p, 7, p, p, p, p, None) == ERR
    assert L.nisqa_lstm_train_fwd(p, p, 2, p, p, p, p, 2, p, p, p, None, None) == ERR        # max pooling needs argmax
    assert L.nisqa_lstm_train_bptt(p, 2, p, p, 1, p, p, None, None, None) == ERR
    assert L.nisqa_lstm_train_bptt(p, -1, p, p, 1, p, p, p, None, None) == ERR
    assert L.nisqa_lstm_train_bptt(p, 2, p, p, 2, p, None, p, None, None) == ERR
    assert L.nisqa_lstm_train_bptt(p, 2, p, p, 9, p, p, p, None, None) == ERR
    args13 = [p] * 4 + [2, 3, 1] + [p] * 13
    assert L.nisqa_conv1_bn_act_pool_std_fwd(*([None] + args13[1:])) == ERR
    assert L.nisqa_conv1_bn_act_pool_std_fwd(*(args13[:4] + [2, 0, 1] + args13[7:])) == ERR
    args14 = [p] * 4 + [2, 3, 1] + [p] * 14
    assert L.nisqa_conv1_bn_act_pool_std_bwd(*(args14[:-2] + [None, None])) == ERR
    assert L.nisqa_conv1_bn_act_pool_std_bwd(*(args14[:4] + [2, 3, 0] + args14[7:])) == ERR


@pytest.mark.parametrize('name', ['avg', 'max'])
def test_float64_oracle_matches_reference_fixture(name):
    g = dict(helpers.golden('train_lstm_%s.npz' % name))
    g.update(dict(helpers.golden('train_lstm_%s_cnn.npz' % name)))
    args = dict(LT.AVG_ARGS if name == 'avg' else LT.MAX_ARGS, cnn_dropout=0.0)
    sd = synth.random_state_dict(int(g['seed_sd']), 'NISQA_TTS')
    specs, y = LT.batch(int(g['seed_batch']))
    segs, n_wins = LT.segments(specs, args)
    assert list(n_wins) == list(g['n_wins']) and n_wins.min() == 1 and n_wins.max() == 329
    r = LT.train_step(sd, args, segs, n_wins, y)
    assert r['loss'] == pytest.approx(float(g['loss1']), rel=1e-5)
    assert np.abs(r['y_hat'] - g['y_hat1']).max() < 1e-5
    for k, gr in r['grads'].items():
        if k.startswith('cnn.model.conv') and k.endswith('.bias'):
            continue
        want = g['grad/' + k]
        assert np.abs(gr - want).max() < 1e-3 * max(1e-3, np.abs(want).max()), k
    for k, v in r['bufs'].items():
        assert np.abs(v - g['sd1/' + k]).max() < 1e-5 * max(1.0, np.abs(v).max()), k
