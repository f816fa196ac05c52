"""One training step with self-attention blocks of 1, 3, 4 and 5 layers on the MI355X (run with -m gpu).  csrc/train_td.hip lays
out its workspace, fragment buffer, weight-gradient groups, column-sum jobs and pack jobs from the layer count (at most four);
deeper stacks take the operator-by-operator path; the double-ended trainer keeps two counts.  Every fixture has two layers.
Yardstick: the operators of oracle/train.py (tests/de_train_oracle.py for NISQA_DE) in float64 with the same explicit dropout
masks at every site of every layer and a bias mapping; bars: those of the two-layer tests of tests/test_gpu_train.py and
tests/test_gpu_train_de.py.  One step only."""
import numpy as np
import pytest
import torch

import de_oracle as DO
import de_train_oracle as DT
import helpers
import lstm_train_oracle as LT
import sa_layers as SL
from nisqa_amd import synth
from oracle import net as onet, train as otrain
from test_gpu_train_de import _grad_errors

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_WINS = [1, 33, 64, 5]                      # a 1 x 1 attention matrix, one past a 32-token tile, two tiles exactly, a short clip
_CACHE = {}


def _conv_bias(k):
    return k.startswith('cnn.model.conv') and k.endswith('.bias')


def _case(L):
    """(args, state dict, specs, y, bias, the trainer's masks, the float64 step) of NISQA_DIM with L layers"""
    if ('case', L) in _CACHE:
        return _CACHE[('case', L)]
    args = SL.args_with_layers(synth.DIM_ARGS, L)
    sd = SL.with_layers(helpers.random_state_dict(7, 'NISQA_DIM'), L)
    rng = np.random.default_rng(9)
    specs = [(-40 + 18 * rng.standard_normal((48, 15 + 4 * (n - 1)))).astype(np.float32) for n in N_WINS]
    y = rng.uniform(1, 5, (len(N_WINS), 5)).astype(np.float32)
    y[1, 0] = y[3, 2] = np.nan
    segs, n_wins = zip(*[onet.segment_specs(s, 15, 4, None) for s in specs])
    assert list(n_wins) == N_WINS
    S = sum(N_WINS)
    drop = lambda shape, p: ((rng.random(shape) >= p).astype(np.float32) / (1 - p))
    mk, mo = {}, {}
    for key, c in (('cnn_d1', 32), ('cnn_d2', 64), ('cnn_d3', 64), ('cnn_d4', 64)):
        mk[key] = drop((S, c), 0.2)
        mo[key] = torch.as_tensor(mk[key]).double()[:, :, None, None]
    tok = np.concatenate(([0], np.cumsum(N_WINS)))
    for l in range(L):
        pk = []
        for b, n in enumerate(N_WINS):
            m = drop((n, n), 0.1)
            mo[(b, 'td%d_p' % l)] = torch.as_tensor(m).double()
            pk.append(m.reshape(-1))
        mk['td%d_p' % l] = np.concatenate(pk)
        for t in ('1', 'f', '2'):
            m = drop((S, 64), 0.1)
            mk['td%d_%s' % (l, t)] = m
            for b in range(len(N_WINS)):
                mo[(b, 'td%d_%s' % (l, t))] = torch.as_tensor(m[tok[b]:tok[b + 1]]).double()
    bias = np.tile(np.array([[0.1, 0.9, 0.02, -0.001]], np.float32), (len(N_WINS), 1))
    # oracle.train.train_step computes in float32; the same operators in float64
    s = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keys = otrain.param_keys(s)
    for k in keys:
        s[k].requires_grad_(True)
    y_hat, _ = otrain.forward_train(s, args, torch.cat(segs).double(), N_WINS, mo)
    loss = otrain.nan_mse_loss(y_hat, torch.from_numpy(y).double(), torch.from_numpy(bias).double())
    grads = torch.autograd.grad(loss, [s[k] for k in keys])
    ref = {'loss': float(loss.detach()), 'y_hat': y_hat.detach().numpy(), 'grads': {k: g.numpy() for k, g in zip(keys, grads)}}
    _CACHE[('case', L)] = (args, sd, specs, y, bias, mk, ref)
    return _CACHE[('case', L)]


def _step(L, fused, monkeypatch):
    """one HipTrainer step in 'f32' on the fused block (NISQA_HIP_TRAIN_FUSED_TD=1), on the operator path (=0), or on whatever the
    trainer chooses by itself (None) -> (fused_td, loss, y_hat, grads)"""
    if ('step', L, fused) in _CACHE:
        return _CACHE[('step', L, fused)]
    from nisqa_amd.train import HipTrainer
    args, sd, specs, y, bias, mk, _ = _case(L)
    if fused is None:
        monkeypatch.delenv('NISQA_HIP_TRAIN_FUSED_TD', raising=False)
    else:
        monkeypatch.setenv('NISQA_HIP_TRAIN_FUSED_TD', '1' if fused else '0')
    tr = HipTrainer(args, sd, DEV, lr=1e-3, precision='f32')
    assert tr.n_layers == L
    loss = tr.step_spec(specs, y, masks=mk, bias=bias)
    torch.cuda.synchronize()
    _CACHE[('step', L, fused)] = (tr.fused_td, float(loss), tr.last['y_hat'].cpu().numpy().copy(), tr.grads())
    return _CACHE[('step', L, fused)]


def _against_oracle(what, L, loss, y_hat, grads):
    """the bars of test_training_step_at_configs4_size_with_dropout_masks_matches_oracle: loss to 1e-4 relative, every gradient
    tensor to 3e-3 of max(1e-3, its largest entry); a layer whose gradients are missing is noticed"""
    ref = _case(L)[6]
    assert set(grads) == set(ref['grads'])
    assert all(any(SL.layer_of(k) == l for k in grads) for l in range(L))
    worst, wk = 0.0, None
    for k, gr in grads.items():
        if _conv_bias(k):
            continue
        want = ref['grads'][k]
        assert tuple(gr.shape) == tuple(want.shape), k
        e = float(np.abs(gr.numpy() - want).max()) / max(1e-3, float(np.abs(want).max()))
        if e > worst:
            worst, wk = e, k
    dy = float(np.abs(y_hat - ref['y_hat']).max())
    print('x%d, %s: loss %.6f (float64 %.6f), y_hat err %.2e, worst relative gradient error %.2e (%s)' % (
        L, what, loss, ref['loss'], dy, worst, wk))
    assert loss == pytest.approx(ref['loss'], rel=1e-4)
    assert worst < 3e-3, (worst, wk)


@pytest.mark.parametrize('path', ['fused', 'operator'])
@pytest.mark.parametrize('L', [1, 3, 4])
def test_training_step_at_other_depths(L, path, monkeypatch):
    fused_td, loss, y_hat, grads = _step(L, path == 'fused', monkeypatch)
    assert fused_td == (path == 'fused')
    _against_oracle(path, L, loss, y_hat, grads)
    if path == 'fused':
        return
    # the two paths against each other, as test_fused_self_attention_block_matches_the_operator_by_operator_path holds them
    _, l1, y1, g1 = _step(L, True, monkeypatch)
    assert l1 == pytest.approx(loss, rel=1e-5)
    assert np.abs(y1 - y_hat).max() < 1e-5
    worst, wk = 0.0, None
    for k in grads:
        if _conv_bias(k):
            continue
        g0 = grads[k].numpy()
        if float(np.abs(g0).max()) < 1e-4:                           # analytically zero (the score bias under the softmax): rounding noise
            assert float(np.abs(g1[k].numpy()).max()) < 1e-4, k
            continue
        e = float(np.abs(g1[k].numpy() - g0).max()) / max(1e-3, float(np.abs(g0).max()))
        if e > worst:
            worst, wk = e, k
    print('x%d: fused against operator path: loss %.6f %.6f, worst relative gradient difference %.2e (%s)' % (L, l1, loss, worst, wk))
    assert worst < 2e-5, (worst, wk)


def test_a_stack_deeper_than_the_fused_block_takes_the_operator_path(monkeypatch):
    fused_td, loss, y_hat, grads = _step(5, None, monkeypatch)
    assert fused_td is False
    _against_oracle('five layers', 5, loss, y_hat, grads)


# ---- double-ended ---------------------------------------------------------------------------------------------------------------
DE_LAYERS, DE_SEED = (1, 3), 70              # the seed: found on the CPU so that no argmax of the float64 step is within 1e-4 of a tie


def de_case():
    """one layer in the first block, three in the second, cosine / hard / 'x/y/-', the pairs and the mapping of
    tests/test_gpu_train_de.py's masked step -> (args, sd, specs_d, specs_r, y, masks, bias, the float64 step)"""
    if 'de' in _CACHE:
        return _CACHE['de']
    args = DT.de_train_args('cosine', 'x/y/-', cnn_dropout=0.2, td_sa_dropout=0.1, td_2_sa_dropout=0.1,
                            td_sa_num_layers=DE_LAYERS[0], td_2_sa_num_layers=DE_LAYERS[1])
    sd = SL.with_layers(DO.random_de_state_dict(DE_SEED, 'x/y/-', n_layers2=DE_LAYERS[1]), DE_LAYERS[0], seed=DE_SEED)
    specs_d, y = LT.batch(100 + DE_SEED, [15, 97, 300])
    specs_r, _ = LT.batch(1100 + DE_SEED, [40, 97, 260])
    y[1, 0], y[2, 0] = 3.0, np.nan
    segs_d, nw_d = DT.segments(specs_d, args)
    segs_r, nw_r = DT.segments(specs_r, args)
    assert nw_d.tolist() == [1, 21, 72] and nw_r.tolist() == [7, 21, 62]
    masks = DT.random_masks(DE_SEED, nw_d, nw_r, DE_LAYERS[0], DE_LAYERS[1], 0.2)
    bias = np.array([[0.1, 0.9, 0.02, -0.003], [-0.2, 1.1, -0.01, 0.002], [0.05, 1.0, 0.0, 0.001]], np.float32)
    ref = DT.train_step(sd, args, segs_d, nw_d, segs_r, nw_r, y, masks=masks, bias=bias)
    _CACHE['de'] = (args, sd, specs_d, specs_r, y, masks, bias, ref)
    return _CACHE['de']


def test_double_ended_training_step_with_blocks_of_different_depth():
    """the bars of test_step_with_masks_and_bias_mapping_matches_the_float64_oracle"""
    from nisqa_amd.train_de import HipTrainerDE
    args, sd, specs_d, specs_r, y, masks, bias, ref = de_case()
    assert ref['gap'] >= 1e-4
    tr = HipTrainerDE(args, sd, DEV, lr=1e-3, precision='f32')
    assert (tr.n_layers, tr.n_layers2) == DE_LAYERS
    loss = float(tr.step_spec(specs_d, specs_r, y, masks=masks, bias=bias))
    torch.cuda.synchronize()
    assert np.array_equal(tr.last_idx.cpu().numpy(), np.concatenate(ref['idx']))
    grads = tr.grads()
    for pfx, n in ((SL.TD, DE_LAYERS[0]), (SL.TD2, DE_LAYERS[1])):
        assert SL.depth(grads, pfx) == n
    worst, wk = _grad_errors(grads, ref['grads'])
    dy = float(np.abs(tr.last['y_hat'].cpu().numpy() - ref['y_hat']).max())
    print('DE x%d / x%d: loss %.6f (float64 %.6f), y_hat err %.2e, worst relative gradient error %.2e (%s)' % (
        DE_LAYERS + (loss, ref['loss'], dy, worst, wk)))
    assert loss == pytest.approx(ref['loss'], rel=1e-4)
    assert dy < 1e-4
    assert worst < 1e-3, (worst, wk)
    bufs = {k: v.numpy() for k, v in tr.state_dict().items() if 'running' in k}
    for k, w in ref['bufs'].items():
        e = float(np.abs(bufs[k] - w).max()) / max(1.0, float(np.abs(w).max()))
        assert e < (1e-5 if k.endswith('running_mean') else 1e-4), (k, e)
