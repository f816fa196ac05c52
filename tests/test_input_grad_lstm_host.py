"""d model(x, n_wins) / d x of the StandardCNN + BiLSTM models, host side without a GPU: the float64 oracle
(tests/input_grad_lstm_oracle.py) against the reference's own modules in eval mode and against the committed fixtures, the tie
margins of the seeded cases, the two new C entries' argument guards, and the refusal of the fast precisions."""
import os
import re

import numpy as np
import pytest
import torch

import helpers
import input_grad_lstm_oracle as IL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'nisqa_bn_eval_act_maxpool2_fwd': 13, 'nisqa_bn_eval_act_maxpool2_bwd': 14}
TIE = 1e-5
_CACHE = {}


def _oracle(pool, spec_name='SMALL'):
    key = (pool, spec_name)
    if key not in _CACHE:
        sd, args, x, n_wins, g = IL.case(pool, getattr(IL, spec_name))
        _CACHE[key] = IL.oracle(sd, args, x, n_wins, [g])
    return _CACHE[key]


@pytest.mark.parametrize('pool', IL.POOLS)
def test_oracle_gradient_matches_the_reference_modules_in_eval_mode(pool):
    """x.grad of the reference's module (float32, eval mode) against the float64 oracle, per clip: within 5e-5 of the clip's
    largest entry (measured <= 4.4e-6).  Padding rows get exactly zero on both sides."""
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip('reference tree not staged')
    sd, args, x, n_wins, g = IL.case(pool)
    B = len(n_wins)
    want = _oracle(pool)
    ref = ref_shim.build_reference_model(args, sd)[0]
    assert not ref.training
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    y = ref(xt, torch.as_tensor(n_wins))
    y.backward(torch.from_numpy(g))
    got, w = xt.grad.numpy(), want['dx'][0]
    assert (np.abs(w).reshape(B, -1).max(1) > 0).all()
    err = IL.clip_error(got, w)
    print(pool, 'max |dx| per clip', np.abs(w).reshape(B, -1).max(1), 'relative distance', err)
    assert (err <= 5e-5).all(), err
    np.testing.assert_allclose(y.detach().numpy(), want['y'], rtol=0, atol=1e-4)
    for b, n in enumerate(n_wins):
        assert (got[b, n:] == 0).all() and (w[b, n:] == 0).all()


@pytest.mark.parametrize('pool', IL.POOLS)
def test_fixture_holds_the_reference_gradient_of_the_small_case(pool):
    """tests/golden/input_grad_lstm_*.npz (written by the reference's module, make_golden_input_grad_lstm.py) against the oracle on
    the case rebuilt from the stored seeds, at the same 5e-5."""
    fx = helpers.golden('input_grad_lstm_%s.npz' % pool)
    spec = IL.SMALL
    assert (int(fx['seed_sd']), int(fx['seed_batch']), fx['frames'].tolist(), int(fx['L'])) == \
        (spec['seed_sd'], spec['seed_batch'], spec['frames'], spec['L'])
    sd, args, x, n_wins, g = IL.case(pool)
    assert fx['n_wins'].tolist() == n_wins.tolist() and np.array_equal(fx['g'], g) and fx['dx'].shape == x.shape
    want = _oracle(pool)
    err = IL.clip_error(fx['dx'], want['dx'][0])
    print(pool, 'fixture against the oracle', err)
    assert (err <= 5e-5).all()
    np.testing.assert_allclose(fx['y'], want['y'], rtol=0, atol=1e-4)


def test_padding_rows_do_not_reach_the_oracle():
    sd, args, x, n_wins, g = IL.case('avg')
    xn = IL.case('avg', fill=np.nan)[2]
    assert np.isnan(xn[0, 1:]).all() and np.array_equal(xn[0, :1], x[0, :1])
    b = IL.oracle(sd, args, xn, n_wins, [g])
    assert np.array_equal(_oracle('avg')['dx'][0], b['dx'][0]) and np.isfinite(b['dx'][0]).all()


def test_tie_margins_of_the_seeded_cases():
    """SMALL: nothing sits on a tie (smallest margin 2.87e-5).  EDGE: 98 segments, 5 below 1e-5 (clip 0: 5, 19, 22, 31; clip 2:
    14), the smallest kept margin 1.02e-5.  The margin belongs to the CNN: it is the same for the three poolings."""
    m = _oracle('last_step_bi')['margin']
    assert np.isfinite(m).sum() == 6 and m[np.isfinite(m)].min() >= TIE
    assert np.isinf(m[0, 1:]).all() and np.isinf(m[2, 2:]).all()
    e = _oracle('max', 'EDGE')['margin']
    valid = np.isfinite(e)
    out = valid & (e < TIE)
    print('SMALL smallest margin', m[np.isfinite(m)].min(), 'EDGE segments', int(valid.sum()), 'below TIE', np.argwhere(out).tolist(),
          'smallest kept', e[valid & ~out].min())
    assert valid.sum() == 98 and 0 < out.sum() <= 0.25 * valid.sum()


def test_entries_are_declared_bound_exported_and_guarded():
    from nisqa_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_train.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(nisqa_[a-z0-9_]+)\s*\(', hdr, re.M))
    for name, n_args in ENTRIES.items():
        assert name in declared and len(lib.TRAIN_SYMBOLS[name][1]) == n_args
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert set(ENTRIES) <= set(lib.exported_symbols(lib.LIB_PATH, 'nisqa_'))
    L = lib.load()
    one = 16                                               # a non-NULL pointer that is never followed: the guards come first
    E = lib.NISQA_ERR_ARG
    fwd = lambda *dims, z=one, y=one, arg=one: L.nisqa_bn_eval_act_maxpool2_fwd(z, one, one, one, one, *dims, y, arg, None)
    bwd = lambda *dims, dy=one, arg=one, dz=one: L.nisqa_bn_eval_act_maxpool2_bwd(dy, arg, one, one, one, one, one, *dims, dz, None)
    ok = (1, 48, 15, 16, 1)
    # NULL pointers, one at a time where the entry has its own: arg is needed by every shape
    assert L.nisqa_bn_eval_act_maxpool2_fwd(None, None, None, None, None, *ok, None, None, None) == E
    assert L.nisqa_bn_eval_act_maxpool2_bwd(None, None, None, None, None, None, None, *ok, None, None) == E
    assert fwd(*ok, z=None) == E and fwd(*ok, y=None) == E and fwd(*ok, arg=None) == E
    assert bwd(*ok, dy=None) == E and bwd(*ok, arg=None) == E and bwd(*ok, dz=None) == E
    for k in range(4):                                     # gamma, beta, running_mean, running_var
        par = [one] * 4
        par[k] = None
        assert L.nisqa_bn_eval_act_maxpool2_fwd(one, *par, *ok, one, one, None) == E
        assert L.nisqa_bn_eval_act_maxpool2_bwd(one, one, one, *par, *ok, one, None) == E
    # (n_segments, h, w, c, pad_w): non-positive sizes, c % 4 != 0, c > 256, odd h, pad_w outside {0, 1}, w + 2 pad_w < 2
    for dims in ((0, 48, 15, 16, 1), (-1, 48, 15, 16, 1), (1, 0, 15, 16, 1), (1, -2, 15, 16, 1), (1, 48, 0, 16, 1), (1, 48, -1, 16, 1),
                 (1, 48, 15, 0, 1), (1, 48, 15, -4, 1), (1, 48, 15, 18, 1), (1, 48, 15, 260, 1), (1, 47, 15, 16, 1), (1, 1, 15, 16, 1),
                 (1, 48, 15, 16, 2), (1, 48, 15, 16, -1), (1, 48, 1, 16, 0)):
        assert fwd(*dims) == E, dims
        assert bwd(*dims) == E, dims


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3', 'bf16x3'])
@pytest.mark.parametrize('pool', IL.POOLS)
def test_fast_precisions_refuse_a_gradient_before_any_gpu_work(monkeypatch, pool, precision):
    """the refusal names the precision and comes before the engine is built (building it is GPU work, and raises RuntimeError
    where there is no GPU)"""
    from nisqa_amd import NISQA_lib as NL
    from oracle import ref_shim
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    sd, args, x, n_wins, _ = IL.case(pool)
    m = NL.NISQA(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
    m.load_state_dict(sd, strict=True)
    m.eval()
    with pytest.raises(NotImplementedError, match=precision):
        m(torch.from_numpy(x).requires_grad_(True), torch.as_tensor(n_wins))
    assert m._engine is None
