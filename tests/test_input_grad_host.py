"""d model(x, n_wins) / d x, host side without a GPU: the float64 oracle (tests/input_grad_oracle.py) against the reference's own
modules in eval mode and against the committed fixtures, the C entries' argument guards, and the refusal of the fast precisions."""
import os
import re

import numpy as np
import pytest
import torch

import helpers
import input_grad_oracle as IG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'nisqa_bn_eval_act_pool_fwd': 14, 'nisqa_bn_eval_act_pool_bwd': 15, 'nisqa_conv1_segments_fwd': 9,
           'nisqa_conv1_segments_dgrad': 7}


def _reference_model(args, sd):
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip('reference tree not staged')
    return ref_shim.build_reference_model(args, sd)[0]


@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_oracle_gradient_matches_the_reference_modules_in_eval_mode(model):
    """x.grad of the reference's module (float32, eval mode) against the float64 oracle, per clip and head: within 5e-5 of the
    clip's largest entry (measured <= 4.6e-6).  Padding rows get exactly zero on both sides."""
    sd, args, x, n_wins, _ = IG.case(model)
    B, H = len(n_wins), len(IG.heads_of(model))
    gs = [IG.one_hot(B, H, h) for h in range(H)]
    want = IG.oracle(sd, args, x, n_wins, gs)
    ref = _reference_model(args, sd)
    assert not ref.training
    for h, g in enumerate(gs):
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        y = ref(xt, torch.as_tensor(n_wins))
        y.backward(torch.from_numpy(g))
        got, w = xt.grad.numpy(), want['dx'][h]
        assert (np.abs(w).reshape(B, -1).max(1) > 0).all()
        err = IG.clip_error(got, w)
        print(model, 'head', h, 'max |dx| per clip', np.abs(w).reshape(B, -1).max(1), 'relative distance', err)
        assert (err <= 5e-5).all(), (h, err)
        np.testing.assert_allclose(y.detach().numpy(), want['y'], rtol=0, atol=1e-4)
        for b, n in enumerate(n_wins):
            assert (got[b, n:] == 0).all() and (w[b, n:] == 0).all()
    assert want['margin'][np.isfinite(want['margin'])].min() >= 1e-5


@pytest.mark.parametrize('model,name', [('NISQA_DIM', 'dim'), ('NISQA', 'mos')])
def test_fixture_holds_the_reference_gradient_of_the_small_case(model, name):
    """tests/golden/input_grad_*.npz (written by the reference's modules, make_golden_input_grad.py) against the oracle on the case
    rebuilt from the stored seeds, at the same 5e-5."""
    fx = helpers.golden('input_grad_%s.npz' % name)
    spec = IG.SMALL
    assert (int(fx['seed_sd']), int(fx['seed_batch']), fx['frames'].tolist(), int(fx['L'])) == \
        (spec['seed_sd'], spec['seed_batch'], spec['frames'], spec['L'])
    sd, args, x, n_wins, g = IG.case(model)
    assert fx['n_wins'].tolist() == n_wins.tolist() and np.array_equal(fx['g'], g) and fx['dx'].shape == x.shape
    want = IG.oracle(sd, args, x, n_wins, [g])
    err = IG.clip_error(fx['dx'], want['dx'][0])
    print(model, 'fixture against the oracle', err)
    assert (err <= 5e-5).all()
    np.testing.assert_allclose(fx['y'], want['y'], rtol=0, atol=1e-4)


def test_padding_rows_do_not_reach_the_oracle():
    sd, args, x, n_wins, g = IG.case('NISQA')
    xn = IG.case('NISQA', fill=np.nan)[2]
    a, b = IG.oracle(sd, args, x, n_wins, [g]), IG.oracle(sd, args, xn, n_wins, [g])
    assert np.array_equal(a['dx'][0], b['dx'][0]) and np.isfinite(b['dx'][0]).all()


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
    # NULL pointers
    assert L.nisqa_bn_eval_act_pool_fwd(None, None, None, None, None, 1, 12, 5, 64, 6, 3, None, None, None) == E
    assert L.nisqa_bn_eval_act_pool_bwd(None, None, None, None, None, None, None, 1, 12, 5, 64, 6, 3, None, None) == E
    assert L.nisqa_conv1_segments_fwd(None, 4, None, 1, 1, None, None, None, None) == E
    assert L.nisqa_conv1_segments_dgrad(None, None, 1, 4, None, None, None) == E
    # a pooled layer needs arg
    assert L.nisqa_bn_eval_act_pool_fwd(one, one, one, one, one, 1, 12, 5, 64, 6, 3, one, None, None) == E
    assert L.nisqa_bn_eval_act_pool_bwd(one, None, one, one, one, one, one, 1, 12, 5, 64, 6, 3, one, None) == E
    # non-positive or impossible sizes
    for dims in ((0, 12, 5, 64, 6, 3), (-1, 12, 5, 64, 6, 3), (1, 0, 5, 64, 6, 3), (1, 12, 0, 64, 6, 3), (1, 12, 5, 0, 6, 3),
                 (1, 12, 5, 62, 6, 3), (1, 12, 5, 64, 0, 3), (1, 12, 5, 64, 6, 0), (1, 12, 5, 64, 13, 3), (1, 12, 5, 64, 6, 6)):
        assert L.nisqa_bn_eval_act_pool_fwd(one, one, one, one, one, *dims, one, one, None) == E, dims
        assert L.nisqa_bn_eval_act_pool_bwd(one, one, one, one, one, one, one, *dims, one, None) == E, dims
    for l_max, n_clips, n_seg in ((0, 1, 1), (4, 0, 1), (4, 1, 0), (-4, 1, 1)):
        assert L.nisqa_conv1_segments_fwd(one, l_max, one, n_clips, n_seg, one, one, one, None) == E
    for n_clips, l_max in ((0, 4), (1, 0), (-1, 4), (1 << 20, 1 << 12)):
        assert L.nisqa_conv1_segments_dgrad(one, one, n_clips, l_max, one, one, None) == E


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3', 'bf16x3'])
@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_fast_precisions_refuse_a_gradient_before_any_gpu_work(monkeypatch, model, precision):
    """the refusal names the precision and comes before the engine is built (building it is GPU work, and raises RuntimeError
    where there is no GPU)"""
    from nisqa_amd import NISQA_lib as NL, input_grad
    from oracle import ref_shim
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    sd, args, x, n_wins, _ = IG.case(model)
    m = getattr(NL, model)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
    m.load_state_dict(sd, strict=True)
    m.eval()
    with pytest.raises(NotImplementedError, match=precision):
        m(torch.from_numpy(x).requires_grad_(True), torch.as_tensor(n_wins))
    assert m._engine is None
    with pytest.raises(NotImplementedError, match=precision):
        input_grad.check_precision(precision)
    assert [input_grad.check_precision(p) for p in ('f32', 'bf16x6')] == ['f32', 'bf16x6']
