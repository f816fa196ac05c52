"""The cases of tests/train_history_cases.py, checked on the CPU before a GPU is involved: every shape is in the class of the
fused self-attention block it is there for, and at every (model, shape, data seed) torch's float32 evaluation of the oracle
operators stays within 3e-4 of the float64 one on every gradient tensor (1e-5 on the loss, 1e-4 on y_hat) -- a tenth of the bar
tests/test_gpu_train_history.py holds the HIP step to, so that its float64 anchor never rests on a gate flip.  Whoever changes a
shape or a seed hears it here."""
import numpy as np
import pytest

import train_history_cases as C


@pytest.mark.parametrize('shape', sorted(C.SHAPES))
def test_shapes_are_in_the_classes_they_are_there_for(shape):
    L = C.SHAPES[shape]
    S, NP, ksplit, colsum = C.TABLE[shape]
    assert (sum(L), C.padded_tokens(L)) == (S, NP)
    assert C.td_classes(NP) == (ksplit, colsum)
    assert S <= 1048


def test_shapes_cover_what_the_walk_relies_on():
    L = C.SHAPES
    assert sorted(L['EDGE']) == sorted(L['PERM']) and L['EDGE'] != L['PERM']      # same B, S, NP: only the cache key tells them apart
    assert C.TABLE['EDGE'] == C.TABLE['PERM']
    assert {C.TABLE[s][2] for s in L} == {1, 4, 16} and {C.TABLE[s][3] for s in L} == {1, 4}
    for s in ('EDGE', 'TINY'):                                                    # a tile with one valid row, a full tile, one past it
        assert 1 in L[s] and 33 in L[s] and (32 in L[s] or 64 in L[s])
    assert C.WALK.count('TINY') == 2 and C.WALK[0] == C.WALK[-1] == 'BIG'
    assert all(C.padded_tokens(L[s]) < C.TABLE['BIG'][1] for s in L if s != 'BIG')   # everything after BIG reuses its workspace


@pytest.mark.parametrize('model,shape', C.CASES)
def test_float32_oracle_is_close_to_float64_at_the_chosen_seed(model, shape):
    dl, dy, ge = C.f32_oracle_margin(model, shape)
    wk = max(ge, key=ge.get)
    print('%s %s seed %d: float32 oracle against float64: loss %.2e relative, y_hat %.2e, worst gradient tensor %.2e (%s)' % (
        model, shape, C.SEEDS[(model, shape)], dl, dy, ge[wk], wk))
    assert len(ge) > 40
    assert dl < 1e-5
    assert dy < 1e-4
    assert ge[wk] < C.F32_ORACLE_BAR, (wk, ge[wk])


@pytest.mark.parametrize('name', sorted(C.DE_CASES))
def test_double_ended_batches_are_away_from_argmax_ties(name):
    for which in sorted(C.DE_FRAMES):
        gap = C.de_gap(name, which)
        print('%s %s: smallest top-2 gap of the alignment %.3g' % (name, which, gap))
        assert gap >= 1e-4, (which, gap)


def test_adam_restatement_is_torch_optim_adam():
    import torch
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(257)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=1e-3)
    q, m, v = p0, np.zeros(257), np.zeros(257)
    for t in (1, 2, 3):
        g = rng.standard_normal(257) * 10.0 ** rng.integers(-6, 1, 257)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        q, m, v = C.adam_f64(q, g, m, v, t, 1e-3)
        assert np.abs(q - p.detach().numpy()).max() < 1e-12
