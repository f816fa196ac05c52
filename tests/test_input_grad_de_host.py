"""d model(x, n_wins) / d x of NISQA_DE, host side without a GPU: the float64 oracle (tests/input_grad_de_oracle.py) against the
fixtures the reference's own NISQA_DE module wrote in eval mode, the seeded cases' tie statistics, the new C entries' declaration,
binding and argument guards, and the refusal of the fast precisions."""
import os
import re

import numpy as np
import pytest
import torch

import de_oracle as DO
import helpers
import input_grad_de_oracle as IGD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'nisqa_de_align_soft_packed': 15, 'nisqa_de_align_soft_bwd': 16}
BAR = 5e-5                  # the bar of tests/test_input_grad_host.py for the reference's fp32 gradient against float64
_CACHE = {}


def _oracle(config, spec_name):
    key = (config, spec_name)
    if key not in _CACHE:
        sd, args, x, n_wins, g = IGD.case(config, getattr(IGD, spec_name))
        _CACHE[key] = (x, n_wins, g, IGD.oracle(sd, args, x, n_wins, [g]))
    return _CACHE[key]


@pytest.mark.parametrize('config', IGD.CONFIGS, ids=lambda c: IGD.NAMES[c])
def test_fixture_holds_the_reference_gradient_of_the_small_case(config):
    """tests/golden/input_grad_de_*.npz (y and x.grad of the reference's NISQA_DE in eval mode, float32; make_golden_input_grad_de.py)
    against the float64 oracle on the case rebuilt from the stored seeds, per clip and channel, within 5e-5 of that channel's
    largest entry.  Measured: cos_hard <= 4.0e-6, dot_soft <= 3.0e-6, cos_soft <= 3.9e-6 (an fp32 CPU run of the oracle chain itself:
    4.3e-6, 3.2e-6, 3.7e-6).  Padding rows are exact zeros on both sides."""
    fx = helpers.golden('input_grad_de_%s.npz' % IGD.NAMES[config])
    spec = IGD.SMALL
    assert (int(fx['seed_sd']), int(fx['seed_batch']), fx['pairs'].tolist(), int(fx['L'])) == \
        (spec['seed_sd'], spec['seed_batch'], [list(p) for p in spec['pairs']], spec['L'])
    assert (str(fx['align']), str(fx['apply']), str(fx['fuse'])) == config
    x, n_wins, g, want = _oracle(config, 'SMALL')
    assert fx['n_wins'].tolist() == n_wins.tolist() and np.array_equal(fx['g'], g) and fx['dx'].shape == x.shape
    w = want['dx'][0]
    assert (np.abs(w).reshape(len(n_wins), x.shape[1], 2, -1).max((1, 3)) > 0).all()
    err = IGD.channel_error(fx['dx'], w)
    print(IGD.NAMES[config], 'reference fp32 x.grad against the float64 oracle, per clip and channel', err)
    assert (err <= BAR).all()
    np.testing.assert_allclose(fx['y'], want['y'], rtol=0, atol=1e-4)
    for b in range(len(n_wins)):
        for c in range(2):
            assert (fx['dx'][b, n_wins[b, c]:, c] == 0).all() and (w[b, n_wins[b, c]:, c] == 0).all()


def test_small_case_sits_on_no_tie():
    """nothing is left out of SMALL and every hard index is comparable: the smallest CNN tie margin is 1.78e-5, the smallest top-2
    gap of the cosine scores 1.04e-4"""
    for config in IGD.CONFIGS:
        want = _oracle(config, 'SMALL')[3]
        m = want['margin']
        assert np.isfinite(m).sum() == 12 and m[np.isfinite(m)].min() >= IGD.TIE
        assert min(float(gp.min()) for gp in want['gap']) > IGD.TIE


def test_edge_case_leaves_out_at_most_15_percent():
    """(65, 3), (1, 65), (64, 64): 28 of the 262 segments have a float64 CNN tie margin under 1e-5 (10.7 %), and cosine scores come
    within 1.2e-6 of each other: hence the index override at gaps <= 1e-5"""
    config = IGD.CONFIGS[0]
    sd, args, x, n_wins, g = IGD.case(config, IGD.EDGE)
    want = IGD.oracle(sd, args, x, n_wins, [])
    m = want['margin']
    valid = np.isfinite(m)
    out = valid & (m < IGD.TIE)
    print('segments', int(valid.sum()), 'left out', int(out.sum()), 'near-tie tokens', sum(int((gp <= IGD.TIE).sum()) for gp in want['gap']))
    assert valid.sum() == 262 and 0 < out.sum() <= 0.15 * valid.sum()
    assert min(float(gp.min()) for gp in want['gap']) <= IGD.TIE
    # the override gathers the given row only at a near-tie
    flipped = [np.where(gp <= IGD.TIE, (own + 1) % n_wins[b, 1], own) for b, (gp, own) in enumerate(zip(want['gap'], want['own']))]
    again = IGD.oracle(sd, args, x, n_wins, [], idx=flipped, margins=False)
    for b in range(len(n_wins)):
        near = want['gap'][b] <= IGD.TIE
        assert (again['idx'][b][near] == flipped[b][near]).all() and (again['idx'][b][~near] == want['own'][b][~near]).all()


def test_padding_rows_do_not_reach_the_oracle():
    config = IGD.CONFIGS[1]
    sd, args, x, n_wins, g = IGD.case(config)
    xn = IGD.case(config, fill=np.nan)[2]
    a, b = IGD.oracle(sd, args, x, n_wins, [g]), IGD.oracle(sd, args, xn, n_wins, [g])
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
    fwd = lambda p=one, n_pairs=1, n_tiles=1, align=0, fuse=0, ld=192: L.nisqa_de_align_soft_packed(
        p, p, p, p, p, p, n_pairs, n_tiles, align, fuse, ld, p, p, p, None)
    bwd = lambda p=one, n_pairs=1, n_max=1, align=0, fuse=0, ld=192: L.nisqa_de_align_soft_bwd(
        p, p, ld, p, p, p, p, p, p, n_pairs, n_max, align, fuse, p, p, None)
    assert fwd(None) == E and bwd(None) == E
    for k in range(15):                                    # every pointer on its own
        if lib.TRAIN_SYMBOLS['nisqa_de_align_soft_packed'][1][k] is lib.c_p and k != 14:
            a = [one, one, one, one, one, one, 1, 1, 0, 0, 192, one, one, one, None]
            a[k] = None
            assert L.nisqa_de_align_soft_packed(*a) == E, k
    for k in range(16):
        if lib.TRAIN_SYMBOLS['nisqa_de_align_soft_bwd'][1][k] is lib.c_p and k != 15:
            a = [one, one, 192, one, one, one, one, one, one, 1, 1, 0, 0, one, one, None]
            a[k] = None
            assert L.nisqa_de_align_soft_bwd(*a) == E, k
    for kw in (dict(align=-1), dict(align=2), dict(fuse=-1), dict(fuse=3), dict(ld=191), dict(ld=190), dict(fuse=1, ld=127),
               dict(fuse=2, ld=124), dict(n_pairs=0)):
        assert fwd(**kw) == E and bwd(**kw) == E, kw
    assert fwd(n_pairs=2, n_tiles=1) == E and bwd(n_max=0) == E and bwd(n_pairs=65536) == E


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3'])
@pytest.mark.parametrize('config', IGD.CONFIGS, ids=lambda c: IGD.NAMES[c])
def test_fast_precisions_refuse_a_gradient_before_any_gpu_work(monkeypatch, config, precision):
    """the refusal names the precision and comes before the engine is built (building it is GPU work)"""
    from nisqa_amd import NISQA_lib as NL
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    sd, args, x, n_wins, _ = IGD.case(config)
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    m.load_state_dict(sd, strict=True)
    m.eval()
    with pytest.raises(NotImplementedError, match=precision):
        m(torch.from_numpy(x).requires_grad_(True), torch.as_tensor(n_wins))
    assert m._engine is None
