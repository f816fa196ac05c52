"""NISQA_DE.forward_audio, host side without a GPU: its refusals before any GPU work, the float64 composition the GPU tests are held
to (tests/de_audio_grad_oracle.py) against central differences, the seeded signals' tie margins, and the new C entry's declaration,
binding, export and argument guards."""
import os
import re

import numpy as np
import pytest
import torch

import audio_grad_oracle as AG
import de_audio_grad_oracle as DA
import de_oracle as DO
import input_grad_de_oracle as IGD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(args):
    from nisqa_amd import NISQA_lib as NL
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    m.eval()
    return m


def test_forward_audio_refuses_malformed_arguments_before_any_gpu_work():
    args = DA.case(IGD.CONFIGS[0])[1]
    m = _model(args)
    y, z = torch.zeros(2, 9600), torch.zeros(2, 12000)
    bad = [(torch.zeros(2, 9600, dtype=torch.int16), z, None, None), (y, torch.zeros(2, 12000, dtype=torch.int32), None, None),
           (torch.zeros(2, 3, 9600), z, None, None), (y, torch.zeros(()), None, None), (torch.zeros(0, 9600), torch.zeros(0, 12000), None, None),
           (y, torch.zeros(2, 0), None, None), (y.numpy(), z, None, None), (y, z.numpy(), None, None),
           (y, torch.zeros(3, 12000), None, None),                            # another B
           (y[0], z, None, None), (y, z[0], None, None),                      # another rank
           (y, z, [9600], None), (y, z, None, [12000]), (y, z, [9600, 0], None), (y, z, None, [12000, 12001]),
           (y, z, [9600.5, 9600], None), (y, z, None, torch.tensor([-1, 12000]))]
    for yd, yr, ld, lr in bad:
        with pytest.raises(ValueError):
            m.forward_audio(yd, yr, 48000, ld, lr)
        assert m._engine is None
    for sr in (48000.5, 0, -48000):
        with pytest.raises(ValueError):
            m.forward_audio(y, z, sr)
    if torch.cuda.device_count() >= 2:
        with pytest.raises(ValueError, match='different GPUs'):
            m.forward_audio(y.to('cuda:0'), z.to('cuda:1'), 48000)
    # BatchPlan's refusals, on either side, counted at each clip's OWN length
    with pytest.raises(ValueError, match='Sample too short'):
        m.forward_audio(torch.zeros(14 * 480 - 1), torch.zeros(9600), 48000)
    with pytest.raises(ValueError, match='Sample too short'):
        m.forward_audio(torch.zeros(9600), torch.zeros(14 * 480 - 1), 48000)
    with pytest.raises(ValueError, match='Sample too short'):
        m.forward_audio(y, z, 48000, [9600, 9600], [12000, 6000])
    assert m._engine is None
    m2 = _model(dict(args, ms_max_segments=2))
    for yd, yr in ((torch.zeros(30 * 480), torch.zeros(9600)), (torch.zeros(9600), torch.zeros(30 * 480))):
        with pytest.raises(ValueError, match='ms_max_segments'):
            m2.forward_audio(yd, yr, 48000)
    assert m2._engine is None


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3'])
@pytest.mark.parametrize('side', [0, 1])
def test_fast_precisions_refuse_an_audio_gradient_before_any_gpu_work(monkeypatch, side, precision):
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    m = _model(DA.case(IGD.CONFIGS[side])[1])
    with pytest.raises(NotImplementedError, match=precision):
        m.forward_audio(torch.zeros(9600, requires_grad=side == 0), torch.zeros(12000, requires_grad=side == 1), 48000)
    assert m._engine is None


def test_an_audio_gradient_through_the_resampler_is_refused_before_any_gpu_work(monkeypatch):
    monkeypatch.delenv('NISQA_HIP_PRECISION', raising=False)
    m = _model(dict(DA.case(IGD.CONFIGS[0])[1], ms_sr=16000))
    for side in (0, 1):
        with pytest.raises(NotImplementedError, match='resampler'):
            m.forward_audio(torch.zeros(2, 9600, requires_grad=side == 0), torch.zeros(2, 12000, requires_grad=side == 1), 48000)
        assert m._engine is None
    with pytest.raises(ValueError, match='Sample too short'):          # counted at ms_sr: 0.13 s is 14 frames there too
        m.forward_audio(torch.zeros(9600), torch.zeros(6500), 48000)
    assert m._engine is None


def test_compose_de_against_central_differences():
    """One pair of (2, 1) segments (19 and 15 frames) at 48 kHz, the dot_soft config: the float64 composition's d / d y_deg and
    d / d y_ref against central differences of the composed float64 function (restatement -> segments -> double-ended oracle) along
    two random directions per side, within 1e-8 of the directional derivative's scale.  Measured: <= 8.7e-11."""
    config = IGD.CONFIGS[1]
    assert IGD.NAMES[config] == 'dot_soft'
    sd, args, _ = DA.case(config)
    sr, hop = DA.SR, args['ms_seg_hop_length']
    ld, lr = AG.lengths_of(sr, (19, 15))[0], AG.lengths_of(sr, (15, 15))[1]
    yd, yr = AG.smooth_signal(sr, ld, 31).astype(np.float64), AG.smooth_signal(sr, lr, 32).astype(np.float64)
    g = np.array([[0.9]])

    def f(vd, vr, rows_only=False):
        """the composed function in float64 throughout (no rounding of the rows to float32): sum g * y"""
        rows = []
        for v in (vd, vr):
            with torch.no_grad():
                rows.append(AG.mel_forward(torch.from_numpy(v), sr, args['ms_fmax'])[0].numpy())
        if rows_only:
            return rows
        x = np.zeros((1, 2, 2, 48, 15))
        sg = [AG.segments_of(r, hop) for r in rows]
        assert [len(s) for s in sg] == [2, 1]
        x[0, :2, 0:1], x[0, :1, 1:2] = sg[0], sg[1]
        return float((IGD.oracle(sd, args, x, np.array([[2, 1]]), [], margins=False)['y'] * g).sum())

    rows = f(yd, yr, rows_only=True)
    want = DA.compose_de(sd, args, [rows[0]], [rows[1]], [yd], [yr], sr, [g])      # float64 rows: the point is not rounded
    assert want['n_wins'].tolist() == [[2, 1]] and want['x'].dtype == np.float64
    dyd, dyr = want['dy_deg'][0][0], want['dy_ref'][0][0]
    rng = np.random.default_rng(9)
    eps = 1e-7
    for side, (dy, n) in enumerate(((dyd, len(yd)), (dyr, len(yr)))):
        assert np.isfinite(dy).all() and np.abs(dy).max() > 0
        for k in range(2):
            v = rng.standard_normal(n)
            vd, vr = (v, 0.0) if side == 0 else (0.0, v)
            fd = (f(yd + eps * vd, yr + eps * vr) - f(yd - eps * vd, yr - eps * vr)) / (2 * eps)
            an = float(dy @ v)
            scale = float(np.abs(dy) @ np.abs(v))
            print(('degraded', 'reference')[side], 'direction', k, 'finite difference', fd, 'gradient', an, 'difference / scale',
                  abs(fd - an) / scale)
            assert abs(fd - an) <= 1e-8 * scale


@pytest.mark.parametrize('config', IGD.CONFIGS, ids=lambda c: IGD.NAMES[c])
def test_seeded_signals_sit_on_no_tie(config):
    """the end-to-end signals at the float64 restatement's rows: 13 segments in pairs of (1, 2), (3, 1), (2, 4); CNN tie margin and
    top-2 score gap >= 1e-4 = 10 TIE, mel margin >= 1e-2 dB"""
    margin, gap, mel_margin, n_wins = DA.seed_margins(config)
    print(IGD.NAMES[config], 'tie margin', margin, 'score gap', gap, 'mel margin', mel_margin)
    assert n_wins.tolist() == [list(p) for p in DA.PAIRS]
    assert margin >= DA.SEED_MARGIN and gap >= DA.SEED_MARGIN and mel_margin >= AG.MARGIN_DB


def test_entry_is_declared_bound_exported_and_guarded():
    from nisqa_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_train.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(nisqa_[a-z0-9_]+)\s*\(', hdr, re.M))
    name = 'nisqa_mel_segments_fwd'
    assert name in declared and len(lib.TRAIN_SYMBOLS[name][1]) == 10
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert name in set(lib.exported_symbols(lib.LIB_PATH, 'nisqa_'))
    L = lib.load()
    one = 16                                               # a non-NULL, aligned pointer that is never followed: the guards come first
    E = lib.NISQA_ERR_ARG
    seg = lambda mel=one, fl=one, fo=one, nw=one, b=3, tt=57, hop=4, l=4, x=one: L.nisqa_mel_segments_fwd(mel, fl, fo, nw, b, tt, hop, l, x, None)
    for kw in ('mel', 'fl', 'fo', 'nw', 'x'):
        assert seg(**{kw: None}) == E, kw
    for b, tt in ((0, 57), (-1, 57), (3, 0), (3, -5), (58, 57)):
        assert seg(b=b, tt=tt) == E, (b, tt)
    assert seg(hop=0) == E and seg(hop=-4) == E and seg(l=0) == E and seg(l=-1) == E
    assert seg(b=70000, tt=70000, l=40000) == E            # n_clips * L past 2^31
    assert seg(mel=20) == E and seg(x=24) == E             # 128-bit words: 16-byte alignment
