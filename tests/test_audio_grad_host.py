"""The gradient with respect to the audio samples, host side without a GPU: the float64 restatement of the mel front end
(tests/audio_grad_oracle.py) against the project's mel oracle and against finite differences, the seeded signals' three regimes,
the new C entries' declarations and argument guards, and the refusals of forward_audio before any GPU work."""
import os
import re

import numpy as np
import pytest
import torch

import audio_grad_oracle as AG
import input_grad_oracle as IG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'nisqa_segments_to_mel_bwd': 9, 'nisqa_mel_db_bwd_gate': 9, 'nisqa_mel_bwd_workspace_bytes': 2, 'nisqa_mel_frame_bwd': 16,
           'nisqa_mel_overlap_add_bwd': 9}


@pytest.mark.parametrize('sr', [48000, 16000])
def test_restatement_forward_matches_the_mel_oracle(sr):
    """within 1e-3 dB of oracle.mel.melspec_db_from_audio (librosa's float32 pipeline restated), on the gate signals; measured
    <= 1.1e-5 dB"""
    from oracle import mel as omel
    ys, _ = AG.gate_batch(sr)
    for y in ys:
        with torch.no_grad():
            out = AG.mel_forward(torch.from_numpy(y), sr)[0].numpy()
        want = omel.melspec_db_from_audio(y, sr, fmax=AG.fmax_of(sr))               # [48, T]
        assert out.shape == want.T.shape
        d = np.abs(out - want.T).max()
        print(sr, len(y), 'max |restatement - oracle.mel| dB', d)
        assert d <= 1e-3


@pytest.mark.parametrize('sr', AG.RATES)
def test_signals_hold_the_three_regimes_and_the_gradient_matches_finite_differences(sr):
    """every seeded signal: at least one element clamped by the floor alone with a non-zero g, at least one under amin, the margin
    and the gap of the two largest elements >= 1e-2 dB; the float64 gradient against central differences along three random
    directions, to 1e-6 of the directional derivative's scale"""
    ys, lengths = AG.gate_batch(sr)
    hop = AG.hop_win(sr)[0]
    for b, y in enumerate(ys):
        T = 1 + len(y) // hop
        assert len(y) == lengths[b] and T == AG.FRAMES[b]
        rng = np.random.default_rng(50 + b)
        g = rng.standard_normal((T, 48))
        dy, out, db, margin, gap = AG.mel_vjp(y, sr, g)
        n_floor, n_under = AG.regimes(db, g)
        print(sr, 'clip', b, 'margin', margin, 'gap', gap, 'floor-only', n_floor, 'under amin', n_under)
        assert n_floor >= 1 and n_under >= 1 and margin >= AG.MARGIN_DB and gap >= AG.MARGIN_DB
        assert np.isfinite(dy).all()
        f = lambda v: float((AG.mel_forward(torch.from_numpy(v), sr)[0] * torch.from_numpy(g)).sum())
        y64 = y.astype(np.float64)
        for k in range(3):
            v = rng.standard_normal(len(y))
            eps = 1e-7
            fd = (f(y64 + eps * v) - f(y64 - eps * v)) / (2 * eps)
            an = float(dy @ v)
            scale = float(np.abs(dy) @ np.abs(v))
            print('   direction', k, 'finite difference', fd, 'gradient', an, 'difference / scale', abs(fd - an) / scale)
            assert abs(fd - an) <= 1e-6 * scale


def test_segment_indexing_is_the_oracles():
    """segments_of on time-major rows = oracle.net.segment_specs on the [48, T] spectrogram, and segments_adjoint is its transpose"""
    from oracle import net as onet
    rng = np.random.default_rng(3)
    for T, hop in ((15, 4), (18, 4), (19, 4), (78, 4), (19, 1)):
        rows = rng.standard_normal((T, 48)).astype(np.float32)
        x, n = onet.segment_specs(rows.T, 15, hop, None)
        got = AG.segments_of(rows, hop)
        assert got.shape == (n, 1, 48, 15) and np.array_equal(got, x.numpy())
        dx = rng.standard_normal(got.shape)
        assert abs(float((AG.segments_adjoint(dx, T, hop) * rows).sum()) - float((dx * got).sum())) <= 1e-9 * np.abs(dx).sum()


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
    cfg = lib.MelCfg(4096, 480, 960, 48, 1707, 4000, 1e-8, 80.0)
    import ctypes
    ok = ctypes.byref(cfg)
    tabs = [one] * 6
    gate = lambda g=one, db=one, fl=one, fo=one, b=3, tt=57, c=ok, out=one: L.nisqa_mel_db_bwd_gate(g, db, fl, fo, b, tt, c, out, None)
    frame = lambda pcm=one, co=one, fo=one, b=3, tt=57, c=ok, t=tabs, dm=one, ws=one, nb=57 * 960 * 4: \
        L.nisqa_mel_frame_bwd(pcm, co, fo, b, tt, c, *t, dm, ws, nb, None)
    ola = lambda ws=one, co=one, fo=one, b=3, tt=57, n=30000, c=ok, out=one: L.nisqa_mel_overlap_add_bwd(ws, co, fo, b, tt, n, c, out, None)
    seg = lambda dx=one, l=4, nw=one, fo=one, b=3, tt=57, hop=4, out=one: L.nisqa_segments_to_mel_bwd(dx, l, nw, fo, b, tt, hop, out, None)
    # NULL pointers, one at a time
    for kw in ('g', 'db', 'fl', 'fo', 'c', 'out'):
        assert gate(**{kw: None}) == E, kw
    for kw in ('pcm', 'co', 'fo', 'c', 'dm', 'ws'):
        assert frame(**{kw: None}) == E, kw
    for i in range(6):
        assert frame(t=[None if j == i else one for j in range(6)]) == E, i
    for kw in ('ws', 'co', 'fo', 'c', 'out'):
        assert ola(**{kw: None}) == E, kw
    for kw in ('dx', 'nw', 'fo', 'out'):
        assert seg(**{kw: None}) == E, kw
    # non-positive or impossible sizes
    for b, tt in ((0, 57), (-1, 57), (3, 0), (3, -5), (58, 57)):
        assert gate(b=b, tt=tt) == E and frame(b=b, tt=tt) == E and ola(b=b, tt=tt) == E and seg(b=b, tt=tt) == E, (b, tt)
    assert ola(n=0) == E and ola(n=2) == E and ola(n=-7) == E
    assert seg(l=0) == E and seg(l=-1) == E and seg(hop=0) == E and seg(hop=-4) == E
    for bad in (lib.MelCfg(2048, 480, 960, 48, 1707, 4000, 1e-8, 80.0), lib.MelCfg(4096, 0, 960, 48, 1707, 4000, 1e-8, 80.0),
                lib.MelCfg(4096, 480, 1, 48, 1707, 4000, 1e-8, 80.0), lib.MelCfg(4096, 480, 4097, 48, 1707, 4000, 1e-8, 80.0),
                lib.MelCfg(4096, 480, 960, 40, 1707, 4000, 1e-8, 80.0), lib.MelCfg(4096, 480, 960, 48, 1707, 0, 1e-8, 80.0),
                lib.MelCfg(4096, 480, 960, 48, 1707, 9000, 1e-8, 80.0), lib.MelCfg(4096, 480, 960, 48, 1707, 4000, 0.0, 80.0)):
        c = ctypes.byref(bad)
        assert gate(c=c) == E and frame(c=c) == E and ola(c=c) == E
    # the workspace: sized by the library, refused when smaller
    assert L.nisqa_mel_bwd_workspace_bytes(57, 960) == 57 * 960 * 4
    assert [L.nisqa_mel_bwd_workspace_bytes(*a) for a in ((0, 960), (-1, 960), (57, 1), (57, 4097))] == [0, 0, 0, 0]
    assert frame(nb=57 * 960 * 4 - 1) == lib.NISQA_ERR_WORKSPACE


def _model(model, args):
    from nisqa_amd import NISQA_lib as NL
    from oracle import ref_shim
    m = getattr(NL, model)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
    m.eval()
    return m


def test_forward_audio_refuses_malformed_arguments_before_any_gpu_work():
    args = dict(IG.ARGS['NISQA_DIM'])
    m = _model('NISQA_DIM', args)
    y = torch.zeros(2, 9600)
    bad = [(torch.zeros(2, 9600, dtype=torch.int16), None), (torch.zeros(2, 3, 9600), None), (torch.zeros(()), None),
           (torch.zeros(0, 9600), None), (torch.zeros(2, 0), None), (y.numpy(), None),
           (y, [9600]), (y, [9600, 0]), (y, [9600, 9601]), (y, [9600.5, 9600]), (y, torch.tensor([-1, 9600]))]
    for yy, lengths in bad:
        with pytest.raises(ValueError):
            m.forward_audio(yy, 48000, lengths)
        assert m._engine is None
    with pytest.raises(ValueError):
        m.forward_audio(y, 48000.5)
    with pytest.raises(ValueError, match='Sample too short'):          # 14 frames
        m.forward_audio(torch.zeros(14 * 480 - 1), 48000)
    with pytest.raises(ValueError, match='Sample too short'):          # the second clip's OWN length counts, not the padded row's
        m.forward_audio(torch.zeros(2, 9600), 48000, [9600, 6000])
    assert m._engine is None
    m2 = _model('NISQA_DIM', dict(args, ms_max_segments=2))
    with pytest.raises(ValueError, match='ms_max_segments'):
        m2.forward_audio(torch.zeros(30 * 480), 48000)
    assert m2._engine is None


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3', 'bf16x3'])
@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_fast_precisions_refuse_an_audio_gradient_before_any_gpu_work(monkeypatch, model, precision):
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    m = _model(model, dict(IG.ARGS[model]))
    with pytest.raises(NotImplementedError, match=precision):
        m.forward_audio(torch.zeros(9600, requires_grad=True), 48000)
    assert m._engine is None


def test_an_audio_gradient_through_the_resampler_is_refused_before_any_gpu_work(monkeypatch):
    monkeypatch.delenv('NISQA_HIP_PRECISION', raising=False)
    m = _model('NISQA', dict(IG.ARGS['NISQA'], ms_sr=16000))
    with pytest.raises(NotImplementedError, match='resampler'):
        m.forward_audio(torch.zeros(2, 9600, requires_grad=True), 48000)
    assert m._engine is None
    with pytest.raises(ValueError, match='Sample too short'):          # counted at ms_sr: 0.13 s is 14 frames there too
        m.forward_audio(torch.zeros(6500), 48000)
    assert m._engine is None
