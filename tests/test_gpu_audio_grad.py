"""The gradient of the NISQA scores with respect to the audio samples on the MI355X: the kernels of csrc/mel_bwd.hip one by one against
the float64 restatement (tests/audio_grad_oracle.py), the wiring of forward_audio's backward, and forward_audio end to end
against the float64 network oracles pulled back through that restatement, for NISQA_DIM, NISQA and the three StandardCNN +
BiLSTM poolings."""
import ctypes

import numpy as np
import pytest
import torch

import audio_grad_oracle as AG
import input_grad_lstm_oracle as IL
import input_grad_oracle as IG

pytestmark = pytest.mark.gpu
PRECISIONS = ['f32', 'bf16x6']
BAR = 1e-3                  # max |dy - want| <= BAR * max |want| per clip: the bar of tests/test_gpu_input_grad.py
TIE = 1e-5                  # below this gap fp32 may choose differently from float64
MEL_BAR = 1e-4              # the mel backward alone: the mel kernel is allowed 1e-3 dB = 1.15e-4 relative in M, the gradient carries 1 / M
DEV = 'cuda:0'
SR = 48000
FAMILIES = ['NISQA_DIM', 'NISQA'] + list(IL.POOLS)
# seeds of audio_grad_oracle.smooth_signal per family and clip: chosen so that the float64 tie margin of the network at the engine's own
# spectrogram is >= TIE for every segment (nothing is left out)
E2E_SEEDS = dict({f: (13, 417, 811) for f in ('NISQA_DIM', 'NISQA')}, **{f: (13, 487, 888) for f in IL.POOLS})
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _family(family):
    """-> (model class name, state_dict, args, the float64 network oracle, g [3, heads])"""
    if family in IL.POOLS:
        sd, args, _, _, g = IL.case(family)
        return 'NISQA', sd, args, IL.oracle, g
    sd, args, _, _, g = IG.case(family)
    return family, sd, args, IG.oracle, g


def _model(family, precision):
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqa
        from oracle import ref_shim
        cls, sd, args = _family(family)[:3]
        m = getattr(NL, cls)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqa(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model', family, precision), make)


def _mel_engine(sr):
    """an engine whose mel tables are the restatement's at ``sr`` (fmax = min(20000, sr / 2))"""
    def make():
        from nisqa_amd.engine import HipNisqa
        args = dict(IG.ARGS['NISQA'], ms_fmax=AG.fmax_of(sr))
        return HipNisqa(args, IG.case('NISQA')[0], DEV, precision='f32')
    return _cached(('mel engine', sr), make)


def _mel_bwd_c_abi(eng, pcm, plan, sr, g, mel_db, floor):
    """the three entries of the mel backward, straight through the C ABI -> d / d pcm"""
    from nisqa_amd import lib
    L, mt, d = eng.lib, eng.mel_tables(sr), plan.to(eng.device)
    cfg, st = ctypes.byref(mt['cfg']), eng._stream()
    dm = torch.full_like(mel_db, float('nan'))
    lib.check(L.nisqa_mel_db_bwd_gate(_p(g), _p(mel_db), _p(floor), _p(d['frame_off']), plan.n_clips, plan.total_frames, cfg, _p(dm),
                                      st), 'nisqa_mel_db_bwd_gate')
    nb = L.nisqa_mel_bwd_workspace_bytes(plan.total_frames, mt['cfg'].win)
    assert nb == plan.total_frames * mt['cfg'].win * 4
    ws = torch.full((nb // 4,), float('nan'), dtype=torch.float32, device=DEV)
    lib.check(L.nisqa_mel_frame_bwd(_p(pcm), _p(d['clip_off']), _p(d['frame_off']), plan.n_clips, plan.total_frames, cfg,
                                    _p(mt['window']), _p(mt['twiddle']), _p(mt['band_start']), _p(mt['band_len']), _p(mt['band_woff']),
                                    _p(mt['band_w']), _p(dm), _p(ws), nb, st), 'nisqa_mel_frame_bwd')
    dpcm = torch.full((plan.total_samples,), float('nan'), dtype=torch.float32, device=DEV)
    lib.check(L.nisqa_mel_overlap_add_bwd(_p(ws), _p(d['clip_off']), _p(d['frame_off']), plan.n_clips, plan.total_frames,
                                          plan.total_samples, cfg, _p(dpcm), st), 'nisqa_mel_overlap_add_bwd')
    return dpcm


@pytest.mark.parametrize('sr', AG.RATES)
def test_mel_backward_against_the_float64_restatement(sr):
    """Three clips of 15, 23 and 19 frames packed back to back, lengths (T - 1) hop + r with r = 0, an odd remainder, hop - 1; each
    with a loud stretch, exact zeros and quiet noise between amin and the floor (audio_grad_oracle.gate_signal).  A random g on
    the clamped rows; wanted: the float64 restatement's autograd of sum g * out.  Nothing is left out: the signals' margin is
    >= 1e-2 dB (checked here again at the float64 evaluation).  Bar 1e-4 of the clip's largest entry, or ten times the distance of
    the SAME restatement evaluated in float32 on the CPU where that is larger.
    Measured max |got - want| / max |want| per clip (the float32 restatement on the CPU in brackets): 48 kHz 2.4e-7 .. 8.8e-7
    (2.1e-7 .. 6.9e-7), 16 kHz 2.8e-7 .. 4.7e-7 (2.5e-7 .. 5.0e-7), 22.05 kHz 3.0e-7 .. 7.8e-7 (2.7e-7 .. 1.3e-6), 96 kHz
    3.9e-7 .. 1.0e-6 (4.6e-7 .. 1.1e-6); DESIGN.md 4.6.3."""
    eng = _mel_engine(sr)
    ys, lengths = AG.gate_batch(sr)
    plan = eng.plan(lengths, sr)
    assert plan.T.tolist() == list(AG.FRAMES)
    rng = np.random.default_rng(sr)
    g = rng.standard_normal((plan.total_frames, 48)).astype(np.float32)
    pcm = _t(np.concatenate(ys))
    mel_db, floor = eng.mel(pcm, plan, sr, clamp=False)
    gd = _t(g)
    runs = [_mel_bwd_c_abi(eng, pcm, plan, sr, gd, mel_db, floor) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1])                                     # no atomics: the same bits
    got = runs[0].cpu().numpy()
    assert np.isfinite(got).all()
    fo, co = plan.frame_off, plan.clip_off
    for b, y in enumerate(ys):
        gb = g[fo[b]:fo[b + 1]].astype(np.float64)
        want, _, db, margin, gap = AG.mel_vjp(y, sr, gb)
        n_floor, n_under = AG.regimes(db, gb)
        assert n_floor >= 1 and n_under >= 1 and margin >= AG.MARGIN_DB and gap >= AG.MARGIN_DB
        # the forward the backward gates on agrees with the restatement to the project's mel bar
        assert np.abs(mel_db[fo[b]:fo[b + 1]].cpu().numpy() - db).max() <= 1e-3
        f32 = AG.mel_vjp(y, sr, gb, dtype=torch.float32)[0]
        top = np.abs(want).max()
        e32 = np.abs(f32 - want).max() / top
        e = np.abs(got[co[b]:co[b + 1]] - want).max() / top
        print(sr, 'clip', b, 'samples', len(y), 'max |want|', top, 'kernel distance', e, 'float32 restatement distance', e32)
        assert top > 0 and e <= max(MEL_BAR, 10 * e32)
        silent = want == 0                                                   # samples only silent frames read
        assert silent.any() and (got[co[b]:co[b + 1]][silent] == 0).all()
    # the neighbours' samples replaced by other data: a clip's gradient keeps its bits
    for keep in ((1,), (0, 2)):
        other = [y if b in keep else (0.3 * np.random.default_rng(7 + b).standard_normal(len(y))).astype(np.float32)
                 for b, y in enumerate(ys)]
        pcm2 = _t(np.concatenate(other))
        mel2, floor2 = eng.mel(pcm2, plan, sr, clamp=False)
        got2 = _mel_bwd_c_abi(eng, pcm2, plan, sr, gd, mel2, floor2)
        for b in keep:
            assert torch.equal(got2[co[b]:co[b + 1]], runs[0][co[b]:co[b + 1]]), (keep, b)


@pytest.mark.parametrize('seg_hop', [4, 1])
def test_segment_adjoint_against_index_add(seg_hop):
    """T = 15, 18, 19 and 78 frames (seg_hop 4: 1, 1, 2 and 16 segments; the 18-frame clip has three trailing frames no segment
    holds), dx padded to L > the largest count with NaN in the padding rows; against index_add in float64, to 1e-6"""
    from nisqa_amd import lib
    L = lib.load()
    frames = [15, 18, 19, 78]
    n_wins = [len(AG.segment_index(T, seg_hop)) for T in frames]
    if seg_hop == 4:
        assert n_wins == [1, 1, 2, 16]
    l_max = max(n_wins) + 2
    rng = np.random.default_rng(seg_hop)
    dx = np.full((len(frames), l_max, 1, 48, 15), np.nan, dtype=np.float32)
    for b, n in enumerate(n_wins):
        dx[b, :n] = rng.standard_normal((n, 1, 48, 15)).astype(np.float32)
    frame_off = np.concatenate(([0], np.cumsum(frames))).astype(np.int32)
    tt = int(frame_off[-1])
    out = torch.full((tt + 1, 48), 12345.0, dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dxd, nw, fo = _t(dx), _t(np.asarray(n_wins, dtype=np.int32)), _t(frame_off)
    lib.check(L.nisqa_segments_to_mel_bwd(_p(dxd), l_max, _p(nw), _p(fo), len(frames), tt, seg_hop, _p(out), st),
              'nisqa_segments_to_mel_bwd')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[tt] == 12345.0).all() and np.isfinite(got).all()
    for b, (T, n) in enumerate(zip(frames, n_wins)):
        want = AG.segments_adjoint(dx[b, :n].astype(np.float64), T, seg_hop)
        gb = got[frame_off[b]:frame_off[b + 1]]
        e = np.abs(gb - want).max() / np.abs(want).max()
        print('seg_hop', seg_hop, 'T', T, 'segments', n, 'relative distance', e)
        assert e <= 1e-6
        covered = seg_hop * (n - 1) + 15
        assert (gb[covered:] == 0).all() and (want[covered:] == 0).all()
    if seg_hop == 4:
        assert (got[frame_off[1] + 15:frame_off[2]] == 0).all() and frame_off[2] - frame_off[1] - 15 == 3


def _signals(family, nan_padding=True):
    """three clips of 15, 23 and 19 frames at 48 kHz -> (y [3, N] float32 with NaN beyond the lengths, lengths, per-clip samples)"""
    lengths = AG.lengths_of(SR)
    ys = [AG.smooth_signal(SR, n, s) for n, s in zip(lengths, E2E_SEEDS[family])]
    y = np.full((3, max(lengths) + 5), np.nan if nan_padding else 0.0, dtype=np.float32)
    for b, yb in enumerate(ys):
        y[b, :len(yb)] = yb
    return y, np.asarray(lengths), ys


def test_backward_of_forward_audio_is_the_stage_by_stage_composition():
    """mel -> segments -> grad_segments -> segment adjoint -> mel backward through the engine's stage-by-stage API gives
    forward_audio's gradient bit for bit; the segment tensor cut on the device is the oracle's indexing of the clamped rows"""
    m = _model('NISQA_DIM', 'bf16x6')
    eng = m._engine
    y, lengths, ys = _signals('NISQA_DIM')
    g = _t(_family('NISQA_DIM')[4])
    yd = _t(y).requires_grad_(True)
    m.forward_audio(yd, SR, lengths).backward(g)
    plan = eng.plan(lengths, SR)
    pcm = _t(np.concatenate(ys))
    mel_db, floor = eng.mel(pcm, plan, SR, clamp=False)
    clamped, floor2 = eng.mel(pcm, plan, SR, clamp=True)
    assert torch.equal(floor, floor2)
    x = eng.segments_from_mel(clamped, plan)
    for b in range(3):
        rows = clamped[plan.frame_off[b]:plan.frame_off[b + 1]].cpu().numpy()
        n = int(plan.n_wins[b])
        assert np.array_equal(x[b, :n].cpu().numpy(), AG.segments_of(rows, eng.seg_hop)) and (x[b, n:] == 0).all()
    dx = eng.grad_segments(x, plan.n_wins, g)
    dpcm = eng.mel_bwd(pcm, plan, SR, eng.segments_to_mel_bwd(dx, plan), mel_db, floor)
    assert torch.equal(dpcm, eng.grad_audio(pcm, plan, SR, g))
    for b in range(3):
        assert torch.equal(yd.grad[b, :lengths[b]], dpcm[plan.clip_off[b]:plan.clip_off[b + 1]])
        assert (yd.grad[b, lengths[b]:] == 0).all()
    with pytest.raises(AssertionError):
        eng.grad_audio((pcm * 32767).to(torch.int16), plan, SR, g)           # int16 PCM has no gradient


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('family', FAMILIES)
def test_forward_audio_end_to_end_against_float64(family, precision):
    """Three clips of 15, 23 and 19 frames at 48 kHz in a [3, N] batch with NaN beyond the lengths; a random g and, for NISQA_DIM,
    every one-hot head.  Wanted: the float64 network gradient at the segment tensor cut from the engine's own clamped rows,
    pulled back through the float64 restatement at y (audio_grad_oracle.compose).  The network's tie margin at that point is
    >= 1e-5 for every segment and the mel margin >= 1e-2 dB: nothing is left out.
    Measured max |dy - want| / max |want| over clips and heads, f32 / bf16x6: NISQA_DIM 5.2e-6 / 3.4e-6, NISQA 2.3e-6 / 3.7e-6,
    last_step_bi 1.8e-6, avg 1.7e-6, max 1.4e-6 (the BiLSTM family's backward is exact fp32 under either precision); smallest tie
    margin 4.1e-5."""
    cls, sd, args, net_oracle, g = _family(family)
    m = _model(family, precision)
    eng = m._engine
    y, lengths, ys = _signals(family)
    gs = [g] + ([IG.one_hot(3, 5, h) for h in range(5)] if family == 'NISQA_DIM' else [])
    yd = _t(y).requires_grad_(True)
    out = m.forward_audio(yd, SR, lengths)
    assert out.grad_fn is not None and out.is_cuda and tuple(out.shape) == tuple(g.shape)
    with torch.no_grad():
        plain = m.forward_audio(yd, SR, lengths)
    assert plain.grad_fn is None and torch.equal(out.detach(), plain)
    assert m.forward_audio(_t(y), SR, lengths).grad_fn is None               # a plain y: nothing to differentiate
    plan = eng.plan(lengths, SR)
    pcm = _t(np.concatenate(ys))
    assert torch.equal(plain, eng.forward_pcm(pcm, plan, SR))
    clamped = eng.mel(pcm, plan, SR, clamp=True)[0].cpu().numpy()
    rows = [clamped[plan.frame_off[b]:plan.frame_off[b + 1]] for b in range(3)]
    want = _cached(('want', family), lambda: AG.compose(net_oracle, sd, args, rows, ys, SR, gs))
    assert want['n_wins'].tolist() == plan.n_wins.tolist()
    margin = want['margin'][np.isfinite(want['margin'])]
    print(family, precision, 'smallest tie margin', margin.min(), 'mel margin', want['mel_margin'], 'gap', want['mel_gap'])
    assert margin.min() >= TIE and (want['mel_margin'] >= AG.MARGIN_DB).all()
    np.testing.assert_allclose(plain.cpu().numpy(), want['y'], rtol=0, atol=1e-3)
    worst = 0.0
    for k, gk in enumerate(gs):
        dy, = torch.autograd.grad(out, yd, _t(gk), retain_graph=True)
        assert dy.shape == yd.shape and dy.dtype == torch.float32 and dy.device == yd.device
        got = dy.cpu().numpy()
        assert np.isfinite(got).all()
        for b, n in enumerate(lengths):
            assert (got[b, n:] == 0).all()                                   # exact zeros: the NaN there does not leak
        err = AG.clip_errors([got[b, :n] for b, n in enumerate(lengths)], want['dy'][k])
        print(family, precision, 'random g' if k == 0 else 'head %d' % (k - 1), 'max |want| per clip',
              [float(np.abs(w).max()) for w in want['dy'][k]], 'relative distance', err)
        worst = max(worst, float(err.max()))
        assert (err <= BAR).all(), (k, err)
    print(family, precision, 'worst relative distance', worst)
    a, = torch.autograd.grad(out, yd, _t(g), retain_graph=True)
    b_, = torch.autograd.grad(out, yd, _t(g))
    assert torch.equal(a, b_)                                                # twice the same bits
    # a float64 y on the host gets a float64 gradient on the host
    yh = torch.from_numpy(y).double().requires_grad_(True)
    oh = m.forward_audio(yh, SR, lengths)
    assert oh.grad_fn is not None and torch.equal(oh.detach(), plain)
    oh.backward(_t(g))
    assert yh.grad.device.type == 'cpu' and yh.grad.dtype == torch.float64 and yh.grad.shape == yh.shape
    assert torch.equal(yh.grad.float(), a.cpu())


def test_one_clip_without_lengths_is_the_batch_of_one():
    m = _model('NISQA', 'bf16x6')
    y1 = AG.smooth_signal(SR, AG.lengths_of(SR)[1], 5)
    g = _t(np.array([[0.7]], dtype=np.float32))
    a = _t(y1).requires_grad_(True)
    b = _t(y1[None]).requires_grad_(True)
    oa, ob = m.forward_audio(a, SR), m.forward_audio(b, SR, [len(y1)])
    assert tuple(oa.shape) == (1, 1) and torch.equal(oa, ob)
    oa.backward(g)
    ob.backward(g)
    assert a.grad.shape == a.shape and torch.equal(a.grad, b.grad[0]) and np.isfinite(a.grad.cpu().numpy()).all()
    assert float(a.grad.abs().max()) > 0


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3', 'bf16x3'])
def test_plain_call_in_the_fast_precisions_is_forward_pcm(precision):
    m = _model('NISQA_DIM', precision)
    y, lengths, ys = _signals('NISQA_DIM')
    out = m.forward_audio(_t(y), SR, lengths)
    eng = m._engine
    assert torch.equal(out, eng.forward_pcm(_t(np.concatenate(ys)), eng.plan(lengths, SR), SR))
    with pytest.raises(NotImplementedError, match=precision):
        m.forward_audio(_t(y).requires_grad_(True), SR, lengths)


def test_plain_call_resamples_when_the_checkpoint_sets_ms_sr():
    """ms_sr = 16 kHz, audio at 48 kHz: the plain call is the engine's forward_audio (resample + forward_pcm); a gradient is refused"""
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import HipNisqa
    from oracle import ref_shim
    sd, args = IG.case('NISQA')[:2]
    args = dict(args, ms_sr=16000)
    m = NL.NISQA(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
    m.load_state_dict(sd, strict=True)
    m.eval()
    eng = m._engine = HipNisqa(args, m.state_dict(), DEV, precision='bf16x6')
    y, lengths, ys = _signals('NISQA')
    out = m.forward_audio(_t(y), SR, lengths)
    pcm = _t(np.concatenate(ys))
    assert torch.equal(out, eng.forward_audio(pcm, lengths, SR, eng.audio_plan(lengths, SR)))
    with pytest.raises(NotImplementedError, match='resampler'):
        m.forward_audio(_t(y).requires_grad_(True), SR, lengths)
