"""NISQA_DE.forward_audio on the MI355X: the device kernel that clamps and cuts the segment tensor (nisqa_mel_segments_fwd) bit for
bit against the indexing path, the plain call against HipNisqaDE.forward_pcm in every precision, the wiring of the backward stage by
stage, both gradients end to end against the float64 oracle (tests/de_audio_grad_oracle.py), and the contract around them
(needs_input_grad, ranks, dtypes, devices)."""
import ctypes

import numpy as np
import pytest
import torch

import audio_grad_oracle as AG
import de_audio_grad_oracle as DA
import de_oracle as DO
import input_grad_de_oracle as IGD

pytestmark = pytest.mark.gpu
BAR = 1e-3                  # the project's input-gradient bar: max |d - want| <= BAR * max |want| per clip and side
DEV = 'cuda:0'
SR = DA.SR
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _model(config, precision, **extra):
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqaDE
        sd, args, _ = DA.case(config)
        args = dict(args, **extra)
        m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqaDE(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model', config, precision, tuple(sorted(extra.items()))), make)


def _batch(ys, lengths, fill=np.nan, extra=5):
    """per-clip samples -> [B, N] float32 with ``fill`` beyond the lengths"""
    y = np.full((len(ys), int(max(lengths)) + extra), fill, dtype=np.float32)
    for b, yb in enumerate(ys):
        y[b, :len(yb)] = yb
    return y


def _signals(config):
    """-> (y_deg [3, N], y_ref [3, M] with NaN beyond the lengths, N != M; lengths; per-clip samples; the packed 2B clips)"""
    def make():
        ys_d, ys_r, ld, lr = DA.signals(IGD.NAMES[config])
        yd, yr = _batch(ys_d, ld, extra=5), _batch(ys_r, lr, extra=9)
        assert yd.shape[1] != yr.shape[1]
        return yd, yr, ld, lr, ys_d, ys_r, np.concatenate(ys_d + ys_r)
    return _cached(('signals', config), make)


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seg_hop', [4, 1])
def test_segment_kernel_is_the_indexing_path_bit_for_bit(seg_hop):
    """Clips of 15, 18, 19 and 78 frames (seg_hop 4: one segment; one segment and three trailing frames no segment holds; two
    overlapping segments; 16 segments), L = the largest count + 2, x pre-filled with NaN with a guard region behind it.  Random dB
    rows, per-clip floors at the clip's 30 % quantile with one element set to the floor exactly.  torch.equal with
    segments_from_mel(torch.maximum(mel_db, floor of the frame's clip)), exact zeros in the rows k >= n_wins[b], the guard
    untouched, two runs the same bits; the entry's NULL and size checks.  (At 64 clips x 10 s the kernel takes 13.1 us against
    0.675 ms for the indexing path: DESIGN.md 4.8.3.)"""
    from nisqa_amd import lib
    from nisqa_amd.engine import BatchPlan, HipNisqaDE
    Lb = lib.load()
    config = IGD.CONFIGS[0]
    eng = _model(config, 'f32')._engine.base if seg_hop == 4 else \
        _cached(('hop1',), lambda: HipNisqaDE(dict(DA.case(config)[1], ms_seg_hop_length=1), DA.case(config)[0], DEV, precision='f32')).base
    assert eng.seg_hop == seg_hop
    frames = [15, 18, 19, 78]
    hop = 480
    plan = BatchPlan([(T - 1) * hop for T in frames], hop, seg_hop, None)
    assert plan.T.tolist() == frames
    n_wins = [len(AG.segment_index(T, seg_hop)) for T in frames]
    assert plan.n_wins.tolist() == n_wins and (seg_hop != 4 or n_wins == [1, 1, 2, 16])
    L = max(n_wins) + 2
    rng = np.random.default_rng(20 + seg_hop)
    mel = (rng.standard_normal((plan.total_frames, 48)) * 20.0 - 30.0).astype(np.float32)
    floor = np.zeros(len(frames), np.float32)
    for b in range(len(frames)):
        rows = mel[plan.frame_off[b]:plan.frame_off[b + 1]]
        floor[b] = np.quantile(rows[:15], 0.3).astype(np.float32)
        rows[7, 5 + b] = floor[b]                                             # inside the first segment: exactly the floor
        under = float((rows[:15] < floor[b]).mean())
        assert 0.1 < under < 0.6
    mel_d, floor_d = _t(mel), _t(floor)
    d = plan.to(torch.device(DEV))
    n_x = len(frames) * L * 720
    guard = 4096
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        buf = torch.full((n_x + guard,), float('nan'), dtype=torch.float32, device=DEV)
        lib.check(Lb.nisqa_mel_segments_fwd(_p(mel_d), _p(floor_d), _p(d['frame_off']), _p(d['n_wins']), len(frames),
                                            plan.total_frames, seg_hop, L, _p(buf), st), 'nisqa_mel_segments_fwd')
        runs.append(buf)
    torch.cuda.synchronize()
    assert torch.isnan(runs[0][n_x:]).all() and torch.isnan(runs[1][n_x:]).all()          # the guard is untouched
    x = runs[0][:n_x].view(len(frames), L, 1, 48, 15)
    assert torch.equal(x, runs[1][:n_x].view_as(x))
    clip_of_frame = torch.from_numpy(np.repeat(np.arange(plan.n_clips), plan.T)).to(DEV)
    want = eng.segments_from_mel(torch.maximum(mel_d, floor_d[clip_of_frame][:, None]), plan)     # [B, max n_wins, 1, 48, 15]
    assert torch.equal(x[:, :max(n_wins)], want)
    for b, n in enumerate(n_wins):
        assert (x[b, n:] == 0).all() and bool((x[b, :n] == floor[b]).any()) and bool((x[b, :n] > floor[b]).any())
    # the engine's entry: the same bits at its default L, and at a larger one; a smaller one is refused
    assert torch.equal(eng.segments_from_mel_db(mel_d, floor_d, plan), want)
    assert torch.equal(eng.segments_from_mel_db(mel_d, floor_d, plan, L=L), x)
    with pytest.raises(ValueError):
        eng.segments_from_mel_db(mel_d, floor_d, plan, L=max(n_wins) - 1)
    # NULL pointers and sizes: NISQA_ERR_ARG before any launch
    E = lib.NISQA_ERR_ARG
    ok = [_p(mel_d), _p(floor_d), _p(d['frame_off']), _p(d['n_wins']), len(frames), plan.total_frames, seg_hop, L, _p(runs[1]), st]
    for k in (0, 1, 2, 3, 8):
        a = list(ok)
        a[k] = None
        assert Lb.nisqa_mel_segments_fwd(*a) == E, k
    for k, bad in ((4, 0), (4, -1), (4, plan.total_frames + 1), (5, 0), (5, -3), (6, 0), (6, -4), (7, 0), (7, -1)):
        a = list(ok)
        a[k] = bad
        assert Lb.nisqa_mel_segments_fwd(*a) == E, (k, bad)
    torch.cuda.synchronize()
    assert torch.equal(runs[1][:n_x], runs[0][:n_x]) and torch.isnan(runs[1][n_x:]).all()          # a refused call wrote nothing


# ---- the plain call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16x6', 'f16x4', 'f16x3'])
def test_plain_call_is_forward_pcm(precision):
    """[3, N] / [3, M] batches, N != M, NaN beyond the lengths: bit for bit HipNisqaDE.forward_pcm on the packed samples, degraded
    clips first; the two fast precisions refuse a gradient, naming themselves"""
    config = IGD.CONFIGS[0]
    m = _model(config, precision)
    eng = m._engine
    yd, yr, ld, lr, ys_d, ys_r, packed = _signals(config)
    out = m.forward_audio(_t(yd), _t(yr), SR, ld, lr)
    assert tuple(out.shape) == (3, 1) and out.is_cuda and out.grad_fn is None
    plan = eng.plan(ld, lr, SR)
    assert torch.equal(out, eng.forward_pcm(_t(packed), plan, SR))
    assert np.isfinite(out.cpu().numpy()).all()
    if precision in ('f16x4', 'f16x3'):
        for req in ((True, False), (False, True)):
            with pytest.raises(NotImplementedError, match=precision):
                m.forward_audio(_t(yd).requires_grad_(req[0]), _t(yr).requires_grad_(req[1]), SR, ld, lr)


def test_plain_call_resamples_when_the_checkpoint_sets_ms_sr():
    """ms_sr = 16 kHz, audio at 48 kHz: the plain call is HipNisqaDE.forward_audio (resample + forward_pcm); a gradient is refused"""
    config = IGD.CONFIGS[0]
    m = _model(config, 'bf16x6', ms_sr=16000)
    eng = m._engine
    yd, yr, ld, lr, ys_d, ys_r, packed = _signals(config)
    out = m.forward_audio(_t(yd), _t(yr), SR, ld, lr)
    assert torch.equal(out, eng.forward_audio(_t(packed), ld, lr, SR, eng.audio_plan(ld, lr, SR)))
    assert np.isfinite(out.cpu().numpy()).all()
    with pytest.raises(NotImplementedError, match='resampler'):
        m.forward_audio(_t(yd).requires_grad_(True), _t(yr), SR, ld, lr)


# ---- the backward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('config', IGD.CONFIGS[:2], ids=lambda c: IGD.NAMES[c])
def test_backward_is_the_stage_by_stage_composition(config):
    """mel -> nisqa_mel_segments_fwd -> grad_segments on the [B, L, 2, 48, 15] view of the same values -> segment adjoint -> mel
    backward, through the engine's public stages, gives forward_audio's two gradients bit for bit"""
    m = _model(config, 'bf16x6')
    eng, b = m._engine, m._engine.base
    yd, yr, ld, lr, ys_d, ys_r, packed = _signals(config)
    g = _t(DA.case(config)[2])
    a, r = _t(yd).requires_grad_(True), _t(yr).requires_grad_(True)
    m.forward_audio(a, r, SR, ld, lr).backward(g)
    plan = eng.plan(ld, lr, SR)
    pcm = _t(packed)
    mel_db, floor = b.mel(pcm, plan, SR, clamp=False)
    x2 = b.segments_from_mel_db(mel_db, floor, plan)
    assert torch.equal(x2, b.segments_from_mel(b.mel(pcm, plan, SR, clamp=True)[0], plan))
    B = 3
    x = torch.cat([x2[:B], x2[B:]], 2)
    n = np.stack([plan.n_wins[:B], plan.n_wins[B:]], 1)
    assert n.tolist() == [list(p) for p in DA.PAIRS]
    dx = eng.grad_segments(x, n, g)
    dx2 = torch.cat([dx[:, :, 0:1], dx[:, :, 1:2]], 0).contiguous()
    dpcm = b.mel_bwd(pcm, plan, SR, b.segments_to_mel_bwd(dx2, plan), mel_db, floor)
    d_deg, d_ref = eng.grad_audio(pcm, plan, SR, g)
    assert torch.equal(torch.cat([d_deg, d_ref]), dpcm)
    co = plan.clip_off
    for k in range(B):
        assert torch.equal(a.grad[k, :ld[k]], dpcm[co[k]:co[k + 1]]) and (a.grad[k, ld[k]:] == 0).all()
        assert torch.equal(r.grad[k, :lr[k]], dpcm[co[B + k]:co[B + k + 1]]) and (r.grad[k, lr[k]:] == 0).all()
    assert float(a.grad.abs().max()) > 0 and float(r.grad.abs().max()) > 0


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
@pytest.mark.parametrize('config', IGD.CONFIGS, ids=lambda c: IGD.NAMES[c])
def test_forward_audio_end_to_end_against_float64(config, precision):
    """Three pairs at 48 kHz, degraded clips of 15 / 23 / 19 frames and reference clips of 19 / 15 / 27 frames -- (1, 2), (3, 1) and
    (2, 4) segments -- in [3, N] / [3, M] batches with NaN beyond the lengths.  Wanted: de_audio_grad_oracle.compose_de at the
    segment tensors cut from the engine's own clamped rows (hard alignment: idx from InputGradDE.last_idx).  Nothing is left out:
    the float64 CNN tie margin of every segment is >= TIE, every degraded token's top-2 score gap > TIE and the mel margin
    >= 1e-2 dB at the engine's rows (the seeds were chosen with ten times that room at the restatement's rows), and the hard
    indices are float64's own.  Bar: max |d - want| <= 1e-3 max |want| per clip and side; dot_soft max(1e-3, 2 x the float32 CPU run
    of the same oracle chain).
    Measured max |d - want| / max |want| over clips and sides, f32 / bf16x6: cos_hard 8.0e-6 / 8.5e-6, dot_soft 5.0e-6 / 6.5e-6 (the
    float32 CPU run of the oracle chain: <= 3.1e-6, so its bar stayed 1e-3), cos_soft 5.4e-6 / 6.1e-6; at the engine's rows the
    smallest tie margin is 1.03e-4, the smallest score gap 2.0e-4 (cosine) / 8.3e-3 (dot), the mel margin 28 dB."""
    sd, args, g = DA.case(config)
    m = _model(config, precision)
    eng = m._engine
    hard = config[1] == 'hard'
    yd, yr, ld, lr, ys_d, ys_r, packed = _signals(config)
    a, r = _t(yd).requires_grad_(True), _t(yr).requires_grad_(True)
    out = m.forward_audio(a, r, SR, ld, lr)
    assert out.grad_fn is not None and out.is_cuda and tuple(out.shape) == (3, 1)
    with torch.no_grad():
        plain = m.forward_audio(a, r, SR, ld, lr)
    assert plain.grad_fn is None and torch.equal(out.detach(), plain)
    da, dr = torch.autograd.grad(out, (a, r), _t(g), retain_graph=True)
    idx = None
    if hard:
        flat = eng._input_grad.last_idx.cpu().numpy()
        idx = np.split(flat, np.cumsum([p[0] for p in DA.PAIRS])[:-1])
    da2, dr2 = torch.autograd.grad(out, (a, r), _t(g))
    assert torch.equal(da, da2) and torch.equal(dr, dr2)                     # twice the same bits
    plan = eng.plan(ld, lr, SR)
    clamped = eng.base.mel(_t(packed), plan, SR, clamp=True)[0].cpu().numpy()
    rows = [clamped[plan.frame_off[c]:plan.frame_off[c + 1]] for c in range(6)]

    def make():
        want = DA.compose_de(sd, args, rows[:3], rows[3:], ys_d, ys_r, SR, [g], idx=idx)
        want['dx32'] = None
        if config[:2] == ('dot', 'soft'):                                    # what float32 arithmetic alone costs the same chain
            net32 = IGD.oracle(sd, args, want['x'], want['n_wins'], [g], dtype=torch.float32, margins=False)['dx'][0]
            want['dx32'] = [[AG.mel_vjp(y, SR, AG.segments_adjoint(net32[k, :want['n_wins'][k, c], c:c + 1].astype(np.float64),
                                                                   rows[3 * c + k].shape[0], args['ms_seg_hop_length']),
                                        args['ms_fmax'], dtype=torch.float32)[0] for k, y in enumerate(ys)]
                            for c, ys in enumerate((ys_d, ys_r))]
        return want
    key = None if idx is None else tuple(np.concatenate(idx).tolist())
    want = _cached(('want', config, key, clamped.tobytes()), make)
    assert want['n_wins'].tolist() == [list(p) for p in DA.PAIRS]
    margin = want['margin'][np.isfinite(want['margin'])]
    gap = min(float(gp.min()) for gp in want['gap'])
    print(IGD.NAMES[config], precision, 'smallest tie margin', margin.min(), 'smallest score gap', gap, 'mel margin',
          want['mel_margin'].min())
    assert margin.size == 13 and margin.min() >= IGD.TIE and gap > IGD.TIE and (want['mel_margin'] >= AG.MARGIN_DB).all()
    if hard:
        for k in range(3):
            assert (idx[k] == want['own'][k]).all() and ((idx[k] >= 0) & (idx[k] < DA.PAIRS[k][1])).all()
    np.testing.assert_allclose(plain.cpu().numpy(), want['y'], rtol=0, atol=1e-3)
    worst = 0.0
    for c, (d, y_in, lengths, w) in enumerate(((da, a, ld, want['dy_deg'][0]), (dr, r, lr, want['dy_ref'][0]))):
        assert d.shape == y_in.shape and d.dtype == torch.float32 and d.device == y_in.device
        got = d.cpu().numpy()
        assert np.isfinite(got).all()
        for k, n in enumerate(lengths):
            assert (got[k, n:] == 0).all()                                   # exact zeros: the NaN there does not leak
        err = AG.clip_errors([got[k, :n] for k, n in enumerate(lengths)], w)
        bar = BAR
        if want['dx32'] is not None:
            e32 = AG.clip_errors(want['dx32'][c], w)
            bar = max(BAR, 2.0 * float(e32.max()))
            print('   float32 CPU run of the oracle chain against float64', e32)
        print(IGD.NAMES[config], precision, ('degraded', 'reference')[c], 'max |want| per clip', [float(np.abs(v).max()) for v in w],
              'relative distance', err, 'bar', bar)
        worst = max(worst, float(err.max()))
        assert all(np.abs(v).max() > 0 for v in w) and (err <= bar).all(), (c, err)
    print(IGD.NAMES[config], precision, 'worst relative distance', worst)


@pytest.mark.parametrize('config', IGD.CONFIGS[:2], ids=lambda c: IGD.NAMES[c])
def test_only_the_side_that_requires_a_gradient_gets_one(config):
    m = _model(config, 'bf16x6')
    yd, yr, ld, lr = _signals(config)[:4]
    g = _t(DA.case(config)[2])
    a, r = _t(yd).requires_grad_(True), _t(yr).requires_grad_(True)
    m.forward_audio(a, r, SR, ld, lr).backward(g)
    a1, r1 = _t(yd).requires_grad_(True), _t(yr)
    o1 = m.forward_audio(a1, r1, SR, ld, lr)
    assert o1.grad_fn is not None
    o1.backward(g)
    assert r1.grad is None and torch.equal(a1.grad, a.grad)
    a2, r2 = _t(yd), _t(yr).requires_grad_(True)
    o2 = m.forward_audio(a2, r2, SR, ld, lr)
    assert o2.grad_fn is not None and torch.equal(o2.detach(), o1.detach())
    o2.backward(g)
    assert a2.grad is None and torch.equal(r2.grad, r.grad)
    assert m.forward_audio(_t(yd), _t(yr), SR, ld, lr).grad_fn is None
    # the engine's entry: None for the side not named
    eng = m._engine
    plan = eng.plan(ld, lr, SR)
    pcm = _t(_signals(config)[6])
    both = eng.grad_audio(pcm, plan, SR, g)
    d0 = eng.grad_audio(pcm, plan, SR, g, need=(True, False))
    d1 = eng.grad_audio(pcm, plan, SR, g, need=(False, True))
    assert d0[1] is None and d1[0] is None and torch.equal(d0[0], both[0]) and torch.equal(d1[1], both[1])


def test_ranks_dtypes_and_devices():
    """rank-1 y_deg / y_ref without lengths is the batch of one; a float64 host y_deg with a float32 device y_ref gets a float64
    host gradient and a float32 device gradient, equal after conversion to the all-device float32 run's"""
    config = IGD.CONFIGS[1]
    m = _model(config, 'bf16x6')
    ys_d, ys_r = _signals(config)[4:6]
    yd, yr = ys_d[1], ys_r[2]
    g = _t(np.array([[0.7]], dtype=np.float32))
    a, r = _t(yd).requires_grad_(True), _t(yr).requires_grad_(True)
    ab, rb = _t(yd[None]).requires_grad_(True), _t(yr[None]).requires_grad_(True)
    oa, ob = m.forward_audio(a, r, SR), m.forward_audio(ab, rb, SR, [len(yd)], [len(yr)])
    assert tuple(oa.shape) == (1, 1) and torch.equal(oa, ob)
    oa.backward(g)
    ob.backward(g)
    assert a.grad.shape == a.shape and r.grad.shape == r.shape
    assert torch.equal(a.grad, ab.grad[0]) and torch.equal(r.grad, rb.grad[0])
    assert float(a.grad.abs().max()) > 0 and float(r.grad.abs().max()) > 0
    ah = torch.from_numpy(yd).double().requires_grad_(True)                   # float64 on the host
    rd = _t(yr).requires_grad_(True)
    oh = m.forward_audio(ah, rd, SR)
    assert oh.grad_fn is not None and oh.is_cuda and torch.equal(oh.detach(), oa.detach())
    oh.backward(g)
    assert ah.grad.device.type == 'cpu' and ah.grad.dtype == torch.float64 and ah.grad.shape == ah.shape
    assert rd.grad.is_cuda and rd.grad.dtype == torch.float32
    assert torch.equal(ah.grad.float(), a.grad.cpu()) and torch.equal(rd.grad, r.grad)
