"""The gradient of the per-segment profile on the MI355X: nisqa_pool_profile_bwd against float64 autograd of the restatement
(tests/profile_grad_oracle.py), the identity that ties grad_profile_segments to grad_segments, and
profile_audio(..., differentiable=True) end to end from the samples for NISQA, NISQA_DIM and NISQA_DE.

The kernel's bar, per clip: max |dx - want| / max |want| <= max(1e-5, 2 x the same distance of the float32 CPU evaluation of the
restatement's gradient) -- profile_oracle.bars' rule, computed from the rows the kernel read, never from its results.  Everything
behind the kernel is held to the project's input-gradient bar of 1e-3 per clip (tests/test_gpu_input_grad.py)."""
import ctypes

import numpy as np
import pytest
import torch

import audio_grad_oracle as AG
import de_audio_grad_oracle as DA
import de_oracle as DO
import input_grad_de_oracle as IGD
import input_grad_oracle as IG
import profile_grad_oracle as PG
import profile_oracle as PO
from nisqa_amd import synth

pytestmark = pytest.mark.gpu
PRECISIONS = ['f32', 'bf16x6']
BAR = 1e-3                  # max |d - want| <= BAR * max |want| per clip: the bar of tests/test_gpu_input_grad.py
TIE = 1e-5                  # below this gap fp32 may choose differently from float64
DEV = 'cuda:0'
SR = 48000
N_TOKENS = [1, 63, 64, 65, 255, 256, 257, 513, 1300]      # the forward's sizes and the edges of the 256-thread token loop
E2E_SEEDS = (13, 417, 811)  # the signals of tests/test_gpu_audio_grad.py for NISQA and NISQA_DIM: tie margin >= TIE at every segment
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
def _kernel_case(n_heads):
    """-> (engine, state_dict, head prefixes, plan, x [NP, 64]: the engine's own self-attention rows with NaN in every padding row,
    cotangents (d_weights, d_local [NP, heads], d_embed [NP, 64]) with NaN in every padding row, the valid-row mask)"""
    def make():
        from nisqa_amd.engine import BatchPlan, HipNisqa
        model = 'NISQA_DIM' if n_heads == 5 else 'NISQA'
        args = dict(synth.DIM_ARGS if n_heads == 5 else synth.MOS_ARGS)
        sd = synth.random_state_dict(7 if n_heads == 5 else 8, model)
        eng = HipNisqa(args, sd, DEV, precision='f32')
        plan = BatchPlan.from_n_wins(N_TOKENS)
        idx = torch.from_numpy(plan.token_index()).to(DEV)
        keep = torch.zeros(plan.total_tok, dtype=torch.bool, device=DEV)
        keep[idx] = True
        gen = torch.Generator(DEV).manual_seed(3)
        feat = torch.zeros((plan.total_tok, 384), device=DEV)
        feat[idx] = torch.randn((len(idx), 384), device=DEV, generator=gen)
        nan = torch.full((), float('nan'), device=DEV)
        pad = lambda t: torch.where(keep[:, None], t, nan).contiguous()
        x = pad(eng.td(feat, plan))
        cot = tuple(pad(torch.randn((plan.total_tok, w), device=DEV, generator=gen)) for w in (n_heads, n_heads, 64))
        return eng, sd, (PO.DIM_HEADS if n_heads == 5 else PO.MOS_HEADS), plan, x, cot, keep
    return _cached(('kernel', n_heads), make)


def _bwd(eng, x, plan, n_heads, dw, dl, de):
    """nisqa_pool_profile_bwd straight through the C ABI into a dx prefilled with NaN"""
    from nisqa_amd import lib
    d = plan.to(eng.device)
    dx = torch.full((plan.total_tok, 64), float('nan'), dtype=torch.float32, device=DEV)
    lib.check(eng.lib.nisqa_pool_profile_bwd(_p(x), 64, _p(d['tok_off']), _p(d['n_wins']), plan.n_clips, plan.total_tok, n_heads, 0,
                                             _p(eng.profile_weights()), _p(dw), _p(dl), _p(de), _p(dx), eng._stream()),
              'nisqa_pool_profile_bwd')
    torch.cuda.synchronize()
    return dx


def _clip_rows(plan, c):
    r0 = int(plan.tok_off[c])
    return r0, r0 + int(plan.n_wins[c]), int(plan.tok_off[c + 1])


@pytest.mark.parametrize('which', ['weights', 'local', 'embed', 'all'])
@pytest.mark.parametrize('n_heads', [1, 5])
def test_kernel_against_float64_autograd_of_the_restatement(n_heads, which):
    """ONE launch over clips of 1, 63, 64, 65, 255, 256, 257, 513 and 1300 tokens; every cotangent alone (NULL for the other two)
    and all three together; NaN in x and in the cotangents at every padding row, NaN in dx before the call.
    Measured worst max |dx - want| / max |want| per clip, 1 head / 5 heads: d_weights alone 1.1e-6 / 2.0e-6, d_local alone 4.7e-8 /
    1.2e-7, d_embed alone 0 / 0 (a copy), all three 5.5e-7 / 1.3e-6 (the float32 CPU evaluation of the restatement: up to 1.2e-6);
    every bar evaluated to 1e-5."""
    eng, sd, heads, plan, x, cot, keep = _kernel_case(n_heads)
    use = [which in (name, 'all') for name in ('weights', 'local', 'embed')]
    args = [t if u else None for t, u in zip(cot, use)]
    dx = _bwd(eng, x, plan, n_heads, *args)
    assert torch.equal(dx, _bwd(eng, x, plan, n_heads, *args))               # no atomics, fixed orders: the same bits again
    got, rows = dx.cpu().numpy(), x.cpu().numpy()
    host = [t.cpu().numpy() if u else None for t, u in zip(cot, use)]
    assert np.isfinite(got).all()                                            # every row written, no NaN of a padding row read
    assert (got[~keep.cpu().numpy()] == 0).all()                             # padding rows: exact zeros
    worst = worst32 = 0.0
    for c, n in enumerate(N_TOKENS):
        r0, r1, _ = _clip_rows(plan, c)
        cs = [None if h is None else h[r0:r1] for h in host]
        want = PG.pool_grad(sd, rows[r0:r1], heads, *cs)
        if n == 1 and which == 'weights':
            assert (want == 0).all() and (got[r0:r1] == 0).all()             # one token: its weight is 1 whatever x is -- exactly
            continue
        top = np.abs(want).max()
        e32 = np.abs(PG.pool_grad(sd, rows[r0:r1], heads, *cs, dtype=torch.float32).astype(np.float64) - want).max() / top
        err = np.abs(got[r0:r1] - want).max() / top
        bar = max(1e-5, 2.0 * e32)
        print('%d head(s) d_%s clip %d n %4d: max |want| %.3g kernel distance %.3g float32 restatement %.3g bar %.3g'
              % (n_heads, which, c, n, top, err, e32, bar))
        worst, worst32 = max(worst, err), max(worst32, e32)
        assert top > 0 and err <= bar, (c, n, err, bar)
    print('%d head(s) d_%s: worst kernel distance %.3g, worst float32 restatement distance %.3g' % (n_heads, which, worst, worst32))


@pytest.mark.parametrize('n_heads', [1, 5])
def test_one_token_takes_nothing_from_d_weights(n_heads):
    """the clip of one token: with all three cotangents its dx row is, bit for bit, the row without d_weights"""
    eng, sd, heads, plan, x, cot, keep = _kernel_case(n_heads)
    r0, r1, _ = _clip_rows(plan, N_TOKENS.index(1))
    a, b = _bwd(eng, x, plan, n_heads, *cot), _bwd(eng, x, plan, n_heads, None, cot[1], cot[2])
    assert r1 - r0 == 1 and torch.equal(a[r0:r1], b[r0:r1]) and float(a[r0:r1].abs().max()) > 0
    assert not torch.equal(a, b)


@pytest.mark.parametrize('n_heads', [1, 5])
def test_a_constant_d_weights_per_clip_cancels(n_heads):
    """sum_t a_t = 1, so a d_weights that is one constant per clip and head has no gradient.  The scale it is judged on: the same
    magnitudes with random signs, where nothing cancels (float64); the bar: max(1e-5, 2 x the float32 CPU evaluation of the constant
    case's gradient on that scale), as everywhere in this file.  Measured |dx| / scale <= 1.3e-7 (float32 restatement: <= 1.6e-7)."""
    eng, sd, heads, plan, x, cot, keep = _kernel_case(n_heads)
    rng = np.random.default_rng(11)
    const = np.full((plan.total_tok, n_heads), np.nan, dtype=np.float32)
    signed = const.copy()
    for c, n in enumerate(N_TOKENS):
        r0, r1, _ = _clip_rows(plan, c)
        const[r0:r1] = rng.uniform(0.5, 2.0, (1, n_heads)).astype(np.float32)
        signed[r0:r1] = const[r0:r1] * rng.choice([-1.0, 1.0], (n, n_heads)).astype(np.float32)
    got, rows = _bwd(eng, x, plan, n_heads, _t(const), None, None).cpu().numpy(), x.cpu().numpy()
    assert np.isfinite(got).all()
    for c, n in enumerate(N_TOKENS):
        r0, r1, _ = _clip_rows(plan, c)
        if n == 1:
            assert (got[r0:r1] == 0).all()
            continue
        scale = np.abs(PG.pool_grad(sd, rows[r0:r1], heads, cw=signed[r0:r1])).max()
        e32 = np.abs(PG.pool_grad(sd, rows[r0:r1], heads, cw=const[r0:r1], dtype=torch.float32)).max() / scale
        err = np.abs(got[r0:r1]).max() / scale
        print('%d head(s) constant d_weights clip %d n %4d: scale %.3g |dx| / scale %.3g float32 restatement %.3g'
              % (n_heads, c, n, scale, err, e32))
        assert scale > 0 and err <= max(1e-5, 2.0 * e32), (c, n, err, e32)


# ---- the identity between the two code paths --------------------------------------------------------------------------------------
def _engine(model, precision, spec_name):
    def make():
        from nisqa_amd.engine import HipNisqa
        sd, args = IG.case(model, getattr(IG, spec_name))[:2]
        return HipNisqa(args, sd, DEV, precision=precision)
    return _cached(('engine', model, precision, spec_name), make)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('spec_name', ['SMALL', 'EDGE'])
@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_profile_gradient_reproduces_the_score_gradient(model, spec_name, precision):
    """score = sum_t weights_t local_t: with d_weights = g * local, d_local = g * weights (the engine's own profile) and no d_embed,
    grad_profile_segments -- the new kernel in front of the chain -- agrees with grad_segments(x, n_wins, g) -- the pooling heads'
    operator-by-operator backward in front of the same chain -- within 1e-3 of each clip's largest entry; n_wins 1 / 3 / 2 and
    65 / 1 / 32, NaN in the padding rows of x and of the cotangents.
    Measured max |d - want| / max |want| per clip: <= 1.3e-6 in every case."""
    from nisqa_amd.engine import BatchPlan
    sd, args, x, n_wins, g = IG.case(model, getattr(IG, spec_name), fill=np.nan)
    eng = _engine(model, precision, spec_name)
    xd, gd = _t(x), _t(g)
    prof = eng.profile_segments(xd, n_wins)
    plan = BatchPlan.from_n_wins(n_wins)
    clip = torch.from_numpy(np.repeat(np.arange(len(n_wins)), np.diff(plan.tok_off))).to(DEV)
    valid = torch.zeros(plan.total_tok, dtype=torch.bool, device=DEV)
    valid[torch.from_numpy(plan.token_index()).to(DEV)] = True
    nan = torch.full((), float('nan'), device=DEV)
    d_weights = torch.where(valid[:, None], gd[clip] * prof.local, nan)
    d_local = torch.where(valid[:, None], gd[clip] * prof.weights, nan)
    want = eng.grad_segments(xd, n_wins, gd)
    got = eng.grad_profile_segments(xd, n_wins, d_weights=d_weights, d_local=d_local)
    torch.cuda.synchronize()
    assert got.shape == want.shape == xd.shape and got.dtype == torch.float32
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.isfinite(got).all()
    for b, n in enumerate(n_wins):
        assert (got[b, n:] == 0).all()
    err = IG.clip_error(got, want.astype(np.float64))
    print(model, spec_name, precision, 'relative distance per clip', err)
    assert (np.abs(want).reshape(len(n_wins), -1).max(1) > 0).all() and (err <= BAR).all(), err
    # d_scores beside them: the two seeds add up
    both = eng.grad_profile_segments(xd, n_wins, d_scores=gd, d_weights=d_weights, d_local=d_local).cpu().numpy()
    assert (IG.clip_error(both, 2.0 * want.astype(np.float64)) <= BAR).all()
    with pytest.raises(ValueError):
        eng.grad_profile_segments(xd, n_wins)                                # nothing to differentiate
    with pytest.raises(ValueError, match='d_local'):
        eng.grad_profile_segments(xd, n_wins, d_local=d_local[:-1])


# ---- end to end from audio --------------------------------------------------------------------------------------------------------
def _model(family, precision):
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqa
        from oracle import ref_shim
        sd, args = IG.case(family)[:2]
        m = getattr(NL, family)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqa(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model', family, precision), make)


def _signals():
    """three clips of 15, 23 and 19 frames at 48 kHz -> (y [3, N] float32 with NaN beyond the lengths, lengths, per-clip samples)"""
    lengths = AG.lengths_of(SR)
    ys = [AG.smooth_signal(SR, n, s) for n, s in zip(lengths, E2E_SEEDS)]
    y = np.full((3, max(lengths) + 5), np.nan, dtype=np.float32)
    for b, yb in enumerate(ys):
        y[b, :len(yb)] = yb
    return y, np.asarray(lengths), ys


def _device_cotangents(cot, n_wins):
    """a cotangent dict -> the four autograd cotangents (scores, weights, local, embed) on the device, None for an absent key, NaN in
    every row l >= n_wins[b]"""
    out = []
    for k in 'gwle':
        a = cot.get(k)
        if a is not None and k != 'g':
            a = a.copy()
            for b, n in enumerate(n_wins):
                a[b, n:] = np.nan
        out.append(None if a is None else _t(a))
    return out


def _grad(res, inputs, cots, retain=True):
    outs = [res.scores, res.weights, res.local, res.embed]
    pairs = [(o, c) for o, c in zip(outs, cots) if c is not None]
    return torch.autograd.grad([o for o, _ in pairs], inputs, [c for _, c in pairs], retain_graph=retain, allow_unused=True)


def _assert_same_values(res, plain):
    for k in ('scores', 'weights', 'local', 'embed'):
        assert getattr(plain, k).grad_fn is None and torch.equal(getattr(res, k).detach(), getattr(plain, k)), k
    assert torch.equal(res.n_wins, plain.n_wins) and torch.equal(res.t_start, plain.t_start) and torch.equal(res.t_end, plain.t_end)
    assert res.heads == plain.heads
    fns = {getattr(res, k).grad_fn for k in ('scores', 'weights', 'local', 'embed')}
    assert len(fns) == 1 and None not in fns                                 # the four outputs of ONE function


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('family', ['NISQA_DIM', 'NISQA'])
def test_profile_audio_end_to_end_against_float64(family, precision):
    """Three clips of 15, 23 and 19 frames at 48 kHz in a [3, N] batch with NaN beyond the lengths; random cotangents on all four
    outputs and, for NISQA_DIM, on one head's local alone, with NaN in their rows l >= n_wins[b].  Wanted: the restatement's dx at the
    segment tensor cut from the engine's own clamped rows, pulled back through the float64 mel restatement
    (audio_grad_oracle.compose).  The network's tie margin is >= 1e-5 at every segment and the mel margin >= 1e-2 dB: nothing is left
    out.
    Measured max |dy - want| / max |want| over clips, f32 / bf16x6: NISQA_DIM 2.3e-6 / 2.1e-6 (one head's local alone 2.5e-6 /
    2.8e-6), NISQA 3.0e-6 / 4.2e-6; smallest tie margin 4.1e-5."""
    sd, args = IG.case(family)[:2]
    m = _model(family, precision)
    eng = m._engine
    y, lengths, ys = _signals()
    H = len(IG.heads_of(family))
    plan = eng.plan(lengths, SR)
    n_wins, L = plan.n_wins.tolist(), int(plan.n_wins.max())
    cots = [PG.random_cotangents(21, 3, L, H)]
    if family == 'NISQA_DIM':
        one = np.zeros((3, L, H), dtype=np.float32)
        one[:, :, 2] = PG.random_cotangents(22, 3, L, 1, 'l')['l'][:, :, 0]
        cots.append({'l': one})
    yd = _t(y).requires_grad_(True)
    res = m.profile_audio(yd, SR, lengths, differentiable=True)
    plain = m.profile_audio(yd, SR, lengths)
    _assert_same_values(res, plain)
    with torch.no_grad():
        assert torch.equal(res.scores.detach(), m.forward_audio(yd, SR, lengths))
        assert m.profile_audio(yd, SR, lengths, differentiable=True).scores.grad_fn is None
    assert m.profile_audio(_t(y), SR, lengths, differentiable=True).local.grad_fn is None      # a plain y: nothing to differentiate
    pcm = _t(np.concatenate(ys))
    clamped = eng.mel(pcm, plan, SR, clamp=True)[0].cpu().numpy()
    rows = [clamped[plan.frame_off[b]:plan.frame_off[b + 1]] for b in range(3)]
    want = _cached(('want', family, clamped.tobytes()), lambda: AG.compose(PG.oracle, sd, args, rows, ys, SR, cots))
    assert want['n_wins'].tolist() == n_wins
    margin = want['margin'][np.isfinite(want['margin'])]
    print(family, precision, 'smallest tie margin', margin.min(), 'mel margin', want['mel_margin'])
    assert margin.min() >= TIE and (want['mel_margin'] >= AG.MARGIN_DB).all()
    np.testing.assert_allclose(plain.scores.cpu().numpy(), want['y'], rtol=0, atol=1e-3)
    for k, cot in enumerate(cots):
        dy, = _grad(res, yd, _device_cotangents(cot, n_wins))
        assert dy.shape == yd.shape and dy.dtype == torch.float32 and dy.device == yd.device
        got = dy.cpu().numpy()
        assert np.isfinite(got).all()
        for b, n in enumerate(lengths):
            assert (got[b, n:] == 0).all()                                   # exact zeros: the NaN there does not leak
        err = AG.clip_errors([got[b, :n] for b, n in enumerate(lengths)], want['dy'][k])
        print(family, precision, 'all four outputs' if k == 0 else 'local of head 2 alone', 'max |want| per clip',
              [float(np.abs(w).max()) for w in want['dy'][k]], 'relative distance', err)
        assert all(np.abs(w).max() > 0 for w in want['dy'][k]) and (err <= BAR).all(), (k, err)
    dev_cot = _device_cotangents(cots[0], n_wins)
    a, = _grad(res, yd, dev_cot)
    b_, = _grad(res, yd, dev_cot)
    assert torch.equal(a, b_)                                                # twice the same bits
    # a float64 y on the host gets a float64 gradient on the host
    yh = torch.from_numpy(y).double().requires_grad_(True)
    rh = m.profile_audio(yh, SR, lengths, differentiable=True)
    _assert_same_values(rh, plain)
    dh, = _grad(rh, yh, dev_cot, retain=False)
    assert dh.device.type == 'cpu' and dh.dtype == torch.float64 and dh.shape == yh.shape and torch.equal(dh.float(), a.cpu())
    # a loss on the worst segment
    pad = torch.arange(L, device=DEV)[None, :] >= res.n_wins.to(DEV)[:, None]
    worst = res.local[..., 0].masked_fill(pad, float('inf')).amin(1).sum()
    dw, = torch.autograd.grad(worst, yd)
    assert torch.isfinite(dw).all() and all(float(dw[b, :n].abs().max()) > 0 for b, n in enumerate(lengths))
    assert all((dw[b, n:] == 0).all() for b, n in enumerate(lengths))


# ---- NISQA_DE ---------------------------------------------------------------------------------------------------------------------
def _model_de(config, precision):
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqaDE
        sd, args, _ = DA.case(config)
        m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqaDE(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model de', config, precision), make)


def _batch(ys, lengths, extra):
    y = np.full((len(ys), int(max(lengths)) + extra), np.nan, dtype=np.float32)
    for b, yb in enumerate(ys):
        y[b, :len(yb)] = yb
    return y


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config', IGD.CONFIGS[:2], ids=lambda c: IGD.NAMES[c])
def test_double_ended_profile_audio_end_to_end_against_float64(config, precision):
    """cosine / hard and dot / soft on de_audio_grad_oracle's three pairs ((1, 2), (3, 1) and (2, 4) segments, NaN beyond the
    lengths): random cotangents on local and embed over the degraded clips' segments, with requires_grad on both sides, on the
    degraded side only and on the reference side only.  Wanted: profile_grad_oracle.compose_de at the segment tensors cut from the
    engine's own clamped rows (hard alignment: the recomputation's indices, which are float64's own).  Tie margins, score gaps and
    mel margins as tests/test_gpu_de_audio_grad.py asserts them.  A side that requires no gradient gets none.
    Measured max |d - want| / max |want| over clips and sides, f32 / bf16x6: cos_hard 3.8e-6 / 4.4e-6, dot_soft 3.4e-6 / 7.5e-6
    (DESIGN.md 4.10)."""
    sd, args, _ = DA.case(config)
    m = _model_de(config, precision)
    eng = m._engine
    hard = config[1] == 'hard'
    ys_d, ys_r, ld, lr = DA.signals(IGD.NAMES[config])
    yd, yr = _batch(ys_d, ld, 5), _batch(ys_r, lr, 9)
    n_deg = [p[0] for p in DA.PAIRS]
    cot = PG.random_cotangents(31, 3, max(n_deg), 1, 'le')
    dev_cot = _device_cotangents(cot, n_deg)
    a, r = _t(yd).requires_grad_(True), _t(yr).requires_grad_(True)
    res = m.profile_audio(a, r, SR, ld, lr, differentiable=True)
    plain = m.profile_audio(a, r, SR, ld, lr)
    _assert_same_values(res, plain)
    assert torch.equal(res.aligned_to, plain.aligned_to) and res.aligned_to.grad_fn is None
    with torch.no_grad():
        assert torch.equal(res.scores.detach(), m.forward_audio(a, r, SR, ld, lr))
    da, dr = _grad(res, (a, r), dev_cot)
    idx = None
    if hard:
        idx = np.split(eng._input_grad.last_idx.cpu().numpy(), np.cumsum(n_deg)[:-1])
    plan = eng.plan(ld, lr, SR)
    clamped = eng.base.mel(_t(np.concatenate(ys_d + ys_r)), plan, SR, clamp=True)[0].cpu().numpy()
    rows = [clamped[plan.frame_off[c]:plan.frame_off[c + 1]] for c in range(6)]
    key = None if idx is None else tuple(np.concatenate(idx).tolist())
    want = _cached(('want de', config, key, clamped.tobytes()),
                   lambda: PG.compose_de(sd, args, rows[:3], rows[3:], ys_d, ys_r, SR, [cot], idx=idx))
    assert want['n_wins'].tolist() == [list(p) for p in DA.PAIRS]
    margin = want['margin'][np.isfinite(want['margin'])]
    gap = min(float(gp.min()) for gp in want['gap'])
    print(IGD.NAMES[config], precision, 'smallest tie margin', margin.min(), 'smallest score gap', gap, 'mel margin',
          want['mel_margin'].min())
    assert margin.size == 13 and margin.min() >= IGD.TIE and gap > IGD.TIE and (want['mel_margin'] >= AG.MARGIN_DB).all()
    if hard:
        for k in range(3):
            assert (idx[k] == want['own'][k]).all()
            assert (plain.aligned_to[k, :n_deg[k]].cpu().numpy() == idx[k]).all()
    np.testing.assert_allclose(plain.scores.cpu().numpy(), want['y'], rtol=0, atol=1e-3)

    def check(d, y_in, lengths, w, what):
        assert d.shape == y_in.shape and d.dtype == torch.float32 and d.device == y_in.device
        got = d.cpu().numpy()
        assert np.isfinite(got).all()
        for k, n in enumerate(lengths):
            assert (got[k, n:] == 0).all()
        err = AG.clip_errors([got[k, :n] for k, n in enumerate(lengths)], w)
        print(IGD.NAMES[config], precision, what, 'max |want| per clip', [float(np.abs(v).max()) for v in w], 'relative distance', err)
        assert all(np.abs(v).max() > 0 for v in w) and (err <= BAR).all(), (what, err)
    check(da, a, ld, want['dy_deg'][0], 'both sides: degraded')
    check(dr, r, lr, want['dy_ref'][0], 'both sides: reference')
    a1, r1 = _t(yd).requires_grad_(True), _t(yr)
    res1 = m.profile_audio(a1, r1, SR, ld, lr, differentiable=True)
    torch.autograd.backward([res1.local, res1.embed], dev_cot[2:])
    assert r1.grad is None
    check(a1.grad, a1, ld, want['dy_deg'][0], 'degraded side only')
    a2, r2 = _t(yd), _t(yr).requires_grad_(True)
    res2 = m.profile_audio(a2, r2, SR, ld, lr, differentiable=True)
    _assert_same_values(res2, plain)
    torch.autograd.backward([res2.local, res2.embed], dev_cot[2:])
    assert a2.grad is None
    check(r2.grad, r2, lr, want['dy_ref'][0], 'reference side only')
    assert m.profile_audio(_t(yd), _t(yr), SR, ld, lr, differentiable=True).embed.grad_fn is None
