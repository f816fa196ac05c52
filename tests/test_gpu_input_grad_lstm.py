"""d model(x, n_wins) / d x on the MI355X for the StandardCNN + BiLSTM models (pool = last_step_bi, avg, max): model(x, n_wins) with
x.requires_grad against the float64 oracle (tests/input_grad_lstm_oracle.py) and the reference's fixtures, the contract around it
(values unchanged, padding rows, dtype and device of the gradient, determinism), and the two kernels of the StandardCNN's pools
(csrc/input_grad.hip) against torch float64 autograd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import input_grad_lstm_oracle as IL

pytestmark = pytest.mark.gpu
PRECISIONS = ['f32', 'bf16x6']
BAR = 1e-3                  # max |dx - want| <= BAR * max |want| per clip: the bar of tests/test_gpu_input_grad.py
TIE = 1e-5                  # below this gap fp32 may choose differently from float64
DEV = 'cuda:0'
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _case(pool, spec_name):
    return _cached(('case', pool, spec_name), lambda: IL.case(pool, getattr(IL, spec_name), fill=np.nan))


def _model(pool, precision, spec_name):
    """the package's module with the case's weights and an engine of ``precision``"""
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqa
        from oracle import ref_shim
        sd, args = _case(pool, spec_name)[:2]
        m = NL.NISQA(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqa(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model', pool, precision, spec_name), make)


def _oracle(pool, spec_name):
    def make():
        sd, args, x, n_wins, g = _case(pool, spec_name)
        return IL.oracle(sd, args, x, n_wins, [g])
    return _cached(('oracle', pool, spec_name), make)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('pool', IL.POOLS)
def test_small_case_against_the_float64_oracle(pool, precision):
    """Three clips of 1, 3 and 2 segments padded to L = 4 with NaN.  Measured max |dx - want| / max |want| over the clips:
    last_step_bi 7.8e-6, avg 5.0e-6, max 7.8e-6, the same under both precisions (the backward is exact fp32 under either); the
    reference's own fp32 modules on the CPU are within 4.4e-6 of the oracle on this case."""
    sd, args, x, n_wins, g = _case(pool, 'SMALL')
    want = _oracle(pool, 'SMALL')
    assert want['margin'][np.isfinite(want['margin'])].min() >= TIE          # nothing sits on a tie: nothing is excluded
    m = _model(pool, precision, 'SMALL')
    B = len(n_wins)
    xd = _t(x).requires_grad_(True)
    y = m(xd, torch.as_tensor(n_wins))
    assert y.grad_fn is not None and y.device == xd.device and tuple(y.shape) == (B, 1)
    with torch.no_grad():
        y_plain = m(_t(x), torch.as_tensor(n_wins))
    assert y_plain.grad_fn is None and torch.equal(y.detach(), y_plain)
    assert m(_t(x), torch.as_tensor(n_wins)).grad_fn is None                 # a plain x: nothing to differentiate
    assert not any(p.requires_grad for p in m.parameters())
    np.testing.assert_allclose(y_plain.cpu().numpy(), want['y'], rtol=0, atol=1e-3)
    dx, = torch.autograd.grad(y, xd, _t(g), retain_graph=True)
    assert dx.shape == xd.shape and dx.dtype == torch.float32 and dx.device == xd.device
    got, w = dx.cpu().numpy(), want['dx'][0]
    assert (np.abs(w).reshape(B, -1).max(1) > 0).all()
    for b, n in enumerate(n_wins):
        assert (got[b, n:] == 0).all()                                       # exactly zero: the NaN there does not leak
    assert np.isfinite(got).all()
    err = IL.clip_error(got, w)
    print(pool, precision, 'max |want| per clip', np.abs(w).reshape(B, -1).max(1), 'relative distance', err)
    assert (err <= BAR).all(), err
    # twice the same bits
    a, = torch.autograd.grad(y, xd, _t(g), retain_graph=True)
    b_, = torch.autograd.grad(y, xd, _t(g))
    assert torch.equal(a, dx) and torch.equal(b_, dx)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_gradient_comes_back_in_the_dtype_and_on_the_device_of_x(precision):
    pool = 'last_step_bi'
    sd, args, x, n_wins, g = _case(pool, 'SMALL')
    m = _model(pool, precision, 'SMALL')
    want = _oracle(pool, 'SMALL')['dx'][0]
    xh = torch.from_numpy(x.copy()).requires_grad_(True)                      # on the host
    y = m(xh, torch.as_tensor(n_wins))
    assert y.grad_fn is not None and y.is_cuda
    y.backward(_t(g))
    assert xh.grad.device.type == 'cpu' and xh.grad.dtype == torch.float32 and xh.grad.shape == xh.shape
    assert (IL.clip_error(xh.grad.numpy(), want) <= BAR).all()
    x64 = _t(x).double().requires_grad_(True)                                 # float64 on the device
    m(x64, torch.as_tensor(n_wins)).backward(_t(g))
    assert x64.grad.is_cuda and x64.grad.dtype == torch.float64
    assert (IL.clip_error(x64.grad.cpu().numpy(), want) <= BAR).all()
    assert torch.equal(x64.grad.float().cpu(), xh.grad)
    with torch.no_grad():
        assert m(torch.from_numpy(x.copy()).requires_grad_(True), torch.as_tensor(n_wins)).grad_fn is None


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('pool', IL.POOLS)
def test_tile_edge_case_against_the_float64_oracle(pool, precision):
    """65, 1 and 32 segments (98: no multiple of a GEMM or convolution row tile, and a one-step LSTM sequence).  Segments whose
    float64 tie margin is below 1e-5 may differ legitimately and are left out (at most a quarter of them); their gradients must
    still be finite.  Near-ties of PoolMax over time are no ground for leaving anything out.  Measured, worst clip: last_step_bi
    8.4e-5 (clip 0), avg 1.4e-5, max 8.3e-6; 5 of 98 segments left out."""
    sd, args, x, n_wins, g = _case(pool, 'EDGE')
    want = _oracle(pool, 'EDGE')
    valid = np.isfinite(want['margin'])
    out = valid & (want['margin'] < TIE)
    print('segments', int(valid.sum()), 'left out', int(out.sum()), 'smallest margin kept', want['margin'][valid & ~out].min())
    assert valid.sum() == 98 and out.sum() <= 0.25 * valid.sum()
    m = _model(pool, precision, 'EDGE')
    xd = _t(x).requires_grad_(True)
    m(xd, torch.as_tensor(n_wins)).backward(_t(g))
    got, w = xd.grad.cpu().numpy(), want['dx'][0]
    assert np.isfinite(got).all()
    for b, n in enumerate(n_wins):
        assert (got[b, n:] == 0).all()
        keep = ~out[b, :n]
        top = np.abs(w[b, :n][keep]).max()
        d = np.abs(got[b, :n][keep] - w[b, :n][keep]).max()
        print(pool, precision, 'clip', b, 'segments', n, 'kept', int(keep.sum()), 'max |want|', top, 'relative distance', d / top)
        assert top > 0 and d <= BAR * top


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('pool', IL.POOLS)
def test_small_case_against_the_reference_fixture(pool, precision):
    """tests/golden/input_grad_lstm_*.npz: y and x.grad of the reference's own module (float32, eval mode)"""
    fx = helpers.golden('input_grad_lstm_%s.npz' % pool)
    sd, args, x, n_wins, g = _case(pool, 'SMALL')
    assert np.array_equal(fx['g'], g) and fx['n_wins'].tolist() == n_wins.tolist()
    m = _model(pool, precision, 'SMALL')
    xd = _t(x).requires_grad_(True)
    y = m(xd, torch.as_tensor(n_wins))
    y.backward(_t(g))
    err = IL.clip_error(xd.grad.cpu().numpy(), fx['dx'].astype(np.float64))
    print(pool, precision, 'against the fixture', err)
    assert (err <= BAR).all()
    np.testing.assert_allclose(y.detach().cpu().numpy(), fx['y'], rtol=0, atol=1e-3)


# ---- the two kernels of the StandardCNN's pools ---------------------------------------------------------------------------------
GUARD = 12345.0


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('h,w,c,pad', [(48, 15, 16, 1), (24, 8, 32, 0), (12, 4, 64, 0), (6, 5, 8, 1), (4, 5, 8, 0)])
def test_frozen_batchnorm_relu_maxpool2_forward_and_backward(h, w, c, pad):
    """against torch float64 autograd of F.batch_norm(training=False) -> relu -> max_pool2d(2, 2, padding (0, pad)), S = 3, a few
    negative gammas: the three compiled shapes and two generic ones (the last column of 4 x 5 without padding belongs to no
    window).  Exact ties inside a window go to the first maximum, the padding column never wins, the rows behind the last segment
    stay as they were, two runs give the same bits."""
    from nisqa_amd import lib
    L = lib.load()
    S = 3
    ho, wo = h // 2, (w + 2 * pad - 2) // 2 + 1
    rng = np.random.default_rng(h * 100 + w)
    z = rng.standard_normal((S, h, w, c)).astype(np.float32)
    z[:, 0, pad] = z[:, 0, pad + 1]                          # exact ties inside windows: along a row (columns pad, pad + 1 share a
    z[:, 2, 0] = z[:, 3, 0]                                  # window) and along a column (rows 2, 3)
    z = z.reshape(S, h * w, c)
    gamma = (1 + 0.2 * rng.standard_normal(c)).astype(np.float32)
    gamma[::7] *= -1
    beta, mean = (0.3 * rng.standard_normal((2, c))).astype(np.float32)
    var = rng.uniform(0.5, 2.0, c).astype(np.float32)
    dy = rng.standard_normal((S, ho * wo, c)).astype(np.float32)

    z64 = torch.from_numpy(z).double().reshape(S, h, w, c).permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = F.relu(F.batch_norm(z64, torch.from_numpy(mean).double(), torch.from_numpy(var).double(), torch.from_numpy(gamma).double(),
                            torch.from_numpy(beta).double(), False, 0.0, 1e-5))
    y64, idx64 = F.max_pool2d(a, 2, stride=2, padding=(0, pad), return_indices=True)
    assert tuple(y64.shape[2:]) == (ho, wo)
    dy64 = torch.from_numpy(dy).double().reshape(S, ho, wo, c).permute(0, 3, 1, 2)
    dz64, = torch.autograd.grad((y64 * dy64).sum(), z64)
    to_rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(S, -1, c).numpy()
    y_w, idx_w, dz_w, a_rows = to_rows(y64), to_rows(idx64), to_rows(dz64), to_rows(a)

    zd, dyd = _t(z), _t(dy)
    par = [_t(v) for v in (gamma, beta, mean, var)]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        y = torch.full((S + 1, ho * wo, c), GUARD, dtype=torch.float32, device=DEV)
        arg = torch.full((S + 1, ho * wo, c), -7, dtype=torch.int32, device=DEV)
        dz = torch.full((S + 1, h * w, c), GUARD, dtype=torch.float32, device=DEV)
        lib.check(L.nisqa_bn_eval_act_maxpool2_fwd(_p(zd), *[_p(v) for v in par], S, h, w, c, pad, _p(y), _p(arg), st),
                  'nisqa_bn_eval_act_maxpool2_fwd')
        lib.check(L.nisqa_bn_eval_act_maxpool2_bwd(_p(dyd), _p(arg), _p(zd), *[_p(v) for v in par], S, h, w, c, pad, _p(dz), st),
                  'nisqa_bn_eval_act_maxpool2_bwd')
        runs.append((y, arg, dz))
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    y_g, arg_g, dz_g = (t.cpu().numpy() for t in runs[0])
    assert (y_g[S] == GUARD).all() and (arg_g[S] == -7).all() and (dz_g[S] == GUARD).all()
    y_g, arg_g, dz_g = y_g[:S], arg_g[:S], dz_g[:S]
    e_y = np.abs(y_g - y_w).max() / np.abs(y_w).max()
    e_dz = np.abs(dz_g - dz_w).max() / np.abs(dz_w).max()
    print((h, w, c, pad), 'y', e_y, 'dz', e_dz)
    assert e_y <= 1e-5
    # every winner is a real pixel of its own window: the padding column never wins
    cell = np.arange(ho * wo)[None, :, None]
    assert (arg_g >= 0).all() and (arg_g < h * w).all()
    assert ((arg_g // w) // 2 == cell // wo).all() and ((arg_g % w + pad) // 2 == cell % wo).all()
    # equal to float64's choice wherever the float64 gap is >= 1e-5: a different choice must be within 1e-5 of the float64 maximum
    differ = arg_g != idx_w
    s_i, o_i, c_i = np.nonzero(differ)
    print('argmax differs at', len(s_i), 'of', differ.size)
    assert (a_rows[s_i, arg_g[differ], c_i] > y_w[differ] - TIE).all()
    # the exact ties: where the tied value is the window's positive maximum, the first of the two pixels wins
    n_tied = 0
    for first, second in ((pad, pad + 1), (2 * w, 3 * w)):
        assert np.array_equal(a_rows[:, first], a_rows[:, second])
        o = (first // w) // 2 * wo + (first % w + pad) // 2
        tied = (a_rows[:, first] == y_w[:, o]) & (y_w[:, o] > 0)
        n_tied += int(tied.sum())
        assert (arg_g[:, o][tied] == first).all() and (idx_w[:, o][tied] == first).all()
    assert n_tied > 0
    assert e_dz <= 1e-5
    if pad == 0 and w % 2:                                   # floor mode: the last column belongs to no window
        assert (dz_g.reshape(S, h, w, c)[:, :, w - 1] == 0).all()
