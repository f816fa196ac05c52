"""d model(x, n_wins) / d x on the MI355X for the CNN-SA-AP checkpoints: model(x, n_wins) with x.requires_grad against the float64
oracle (tests/input_grad_oracle.py) and the reference's fixtures, the contract around it (values unchanged, padding rows, dtype and
device of the gradient, determinism), and the new kernels of csrc/input_grad.hip one by one against torch float64 autograd."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import input_grad_oracle as IG

pytestmark = pytest.mark.gpu
PRECISIONS = ['f32', 'bf16x6']
BAR = 1e-3                  # max |dx - want| <= BAR * max |want| per clip: tests/test_gpu_train.py's gradient bar without its floor
TIE = 1e-5                  # below this gap fp32 may choose differently from float64
DEV = 'cuda:0'
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _model(model, precision, spec_name):
    """the package's module with the case's weights and an engine of ``precision``"""
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqa
        from oracle import ref_shim
        sd, args = _case(model, spec_name)[:2]
        m = getattr(NL, model)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqa(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model', model, precision, spec_name), make)


def _case(model, spec_name):
    return _cached(('case', model, spec_name), lambda: IG.case(model, getattr(IG, spec_name), fill=np.nan))


def _gs(model, g):
    B, H = g.shape
    return [g] + ([IG.one_hot(B, H, h) for h in range(H)] if H > 1 else [])


def _oracle(model, spec_name, all_heads):
    def make():
        sd, args, x, n_wins, g = _case(model, spec_name)
        return IG.oracle(sd, args, x, n_wins, _gs(model, g) if all_heads else [g])
    return _cached(('oracle', model, spec_name, all_heads), make)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_small_case_against_the_float64_oracle(model, precision):
    """Three clips of 1, 3 and 2 segments padded to L = 4 with NaN: a random g and, for NISQA_DIM, every one-hot head.
    Measured max |dx - want| / max |want| over clips and heads: f32 4.8e-6, bf16x6 7.1e-6 (the reference's own fp32 modules on the
    CPU: 2.3e-6 on this case, 4.6e-6 at most)."""
    sd, args, x, n_wins, g = _case(model, 'SMALL')
    want = _oracle(model, 'SMALL', True)
    gs = _gs(model, g)
    assert want['margin'][np.isfinite(want['margin'])].min() >= TIE          # nothing sits on a tie: nothing is excluded
    m = _model(model, precision, 'SMALL')
    B = len(n_wins)
    xd = _t(x).requires_grad_(True)
    y = m(xd, torch.as_tensor(n_wins))
    assert y.grad_fn is not None and y.device == xd.device and tuple(y.shape) == tuple(g.shape)
    with torch.no_grad():
        y_plain = m(_t(x), torch.as_tensor(n_wins))
    assert y_plain.grad_fn is None and torch.equal(y.detach(), y_plain)
    assert m(_t(x), torch.as_tensor(n_wins)).grad_fn is None                 # a plain x: nothing to differentiate
    np.testing.assert_allclose(y_plain.cpu().numpy(), want['y'], rtol=0, atol=1e-3)
    worst = 0.0
    for k, gk in enumerate(gs):
        dx, = torch.autograd.grad(y, xd, _t(gk), retain_graph=True)
        assert dx.shape == xd.shape and dx.dtype == torch.float32 and dx.device == xd.device
        got, w = dx.cpu().numpy(), want['dx'][k]
        assert (np.abs(w).reshape(B, -1).max(1) > 0).all()
        for b, n in enumerate(n_wins):
            assert (got[b, n:] == 0).all()                                   # exactly zero: the NaN there does not leak
        assert np.isfinite(got).all()
        err = IG.clip_error(got, w)
        print(model, precision, 'random g' if k == 0 else 'head %d' % (k - 1), 'max |want| per clip',
              np.abs(w).reshape(B, -1).max(1), 'relative distance', err)
        worst = max(worst, float(err.max()))
        assert (err <= BAR).all(), (k, err)
    print(model, precision, 'worst relative distance', worst)
    # twice the same bits
    a, = torch.autograd.grad(y, xd, _t(g), retain_graph=True)
    b_, = torch.autograd.grad(y, xd, _t(g))
    assert torch.equal(a, b_)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_gradient_comes_back_in_the_dtype_and_on_the_device_of_x(precision):
    sd, args, x, n_wins, g = _case('NISQA', 'SMALL')
    m = _model('NISQA', precision, 'SMALL')
    want = _oracle('NISQA', 'SMALL', True)['dx'][0]
    xh = torch.from_numpy(x.copy()).requires_grad_(True)                      # on the host
    y = m(xh, torch.as_tensor(n_wins))
    assert y.grad_fn is not None and y.is_cuda
    y.backward(_t(g))
    assert xh.grad.device.type == 'cpu' and xh.grad.dtype == torch.float32 and xh.grad.shape == xh.shape
    assert (IG.clip_error(xh.grad.numpy(), want) <= BAR).all()
    x64 = _t(x).double().requires_grad_(True)                                 # float64 on the device
    m(x64, torch.as_tensor(n_wins)).backward(_t(g))
    assert x64.grad.is_cuda and x64.grad.dtype == torch.float64
    assert (IG.clip_error(x64.grad.cpu().numpy(), want) <= BAR).all()
    assert torch.equal(x64.grad.float().cpu(), xh.grad)
    with torch.no_grad():
        assert m(torch.from_numpy(x.copy()).requires_grad_(True), torch.as_tensor(n_wins)).grad_fn is None


@pytest.mark.parametrize('precision', PRECISIONS)
def test_tile_edge_case_against_the_float64_oracle(precision):
    """65, 1 and 32 segments: a clip that crosses the 64-token tile and a single-token clip.  Segments whose float64 tie margin is
    below 1e-5 may differ legitimately and are left out (at most a quarter of them); their gradients must still be finite."""
    model = 'NISQA_DIM'
    sd, args, x, n_wins, g = _case(model, 'EDGE')
    want = _oracle(model, 'EDGE', False)
    valid = np.isfinite(want['margin'])
    out = valid & (want['margin'] < TIE)
    print('segments', int(valid.sum()), 'left out', int(out.sum()), 'smallest margin kept', want['margin'][valid & ~out].min())
    assert valid.sum() == 98 and out.sum() <= 0.25 * valid.sum()
    m = _model(model, precision, 'EDGE')
    xd = _t(x).requires_grad_(True)
    m(xd, torch.as_tensor(n_wins)).backward(_t(g))
    got, w = xd.grad.cpu().numpy(), want['dx'][0]
    assert np.isfinite(got).all()
    for b, n in enumerate(n_wins):
        assert (got[b, n:] == 0).all()
        keep = ~out[b, :n]
        top = np.abs(w[b, :n][keep]).max()
        d = np.abs(got[b, :n][keep] - w[b, :n][keep]).max()
        print(precision, 'clip', b, 'segments', n, 'kept', int(keep.sum()), 'max |want|', top, 'relative distance', d / top)
        assert top > 0 and d <= BAR * top


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('model,name', [('NISQA_DIM', 'dim'), ('NISQA', 'mos')])
def test_small_case_against_the_reference_fixture(model, name, precision):
    """tests/golden/input_grad_*.npz: y and x.grad of the reference's own module (float32, eval mode)"""
    fx = helpers.golden('input_grad_%s.npz' % name)
    sd, args, x, n_wins, g = _case(model, 'SMALL')
    assert np.array_equal(fx['g'], g) and fx['n_wins'].tolist() == n_wins.tolist()
    m = _model(model, precision, 'SMALL')
    xd = _t(x).requires_grad_(True)
    y = m(xd, torch.as_tensor(n_wins))
    y.backward(_t(g))
    err = IG.clip_error(xd.grad.cpu().numpy(), fx['dx'].astype(np.float64))
    print(model, precision, 'against the fixture', err)
    assert (err <= BAR).all()
    np.testing.assert_allclose(y.detach().cpu().numpy(), fx['y'], rtol=0, atol=1e-3)


# ---- the kernels of csrc/input_grad.hip one by one ----------------------------------------------------------------------------
GUARD = 12345.0


def _lib():
    from nisqa_amd import lib
    return lib.load(), lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('h,w,c,ho,wo', [(48, 15, 16, 24, 7), (24, 7, 32, 12, 5), (12, 5, 64, 6, 3), (6, 3, 64, 6, 3)])
def test_frozen_batchnorm_relu_pool_forward_and_backward(h, w, c, ho, wo):
    """against torch float64 autograd of F.batch_norm(training=False) -> relu -> adaptive_max_pool2d, S = 3; the rows behind the
    last segment stay as they were"""
    L, lib = _lib()
    S = 3
    rng = np.random.default_rng(h * 100 + ho)
    z = rng.standard_normal((S, h * w, c)).astype(np.float32)
    gamma = (1 + 0.2 * rng.standard_normal(c)).astype(np.float32)
    gamma[::7] *= -1
    beta, mean = (0.3 * rng.standard_normal((2, c))).astype(np.float32)
    var = rng.uniform(0.5, 2.0, c).astype(np.float32)
    dy = rng.standard_normal((S, ho * wo, c)).astype(np.float32)
    identity = (h, w) == (ho, wo)

    z64 = torch.from_numpy(z).double().reshape(S, h, w, c).permute(0, 3, 1, 2).clone().requires_grad_(True)
    a = F.relu(F.batch_norm(z64, torch.from_numpy(mean).double(), torch.from_numpy(var).double(), torch.from_numpy(gamma).double(),
                            torch.from_numpy(beta).double(), False, 0.0, 1e-5))
    y64, idx64 = F.adaptive_max_pool2d(a, (ho, wo), return_indices=True)
    dy64 = torch.from_numpy(dy).double().reshape(S, ho, wo, c).permute(0, 3, 1, 2)
    dz64, = torch.autograd.grad((y64 * dy64).sum(), z64)
    to_rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(S, -1, c).numpy()
    y_w, idx_w, dz_w, a_rows = to_rows(y64), to_rows(idx64), to_rows(dz64), to_rows(a)

    zd, dyd = _t(z), _t(dy)
    par = [_t(v) for v in (gamma, beta, mean, var)]
    y = torch.full((S + 1, ho * wo, c), GUARD, dtype=torch.float32, device=DEV)
    arg = torch.full((S + 1, ho * wo, c), -7, dtype=torch.int32, device=DEV)
    dz = torch.full((S + 1, h * w, c), GUARD, dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.nisqa_bn_eval_act_pool_fwd(_p(zd), *[_p(v) for v in par], S, h, w, c, ho, wo, _p(y), None if identity else _p(arg),
                                           st), 'nisqa_bn_eval_act_pool_fwd')
    lib.check(L.nisqa_bn_eval_act_pool_bwd(_p(dyd), None if identity else _p(arg), _p(zd), *[_p(v) for v in par], S, h, w, c, ho, wo,
                                           _p(dz), st), 'nisqa_bn_eval_act_pool_bwd')
    torch.cuda.synchronize()
    y_g, arg_g, dz_g = y.cpu().numpy(), arg.cpu().numpy(), dz.cpu().numpy()
    assert (y_g[S] == GUARD).all() and (arg_g[S] == -7).all() and (dz_g[S] == GUARD).all()
    e_y = np.abs(y_g[:S] - y_w).max() / np.abs(y_w).max()
    e_dz = np.abs(dz_g[:S] - dz_w).max() / np.abs(dz_w).max()
    print((h, w, c, ho, wo), 'y', e_y, 'dz', e_dz)
    assert e_y <= 1e-5
    if identity:
        assert (arg_g[:S] == -7).all()                     # not written: the winner is the cell itself
    else:
        differ = arg_g[:S] != idx_w
        # equal wherever the float64 gap is >= 1e-5: a different choice must be within 1e-5 of the float64 maximum
        s_i, o_i, c_i = np.nonzero(differ)
        print('argmax differs at', len(s_i), 'of', differ.size)
        assert (a_rows[s_i, arg_g[:S][differ], c_i] > y_w[differ] - TIE).all()
    assert e_dz <= 1e-5


@pytest.mark.parametrize('n_wins,l_max', [([1], 2), ([2, 1, 2], 3)])
def test_conv1_on_segment_rows_forward_and_input_gradient(n_wins, l_max):
    """S = 1 and S = 5 against torch float64 conv2d and its autograd; padding rows are written as zeros (over NaN), the row behind
    the tensor stays as it was, two runs give the same bits"""
    L, lib = _lib()
    B, S = len(n_wins), int(sum(n_wins))
    rng = np.random.default_rng(S)
    x = np.full((B, l_max, 1, 48, 15), np.nan, dtype=np.float32)
    for b, n in enumerate(n_wins):
        x[b, :n] = (20 * rng.standard_normal((n, 1, 48, 15)) - 40).astype(np.float32)
    wgt = (0.5 * rng.standard_normal((16, 1, 3, 3))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(16)).astype(np.float32)
    dz = rng.standard_normal((S, 720, 16)).astype(np.float32)
    seg_off = np.concatenate(([0], np.cumsum(n_wins))).astype(np.int32)

    xs = torch.from_numpy(np.concatenate([x[b, :n] for b, n in enumerate(n_wins)])).double().requires_grad_(True)
    z64 = F.conv2d(xs, torch.from_numpy(wgt).double(), torch.from_numpy(bias).double(), padding=1)
    dz64 = torch.from_numpy(dz).double().reshape(S, 48, 15, 16).permute(0, 3, 1, 2)
    dx64, = torch.autograd.grad((z64 * dz64).sum(), xs)
    z_w = z64.detach().permute(0, 2, 3, 1).reshape(S, 720, 16).numpy()

    xd, wd, bd, dzd, so = _t(x), _t(wgt.reshape(16, 9)), _t(bias), _t(dz), _t(seg_off)
    z = torch.full((S + 1, 720, 16), GUARD, dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.nisqa_conv1_segments_fwd(_p(xd), l_max, _p(so), B, S, _p(wd), _p(bd), _p(z), st), 'nisqa_conv1_segments_fwd')
    runs = []
    for _ in range(2):
        dx = torch.full((B * l_max + 1, 48, 15), GUARD, dtype=torch.float32, device=DEV)
        lib.check(L.nisqa_conv1_segments_dgrad(_p(dzd), _p(so), B, l_max, _p(wd), _p(dx), st), 'nisqa_conv1_segments_dgrad')
        runs.append(dx)
    torch.cuda.synchronize()
    z_g = z.cpu().numpy()
    assert (z_g[S] == GUARD).all()
    e_z = np.abs(z_g[:S] - z_w).max() / np.abs(z_w).max()
    assert torch.equal(runs[0], runs[1])
    dx_g = runs[0].cpu().numpy()
    assert (dx_g[B * l_max] == GUARD).all()
    dx_g = dx_g[:B * l_max].reshape(B, l_max, 48, 15)
    want = np.zeros((B, l_max, 48, 15))
    o = 0
    for b, n in enumerate(n_wins):
        want[b, :n] = dx64[o:o + n, 0].numpy()
        assert (dx_g[b, n:] == 0).all()
        o += n
    e_dx = np.abs(dx_g - want).max() / np.abs(want).max()
    print('S', S, 'z', e_z, 'dx', e_dx)
    assert e_z <= 1e-5 and e_dx <= 1e-5
