"""d model(x, n_wins) / d x of NISQA_DE on the MI355X: the two new entries of csrc/de_align.hip (soft alignment at packed offsets
with kept statistics, and its backward) against torch float64, their write pattern and determinism; then model(x, n_wins) with
x.requires_grad against the float64 oracle (tests/input_grad_de_oracle.py) and the reference's fixtures, with the contract around
it (values unchanged, padding rows, dtype and device of the gradient)."""
import ctypes

import numpy as np
import pytest
import torch

import de_oracle as DO
import helpers
import input_grad_de_oracle as IGD

pytestmark = pytest.mark.gpu
PRECISIONS = ['f32', 'bf16x6']
BAR = 1e-3                  # tests/test_gpu_input_grad.py's bar: max |dx - want| <= BAR * max |want| per clip and channel, no floor
DEV = 'cuda:0'
PAIRS = [(1, 1), (1, 7), (7, 1), (65, 3), (64, 64), (130, 97)]      # tests/test_gpu_train_de.py's: one row, a partial tile, 2+ LDS blocks
ALIGNS, FUSES = ('dot', 'cosine'), ('x/y/-', '+/-', 'x/y')
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * off)


def _lib():
    from nisqa_amd import lib
    return lib.load(), lib


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
class _Layout(object):
    """PAIRS in the packed layout with one guard row behind every clip: the degraded clips, then the reference clips"""

    def __init__(self, pairs, seed, zero_rows=()):
        self.pairs, self.B = pairs, len(pairs)
        n = np.array([p[0] for p in pairs] + [p[1] for p in pairs], dtype=np.int64)
        self.n = n
        self.off = np.concatenate(([0], np.cumsum(n + 1)))[:-1].astype(np.int32)
        self.rows = int((n + 1).sum())
        self.tile_off = np.concatenate(([0], np.cumsum((n[:self.B] + 63) // 64))).astype(np.int32)
        rng = np.random.default_rng(seed)
        self.x = np.full((self.rows, 64), np.nan, np.float32)                     # guard rows are NaN: never read
        self.valid = np.zeros(self.rows, bool)
        for c in range(2 * self.B):
            self.x[self.off[c]:self.off[c] + n[c]] = rng.standard_normal((n[c], 64))     # unit variance, as LayerNorm output
            self.valid[self.off[c]:self.off[c] + n[c]] = True
        for c, r in zero_rows:
            self.x[self.off[c] + r] = 0.0
        self.deg_rows = np.concatenate([self.off[b] + np.arange(n[b]) for b in range(self.B)])
        self.dev = dict(x=_t(self.x), off=_t(self.off), n=_t(n.astype(np.int32)), tile_off=_t(self.tile_off))

    def side(self, b, ref):
        c = b + self.B * ref
        return slice(int(self.off[c]), int(self.off[c] + self.n[c]))

    def table_ptrs(self):
        d, B = self.dev, self.B
        return _p(d['off']), _p(d['n']), _p(d['off'], B), _p(d['n'], B)


def _soft_forward(lay, align, fuse):
    """nisqa_de_align_soft_packed on the layout -> (out [rows][F], lse [rows], aligned [rows][64]) pre-filled with NaN"""
    L, lib = _lib()
    F = DO.FUSE_WIDTH[fuse]
    out = torch.full((lay.rows, F), np.nan, dtype=torch.float32, device=DEV)
    lse = torch.full((lay.rows,), np.nan, dtype=torch.float32, device=DEV)
    al = torch.full((lay.rows, 64), np.nan, dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.nisqa_de_align_soft_packed(_p(lay.dev['x']), *lay.table_ptrs(), _p(lay.dev['tile_off']), lay.B, int(lay.tile_off[-1]),
                                           ALIGNS.index(align), FUSES.index(fuse), F, _p(out), _p(lse), _p(al), st),
              'nisqa_de_align_soft_packed')
    return out, lse, al


def _fp32_bar(err32):
    """1e-5, or twice what torch's fp32 CPU evaluation of the same function is off from float64 (tests/test_gpu_de.py's rule for
    soft outputs: dot-product scores of unit rows reach |s| ~ 30 and the weights carry their fp32 rounding)"""
    return max(1e-5, 2.0 * float(err32))


def _align_autograd(xd, xr, dF, align, fuse, dtype):
    """torch autograd of soft alignment + fusion in ``dtype`` -> (fused, lse, aligned, d_deg, d_ref) as float64 numpy"""
    q = torch.from_numpy(xd).to(dtype).requires_grad_(True)
    y = torch.from_numpy(xr).to(dtype).requires_grad_(True)
    att = IGD.scores(q, y, align)
    a = torch.softmax(att, 1) @ y
    fused = IGD.fuse_rows(q, a, fuse)
    dq, dy = torch.autograd.grad((fused * torch.from_numpy(dF).to(dtype)).sum(), (q, y))
    return [v.detach().double().numpy() for v in (fused, torch.logsumexp(att, 1), a, dq, dy)]


@pytest.mark.parametrize('fuse', FUSES)
@pytest.mark.parametrize('align', ALIGNS)
def test_packed_soft_forward_is_the_inference_kernel_and_keeps_its_statistics(align, fuse):
    """fused rows: bit for bit nisqa_de_align_fuse(apply = 1) on the same valid rows (the same kernel source and arithmetic);
    lse and the aligned rows against float64 within max(1e-5, 2 x torch's fp32 CPU error); guard rows untouched.
    Measured: lse <= 7.0e-6 (dot) / 7.7e-7 (cosine), aligned rows <= 7.7e-6 / 2.1e-7."""
    L, lib = _lib()
    from nisqa_amd.engine import BatchPlan
    lay = _cached(('lay', 7), lambda: _Layout(PAIRS, 7))
    F, B = DO.FUSE_WIDTH[fuse], lay.B
    out, lse, al = _soft_forward(lay, align, fuse)
    # the inference layout: every clip at a multiple of 64 rows
    plan = BatchPlan.from_n_wins(lay.n)
    xp = np.full((plan.total_tok, 64), np.nan, np.float32)
    for c in range(2 * B):
        xp[plan.tok_off[c]:plan.tok_off[c] + lay.n[c]] = lay.x[lay.off[c]:lay.off[c] + lay.n[c]]
    d = plan.to(torch.device(DEV))
    np_deg = int(plan.tok_off[B])
    ref_out = torch.zeros((np_deg, F), dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tk, nk = d['tok_off'], d['n_wins']
    lib.check(L.nisqa_de_align_fuse(_p(_t(xp)), _p(tk), _p(nk), _p(tk, B), _p(nk, B), B, np_deg, ALIGNS.index(align), 1,
                                    FUSES.index(fuse), F, _p(ref_out), None, st), 'nisqa_de_align_fuse')
    torch.cuda.synchronize()
    out, lse, al, ref_out = out.cpu().numpy(), lse.cpu().numpy(), al.cpu().numpy(), ref_out.cpu().numpy()
    written = np.zeros(lay.rows, bool)
    written[lay.deg_rows] = True
    assert np.isnan(out[~written]).all() and np.isnan(lse[~written]).all() and np.isnan(al[~written]).all()
    assert np.isfinite(out[written]).all() and np.isfinite(lse[written]).all() and np.isfinite(al[written]).all()
    for b, (nx, ny) in enumerate(PAIRS):
        rows = lay.side(b, 0)
        assert np.array_equal(out[rows], ref_out[plan.tok_off[b]:plan.tok_off[b] + nx]), b
        if fuse != '+/-':
            assert np.array_equal(al[rows], out[rows, 64:128])               # the aligned row is the fusion's y part
        xd, xr = lay.x[rows], lay.x[lay.side(b, 1)]
        dF = np.zeros((nx, F), np.float32)
        w64 = _align_autograd(xd, xr, dF, align, fuse, torch.float64)
        w32 = _align_autograd(xd, xr, dF, align, fuse, torch.float32)
        for name, got, k in (('lse', lse[rows], 1), ('aligned', al[rows], 2)):
            err, tol = np.abs(got - w64[k]).max(), _fp32_bar(np.abs(w32[k] - w64[k]).max())
            print(align, fuse, (nx, ny), name, 'max |d| %.3g' % err, 'bar %.3g' % tol)
            assert err <= tol, (b, name, err, tol)


@pytest.mark.parametrize('fuse', FUSES)
@pytest.mark.parametrize('align', ALIGNS)
def test_soft_backward_against_float64_autograd(align, fuse):
    """d_deg and d_ref of every pair against torch float64 autograd of alignment + fusion, relative to that side's largest entry,
    within max(1e-5, 2 x the error of torch's fp32 CPU autograd of the same function).  The outputs are pre-filled with NaN and
    every clip has a guard row behind it: every valid row is written, nothing else is touched, two runs give the same bits.
    Measured: <= 5.2e-6 (dot) / 5.0e-7 (cosine)."""
    L, lib = _lib()
    lay = _cached(('lay', 7), lambda: _Layout(PAIRS, 7))
    F, B = DO.FUSE_WIDTH[fuse], lay.B
    dF = np.full((lay.rows, F), np.nan, np.float32)
    dF[lay.deg_rows] = np.random.default_rng(11).standard_normal((len(lay.deg_rows), F))
    out, lse, al = _soft_forward(lay, align, fuse)
    dFd = _t(dF)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        dx = torch.full((lay.rows, 64), np.nan, dtype=torch.float32, device=DEV)
        lib.check(L.nisqa_de_align_soft_bwd(_p(lay.dev['x']), _p(dFd), F, _p(lse), _p(al), *lay.table_ptrs(), B,
                                            int(lay.n.max()), ALIGNS.index(align), FUSES.index(fuse), _p(dx), _p(dx), st),
                  'nisqa_de_align_soft_bwd')
        runs.append(dx)
    torch.cuda.synchronize()
    got = runs[0].cpu().numpy()
    assert np.array_equal(got.view(np.int32), runs[1].cpu().numpy().view(np.int32))              # NaN guards included: bits
    assert np.isfinite(got[lay.valid]).all() and np.isnan(got[~lay.valid]).all()
    # two buffers, each addressed by its own side's offsets: the same values
    d_deg = torch.full((lay.rows, 64), np.nan, dtype=torch.float32, device=DEV)
    d_ref = torch.full((lay.rows, 64), np.nan, dtype=torch.float32, device=DEV)
    lib.check(L.nisqa_de_align_soft_bwd(_p(lay.dev['x']), _p(dFd), F, _p(lse), _p(al), *lay.table_ptrs(), B, int(lay.n.max()),
                                        ALIGNS.index(align), FUSES.index(fuse), _p(d_deg), _p(d_ref), st), 'nisqa_de_align_soft_bwd')
    torch.cuda.synchronize()
    d_deg, d_ref = d_deg.cpu().numpy(), d_ref.cpu().numpy()
    for b, (nx, ny) in enumerate(PAIRS):
        rd, rr = lay.side(b, 0), lay.side(b, 1)
        assert np.array_equal(d_deg[rd], got[rd]) and np.array_equal(d_ref[rr], got[rr])
        assert np.isnan(d_deg[rr]).all() and np.isnan(d_ref[rd]).all()
        w64 = _align_autograd(lay.x[rd], lay.x[rr], dF[rd], align, fuse, torch.float64)
        w32 = _align_autograd(lay.x[rd], lay.x[rr], dF[rd], align, fuse, torch.float32)
        for name, rows, k in (('d_deg', rd, 3), ('d_ref', rr, 4)):
            top = np.abs(w64[k]).max()
            err, tol = np.abs(got[rows] - w64[k]).max() / top, _fp32_bar(np.abs(w32[k] - w64[k]).max() / top)
            print(align, fuse, (nx, ny), name, 'relative distance %.3g' % err, 'bar %.3g' % tol)
            assert top > 0 and err <= tol, (b, name, err, tol)


def test_all_zero_rows_under_cosine_give_a_finite_gradient():
    """the kernel's clamped-denominator convention (a row of norm <= 1e-8 is divided by 1e-8, forward and backward); torch's
    autograd differs there by definition and is not consulted"""
    L, lib = _lib()
    lay = _Layout([(7, 5), (3, 66)], 5, zero_rows=[(0, 2), (2, 1), (3, 65)])         # a degraded row, two reference rows
    F = 192
    dF = np.full((lay.rows, F), np.nan, np.float32)
    dF[lay.deg_rows] = np.random.default_rng(12).standard_normal((len(lay.deg_rows), F))
    out, lse, al = _soft_forward(lay, 'cosine', 'x/y/-')
    dx = torch.full((lay.rows, 64), np.nan, dtype=torch.float32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(L.nisqa_de_align_soft_bwd(_p(lay.dev['x']), _p(_t(dF)), F, _p(lse), _p(al), *lay.table_ptrs(), lay.B, int(lay.n.max()),
                                        1, 0, _p(dx), _p(dx), st), 'nisqa_de_align_soft_bwd')
    torch.cuda.synchronize()
    got = dx.cpu().numpy()
    assert np.isfinite(out.cpu().numpy()[lay.deg_rows]).all() and np.isfinite(lse.cpu().numpy()[lay.deg_rows]).all()
    assert np.isfinite(got[lay.valid]).all() and np.isnan(got[~lay.valid]).all()


# ---- model(x, n_wins) with x.requires_grad ----------------------------------------------------------------------------------------
def _case(config, spec_name):
    return _cached(('case', config, spec_name), lambda: IGD.case(config, getattr(IGD, spec_name), fill=np.nan))


def _model(config, precision):
    """the package's module with the cases' weights (SMALL and EDGE share them) and an engine of ``precision``"""
    def make():
        from nisqa_amd import NISQA_lib as NL
        from nisqa_amd.engine import HipNisqaDE
        sd, args = _case(config, 'SMALL')[:2]
        m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m._engine = HipNisqaDE(args, m.state_dict(), DEV, precision=precision)
        return m
    return _cached(('model', config, precision), make)


def _oracle(config, spec_name, idx):
    """float64, and the float32 CPU run of the same chain for dot/soft; idx: the GPU's hard indices per pair (None: soft)"""
    def make():
        sd, args, x, n_wins, g = _case(config, spec_name)
        want = IGD.oracle(sd, args, x, n_wins, [g], idx=idx)
        want['dx32'] = IGD.oracle(sd, args, x, n_wins, [g], dtype=torch.float32, margins=False)['dx'][0] \
            if config[:2] == ('dot', 'soft') else None
        return want
    key = None if idx is None else tuple(np.concatenate(idx).tolist())
    return _cached(('oracle', config, spec_name, key), make)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('config', IGD.CONFIGS, ids=lambda c: IGD.NAMES[c])
@pytest.mark.parametrize('spec_name', ['SMALL', 'EDGE'])
def test_model_gradient_against_the_float64_oracle(spec_name, config, precision):
    """SMALL: pairs of (1, 3), (3, 1), (2, 2) segments padded to L = 4 with NaN -- nothing is left out and every hard index must be
    float64's.  EDGE: (65, 3), (1, 65), (64, 64) -- segments whose float64 CNN tie margin is under 1e-5 have their own rows of dx
    left out (at most 15 % of them), and where the float64 top-2 score gap is <= 1e-5 the oracle gathers the row the GPU chose.
    Per clip and channel max |dx - want| <= 1e-3 max |want|; for dot/soft max(1e-3, 2 x the fp32-CPU distance of the oracle chain).
    Measured, worst clip and channel, f32 / bf16x6: SMALL cos_hard 4.7e-6 / 5.0e-6, dot_soft 5.1e-6 / 4.3e-6,
    cos_soft 3.2e-6 / 3.7e-6 (against the reference fixture <= 7.3e-6); EDGE (28 of 262 segments left out, 19 near-tie tokens)
    cos_hard 6.1e-6 / 7.4e-6, dot_soft 7.3e-6 / 8.6e-6 (the fp32 CPU run of the oracle chain: 5.3e-6), cos_soft 9.6e-6 / 7.9e-6."""
    sd, args, x, n_wins, g = _case(config, spec_name)
    m = _model(config, precision)
    B, L, hard = len(n_wins), x.shape[1], config[1] == 'hard'
    nt = torch.as_tensor(n_wins)
    xd = _t(x).requires_grad_(True)
    y = m(xd, nt)
    assert y.grad_fn is not None and y.device == xd.device and tuple(y.shape) == (B, 1)
    with torch.no_grad():
        y_plain = m(_t(x), nt)
    assert y_plain.grad_fn is None and torch.equal(y.detach(), y_plain)          # bit for bit the plain call
    assert m(_t(x), nt).grad_fn is None                                          # a plain x: nothing to differentiate
    dx, = torch.autograd.grad(y, xd, _t(g), retain_graph=True)
    assert dx.shape == xd.shape and dx.dtype == torch.float32 and dx.device == xd.device
    y.backward(_t(g))
    assert torch.equal(xd.grad, dx)                                              # backward and autograd.grad: the same bits
    got = dx.cpu().numpy()
    assert np.isfinite(got).all()
    for b in range(B):
        for c in range(2):
            assert (got[b, n_wins[b, c]:, c] == 0).all()                         # exactly zero: the NaN there does not leak
    idx = None
    if hard:
        flat = m._engine._input_grad.last_idx.cpu().numpy()
        idx = np.split(flat, np.cumsum(n_wins[:, 0])[:-1])
    want = _oracle(config, spec_name, idx)
    np.testing.assert_allclose(y_plain.cpu().numpy(), want['y'], rtol=0, atol=1e-3)
    valid = np.isfinite(want['margin'])
    out = valid & (want['margin'] < IGD.TIE)
    near = sum(int((gp <= IGD.TIE).sum()) for gp in want['gap'])
    print(spec_name, IGD.NAMES[config], precision, 'segments', int(valid.sum()), 'left out', int(out.sum()), 'near-tie tokens', near)
    if spec_name == 'SMALL':
        assert valid.sum() == 12 and out.sum() == 0 and near == 0
    else:
        assert valid.sum() == 262 and out.sum() <= 0.15 * valid.sum()
    if hard:
        for b in range(B):                                                       # outside a near-tie the GPU's index is float64's
            sure = want['gap'][b] > IGD.TIE
            assert (idx[b][sure] == want['own'][b][sure]).all(), (b, np.nonzero(idx[b][sure] != want['own'][b][sure]))
            assert ((idx[b] >= 0) & (idx[b] < n_wins[b, 1])).all()
    keep = valid & ~out
    w = want['dx'][0]
    err = IGD.channel_error(got, w, keep)
    bar = BAR
    if want['dx32'] is not None:
        e32 = IGD.channel_error(want['dx32'], w, keep)
        bar = max(BAR, 2.0 * float(e32.max()))
        print('   fp32 CPU run of the oracle chain against float64', e32.ravel())
    print('   relative distance per clip and channel', err.ravel(), 'bar', bar)
    assert (err <= bar).all(), err
    if spec_name == 'SMALL':
        fx = helpers.golden('input_grad_de_%s.npz' % IGD.NAMES[config])
        assert np.array_equal(fx['g'], g) and fx['n_wins'].tolist() == n_wins.tolist()
        efx = IGD.channel_error(got, fx['dx'])
        print('   against the reference fixture', efx.ravel())
        assert (efx <= bar).all(), efx
        np.testing.assert_allclose(y_plain.cpu().numpy(), fx['y'], rtol=0, atol=1e-3)


@pytest.mark.parametrize('config', IGD.CONFIGS[:2], ids=lambda c: IGD.NAMES[c])
def test_gradient_comes_back_in_the_dtype_and_on_the_device_of_x(config):
    sd, args, x, n_wins, g = _case(config, 'SMALL')
    m = _model(config, 'f32')
    nt = torch.as_tensor(n_wins)
    xg = _t(x).requires_grad_(True)
    m(xg, nt).backward(_t(g))
    xh = torch.from_numpy(x.copy()).requires_grad_(True)                      # on the host
    y = m(xh, nt)
    assert y.grad_fn is not None and y.is_cuda
    y.backward(_t(g))
    assert xh.grad.device.type == 'cpu' and xh.grad.dtype == torch.float32 and xh.grad.shape == xh.shape
    assert torch.equal(xh.grad, xg.grad.cpu())
    x64 = _t(x).double().requires_grad_(True)                                 # float64 on the device
    m(x64, nt).backward(_t(g))
    assert x64.grad.is_cuda and x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float(), xg.grad)
    with torch.no_grad():
        assert m(torch.from_numpy(x.copy()).requires_grad_(True), nt).grad_fn is None
