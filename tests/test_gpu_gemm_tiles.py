"""Every tile configuration of the training GEMM (gemm_f32_kernel, csrc/train.hip) against exact integer and float64 products.

nisqa_gemm_f32_one picks one of five tiles from (m, n), each compiled in four operand layouts: 20 instantiations, of which the
operator tests of tests/test_gpu_train.py reach nine.  The shapes of tests/gemm_cases.py select every tile (confirmed here and in
tests/test_gemm_tiles_host.py through the library's own selector, nisqa_gemm_f32_one_tile) with interior and ragged tiles; every
(shape, layout, K) runs five operand / epilogue variants, each under two checks:

  exact   operands and bias are integers in [-8, 8]: every partial sum is an integer below 2^24, so any summation order and the
          split-K atomics give exactly the integer product -- torch.equal with the int64 evaluation, the pad of ldc included;
  width   standard normal operands against float64, per element
          |C - ref| <= 2 (K + ksplit + 3) 2^-24 (|alpha| (|A| |B|) + |bias|) + one fp32 ulp of ref   (gemm_cases.width_bound).

Operand storage is filled with NaN around the matrices, so a load outside a matrix fails both checks.

Worst error / bound of the width check on an MI355X, per configuration over all of its cases (printed by every run):
  64x64 0.116, 128x32 0.155, 128x128 0.158, 256x64 0.148, 64x256 0.139, the grouped 64x64 kernel 0.071
(the worst-case bound of K roundings against the random walk the roundings are; the exact check is the sharp one).  All 20
instantiations of nisqa_gemm_f32_one and the grouped kernel in four layouts with and without split-K ran; the exact check
held everywhere.  327 cases in 5 s.

Cuts of the full product of variants (stated, so that nobody takes them for coverage): alignment class, ksplit, alpha and the
epilogue are not crossed with each other but arranged in the five variants of _VARIANTS -- every (shape, layout, K) still runs
the aligned, the ld % 4 != 0 and the offset-pointer class, ksplit 1, 3 and one with empty chunks, alpha 1 and 0.5, bias + ReLU
and a padded ldc.  The long K (1000) runs on one shape per configuration."""
import pytest
import torch

import gemm_cases as GC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
_WORST = {}                 # label -> worst error / bound seen
_SEEN = set()               # (configuration or 'grouped', ta, tb, ksplit class)
_REF = {}                   # the products of the latest (M, N, K): computed once on the CPU, shared by layouts and variants

# (class of A, class of B, ksplit (0: one with empty chunks), alpha, bias + ReLU, pad of ldc, offset of C in floats)
#   'al'  base 16-byte aligned, ld % 4 == 0: the 128-bit loads, interior tiles unguarded
#   'ld'  ld % 4 != 0: guarded scalar loads
#   'off' base offset by one float (the ao / bo offsets the trainers pass), ld % 4 == 0: guarded scalar loads
_VARIANTS = [('al', 'al', 1, 1.0, False, 3, 0),
             ('al', 'al', 1, 0.5, True, 3, 0),
             ('ld', 'ld', 1, 0.5, True, 0, 0),
             ('off', 'off', 3, 1.0, False, 3, 1),
             ('al', 'off', 0, 0.5, False, 0, 0)]


def _L():
    from nisqa_amd import lib
    return lib, lib.load()


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module', autouse=True)
def _summary():
    yield
    print('\nwidth check, worst error / bound: ' + ', '.join('%s %.3f' % kv for kv in sorted(_WORST.items())))
    one = sorted((c, ta, tb) for c, ta, tb, _ in _SEEN if c != 'grouped')
    print('instantiations of nisqa_gemm_f32_one run (configuration, ta, tb): %d distinct: %s' % (len(set(one)), sorted(set(one))))
    print('grouped 64x64 kernel (ta, tb, split-K): %s' % sorted((ta, tb, ks) for c, ta, tb, ks in _SEEN if c == 'grouped'))


def _reference(M, N, K):
    """-> {kind: (A, B, bias on the device; product and |A| |B| in float64 on the device)}"""
    if _REF.get('key') != (M, N, K):
        _REF.clear()
        _REF['key'] = (M, N, K)
        for kind in ('int', 'normal'):
            A, B, bias = GC.operands(M, N, K, kind)
            _REF[kind] = tuple(t.to(DEV) for t in (A, B, bias) + GC.products(A, B))
    return _REF


def _store(mat, trans, cls):
    """op(A) [M][K] or op(B) [K][N] as the kernel reads it (trans: the transpose is what memory holds: A as [K][M], B as the
    weight [N][K]) -> (flat NaN-filled buffer, offset of the matrix in floats, ld)"""
    s = mat.t() if trans else mat
    rows, cols = s.shape
    ld = (cols + 3) // 4 * 4 + (1 if cls == 'ld' else 0)
    off = 1 if cls == 'off' else 0
    buf = torch.full((off + rows * ld + 4,), NAN, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[off:off + rows * ld].view(rows, ld)[:, :cols] = s
    return buf, off, ld


def _run_one(cfg, M, N, K, ta, tb):
    lib, L = _L()
    got = GC.select_tile(L, M, N)
    assert got == (cfg,) + GC.TILES[cfg], got
    ref = _reference(M, N, K)
    print('(%d, %d, %d) layout (%d, %d): configuration %d, tile %d x %d' % ((M, N, K, ta, tb) + got))
    for ca, cb, ksplit, alpha, epi, pad, co in _VARIANTS:
        ksplit = ksplit or GC.empty_chunk_ksplit(K)
        for kind in ('int', 'normal'):
            A, B, bias, prod, mag = ref[kind]
            a, ao, lda = _store(A, ta, ca)
            b, bo, ldb = _store(B, tb, cb)
            ldc = N + pad
            cbuf = torch.full((co + M * ldc,), GC.SENTINEL, device=DEV)
            C = cbuf[co:].view(M, ldc)
            if ksplit > 1:
                C[:, :N] = 0.0                                           # split-K accumulates into a zeroed C
            lib.check(L.nisqa_gemm_f32_one(_p(a, ao), _p(b, bo), _p(cbuf, co), M, N, K, lda, ldb, ldc, ta, tb, ksplit, alpha,
                                           _p(bias) if epi else None, int(epi), _st()), 'gemm')
            torch.cuda.synchronize()
            assert bool((cbuf[:co] == GC.SENTINEL).all())
            what = (M, N, K, ta, tb, ca, cb, ksplit, alpha, epi, ldc)
            if kind == 'int':
                assert GC.check_exact(C, N, prod, alpha, bias if epi else None, epi), what
            else:
                worst, pad_ok = GC.check_width(C, N, prod, mag, K, ksplit, alpha, bias if epi else None, epi)
                print('  A %s B %s ksplit %d alpha %g epilogue %d ldc %d: error / bound %.3f' % (ca, cb, ksplit, alpha, epi, ldc, worst))
                label = '%dx%d' % GC.TILES[cfg]
                _WORST[label] = max(_WORST.get(label, 0.0), worst) if worst == worst else NAN
                assert pad_ok, what
                assert worst <= 1.0, what
            _SEEN.add((cfg, ta, tb, ksplit > 1))


_ONE_CASES = [pytest.param(cfg, M, N, K, ta, tb, id='%dx%d-%dx%dx%d-%d%d' % (GC.TILES[cfg] + (M, N, K, ta, tb)))
              for cfg, shapes in sorted(GC.TILE_SHAPES.items()) for M, N in shapes for K in GC.K_VALUES for ta, tb in GC.LAYOUTS]
_LONG_CASES = [pytest.param(cfg, M, N, GC.LONG_K, ta, tb, id='%dx%d-%dx%dx%d-%d%d' % (GC.TILES[cfg] + (M, N, GC.LONG_K, ta, tb)))
               for cfg, (M, N) in sorted(GC.LONG_K_SHAPES.items()) for ta, tb in GC.LAYOUTS]


@pytest.mark.parametrize('cfg,M,N,K,ta,tb', _ONE_CASES)
def test_every_tile_and_layout_exact_and_within_fp32_width(cfg, M, N, K, ta, tb):
    _run_one(cfg, M, N, K, ta, tb)


@pytest.mark.parametrize('cfg,M,N,K,ta,tb', _LONG_CASES)
def test_every_tile_and_layout_at_a_long_k(cfg, M, N, K, ta, tb):
    _run_one(cfg, M, N, K, ta, tb)


def test_split_k_with_an_epilogue_is_refused():
    lib, L = _L()
    M, N, K = 130, 70, 33
    A, B, bias = (t.to(DEV) for t in GC.operands(M, N, K, 'int'))
    C = torch.full((M, N), GC.SENTINEL, device=DEV)
    for b, relu in ((_p(bias), 0), (None, 1), (_p(bias), 1)):
        assert L.nisqa_gemm_f32_one(_p(A), _p(B), _p(C), M, N, K, K, N, N, 0, 0, 3, 1.0, b, relu, _st()) == lib.NISQA_ERR_ARG
    torch.cuda.synchronize()
    assert bool((C == GC.SENTINEL).all())


# ---- the grouped entry nisqa_gemm_f32 (64x64 tile, descriptors in device memory) ------------------------------------------------------
def _run_grouped(groups, ta, tb, ksplit, alpha, label):
    lib, L = _L()
    rows, na, nb, nc, tiles = GC.group_table(groups, ta, tb)
    desc = torch.tensor(rows, dtype=torch.int64, device=DEV)
    for kind in ('int', 'normal'):
        a = torch.full((na,), NAN, device=DEV)
        b = torch.full((nb,), NAN, device=DEV)
        c = torch.full((nc,), GC.SENTINEL, device=DEV)
        covered = torch.zeros(nc, dtype=torch.bool, device=DEV)
        ops = []
        for g, (a_off, b_off, c_off, M, N, K, lda, ldb, ldc, _) in enumerate(rows):
            A, B, _ = GC.operands(M, N, K, kind, seed=g + 1)
            sa, sb = (A.t() if ta else A), (B.t() if tb else B)
            a[a_off:a_off + sa.shape[0] * lda].view(sa.shape[0], lda)[:, :sa.shape[1]] = sa.to(DEV)
            b[b_off:b_off + sb.shape[0] * ldb].view(sb.shape[0], ldb)[:, :sb.shape[1]] = sb.to(DEV)
            Cg = c[c_off:c_off + M * ldc].view(M, ldc)
            if ksplit > 1:
                Cg[:, :N] = 0.0
            covered[c_off:c_off + M * ldc].view(M, ldc)[:, :N] = True
            ops.append((Cg, GC.products(A, B)))
        assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        lib.check(L.nisqa_gemm_f32(_p(a), _p(b), _p(c), desc.data_ptr(), len(rows), tiles, ta, tb, ksplit, alpha, _st()), 'gemm')
        torch.cuda.synchronize()
        assert bool((c[~covered] == GC.SENTINEL).all())                  # the gaps between the groups' outputs and every pad
        for g, (Cg, (prod, mag)) in enumerate(ops):
            M, N, K = groups[g]
            if kind == 'int':
                assert GC.check_exact(Cg, N, prod.to(DEV), alpha, None, False), (g, groups[g], ta, tb, ksplit, alpha)
            else:
                worst, pad_ok = GC.check_width(Cg, N, prod.to(DEV), mag.to(DEV), K, ksplit, alpha, None, False)
                print('  group %d (%d, %d, %d): error / bound %.3f' % (g, M, N, K, worst))
                _WORST[label] = max(_WORST.get(label, 0.0), worst) if worst == worst else NAN
                assert pad_ok and worst <= 1.0, (g, groups[g], ta, tb, ksplit, alpha, worst)
    _SEEN.add(('grouped', ta, tb, ksplit > 1))


@pytest.mark.parametrize('alpha', [1.0, 0.125])
@pytest.mark.parametrize('ksplit', [1, 4])
@pytest.mark.parametrize('ta,tb', GC.LAYOUTS)
def test_grouped_entry_six_different_groups(ta, tb, ksplit, alpha):
    _run_grouped(GC.GROUPS, ta, tb, ksplit, alpha, 'grouped 64x64')


@pytest.mark.parametrize('ksplit', [2, 4])
def test_grouped_entry_at_the_attention_weight_gradient_shapes(ksplit):
    _run_grouped(GC.WGRAD_GROUPS, 1, 0, ksplit, 1.0, 'grouped 64x64')
