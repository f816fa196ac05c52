"""The tile tests of the training GEMM, the part that needs no GPU: the library's tile selector (the function the launcher of
nisqa_gemm_f32_one calls) against the shape table of tests/gemm_cases.py and at both sides of every threshold, its declaration
and binding, and the negative control of the two checks of tests/test_gpu_gemm_tiles.py -- three correct fp32 summation orders
pass them, seven planted faults of the kind a tile kernel can have fail them."""
import os
import re

import numpy as np
import pytest
import torch

import gemm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _L():
    from nisqa_amd import lib
    return lib, lib.load()


def test_selector_is_declared_bound_and_exported():
    lib, L = _L()
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_train.h')).read()
    assert re.search(r'^int nisqa_gemm_f32_one_tile\(int64_t m, int64_t n, int32_t\* bm, int32_t\* bn\);', hdr, re.M)
    assert len(lib.TRAIN_SYMBOLS['nisqa_gemm_f32_one_tile'][1]) == 4
    assert 'nisqa_gemm_f32_one_tile' in lib.exported_symbols(lib.LIB_PATH, 'nisqa_gemm_')
    assert L.nisqa_abi_version() == 2                                  # additive: the ABI version stays
    assert L.nisqa_gemm_f32_one_tile(130, 70, None, None) == 0         # either output pointer may be NULL
    # one statement of the rule: the launcher takes tile and configuration from the selector and states no threshold of its own
    src = open(os.path.join(ROOT, 'nisqa_amd', 'csrc', 'train.hip')).read()
    body = src[src.index('extern "C" int nisqa_gemm_f32_one('):]
    body = body[:body.index('\n}\n')]
    assert 'const int cfg = nisqa_gemm_f32_one_tile(m, n, &bm, &bn);' in body and '192' not in body and 'bm =' not in body


def test_shape_table_reaches_every_tile_configuration():
    _, L = _L()
    assert sorted(GC.TILE_SHAPES) == sorted(GC.LONG_K_SHAPES) == list(range(len(GC.TILES)))
    for cfg, shapes in GC.TILE_SHAPES.items():
        assert shapes and GC.LONG_K_SHAPES[cfg] in shapes
        for m, n in shapes:
            got = GC.select_tile(L, m, n)
            print('(%d, %d) -> configuration %d, tile %d x %d' % ((m, n) + got))
            assert got == (cfg,) + GC.TILES[cfg], (m, n, got)
    # two tiles along M and along N where the configuration admits it, and a 1-row or 1-column last tile per configuration
    for cfg, (bm, bn) in enumerate(GC.TILES):
        shapes = GC.TILE_SHAPES[cfg]
        assert any(m > bm for m, n in shapes) or cfg == 4
        assert any(n > bn for m, n in shapes) or cfg == 1
        assert any(m >= bm and n >= bn for m, n in shapes)              # an interior tile: the 128-bit loader runs
        assert any(m % bm == 1 or n % bn == 1 for m, n in shapes)


@pytest.mark.parametrize('shape,tile', GC.THRESHOLD_NEIGHBOURS, ids=lambda v: '%dx%d' % v)
def test_selector_at_both_sides_of_every_threshold(shape, tile):
    _, L = _L()
    cfg, bm, bn = GC.select_tile(L, *shape)
    assert (bm, bn) == tile and GC.TILES[cfg] == tile


def test_what_the_epilogue_test_of_the_operator_suite_selects():
    """the four shapes of test_gemm_bias_relu_epilogue_and_large_tiles (tests/test_gpu_train.py), as its comment states them"""
    _, L = _L()
    got = [GC.select_tile(L, m, n)[1:] for m, n in [(700, 64), (600, 300), (64, 576), (1000, 16)]]
    assert got == [(64, 64), (64, 64), (64, 256), (128, 32)]


# ---- negative control: the checks on correct fp32 products and on planted faults ------------------------------------------------------
def _sum_sequential(A, B, k0=0, k1=None):
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    for k in range(k0, A.shape[1] if k1 is None else k1):
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]                       # float32 product, float32 sum: two roundings a term
    return acc


def _sum_blocked(A, B, k0=0, k1=None, skip=None, drop_tail=False):
    k1 = A.shape[1] if k1 is None else k1
    if drop_tail:
        k1 = k0 + (k1 - k0) // 32 * 32
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    for b0 in range(k0, k1, 32):
        part = np.zeros_like(acc)
        for k in range(b0, min(b0 + 32, k1)):
            if k != skip:
                part = part + A[:, k:k + 1] * B[k:k + 1, :]
        acc = acc + part
    return acc


def _sum_split(A, B, ksplit, twice=None):
    """the launcher's split: chunks of ceil(K / ksplit) rounded up to 32, summed into a zeroed C"""
    K = A.shape[1]
    kc = (-(-K // ksplit) + 31) // 32 * 32
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    for c in range(ksplit):
        if c * kc < K:
            part = _sum_blocked(A, B, c * kc, min(K, (c + 1) * kc))
            acc = acc + part
            if c == twice:
                acc = acc + part
    return acc


def _epilogue(acc, N, alpha, bias, relu, no_bias_from=None):
    """-> Cbuf [M][N + 3] with the sentinel in the pad"""
    v = F32(alpha) * acc
    if bias is not None:
        b = bias.copy()
        if no_bias_from is not None:
            b[no_bias_from:] = 0
        v = v + b[None, :]
    if relu:
        v = np.maximum(v, F32(0))
    C = np.full((acc.shape[0], N + 3), GC.SENTINEL, F32)
    C[:, :N] = v
    return C


def _swap_column_blocks(C):
    C = C.copy()
    C[:, 32:64], C[:, 64:96] = C[:, 64:96].copy(), C[:, 32:64].copy()
    return C


def _duplicate_second_row_block(C):
    C = C.copy()
    C[32:64] = C[0:32]                                                   # a wave's second 32 x 32 block written from its first
    return C


def _write_pad(C, N):
    C = C.copy()
    C[C.shape[0] - 1, N] = 0.0
    return C


def _verdicts(kind, C, N, prod, K, ksplit, alpha, bias, relu):
    """-> passes: the exact check on integer operands, the width check (and the pad's sentinel) on normal ones"""
    C = torch.from_numpy(np.ascontiguousarray(C))
    b = None if bias is None else torch.from_numpy(bias)
    if kind == 'int':
        return GC.check_exact(C, N, prod[0], alpha, b, relu)
    worst, pad_ok = GC.check_width(C, N, prod[0], prod[1], K, ksplit, alpha, b, relu)
    return worst <= 1.0 and pad_ok


# shapes of the table: the 64x64 tile, the 128-wide tile with two blocks of rows per wave (its smallest shape cut to the first
# tile row: the control is about the checks, not about 24 tile rows), the 256-wide tile
_CONTROL = [(130, 70), (128, 901), (64, 576)]


@pytest.mark.parametrize('kind', ['int', 'normal'])
@pytest.mark.parametrize('M,N', _CONTROL)
def test_checks_pass_three_summation_orders_and_fail_every_planted_fault(M, N, kind):
    assert (M, N) in GC.TILE_SHAPES[0] + GC.TILE_SHAPES[4] or (2945, N) in GC.TILE_SHAPES[2]
    K, ksplit = 70, 3
    A, B, bias = (t.numpy() for t in GC.operands(M, N, K, kind, seed=5))
    prod = GC.products(torch.from_numpy(A), torch.from_numpy(B))
    good = {
        'sequential': (_epilogue(_sum_sequential(A, B), N, 1.0, None, 0), 1, 1.0, None, 0),
        'blocked by 32': (_epilogue(_sum_blocked(A, B), N, 0.5, bias, 1), 1, 0.5, bias, 1),
        'split-K': (_epilogue(_sum_split(A, B, ksplit), N, 0.5, None, 0), ksplit, 0.5, None, 0),
        'split-K, empty chunks': (_epilogue(_sum_split(A, B, GC.empty_chunk_ksplit(K)), N, 1.0, None, 0),
                                  GC.empty_chunk_ksplit(K), 1.0, None, 0),
    }
    for name, (C, ks, alpha, b, relu) in good.items():
        assert _verdicts(kind, C, N, prod, K, ks, alpha, b, relu), name
    plain = good['sequential'][0]
    bad = {
        'K tail dropped': (_epilogue(_sum_blocked(A, B, drop_tail=True), N, 1.0, None, 0), 1, 1.0, None, 0),
        'one k term dropped': (_epilogue(_sum_blocked(A, B, skip=41), N, 1.0, None, 0), 1, 1.0, None, 0),
        'rows 32..63 duplicated from 0..31': (_duplicate_second_row_block(plain), 1, 1.0, None, 0),
        'bias skipped from column 64': (_epilogue(_sum_blocked(A, B), N, 0.5, bias, 1, no_bias_from=64), 1, 0.5, bias, 1),
        'a split-K chunk added twice': (_epilogue(_sum_split(A, B, ksplit, twice=1), N, 0.5, None, 0), ksplit, 0.5, None, 0),
        'pad of ldc written': (_write_pad(plain, N), 1, 1.0, None, 0),
    }
    if N >= 128:                                                         # a 128- or 256-wide tile
        bad['two 32-column blocks swapped'] = (_swap_column_blocks(plain), 1, 1.0, None, 0)
    for name, (C, ks, alpha, b, relu) in bad.items():
        caught = not _verdicts(kind, C, N, prod, K, ks, alpha, b, relu)
        print('%s operands, %d x %d: %s -> %s' % (kind, M, N, name, 'caught' if caught else 'MISSED'))
        assert caught, name
