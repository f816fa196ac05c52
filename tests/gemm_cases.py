"""Cases and checks of the training GEMM's tile tests (nisqa_gemm_f32_one / nisqa_gemm_f32, csrc/train.hip): the shape table that
visits every tile configuration, operands and their high-precision products, and the two checks -- exact on small integers, fp32
width against float64 on normal operands.  tests/test_gemm_tiles_host.py proves on the CPU that the checks tell a right product
from planted faults; tests/test_gpu_gemm_tiles.py applies them to the kernels.  Everything here is torch on whatever device the
tensors live on; nothing launches a kernel of the library."""
import ctypes

import torch

TILES = [(64, 64), (128, 32), (128, 128), (256, 64), (64, 256)]          # configuration index -> (BM, BN)
# configuration index -> shapes (M, N) that select it (the host test asks the library's selector).  Two tiles along M and along N
# where the configuration admits it (128x32 has one tile of columns, 64x256 one tile of rows): an interior tile for the 128-bit
# loader and ragged last tiles; 2945 = 23 * 128 + 1, 3969 = 31 * 128 + 1, 48897 = 191 * 256 + 1 and 257 leave a 1-row last tile,
# 1 x 1 a 1-column one; (257, 32) is the only width at which the B loader of 128x32 has an interior tile.
TILE_SHAPES = {
    0: [(130, 70), (1, 1)],
    1: [(300, 17), (1000, 20), (257, 32)],
    2: [(2945, 901), (3969, 768)],
    3: [(48897, 33), (24323, 100)],
    4: [(64, 576), (1, 256), (37, 515)],
}
LONG_K_SHAPES = {0: (130, 70), 1: (300, 17), 2: (2945, 901), 3: (24323, 100), 4: (37, 515)}
K_VALUES = (1, 20, 31, 32, 33, 70)         # around the 32-deep K tile: a tail alone, a full tile, a tile and a tail, two and a tail
LONG_K = 1000                              # 31 K tiles and a tail of 8
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
SENTINEL = -12345.0                        # what the pad of a padded ldc and the gaps between groups must keep, bit for bit
# neighbours of every threshold of the selector: (m, n) -> (BM, BN)
THRESHOLD_NEIGHBOURS = [((3969, 768), (128, 128)), ((3968, 768), (256, 64)), ((2945, 901), (128, 128)), ((2944, 901), (64, 64)),
                        ((48897, 33), (256, 64)), ((48896, 33), (64, 64)), ((65, 32), (128, 32)), ((64, 256), (64, 256)),
                        ((1, 256), (64, 256)), ((65, 256), (64, 64))]


def select_tile(L, m, n):
    """-> (configuration index, BM, BN) from the library's own selector, the function its launcher calls"""
    bm, bn = ctypes.c_int32(-1), ctypes.c_int32(-1)
    cfg = L.nisqa_gemm_f32_one_tile(m, n, ctypes.byref(bm), ctypes.byref(bn))
    return cfg, bm.value, bn.value


def empty_chunk_ksplit(K):
    """a ksplit whose last chunks are empty: chunks are multiples of 32, and ksplit * 32 > K"""
    return K // 32 + 2


def operands(M, N, K, kind, seed=0):
    """A [M][K], B [K][N], bias [N] on the CPU in float32: integers in [-8, 8] ('int') or standard normal ('normal')"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * M + 31 * N + K + (0 if kind == 'int' else 1 << 20))
    if kind == 'int':
        return tuple(torch.randint(-8, 9, s, generator=g).float() for s in ((M, K), (K, N), (N,)))
    return tuple(torch.randn(*s, generator=g) for s in ((M, K), (K, N), (N,)))


def products(A, B):
    """-> (A B, |A| |B|) in float64 on the CPU.  For the integer operands every partial sum is an integer far below 2^53, so the
    float64 product IS the integer product in any summation order; exact_want converts it to int64."""
    a, b = A.double(), B.double()
    return a @ b, a.abs() @ b.abs()


def exact_want(P, alpha, bias, relu):
    """The result of integer operands, evaluated in int64 in units of 1/8: alpha * P (+ bias) (ReLU) -> float32, exact.
    P: the integer product (float64 or int64), bias: integers or None, alpha: a multiple of 1/8."""
    q = int(round(alpha * 8))
    assert q / 8.0 == alpha
    e8 = P.to(torch.int64) * q
    if bias is not None:
        e8 = e8 + 8 * bias.to(torch.int64)
    if relu:
        e8 = e8.clamp_min(0)
    assert e8.numel() == 0 or int(e8.abs().max()) < 1 << 24          # exact in float32, and so was every partial sum
    return (e8.to(torch.float64) / 8).to(torch.float32)


def check_exact(Cbuf, N, P, alpha, bias, relu):
    """Cbuf [M][ldc] as the kernel left it, sentinel in the pad -> True iff bit for bit the integer result, pad included"""
    want = torch.full_like(Cbuf, SENTINEL)
    want[:, :N] = exact_want(P, alpha, bias, relu)
    return torch.equal(Cbuf, want)


def width_bound(ref, mag, K, ksplit, alpha, bias, relu):
    """-> (want, bound) in float64.  |C - want| <= 2 (K + ksplit + 3) 2^-24 (|alpha| (|A| |B|) + |bias|) + one fp32 ulp of want:
    the textbook bound of K fused multiply-adds in any order (plus the ksplit partial sums, alpha, bias and the store), with a
    factor 2 for the MFMA's unspecified internal rounding of its two products.  Derived, not tuned."""
    want = alpha * ref
    mag = abs(alpha) * mag
    if bias is not None:
        want = want + bias.double()
        mag = mag + bias.double().abs()
    if relu:
        want = want.clamp_min(0.0)                                   # 1-Lipschitz: the bound carries over
    _, e = torch.frexp(want)                                         # |want| in [2^(e-1), 2^e): one fp32 ulp is 2^(e-24)
    ulp = torch.ldexp(torch.ones_like(want), (e - 24).clamp_min(-149))
    ulp = torch.where(want == 0, torch.full_like(want, 2.0 ** -149), ulp)          # frexp(0) = (0, 0)
    return want, 2.0 * (K + ksplit + 3) * 2.0 ** -24 * mag + ulp


def check_width(Cbuf, N, ref, mag, K, ksplit, alpha, bias, relu):
    """-> (worst error / bound over the M x N result: NaN if the kernel wrote one; pad intact)"""
    want, bound = width_bound(ref, mag, K, ksplit, alpha, bias, relu)
    ratio = ((Cbuf[:, :N].double() - want).abs() / bound)
    worst = float(ratio.max()) if not bool(torch.isnan(ratio).any()) else float('nan')
    return worst, bool((Cbuf[:, N:] == SENTINEL).all())


# ---- the grouped entry: one descriptor table of six groups -------------------------------------------------------------------------
# (M, N, K): a 1 x 1 group, a single partial tile, several tiles with ragged edges, exactly one full tile (the interior loader),
# a 1-column and a wide group; K = 1, 33, 70, 32, 31, 20
GROUPS = [(1, 1, 1), (37, 50, 33), (130, 70, 70), (64, 64, 32), (65, 1, 31), (5, 200, 20)]
# the attention block's weight-gradient call (nisqa_tdtrain_step: dW = dY^T X, layout (1, 0), K = tokens of a clip)
WGRAD_GROUPS = [(64, 64, 1), (192, 64, 33), (64, 192, 70), (128, 128, 33), (64, 128, 70), (128, 192, 1)]


def group_table(groups, ta, tb):
    """-> (rows [G][10] of int64 as nisqa_gemm_f32 reads them, sizes of the A, B, C buffers in floats).  Every group gets its own
    leading dimensions and offsets: a_off / b_off alternate between 16-byte aligned and odd, lda / ldb between multiples of 4 and
    odd values (so the groups of one launch take all three loader paths), ldc = N + (g mod 3), and a gap of 5 + g floats follows
    every group's output."""
    rows, a_off, b_off, c_off, tile = [], 0, 0, 3, 0
    for g, (M, N, K) in enumerate(groups):
        ar, ac = (K, M) if ta else (M, K)
        br, bc = (N, K) if tb else (K, N)
        lda = (ac + 3) // 4 * 4 + (1 if g % 3 == 1 else 0)
        ldb = (bc + 3) // 4 * 4 + (1 if g % 3 == 2 else 0)
        ldc = N + g % 3
        a_off = (a_off + 3) // 4 * 4 + (1 if g % 2 else 0)
        b_off = (b_off + 3) // 4 * 4 + (1 if g % 4 >= 2 else 0)
        rows.append([a_off, b_off, c_off, M, N, K, lda, ldb, ldc, tile])
        a_off += ar * lda
        b_off += br * ldb
        c_off += M * ldc + 5 + g
        tile += ((M + 63) // 64) * ((N + 63) // 64)
    return rows, a_off + 4, b_off + 4, c_off, tile
