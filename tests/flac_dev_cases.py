"""Streams for the tests of the device FLAC decoder (csrc/flac_frame.hpp, nisqa_flac_decode) -- test infrastructure only.

Every stream is written by flac_enc (an independent writer of the published format); ``streams()`` is the list the CPU and the GPU
tests share, generated once per process.  Clips are 200-5 000 samples (flac_enc is pure Python) and at least one block long: a
shorter clip has min_block != max_block in STREAMINFO and is not eligible for the device path.  ``Stream.sizes`` records, from inside
the writer, how long every frame of a stream is: the independent walk the plan / read tests compare the native frame table with.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np

import flac_enc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def signal(n, ch=1, bits=16, seed=0, amp=0.3):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    a = (1 << (bits - 1)) * amp
    cols = []
    for c in range(ch):
        y = a * (0.6 * np.sin(2 * np.pi * t / (97.0 + 5 * c)) + 0.3 * np.sin(2 * np.pi * t / 13.1 + c)) + rng.normal(0, a * 0.02 + 0.6, n)
        cols.append(np.round(y).astype(np.int64))
    if ch == 2:
        cols[1] = cols[0] + np.round(rng.normal(0, a * 0.01 + 1.0, n)).astype(np.int64)      # correlated: a small, often odd side channel
    x = np.stack(cols, axis=1) if ch > 1 else cols[0]
    return np.clip(x, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)


class Stream(object):
    def __init__(self, name, x, sr, bits, **kw):
        self.name, self.x, self.sr, self.bits, self.kw = name, np.asarray(x, dtype=np.int64), sr, bits, kw
        self.data, self.first_frame, self.sizes = encode_with_frames(self.x, sr, bits, **kw)
        self.blocksize = kw.get('blocksize', 4096)

    @property
    def channels(self):
        return 1 if self.x.ndim == 1 else self.x.shape[1]

    def samples(self):
        """[n, channels] int32: what any decoder must return."""
        return self.x.reshape(len(self.x), -1).astype(np.int32)

    def rows(self):
        """(offset in the region, first sample, block size) of every frame, from the writer's own frame sizes."""
        n, bs = len(self.x), self.blocksize
        off = np.concatenate(([0], np.cumsum(self.sizes[:-1])))
        return [(int(o), k * bs, min(bs, n - k * bs)) for k, o in enumerate(off)]

    def __repr__(self):
        return 'Stream(%s)' % self.name


def encode_with_frames(x, sr, bits, **kw):
    """flac_enc.encode -> (file bytes, offset of the first frame, byte size of every frame): the sizes are taken where the writer
    computes each frame's CRC-16."""
    sizes, orig = [], flac_enc.crc_bitwise

    def spy(data, poly, width):
        if width == 16:
            sizes.append(len(data) + 2)
        return orig(data, poly, width)
    flac_enc.crc_bitwise = spy
    try:
        data = flac_enc.encode(x, sr, bits, **kw)
    finally:
        flac_enc.crc_bitwise = orig
    return data, len(data) - sum(sizes), sizes


@functools.lru_cache(maxsize=None)
def streams():
    """The stream list of the device decoder's tests: every feature of the format the decoder claims, all eligible for the device."""
    S, out = Stream, []
    fx = lambda o, **k: dict({'type': 'fixed', 'order': o}, **k)                      # noqa: E731
    lpc = lambda o, p, **k: dict({'type': 'lpc', 'order': o, 'precision': p}, **k)    # noqa: E731
    for o in range(5):                                                               # fixed 0-4; a last block of 37 samples
        out.append(S('fixed%d' % o, signal(3 * 192 + 37, seed=o), 16000, 16, kinds=fx(o), blocksize=192))
    for o in (1, 2, 8, 12, 32):                                                      # LPC orders x coefficient precisions
        for p in (5, 12, 15):
            out.append(S('lpc%d_%d' % (o, p), signal(600, seed=10 * o + p), 44100, 16, kinds=lpc(o, p), blocksize=256))
    # 24-bit mid/side and left/side at full scale with LPC 32 / 15: 25 + 15 + 5 bits -- the 64-bit restore
    loud = signal(700, ch=2, bits=24, seed=3, amp=0.98)
    out.append(S('wide_ms', loud, 48000, 24, kinds=lpc(32, 15), stereo=10, blocksize=256))
    out.append(S('wide_ls', loud, 48000, 24, kinds=lpc(32, 15, porder=2), stereo=8, blocksize=256))
    quiet = signal(768, seed=4)
    quiet[300:420] = 0                                                               # zero residuals: k = 0 and escape width 0
    for name, kind in (('p0', fx(2, porder=0)), ('p3', fx(2, porder=3)), ('pmax', fx(1, porder=8)), ('pmax_lpc', lpc(8, 12, porder=5)),
                       ('rice5', lpc(6, 12, porder=2, method=1)), ('rice5_fixed', fx(3, porder=1, method=1)),
                       ('esc', fx(2, porder=2, escape=(0, 2))), ('esc5', fx(3, porder=4, method=1, escape=(1, 7, 15))),
                       ('esc_all', fx(0, porder=3, escape=tuple(range(8)))), ('esc_lpc', lpc(4, 12, porder=1, escape=(1,)))):
        out.append(S(name, quiet, 48000, 16, kinds=kind, blocksize=256))
    jump = np.zeros(512, dtype=np.int64)                                             # k = 0 wins a partition of zeros with ONE residual of
    jump[100], jump[300] = 30, -45                                                   # 30 / -45: a unary run of 60 / 89 zeros (> 32, > 64)
    out.append(S('jump', jump, 16000, 16, kinds=fx(0, porder=2), blocksize=256))
    step = np.zeros(600, dtype=np.int64)
    step[200:400] = -1234
    out.append(S('const', step, 8000, 16, kinds=lambda k, c: {'type': 'constant'}, blocksize=200))
    out.append(S('verbatim', signal(500, seed=5), 16000, 16, kinds={'type': 'verbatim'}, blocksize=250))
    w8 = signal(512, seed=6) // 8 * 8                                                # three wasted bits in every block
    for name, kind in (('wasted_v', {'type': 'verbatim'}), ('wasted_f', fx(2)), ('wasted_l', lpc(4, 12)), ('wasted_c', {'type': 'constant'})):
        out.append(S(name, np.full(512, 64, dtype=np.int64) if name == 'wasted_c' else w8, 16000, 16, kinds=kind, blocksize=256))
    edge = signal(600, ch=2, seed=7)                                                 # +-full scale, odd sides
    edge[:8] = [[32767, -32768], [-32768, 32767], [32767, 32767], [-32768, -32768], [1, 0], [0, 1], [-1, 0], [32767, 32766]]
    for ca in (0, 8, 9, 10):
        out.append(S('stereo%d' % ca, edge, 16000, 16, kinds=fx(2), stereo=ca, blocksize=192))
    out.append(S('stereo_mix', edge, 16000, 16, kinds=lambda k, c: (fx(2), lpc(8, 12), {'type': 'verbatim'})[(k + c) % 3],
                 stereo=lambda k: (10, 8, 9, 0)[k % 4], blocksize=192))
    for bits in (8, 12, 16, 20, 24):
        full = signal(600, ch=2, bits=bits, seed=bits, amp=0.9)
        full[:2] = [[(1 << (bits - 1)) - 1, -(1 << (bits - 1))], [-(1 << (bits - 1)), (1 << (bits - 1)) - 1]]
        out.append(S('bits%d' % bits, full[:, 0], 16000, bits, kinds=fx(2), blocksize=256))
        out.append(S('bits%d_st' % bits, full, 16000, bits, kinds=lpc(8, 12), stereo=10, blocksize=256))
        out.append(S('bits%d_si' % bits, full, 16000, bits, kinds=fx(1), stereo=8, blocksize=256, header_from_streaminfo=True))
    out.append(S('block4096', signal(4097, seed=8), 48000, 16, kinds=lpc(8, 12, porder=4), blocksize=4096))      # a last block of 1 sample
    out.append(S('block4096_exact', signal(4096, seed=9), 48000, 16, kinds=fx(2, porder=12), blocksize=4096))    # one frame, the largest partition order it allows
    out.append(S('last1', signal(2 * 192 + 1, ch=2, seed=10), 16000, 16, kinds=fx(2), stereo=10, blocksize=192))
    for sr in (7000, 12345, 88210):                                                  # sample-rate codes 12, 13, 14
        out.append(S('sr%d' % sr, signal(400, seed=sr % 97), sr, 16, kinds=fx(2), blocksize=192))
    out.append(S('id3', signal(500, seed=11), 16000, 16, kinds=fx(2), blocksize=192, id3=300))
    out.append(S('meta', signal(500, seed=12), 16000, 16, kinds=fx(2), blocksize=192, extra_blocks=((4, b'x' * 77), (1, bytes(4100)))))
    out.append(S('number', signal(66 * 64, seed=13), 16000, 16, kinds=fx(1), blocksize=64, first_frame_number=100))   # 66 frames; 2-byte numbers
    out.append(S('number_big', signal(400, seed=14), 16000, 16, kinds=fx(2), blocksize=192, first_frame_number=(1 << 31) - 2))
    out.append(S('nomd5', signal(500, seed=15), 16000, 16, kinds=fx(2), blocksize=192, with_md5=False))
    out.append(S('nomd5_st', signal(500, ch=2, bits=24, seed=16), 16000, 24, kinds=lpc(8, 12), stereo=9, blocksize=192, with_md5=False))
    return tuple(out)


# ---- the shared decoder compiled as host code (tools/flac_frame_fuzz.cpp as a shared object, no sanitizer) -------------------------
class Info(ctypes.Structure):
    _fields_ = [('region_off', ctypes.c_int64), ('region_bytes', ctypes.c_int64), ('n_samples', ctypes.c_int64),
                ('n_frames', ctypes.c_int32), ('block_size', ctypes.c_int32), ('bits', ctypes.c_int32), ('channels', ctypes.c_int32),
                ('md5_set', ctypes.c_int32), ('eligible', ctypes.c_int32), ('md5', ctypes.c_uint8 * 16)]


ROW = np.dtype([('offset', '<i4'), ('first_sample', '<i4'), ('block_size', '<i4'), ('clip', '<i4')])


def build_host_decoder(tmp_dir):
    so = os.path.join(str(tmp_dir), 'libflac_frame_host.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', so, os.path.join(ROOT, 'tools', 'flac_frame_fuzz.cpp')])
    L = ctypes.CDLL(so)
    p8 = ctypes.c_char_p
    L.nqff_plan.argtypes = [p8, ctypes.c_size_t, ctypes.POINTER(Info)]
    L.nqff_index.argtypes = [p8, ctypes.c_size_t, ctypes.POINTER(Info), ctypes.c_void_p]
    L.nqff_decode.argtypes = [p8, ctypes.c_size_t, ctypes.POINTER(Info), ctypes.c_void_p, ctypes.c_void_p]
    L.nqff_compare.argtypes = [p8, ctypes.c_size_t]
    return L


def host_decode(L, data, mutate_rows=None):
    """File bytes through the shared decoder as the device path drives it -> (status, samples [n, ch] or None, rows or None).
    status: 'host' (not eligible / not indexable: the host path), 0 (accepted) or the kernel's status bits."""
    info = Info()
    if L.nqff_plan(data, len(data), ctypes.byref(info)) != 0 or not info.eligible:
        return 'host', None, None
    rows = np.zeros(info.n_frames, dtype=ROW)
    if L.nqff_index(data, len(data), ctypes.byref(info), rows.ctypes.data) != 0:
        return 'host', None, None
    if mutate_rows is not None:
        mutate_rows(rows)
    out = np.full((info.n_samples, info.channels), 0x55555555, dtype=np.int32)
    rc = L.nqff_decode(data, len(data), ctypes.byref(info), rows.ctypes.data, out.ctypes.data)
    return rc, out, rows


# ---- the six fixed mutations of the refusal tests: (name, stream name, mutate(bytearray of the file, Stream)) ------------------------
def _residual_bit(d, s):
    d[s.first_frame + s.sizes[0] + s.sizes[1] // 2] ^= 0x10          # the middle of the second frame: Rice-coded residuals


def _rice_parameter_bit(d, s):
    # frame 0 of 'p0': header (4 + 1 number + 1 CRC-8), subframe header 8 bits, two 16-bit warm-up samples, method 2 bits, partition
    # order 4 bits, then the 4-bit Rice parameter: byte 5 behind the header is [method 2][order 4][parameter's top 2 bits]
    d[s.first_frame + 6 + 5] ^= 0x01


def _warmup_bit(d, s):
    d[s.first_frame + 6 + 2] ^= 0x01                                  # the first 16-bit warm-up sample's low byte


def _crc16_byte(d, s):
    d[s.first_frame + s.sizes[0] - 1] ^= 0xFF


def _md5_byte(d, s):
    d[8 + 18 + 5] ^= 0x01                                             # "fLaC" + block header + 18 bytes of STREAMINFO fields


MUTATIONS = (('residual', 'lpc8_12', _residual_bit), ('rice', 'p0', _rice_parameter_bit), ('warmup', 'p0', _warmup_bit),
             ('crc16', 'stereo10', _crc16_byte), ('md5', 'bits24_st', _md5_byte))


def shift_second_row(rows):
    """The sixth mutation: the table says the second frame starts one byte late (the first frame then ends one byte early for it)."""
    rows['offset'][1] += 1


def by_name(name):
    return next(s for s in streams() if s.name == name)
