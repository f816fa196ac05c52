"""WAV cases of the device decoder's tests (nisqa_wav_decode): data chunks of every encoding the ingest accepts with values at the
edges of each number format, RIFF / RIFX files around them (written with struct), the nisqa_wav_clip table of a set of cases, and
the two summation orders of numpy's mean restated.  The expected samples are always ``wavio._decode``'s."""
import struct

import numpy as np

from nisqa_amd import lib, wavio

F32 = np.float32
PCM, FLOAT, ALAW, MULAW = 1, 3, 6, 7
# name -> (format tag, bits per sample of the header, container bytes)
ENCODINGS = {'u8': (PCM, 8, 1), 'pcm16': (PCM, 16, 2), 'pcm12': (PCM, 12, 2), 'pcm24': (PCM, 24, 3), 'pcm20': (PCM, 20, 3),
             'pcm32': (PCM, 32, 4), 'f32': (FLOAT, 32, 4), 'f64': (FLOAT, 64, 8), 'alaw': (ALAW, 8, 1), 'mulaw': (MULAW, 8, 1)}
CHANNELS = (1, 2, 3, 7, 8, 9, 32)
FRAMES = (1, 2, 63, 64, 65, 255, 256, 257, 4099)      # around the wave, the 256 lanes of a workgroup and its 1024-frame tile; 4099: five tiles


# ---- numpy's mean over the channels of one frame, restated (what the kernel does) --------------------------------------------
def mean_sequential(y):
    """y float32 [n, ch], ch < 8: ((c0 + c1) + c2) + ..., added to the reduction's identity +0.0 (a sum of -0.0 becomes +0.0), then one
    division."""
    s = y[:, 0].copy()
    for c in range(1, y.shape[1]):
        s = s + y[:, c]
    return (F32(0.0) + s) / F32(y.shape[1])


def mean_eight_accumulators(y):
    """y float32 [n, ch], 8 <= ch: eight running sums over the full blocks of eight channels, their pairwise tree, the remaining
    channels one by one, the identity +0.0 as above, then one division."""
    ch = y.shape[1]
    r = [y[:, j].copy() for j in range(8)]
    full = ch // 8
    for k in range(1, full):
        for j in range(8):
            r[j] = r[j] + y[:, 8 * k + j]
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for c in range(8 * full, ch):
        s = s + y[:, c]
    return (F32(0.0) + s) / F32(ch)


def to_mono(y):
    return mean_sequential(y) if y.shape[1] < 8 else mean_eight_accumulators(y)


# ---- data chunks -------------------------------------------------------------------------------------------------------------
def _with_edges(x, edges, on=True):
    """x [n, ch] with the first frames replaced by ``edges`` (each value in every channel of its frame: a mean of equal values
    cannot produce inf - inf), as far as n allows; not ``on``: x as it is (audio that has to stay finite)."""
    k = min(len(edges), x.shape[0]) if on else 0
    x[:k, :] = np.asarray(edges[:k], dtype=x.dtype)[:, None]
    return x


def payload(enc, n, ch, big_endian, rng, edges=True):
    """-> the bytes of a data chunk of n frames x ch channels in encoding ``enc`` (a key of ENCODINGS); ``edges``: with the values at
    the edges of the number format in its first frames."""
    E = '>' if big_endian else '<'
    if enc == 'u8':
        x = _with_edges(rng.integers(0, 256, (n, ch)).astype(np.uint8), [0, 255, 128, 127], edges)
        return x.tobytes()
    if enc in ('alaw', 'mulaw'):                              # every code, in order, from a random start
        return ((np.arange(n * ch) + int(rng.integers(0, 256))) % 256).astype(np.uint8).tobytes()
    if enc in ('pcm16', 'pcm12'):
        x = _with_edges(rng.integers(-32768, 32768, (n, ch)).astype(np.int16), [-32768, 32767, 0, -1], edges)
        if enc == 'pcm12':
            x &= np.int16(-16)                                # 12 bits, left-justified in the container
        return x.astype(E + 'i2').tobytes()
    if enc in ('pcm24', 'pcm20'):
        x = _with_edges(rng.integers(-(1 << 23), 1 << 23, (n, ch)).astype(np.int32), [-(1 << 23), (1 << 23) - 1, 0, -1], edges)
        if enc == 'pcm20':
            x &= np.int32(-16)
        b = x.astype('<i4').view(np.uint8).reshape(n, ch, 4)[..., :3]
        return (b[..., ::-1] if big_endian else b).tobytes()
    if enc == 'pcm32':                                        # (values past 2^24 round on their way to float32)
        x = _with_edges(rng.integers(-(1 << 31), 1 << 31, (n, ch)).astype(np.int32),
                        [-(1 << 31), (1 << 31) - 1, 0, -1, (1 << 24) + 1, (1 << 25) + 2, (1 << 25) + 6, -(1 << 24) - 3], edges)
        return x.astype(E + 'i4').tobytes()
    scale = rng.choice([1e-3, 1.0, 100.0], size=(n, ch))
    if enc == 'f32':
        x = (rng.standard_normal((n, ch)) * scale).astype(np.float32)
        x = _with_edges(x, [0.0, -0.0, 1e-40, -1e-42, 1.4e-45, -1.17549421e-38, 3.4e38, 1.0], edges)      # +-0, denormals, near the largest
        return x.astype(E + 'f4').tobytes()
    x = rng.standard_normal((n, ch)) * scale
    half = 1.0 + 2.0 ** -24                                   # halfway between two float32 neighbours: ties to even, down ...
    x = _with_edges(x, [1e39, -1e39, 1e-46, half, 1.0 + 3 * 2.0 ** -24, -half, 1e-40, 3e-45, 0.0, -0.0, 3.4028235677973366e38], edges)      # ... and up
    return x.astype(E + 'f8').tobytes()


class Case(object):
    """One clip: its data chunk, the header fields that describe it, and what wavio._decode makes of it."""

    def __init__(self, enc, n, ch, big_endian, channel, rng, edges=True):
        self.enc, self.n, self.ch, self.be, self.channel = enc, n, ch, big_endian, channel
        self.tag, self.bits, self.container = ENCODINGS[enc]
        self.data = payload(enc, n, ch, big_endian, rng, edges)
        assert len(self.data) == n * ch * self.container

    def header(self):
        h = wavio.Header()
        h.path, h.fd, h.tag, h.ch, h.sr, h.blk, h.bits, h.be = None, None, self.tag, self.ch, 16000, self.ch * self.container, self.bits, self.be
        h.data_off, h.n, h.ms_channel, h.fast, h.info = 0, self.n, (None if self.channel < 0 else self.channel), False, None
        return h

    def expected(self):
        y = wavio._decode(self.header(), self.data)
        if y.dtype == np.int16:
            y = y.astype(np.float32) / F32(32768.0)
        assert y.dtype == np.float32 and y.shape == (self.n,)
        return y

    def __repr__(self):
        return '%s%s ch=%d n=%d channel=%d' % (self.enc, '/be' if self.be else '', self.ch, self.n, self.channel)


def channel_modes(ch):
    """The ``channel`` values a case list covers for a channel count: the mean, the first and the last channel."""
    return (-1,) if ch == 1 else (-1, 0, ch - 1)


def cases_of(enc, rng, frames=FRAMES, channels=CHANNELS):
    return [Case(enc, n, ch, be, sel, rng) for be in (False, True) for ch in channels for sel in channel_modes(ch) for n in frames]


def pack(cases, gap=0):
    """-> (raw uint8 array: the data chunks on 16-byte boundaries with a 16-byte pad behind the last, the nisqa_wav_clip table with
    ``gap`` samples left free between and behind the clips, the number of output samples)."""
    t = np.zeros(len(cases), dtype=np.dtype(lib.WavClip))
    chunks, at, out_at = [], 0, 0
    for i, c in enumerate(cases):
        t[i] = (at, out_at, c.n, c.ch, c.container, c.tag | (lib.WAVENC_BIG_ENDIAN if c.be else 0), c.channel)
        size = (len(c.data) + 15) // 16 * 16
        chunks.append(np.frombuffer(c.data + bytes(size - len(c.data)), dtype=np.uint8))
        at += size
        out_at += c.n + gap
    return np.concatenate(chunks + [np.zeros(16, np.uint8)]), t, out_at


# ---- files -------------------------------------------------------------------------------------------------------------------
def wav_file_bytes(data, sr, ch, tag, bits, container, big_endian=False):
    """A RIFF (RIFX when big_endian: every header field big-endian too) WAVE file around the data chunk ``data``."""
    E = '>' if big_endian else '<'
    fmt = struct.pack(E + 'HHIIHH', tag, ch, sr, sr * ch * container, ch * container, bits)
    body = b'WAVE' + b'fmt ' + struct.pack(E + 'I', 16) + fmt + b'data' + struct.pack(E + 'I', len(data)) + data + bytes(len(data) & 1)
    return (b'RIFX' if big_endian else b'RIFF') + struct.pack(E + 'I', len(body)) + body


def write_case(path, case, sr):
    with open(path, 'wb') as f:
        f.write(wav_file_bytes(case.data, sr, case.ch, case.tag, case.bits, case.container, case.be))
    return path
