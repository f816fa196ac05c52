"""CPU side of the mel width tests (tests/test_gpu_mel_width.py, tests/test_mel_width_host.py): the probe clips, the
launcher's frames-per-wave rule restated, two mel pipelines from the same samples (float64 / float32) and the judge.

What is measured.  The spectrogram is ``power=1.0``: the bank sums MAGNITUDES, all positive, so nothing cancels and an fp32
evaluation of band m of frame t can be off by about eps32 * W_m * ||frame_t * window||_2 (W_m = sum_k fb[m, k]: an FFT bin's
rounding error scales with the frame's energy, not with the bin's own size).  The dB encoding adds eps32 * |dB| in dB, i.e.
M * |dB| * ln10 / 20 in amplitude.  The error of element (m, t) is therefore

    e = |M - max(M64, amin)| / s,    s = eps32 * (W_m * ||frame_t * window||_2 + max(M64, amin) * |dB64| * ln10 / 20)

with M the amplitude decoded from the float32 dB value.  ``floor`` is max e of a float32 CPU pipeline (numpy's complex64 FFT),
and a kernel is as wide as fp32 if its e stays within FACTOR * floor.
"""
import numpy as np

from nisqa_amd import synth
from oracle import mel as omel

N_FFT, N_MELS, AMIN = 4096, 48, 1e-4
EPS32 = float(np.finfo(np.float32).eps)
# worst e_gpu.max() / floor measured on an MI355X over the five front ends (test_gpu_mel_width.py: 1.42, at 192 kHz) x 1.5 = 2.13,
# rounded up to one digit; the margin is for compiler updates, the kernel itself is deterministic
FACTOR = 3.0


def geometry(sr):
    return int(sr * 0.01), int(sr * 0.02)                          # hop, win (NISQA_lib.py:2308-2309)


# ---- the launcher's rule (csrc/mel.hip, mel_db_launch) ------------------------------------------------------------------------
def launch_shape(total_frames, win):
    """-> (rounds, frames_per_wave, waves_per_workgroup) for a batch of ``total_frames`` frames."""
    nq = 1 if win <= 1024 else (2 if win <= 2048 else 4)
    resident = 256 * {1: 12, 2: 8, 4: 4}[nq]
    rounds = -(-total_frames // (resident * 32))
    fpw = min(32, max(4, -(-total_frames // (resident * rounds))))
    return rounds, fpw, (12 if nq == 1 else 4)


# ---- probe clips --------------------------------------------------------------------------------------------------------------
def _noise(rng, n, amp=32767):
    return rng.integers(-amp, amp + 1, n).astype(np.int16)


def probes(sr, reduced=False):
    """Ordered list of groups; a group is a list of (name, int16 clip) that stays together and in order in every batch (the
    quiet clip sits between two full-scale ones).  reduced: the set for the front ends other than the first."""
    hop, _ = geometry(sr)
    n0 = 14 * hop                                                   # the shortest allowed clip: 15 frames
    rng = np.random.default_rng(20260 + sr)
    imp_last = np.zeros(n0 + 7, np.int16)
    imp_last[-1] = 32767
    quiet = [('loud_a', _noise(rng, n0 + 31)), ('quiet', _noise(rng, n0 + 2 * hop + 1, 3)), ('loud_b', _noise(rng, n0 + 5))]
    if reduced:
        return [[('shortest', _noise(rng, n0))], [('odd', _noise(rng, n0 + 1))], [('zeros', np.zeros(n0 + 3, np.int16))],
                [('impulse_last', imp_last)], quiet, [('synth', synth.synth_pcm16(77, 1.3, sr=sr))]]
    imp_first = np.zeros(n0 + 7, np.int16)
    imp_first[0] = 32767
    n_s = n0 + 3 * hop
    sine = np.round(32767.0 * np.sin(2.0 * np.pi * 300.0 * np.arange(n_s) / N_FFT)).astype(np.int16)   # 300 sr / 4096 Hz: a bin centre
    nyq = np.where(np.arange(n_s) % 2 == 0, 32767, -32767).astype(np.int16)
    n_f = 100 * hop                                                 # 1 s whose level falls by 90 dB: the top_db floor cuts
    fall = np.round(rng.uniform(-32767.0, 32767.0, n_f) * 10.0 ** (-90.0 / 20.0 * np.arange(n_f) / n_f)).astype(np.int16)
    return [[('shortest', _noise(rng, n0))], [('hop_minus_1', _noise(rng, n0 + hop - 1))], [('hop', _noise(rng, n0 + hop))],
            [('odd', _noise(rng, n0 + 1))], [('zeros', np.zeros(n0 + 3, np.int16))],
            [('const_min', np.full(n0 + 9, -32768, np.int16))], [('impulse_first', imp_first)], [('impulse_last', imp_last)],
            [('sine', sine)], [('nyquist', nyq)], quiet, [('synth', synth.synth_pcm16(77, 1.3, sr=sr))], [('fall', fall)]]


def flat(groups):
    return [c for g in groups for c in g]


# ---- the two pipelines --------------------------------------------------------------------------------------------------------
def windowed_frames(x16, sr, dtype, pad_mode='reflect', window_shift=0, frame_dtype=None):
    """int16 clip -> frames * window, [n_fft, T] in ``dtype`` (librosa.stft's framing: centre-padded window, reflect-padded
    signal, T = 1 + len // hop).  pad_mode / window_shift / frame_dtype (the product rounded to that type) build the
    deliberately wrong pipelines of the host test."""
    hop, win = geometry(sr)
    y = x16.astype(dtype) / dtype(32768.0)
    w = np.zeros(N_FFT, dtype)
    lpad = (N_FFT - win) // 2 + window_shift
    w[lpad:lpad + win] = omel.hann_periodic(win).astype(dtype)
    ypad = np.pad(y, N_FFT // 2, mode=pad_mode)
    T = 1 + len(x16) // hop
    idx = np.arange(N_FFT)[:, None] + hop * np.arange(T)[None, :]
    fr = ypad[idx] * w[:, None]
    assert fr.dtype == dtype
    if frame_dtype is not None:
        fr = fr.astype(frame_dtype).astype(dtype)
    return fr


def bank(sr, fmax, shift=0):
    fb = omel.mel_filterbank(sr, N_FFT, N_MELS, 0.0, float(fmax))
    return np.roll(fb, shift, axis=1) if shift else fb


def mel_amplitudes(x16, sr, fmax, dtype, bank_shift=0, **wrong):
    """-> (M [48, T] mel amplitudes, every step in ``dtype``; ||frame_t * window||_2 [T] in float64)."""
    fr = windowed_frames(x16, sr, dtype, **wrong)
    X = np.fft.rfft(fr, axis=0)
    assert X.dtype == (np.complex64 if dtype == np.float32 else np.complex128), X.dtype
    S = np.abs(X)
    M = np.dot(bank(sr, fmax, bank_shift).astype(dtype), S)
    assert M.dtype == dtype
    return M, np.sqrt((fr.astype(np.float64) ** 2).sum(0))


def encode_db(M):
    """The float32 dB value of an amplitude (amplitude_to_db with ref = 1, amin = 1e-4, before the top_db floor)."""
    M = np.asarray(M, np.float32)
    return (np.float32(20.0) * np.log10(np.maximum(np.float32(AMIN), M))).astype(np.float32)


def decode_db(db):
    return 10.0 ** (np.asarray(db).astype(np.float64) / 20.0)


def element_error(db, M64, norms, sr, fmax):
    """db [48, T] float32 (a kernel's or a pipeline's rows), M64 [48, T], norms [T] -> (e [48, T], judged [48, T] bool)."""
    W = bank(sr, fmax).astype(np.float64).sum(1)
    ref = np.maximum(M64, AMIN)
    s = EPS32 * (W[:, None] * norms[None, :] + ref * np.abs(20.0 * np.log10(ref)) * np.log(10.0) / 20.0)
    ok = s > 0
    return np.where(ok, np.abs(decode_db(db) - ref) / np.where(ok, s, 1.0), 0.0), ok


class Yardstick(object):
    """M64, the frame norms and the float32 pipeline's error for every clip of ``clips`` at one front end."""

    def __init__(self, clips, sr, fmax):
        self.sr, self.fmax, self.names = sr, fmax, [n for n, _ in clips]
        self.M64, self.norms, self.e32 = {}, {}, {}
        for name, x in clips:
            M64, nrm = mel_amplitudes(x, sr, fmax, np.float64)
            M32, _ = mel_amplitudes(x, sr, fmax, np.float32)
            self.M64[name], self.norms[name] = M64, nrm
            self.e32[name] = float(self.error(name, encode_db(M32)).max())
        self.floor = max(self.e32.values())

    def error(self, name, db):
        return element_error(db, self.M64[name], self.norms[name], self.sr, self.fmax)[0]

    def judge(self, label, rows, factor=None):
        """rows: name -> [48, T] float32 dB.  Prints one line; with ``factor`` asserts e.max() <= factor * floor per clip.
        -> name -> e.max() / floor."""
        ratio = {n: float(self.error(n, r).max()) / self.floor for n, r in rows.items()}
        worst = max(ratio, key=ratio.get)
        print('%-34s floor %.3g (%s) | worst x%.2f (%s)%s' % (
            label, self.floor, max(self.e32, key=self.e32.get), ratio[worst], worst,
            '' if factor is None else ' | bound x%g' % factor))
        if factor is not None:
            bad = {n: r for n, r in ratio.items() if not r <= factor}
            assert not bad, (label, bad, 'floor', self.floor)
        return ratio
