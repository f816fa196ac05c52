"""Synthetic corpora of the resident-spectrogram tests (tests/test_melstore_host.py, tests/test_gpu_melstore.py): short clips in
every form the file feed stages differently -- 16 kHz and 48 kHz mono PCM16, a float32 WAV, a stereo 24-bit WAV, a mono 16-bit FLAC
stream and a stereo FLAC stream."""
import numpy as np
import pandas as pd

import flac_enc
import wav_cases
from nisqa_amd import synth
from nisqa_amd.NISQA_lib import SpeechQualityDataset

# (name, rate, form); forms: 'i16' mono PCM16, 'f32' float32 WAV, 's24' stereo 24-bit WAV, 'flac' mono 16-bit FLAC, 'flac2' stereo FLAC
FILES = [('a0.wav', 16000, 'i16'), ('a1.wav', 48000, 'i16'), ('a2.wav', 48000, 'f32'), ('a3.wav', 16000, 'i16'),
         ('a4.wav', 48000, 's24'), ('a5.flac', 48000, 'flac'), ('a6.wav', 16000, 'i16'), ('a7.flac', 16000, 'flac2'),
         ('a8.wav', 48000, 'i16'), ('a9.wav', 48000, 'i16'), ('a10.wav', 16000, 'i16'), ('a11.wav', 48000, 'i16'),
         ('a12.wav', 16000, 'i16'), ('a13.wav', 48000, 'i16')]


def write_file(path, seed, seconds, sr, form):
    pcm = synth.synth_pcm16(seed, seconds, sr=sr)
    if form == 'i16':
        synth.write_wav(path, pcm, sr)
    elif form == 'f32':
        synth.write_wav(path, (pcm.astype(np.float32) / np.float32(32768.0)) * np.float32(0.7), sr)
    elif form == 's24':
        v = np.stack([pcm.astype(np.int32) * 256 + 37, np.roll(pcm, 5).astype(np.int32) * 256 - 11], axis=1)
        b = np.stack([(v >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.uint8)       # little-endian 3-byte samples
        with open(path, 'wb') as f:
            f.write(wav_cases.wav_file_bytes(b.tobytes(), sr, 2, 1, 24, 3))
    else:
        data = pcm if form == 'flac' else np.stack([pcm, np.roll(pcm, 7)], axis=1)
        with open(path, 'wb') as f:
            f.write(flac_enc.encode(data, sr, 16, blocksize=4096, stereo=10 if form == 'flac2' else 0,
                                    kinds={'type': 'fixed', 'order': 2, 'porder': 2}))


def write_corpus(d, files=FILES, seed=41, prefix=''):
    """Write ``files`` (0.3-1.6 s each) into directory ``d`` -> their names."""
    rng = np.random.default_rng(seed)
    names = []
    for k, (name, sr, form) in enumerate(files):
        write_file(str(d / (prefix + name)), seed * 100 + k, float(rng.uniform(0.3, 1.6)), sr, form)
        names.append(prefix + name)
    return names


def dataset(d, names, args, ref_names=None, **kw):
    """SpeechQualityDataset over ``names`` in ``d`` with the ms_* parameters of ``args`` (double-ended with ``ref_names``)."""
    df = pd.DataFrame({'deg': names, **{t: np.linspace(1.0, 5.0, len(names)) for t in ('mos', 'noi', 'dis', 'col', 'loud')}})
    if ref_names is not None:
        df['ref'] = ref_names
    p = dict(seg_length=args['ms_seg_length'], max_length=args['ms_max_segments'], seg_hop_length=args['ms_seg_hop_length'],
             ms_n_fft=args['ms_n_fft'], ms_hop_length=args['ms_hop_length'], ms_win_length=args['ms_win_length'],
             ms_n_mels=args['ms_n_mels'], ms_sr=args['ms_sr'], ms_fmax=args['ms_fmax'], ms_channel=args.get('ms_channel'),
             double_ended=ref_names is not None, filename_column_ref='ref' if ref_names is not None else None)
    p.update(kw)
    return SpeechQualityDataset(df, data_dir=str(d), filename_column='deg', mos_column='mos', **p)
