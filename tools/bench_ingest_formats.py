"""File-fed predict rate per input format: nisqaModel(predict_dir, bs 64).predict() over a directory of hard links to 64 ten-second
files, as bench.py's side.predict_dir_bs64 runs it, for mono PCM16 (the control), stereo PCM16, mono / stereo PCM24, mono float32 and
mu-law at 8 kHz, and for FLAC streams (flac16, flac16x2, flac24: written by tests/flac_enc.py, a few seconds per file, so only four
distinct files each; linked under *.wav names because predict_dir lists *.wav -- the ingest goes by the file's magic).  Per leg: clips/s, the bytes one clip puts on the host link, and the fraction of what the link alone carries
(bench.link_only_probe: the loop's own transport with no loop around it).

    python tools/bench_ingest_formats.py [--clips 8192] [--runs 3] [--formats pcm16,pcm24x2] [--host-decode] [--host-flac]

--host-decode sets NISQA_HOST_DECODE=1: the staging thread decodes what is not mono PCM16 (what every commit before the device
decoder did; use a small --clips, it is a Python thread decoding ten-second clips one at a time).  --host-flac sets NISQA_HOST_FLAC=1:
the reader threads decode FLAC (the A/B of nisqa_flac_decode; --alternate N runs device and host N times each, in turn, in one
process).  Not a test: DESIGN.md 6.3."""
import argparse
import contextlib
import io
import json
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                            # noqa: E402  (link_only_probe, model_weights)
from nisqa_amd import synth                              # noqa: E402

SECONDS = 10.0
# name -> (format tag, channels, container bytes, bits, sample rate)
FORMATS = {'pcm16': (1, 1, 2, 16, 48000), 'pcm16x2': (1, 2, 2, 16, 48000), 'pcm24': (1, 1, 3, 24, 48000), 'pcm24x2': (1, 2, 3, 24, 48000),
           'f32': (3, 1, 4, 32, 48000), 'mulaw8k': (7, 1, 1, 8, 8000),
           'flac16': ('flac', 1, 2, 16, 48000), 'flac16x2': ('flac', 2, 2, 16, 48000), 'flac24': ('flac', 1, 3, 24, 48000)}


def _mulaw(pcm16):
    """G.711 mu-law codes of int16 samples (ITU-T G.711, the encoder side of wavio._g711_tables)."""
    x = pcm16.astype(np.int32)
    sign = np.where(x < 0, 0x80, 0)
    mag = np.minimum(np.abs(x), 32635) + 0x84
    e = np.floor(np.log2(mag)).astype(np.int32) - 7
    m = (mag >> (e + 3)) & 0x0F
    return (~(sign | (e << 4) | m) & 0xFF).astype(np.uint8)


def write_file(path, seed, fmt):
    tag, ch, cont, bits, sr = FORMATS[fmt]
    chans = [synth.synth_pcm16(seed + 1000 * c, SECONDS, sr=sr) for c in range(ch)]
    x = np.stack(chans, 1)                                  # int16 [n, ch]
    if tag == 'flac':                                       # fixed block size 4096, LPC 8 / 12: what a stock encoder writes
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import flac_enc
        v = x.astype(np.int64) if bits == 16 else (x.astype(np.int64) << 8) | ((x.astype(np.int64) * 37) & 0xFF)
        data = flac_enc.encode(v[:, 0] if ch == 1 else v, sr, bits, blocksize=4096, stereo=10,
                               kinds={'type': 'lpc', 'order': 8, 'precision': 12, 'porder': 4})
        with open(path, 'wb') as f:
            f.write(data)
        return len(data)
    if tag == 7:
        data = _mulaw(x).tobytes()
    elif tag == 3:
        data = (x.astype(np.float32) / np.float32(32768.0)).astype('<f4').tobytes()
    elif cont == 2:
        data = x.astype('<i2').tobytes()
    else:                                                   # 24-bit: the 16-bit sample and a low byte of its own
        v = (x.astype(np.int32) << 8) | ((x.astype(np.int32) * 37) & 0xFF)
        data = v.astype('<i4').view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    fmt_chunk = struct.pack('<HHIIHH', tag, ch, sr, sr * ch * cont, ch * cont, bits)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt_chunk + b'data' + struct.pack('<I', len(data)) + data
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', len(body)) + body)
    return len(data)


def run_leg(fmt, clips, runs, dev, tmp_dir, bs=64, distinct=64, warm=4):
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.NISQA_model import nisqaModel
    margs, sd, _ = bench.model_weights()
    d = os.path.join(tmp_dir or tempfile.gettempdir(), 'nisqa_bench_formats_' + fmt)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.join(d, 'dir'))
    os.makedirs(os.path.join(d, 'warm'))
    if FORMATS[fmt][0] == 'flac':
        distinct = min(distinct, 4)
    nbytes = [write_file(os.path.join(d, 'c%03d.wav' % i), 3000 + i, fmt) for i in range(distinct)]
    for sub, n in (('dir', clips), ('warm', warm * bs)):
        for i in range(n):
            os.link(os.path.join(d, 'c%03d.wav' % (i % distinct)), os.path.join(d, sub, 'f%06d.wav' % i))
    ck = dict(margs)
    ck.update({'pretrained_model': False, 'tr_bs_val': bs, 'tr_num_workers': 0})
    torch.save({'args': ck, 'model_state_dict': sd}, os.path.join(d, 'model.tar'))

    def args_for(sub):
        return {'mode': 'predict_dir', 'pretrained_model': os.path.join(d, 'model.tar'), 'deg': None, 'data_dir': os.path.join(d, sub),
                'output_dir': None, 'csv_file': None, 'csv_deg': None, 'num_workers': 0, 'bs': bs, 'ms_channel': None, 'tr_bs_val': bs,
                'tr_num_workers': 0}
    quiet = io.StringIO()
    rates = []
    try:
        with contextlib.redirect_stdout(quiet):
            nisqaModel(args_for('warm')).predict()
        for _ in range(runs):
            with contextlib.redirect_stdout(quiet):
                m = nisqaModel(args_for('dir'))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(quiet):
                df = m.predict()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(df) == clips and np.isfinite(df['mos_pred'].to_numpy()).all()
            rates.append(clips / dt)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return rates, float(np.mean(nbytes)), dict(NL.LOOP_STATS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=8192)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--formats', default=','.join(FORMATS))
    ap.add_argument('--host-decode', action='store_true')
    ap.add_argument('--host-flac', action='store_true')
    ap.add_argument('--tmp-dir', default=None)
    a = ap.parse_args()
    if a.host_decode:
        os.environ['NISQA_HOST_DECODE'] = '1'
    else:
        os.environ.pop('NISQA_HOST_DECODE', None)
    if a.host_flac:
        os.environ['NISQA_HOST_FLAC'] = '1'
    else:
        os.environ.pop('NISQA_HOST_FLAC', None)
    dev = torch.device('cuda', 0)
    link = bench.link_only_probe(dev)
    for fmt in a.formats.split(','):
        rates, per_clip, loop = run_leg(fmt, a.clips, a.runs, dev, a.tmp_dir)
        is_flac = FORMATS[fmt][0] == 'flac'
        host_decoded = (a.host_decode and fmt != 'pcm16') or (is_flac and a.host_flac and fmt != 'flac16')
        if is_flac and (a.host_flac or a.host_decode):      # host-decoded mono 16-bit FLAC crosses as int16
            per_clip = FORMATS[fmt][4] * SECONDS * 2
        link_bytes = FORMATS[fmt][4] * SECONDS * 4 if host_decoded else per_clip         # a host-decoded clip crosses as float32
        best = max(rates)
        print(json.dumps({'format': fmt, 'decode': 'host' if a.host_decode or (is_flac and a.host_flac) else 'device', 'clips': a.clips,
                          'clips_per_s': [round(r, 1) for r in rates], 'link_bytes_per_clip': int(link_bytes),
                          'link_only_GBps': round(link, 2), 'link_only_clips_per_s': round(link * 1e9 / link_bytes, 1),
                          'frac_of_link_only': round(best * link_bytes / (link * 1e9), 4),
                          'loop_host_s': {k: round(v, 3) for k, v in loop.items() if isinstance(v, float)}}), flush=True)


if __name__ == '__main__':
    main()
