#!/usr/bin/env python3
"""Seconds per training epoch, file-fed against resident spectrograms (tr_ds_to_memory), on a synthetic corpus in three forms:
ten-second mono PCM16 WAV files, the same clips as FLAC streams, and NISQA_DE pairs.  The two feeds alternate, three
runs each after one discarded warm-up run; an epoch is the training pass plus the validation pass, as nisqaModel.train() runs them.
Also measured once: one nisqa_mel_gather batch against torch.cat of the same slices and against the byte roofline.

The FLAC streams are written here with VERBATIM subframes (16-bit samples as they are, every frame with its CRC-8 / CRC-16 and the
stream with its MD5): a vectorised writer that makes a corpus in seconds.  A real encoder's Rice-coded residuals cost the decoder
more, so the file-fed FLAC figure is a lower bound.

    python tools/bench_train_memory.py --out profiles/r12_train_memory.json
"""
import argparse
import contextlib
import hashlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nisqa_amd import synth  # noqa: E402

DE_ARGS = dict(synth.MOS_ARGS, model='NISQA_DE', name='bench_de', double_ended=True, td_2='self_att', td_2_sa_d_model=64,
               td_2_sa_nhead=1, td_2_sa_pos_enc=False, td_2_sa_num_layers=2, td_2_sa_h=64, td_2_sa_dropout=0.1, de_align='cosine',
               de_align_apply='hard', de_fuse='x/y/-', de_fuse_dim=None)


def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    t = np.zeros(256, dtype=np.uint32)
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t[b] = c
    return t


_CRC8, _CRC16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)


def _crc_rows(rows, table, width):
    """CRC of every row of a uint8 matrix (MSB-first, zero start), all rows advanced together byte by byte."""
    c = np.zeros(rows.shape[0], dtype=np.uint32)
    mask = (1 << width) - 1
    for j in range(rows.shape[1]):
        c = ((c << 8) & mask) ^ table[((c >> (width - 8)) ^ rows[:, j]) & 0xFF]
    return c


def flac_verbatim(pcm, sr, blocksize=4096):
    """int16 mono samples -> a fixed-block-size FLAC stream of VERBATIM subframes (whole blocks vectorised, the short last block
    on its own)."""
    assert pcm.dtype == np.int16 and pcm.ndim == 1 and sr in (16000, 48000) and len(pcm) >= blocksize
    n = len(pcm)
    frames = []
    for bs, first, count in ((blocksize, 0, n // blocksize), (n % blocksize, n // blocksize, 1 if n % blocksize else 0)):
        if not count:
            continue
        k = first + np.arange(count)
        assert int(k.max()) < 2048                                        # frame numbers in one or two UTF-8 bytes
        # sync + fixed block size | block size code 7 (16-bit size - 1 follows), rate code | mono, 16 bit | frame number | size - 1 | CRC-8
        num = [np.where(k < 128, k, 0xC0 | (k >> 6)).astype(np.uint8), (0x80 | (k & 0x3F)).astype(np.uint8)]
        for two in (False, True):
            sel = (k >= 128) == two
            if not sel.any():
                continue
            cols = [np.full(sel.sum(), v, np.uint8) for v in (0xFF, 0xF8, 0x70 | {16000: 5, 48000: 10}[sr], 0x08)]
            cols += [num[0][sel]] + ([num[1][sel]] if two else [])
            cols += [np.full(sel.sum(), (bs - 1) >> 8, np.uint8), np.full(sel.sum(), (bs - 1) & 0xFF, np.uint8)]
            head = np.stack(cols, axis=1)
            head = np.concatenate([head, _crc_rows(head, _CRC8, 8).astype(np.uint8)[:, None]], axis=1)
            blocks = pcm[first * blocksize:][:count * bs].reshape(count, bs)[sel]
            body = np.concatenate([head, np.full((sel.sum(), 1), 0x02, np.uint8),                 # subframe header: verbatim, no wasted bits
                                   blocks.astype('>i2').view(np.uint8).reshape(sel.sum(), 2 * bs)], axis=1)
            crc = _crc_rows(body, _CRC16, 16)
            body = np.concatenate([body, (crc >> 8).astype(np.uint8)[:, None], (crc & 0xFF).astype(np.uint8)[:, None]], axis=1)
            frames.append((k[sel], body))
    order = sorted(((int(kk), row.tobytes()) for ks, body in frames for kk, row in zip(ks, body)))
    sizes = [len(b) for _, b in order]
    # STREAMINFO: block sizes 16 + 16 bits, frame sizes 24 + 24, rate 20, channels - 1 in 3, bits - 1 in 5, total samples 36
    si = (blocksize << 128) | (blocksize << 112) | (min(sizes) << 88) | (max(sizes) << 64) | (sr << 44) | (0 << 41) | (15 << 36) | n
    streaminfo = si.to_bytes(18, 'big') + hashlib.md5(pcm.astype('<i2').tobytes()).digest()
    return b'fLaC' + bytes([0x80]) + (34).to_bytes(3, 'big') + streaminfo + b''.join(b for _, b in order)


def write_corpus(d, form, n_train, n_val, seconds, distinct=16):
    """files.csv + audio under d: ``distinct`` synthetic clips of ``seconds`` written under n_train + n_val names (pairs for 'de')."""
    import pandas as pd
    rng = np.random.default_rng(5)
    clips = [synth.synth_pcm16(900 + i, seconds) for i in range(distinct)]
    blobs = [flac_verbatim(c, 48000) for c in clips] if form == 'flac' else None
    ext = '.flac' if form == 'flac' else '.wav'
    rows = []
    for k in range(n_train + n_val):
        row = {'db': 'TRAIN' if k < n_train else 'VAL', 'mos': float(rng.uniform(1, 5))}
        for col, shift in (('filepath_deg', 0), ('filepath_ref', 7))[:2 if form == 'de' else 1]:
            name = '%s_%05d%s' % (col[-3:], k, ext)
            j = (k + shift) % distinct
            if blobs is not None:
                with open(os.path.join(d, name), 'wb') as f:
                    f.write(blobs[j])
            else:
                synth.write_wav(os.path.join(d, name), clips[j], 48000)
            row[col] = name
        rows.append(row)
    pd.DataFrame(rows).to_csv(os.path.join(d, 'files.csv'), index=False)


def run_once(form, d, out_dir, to_memory, bs, epochs):
    """One nisqaModel.train() -> (seconds per epoch, fill seconds, arena bytes)"""
    import torch
    from nisqa_amd.NISQA_model import nisqaModel
    args = dict(DE_ARGS if form == 'de' else synth.MOS_ARGS)
    args.update({'name': 'bench_' + form, 'mode': 'main', 'data_dir': d, 'output_dir': out_dir, 'pretrained_model': False,
                 'csv_file': 'files.csv', 'csv_con': None, 'csv_deg': 'filepath_deg', 'csv_ref': 'filepath_ref' if form == 'de' else None,
                 'csv_mos_train': 'mos', 'csv_mos_val': 'mos', 'csv_db_train': ['TRAIN'], 'csv_db_val': ['VAL'], 'tr_epochs': epochs,
                 'tr_early_stop': 100, 'tr_bs': bs, 'tr_bs_val': bs, 'tr_lr': 1e-3, 'tr_lr_patience': 100, 'tr_num_workers': 0,
                 'tr_parallel': False, 'tr_ds_to_memory': to_memory, 'tr_ds_to_memory_workers': 0, 'tr_device': None,
                 'tr_checkpoint': None, 'tr_verbose': 0, 'tr_bias_mapping': None, 'tr_bias_min_r': None, 'tr_bias_anchor_db': None,
                 'ms_channel': None})
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        nm = nisqaModel(args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nm.load_to_memory()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        nm.train()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
    stores = [s for ds in (nm.ds_train, nm.ds_val) for s in (ds.store, ds.ref_store) if s is not None]
    return (t2 - t1) / epochs, (t1 - t0) if to_memory else 0.0, sum(s.nbytes for s in stores)


def gather_bench(clips=32, frames=1001, reps=50):
    """One batch of ``clips`` ten-second spectrograms out of a store of 4 x as many: nisqa_mel_gather (with its table upload) against
    torch.cat of the same slices, microseconds per batch by HIP events, and the time the bytes alone take at 6.3 TB/s."""
    import torch
    from nisqa_amd import lib, melstore
    st = melstore.MelStore(None, [None] * (4 * clips))
    st.device, st.lib = torch.device('cuda:0'), lib.load()
    st.frames = np.full(4 * clips, frames, np.int64)
    st.n_wins = np.full(4 * clips, 247, np.int32)
    st.clip_row = np.concatenate(([0], np.cumsum(st.frames))).astype(np.int64)
    st.arena = torch.randn((int(st.clip_row[-1]), 48), device=st.device)
    st.floor = torch.randn(4 * clips, device=st.device)
    st.clip_row_dev = torch.from_numpy(st.clip_row).to(st.device)
    st.filled = True
    ids = np.random.default_rng(2).permutation(4 * clips)[:clips]

    def timed(fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps
    t_gather = timed(lambda: st.batch(ids))
    t_cat = timed(lambda: torch.cat([st.arena[st.clip_row[i]:st.clip_row[i + 1]] for i in ids.tolist()]))
    mel, _, _, _ = st.batch(ids)
    assert torch.equal(mel, torch.cat([st.arena[st.clip_row[i]:st.clip_row[i + 1]] for i in ids.tolist()]))
    nbytes = 2 * clips * frames * 192
    return {'clips': clips, 'frames': frames, 'bytes_moved': nbytes, 'gather_us': round(t_gather, 2), 'torch_cat_us': round(t_cat, 2),
            'roofline_us_at_6.3TBps': round(nbytes / 6.3e12 * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train', type=int, default=256)
    ap.add_argument('--val', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--forms', default='wav,flac,de')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    result = {'tool': 'bench_train_memory', 'train_clips': a.train, 'val_clips': a.val, 'seconds': a.seconds, 'tr_bs': a.bs,
              'epochs_per_run': a.epochs, 'runs': a.runs, 'forms': {}}
    result['gather'] = gather_bench()
    print(json.dumps({'gather': result['gather']}), flush=True)
    for form in a.forms.split(','):
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, 'corpus')
            os.makedirs(d)
            t0 = time.perf_counter()
            write_corpus(d, form, a.train, a.val, a.seconds)
            t_write = time.perf_counter() - t0
            run_once(form, d, os.path.join(tmp, 'warm'), False, a.bs, 1)                     # discarded: kernels loaded, page cache warm
            secs = {'file': [], 'resident': []}
            fills, arena = [], 0
            for r in range(a.runs):
                for feed in ('file', 'resident'):
                    s, fill, nbytes = run_once(form, d, os.path.join(tmp, '%s%d' % (feed, r)), feed == 'resident', a.bs, a.epochs)
                    secs[feed].append(s)
                    if feed == 'resident':
                        fills.append(fill)
                        arena = nbytes
            row = {'corpus_write_s': round(t_write, 2), 'file_s_per_epoch': [round(s, 4) for s in secs['file']],
                   'resident_s_per_epoch': [round(s, 4) for s in secs['resident']],
                   'file_median': round(statistics.median(secs['file']), 4), 'resident_median': round(statistics.median(secs['resident']), 4),
                   'fill_s': [round(f, 3) for f in fills], 'fill_median': round(statistics.median(fills), 3), 'arena_bytes': arena}
            result['forms'][form] = row
            print(json.dumps({form: row}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
