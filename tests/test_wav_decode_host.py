"""Host side of the device WAV decoder (nisqa_wav_decode): what ``Ingest(..., device_decode=True)`` stages -- raw rate groups of
verbatim data chunks with their nisqa_wav_clip table, float32 entries for what the kernel does not take --, numpy's mean orders as the
kernel restates them, the binding's struct, and the NISQA_HOST_DECODE switch.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import flac_enc
import wav_cases as wc
from nisqa_amd import ingest, lib, wavio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _ListDataset(object):
    ms_channel = None

    def __init__(self, paths, ms_channel=None):
        self.paths, self.ms_channel = paths, ms_channel

    def file_path(self, i):
        return self.paths[i]


def _stage_one(ds, idx, **kw):
    """One staged batch -> (groups, a copy of the slot's bytes)."""
    ing = ingest.Ingest(ds, [idx], pin=False, num_workers=2, **kw)
    try:
        staged = next(iter(ing))
        buf = ing.ring.buf[staged.slot].numpy().copy()
        ing.ring.release_after(staged.slot, None)
        return staged.groups, buf
    finally:
        ing.close()


def _forbid_host_decode(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('the host decoder ran')
    monkeypatch.setattr(wavio, '_decode', boom)
    monkeypatch.setattr(wavio, 'read_wav', boom)


def _data_chunk(path):
    h = wavio.probe(path)
    try:
        data = bytearray(h.n * h.blk)
        wavio.read_data_into(h, data)
        return h, bytes(data)
    finally:
        h.close()


def test_raw_staging_copies_data_chunks_verbatim_and_never_calls_the_host_decoder(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    spec = [('stereo16', 'pcm16', 2, False, 16000, 901), ('mono24', 'pcm24', 1, False, 16000, 333), ('rifx16', 'pcm16', 1, True, 16000, 77),
            ('f32st', 'f32', 2, False, 16000, 500), ('mulaw', 'mulaw', 1, False, 16000, 1001), ('mono16a', 'pcm16', 1, False, 16000, 640),
            ('mono16b', 'pcm16', 1, False, 8000, 410), ('mono16c', 'pcm16', 1, False, 8000, 95)]
    paths = [wc.write_case(str(tmp_path / (name + '.wav')), wc.Case(enc, n, ch, be, -1, rng), sr) for name, enc, ch, be, sr, n in spec]
    ds = _ListDataset(paths)
    idx = list(range(len(paths)))
    want_groups, want_buf = _stage_one(ds, idx)                              # the default Ingest: host decode
    assert [g.kind for g in want_groups] == ['f32', 'i16'] and all(g.clips is None for g in want_groups)
    chunks = [_data_chunk(p) for p in paths]
    _forbid_host_decode(monkeypatch)
    groups, buf = _stage_one(ds, idx, device_decode=True)
    assert [(g.ids, g.lengths, g.sr) for g in groups] == [(g.ids, g.lengths, g.sr) for g in want_groups]
    raw, i16 = groups
    assert raw.kind == 'raw' and not raw.is_i16 and raw.sr == 16000 and raw.lengths == [n for *_, sr, n in spec if sr == 16000]
    t = raw.clips
    assert t.dtype == ingest.WAV_CLIP and len(t) == 6 and raw.offset % 64 == 0
    assert (t['src_off'] % 16 == 0).all() and t['src_off'][0] == 0 and (np.diff(t['src_off']) > 0).all()
    assert t['dst_off'].tolist() == np.concatenate(([0], np.cumsum(raw.lengths[:-1]))).tolist()
    for row, k in zip(t, raw.ids):
        h, data = chunks[k]
        at = raw.offset + int(row['src_off'])
        assert bytes(buf[at:at + len(data)]) == data, paths[k]               # the data chunk, byte for byte
        assert at + len(data) <= raw.offset + raw.nbytes
        assert (row['n_frames'], row['channels'], row['container']) == (h.n, h.ch, h.blk // h.ch), paths[k]
        assert row['encoding'] == h.tag | (lib.WAVENC_BIG_ENDIAN if h.be else 0) and row['channel'] == -1
    assert raw.nbytes % 16 == 0 and raw.nbytes >= int(t['src_off'][-1]) + len(chunks[raw.ids[-1]][1])
    # the rate group of mono PCM16 files alone stays the int16 group it was: same bytes, same place in its slot
    w16 = want_groups[1]
    assert i16.kind == 'i16' and i16.is_i16 and i16.clips is None and i16.nbytes == w16.nbytes == 2 * (410 + 95)
    assert bytes(buf[i16.offset:i16.offset + i16.nbytes]) == bytes(want_buf[w16.offset:w16.offset + w16.nbytes])
    assert bytes(buf[i16.offset:i16.offset + i16.nbytes]) == chunks[6][1] + chunks[7][1]


def test_ms_channel_reaches_the_table_and_a_missing_channel_keeps_the_reference_error(tmp_path):
    rng = np.random.default_rng(4)
    paths = [wc.write_case(str(tmp_path / 'st.wav'), wc.Case('pcm24', 50, 2, False, -1, rng), 16000),
             wc.write_case(str(tmp_path / 'mono.wav'), wc.Case('pcm24', 60, 1, False, -1, rng), 16000)]
    (g,), _ = _stage_one(_ListDataset(paths, ms_channel=1), [0, 1], device_decode=True)
    assert g.kind == 'raw' and g.clips['channel'].tolist() == [1, 0] and g.clips['channels'].tolist() == [2, 1]
    with pytest.raises(ValueError, match='Could not load file .*st.wav'):   # a stereo file has no channel 2: the host decoder's error
        _stage_one(_ListDataset(paths, ms_channel=2), [0, 1], device_decode=True)


def test_files_the_kernel_does_not_take_are_float32_entries_of_the_raw_group(tmp_path):
    rng = np.random.default_rng(5)
    st = rng.integers(-20000, 20000, (700, 2)).astype(np.int16)
    mono = rng.integers(-20000, 20000, 450).astype(np.int16)
    paths = [str(tmp_path / n) for n in ('st.flac', 'wide.wav', 'mono.flac', 'st.wav')]
    with open(paths[0], 'wb') as f:
        f.write(flac_enc.encode(st, 16000, 16, stereo=10))
    wc.write_case(paths[1], wc.Case('pcm16', 300, 40, False, -1, rng), 16000)        # a mean over 40 channels
    with open(paths[2], 'wb') as f:
        f.write(flac_enc.encode(mono, 16000, 16))
    wc.write_case(paths[3], wc.Case('pcm16', 123, 2, False, -1, rng), 16000)
    (g,), buf = _stage_one(_ListDataset(paths), [0, 1, 2, 3], device_decode=True)
    t = g.clips
    assert g.kind == 'raw' and g.lengths == [700, 300, 450, 123] and (t['src_off'] % 16 == 0).all()
    for k in (0, 1):                                                           # mono little-endian float32, host-decoded
        assert (t[k]['channels'], t[k]['container'], t[k]['encoding'], t[k]['channel']) == (1, 4, lib.WAVENC_FLOAT, -1)
        h = wavio.probe(paths[k])
        want = wavio.decode_f32(h)
        h.close()
        at = g.offset + int(t[k]['src_off'])
        assert np.array_equal(buf[at:at + 4 * len(want)].view(np.float32), want) and len(want) == g.lengths[k]
    assert (t[2]['channels'], t[2]['container'], t[2]['encoding']) == (1, 2, lib.WAVENC_PCM)       # decoded into the slot as int16
    at = g.offset + int(t[2]['src_off'])
    assert np.array_equal(buf[at:at + 2 * 450].view(np.int16), mono)
    assert (t[3]['channels'], t[3]['container'], t[3]['encoding']) == (2, 2, lib.WAVENC_PCM)
    assert bytes(buf[g.offset + int(t[3]['src_off']):][:123 * 4]) == _data_chunk(paths[3])[1]


def test_byte_cap_is_charged_with_the_staged_widths():
    """LengthAware.cut_raw: a clip costs frames x its own staged width (block_align of a verbatim chunk, 4 of a host-decoded one)
    rounded up to its 16-byte boundary, and mono PCM16 clips come first within a rate."""
    rng = np.random.default_rng(6)
    n = 200
    frames = rng.integers(16000, 160000, n).astype(np.int64)
    srs = np.where(np.arange(n) % 3 == 0, 8000, 16000).astype(np.int64)
    widths = rng.choice([2, 2, 4, 6, 3, 1], n).astype(np.int64)
    fast = (widths == 2) & (rng.random(n) < 0.8)                       # (width 2 is also mono 12-bit or two-channel 8-bit)
    tok = lambda f, r: np.maximum(1, f // 1600)
    cap = 3 << 20
    pol = ingest.LengthAware(range(n), 1, tok, min_tokens=1 << 30, byte_cap=cap)
    cuts = pol.cut_raw(frames, srs, widths, fast)
    assert sorted(k for c in cuts for k in c) == list(range(n)) and len(cuts) > 4
    for c in cuts:
        size = pol.raw_bytes(frames, widths, c)
        assert size == sum((int(frames[k] * widths[k]) + 15) // 16 * 16 for k in c)
        assert size <= cap + cap // 2 or len(c) == 1
        assert len(set(srs[c].tolist())) == 1
    for sr in (8000, 16000):                                           # within a rate: every mono PCM16 clip before any other
        order = [k for c in cuts for k in c if srs[k] == sr]
        flags = fast[order].tolist()
        assert flags == sorted(flags, reverse=True)
    assert pol.cut_raw(frames[:0], srs[:0], widths[:0], fast[:0]) == []


def test_mean_orders_are_the_installed_numpys():
    """The two summation orders the kernel restates against np.mean(y.T, axis=0, dtype=float32) -- librosa.to_mono -- for every channel
    count it takes; a numpy that sums differently shows up here, not on the GPU."""
    rng = np.random.default_rng(7)
    for ch in range(2, 33):
        y = (rng.standard_normal((5000, ch)) * rng.choice([1e-3, 1.0, 100.0], size=(5000, ch))).astype(np.float32)
        y[:8] = np.float32(1e-40) * rng.integers(-9, 9, (8, ch)).astype(np.float32)          # denormal sums and quotients
        y[8:10] = np.float32(-0.0)                                         # a sum of -0.0: the reduction starts from +0.0
        y[10, 0] = np.float32(-0.0)
        want = np.mean(y.T, axis=0, dtype=np.float32)
        got = wc.to_mono(y)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), ch
    y = (rng.standard_normal((5000, 8))).astype(np.float32)
    assert not np.array_equal(wc.mean_sequential(y), np.mean(y.T, axis=0, dtype=np.float32))      # from eight channels on the order matters
    assert np.mean(np.full((2, 3), -0.0, np.float32), axis=0, dtype=np.float32).view(np.uint32).tolist() == [0, 0, 0]


def test_clip_struct_matches_the_header_and_the_entry_is_exported(tmp_path):
    assert ctypes.sizeof(lib.WavClip) == 40 and ingest.WAV_CLIP.itemsize == 40
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nisqa_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(nisqa_wav_clip));']
    for name, _ in lib.WavClip._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(nisqa_wav_clip, %s));' % (name, name))
    lines.append('  printf("enc %d %d %d %d %d\\n", NISQA_WAVENC_PCM, NISQA_WAVENC_FLOAT, NISQA_WAVENC_ALAW, NISQA_WAVENC_MULAW, '
                 'NISQA_WAVENC_BIG_ENDIAN);')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)])
    out = dict(l.split(None, 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out['size']) == 40
    for name, _ in lib.WavClip._fields_:
        assert int(out[name]) == getattr(lib.WavClip, name).offset == ingest.WAV_CLIP.fields[name][1], name
    assert [int(v) for v in out['enc'].split()] == [lib.WAVENC_PCM, lib.WAVENC_FLOAT, lib.WAVENC_ALAW, lib.WAVENC_MULAW,
                                                    lib.WAVENC_BIG_ENDIAN] == [1, 3, 6, 7, 0x10000]
    assert 'nisqa_wav_decode' in lib.SYMBOLS and len(lib.SYMBOLS['nisqa_wav_decode'][1]) == 7
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_hip.h')).read()
    assert re.search(r'#define NISQA_ABI_VERSION 2\b', hdr) and lib.ABI_VERSION == 2
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert 'nisqa_wav_decode' in lib.exported_symbols(lib.LIB_PATH, 'nisqa_wav_')


def test_host_decode_switch_selects_the_host_decoding_ingest(monkeypatch, tmp_path):
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    assert ingest.device_decode_default() is True
    monkeypatch.setenv('NISQA_HOST_DECODE', '1')
    assert ingest.device_decode_default() is False
    monkeypatch.setenv('NISQA_HOST_DECODE', '0')
    assert ingest.device_decode_default() is True
    # and the default Ingest is the host-decoding one
    rng = np.random.default_rng(8)
    p = wc.write_case(str(tmp_path / 'st.wav'), wc.Case('pcm24', 40, 2, False, -1, rng), 16000)
    (g,), _ = _stage_one(_ListDataset([p]), [0])
    assert g.kind == 'f32' and g.clips is None and g.nbytes == 160
