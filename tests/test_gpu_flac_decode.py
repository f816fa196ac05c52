"""nisqa_flac_decode on the GPU: every stream of flac_dev_cases, staged by ``Ingest(..., device_flac=True)`` as frame regions and frame
tables, against what the host path hands the network for the same files (wavio.read_wav: flac.hpp through libnisqa_ingest.so) -- bit
for bit --, the refusals, and the predict loop and group_pcm on top of it against their NISQA_HOST_FLAC=1 selves and WAV twins."""
import os

import numpy as np
import pytest
import torch

import flac_dev_cases as fc
import flac_enc
import helpers
from nisqa_amd import ingest, lib, synth, wavio

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF            # a NaN no decoder produces
GUARD = 4096                     # elements behind the output / bytes behind the workspace that must stay as they were


@pytest.fixture(scope='module')
def eng():
    from nisqa_amd.engine import HipNisqa
    args = dict(helpers.DIM_ARGS)
    args.update({'pretrained_model': False, 'tr_bs_val': 1, 'tr_num_workers': 0})
    return HipNisqa(args, helpers.random_state_dict(7))


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('flac_streams')
    out = {}
    for s in fc.streams():
        out[s.name] = str(d / (s.name + '.flac'))
        with open(out[s.name], 'wb') as f:
            f.write(s.data)
    return out


class _ListDataset(object):
    def __init__(self, paths, ms_channel=None):
        self.paths, self.ms_channel = paths, ms_channel

    def file_path(self, i):
        return self.paths[i]


def _stage(paths, ms_channel=None):
    """One staged batch of ``paths`` for the device decoder -> [(Group, its bytes as a numpy array)]."""
    ing = ingest.Ingest(_ListDataset(paths, ms_channel), [list(range(len(paths)))], pin=False, num_workers=2, device_decode=True,
                        device_flac=True)
    try:
        staged = next(iter(ing))
        buf = ing.ring.buf[staged.slot].numpy()
        out = [(g, buf[g.offset:g.offset + g.nbytes].copy()) for g in staged.groups]
        ing.ring.release_after(staged.slot, None)
        return out
    finally:
        ing.close()


def _launch(eng, g, raw, edit=None):
    """One nisqa_flac_decode launch of a staged flac group whose clips ALL went to the device; output and workspace pre-filled with
    sentinels and followed by guard space -> (output as numpy, status words)."""
    f = g.flac
    assert g.kind == 'flac' and f['pos'].tolist() == list(range(len(g.ids))), 'a stream fell back to the host path: %r' % (g.names,)
    total = int(sum(g.lengths))
    x = torch.from_numpy(raw if edit is None else edit(raw.copy(), g)).to(eng.device)
    if f['as_i16']:
        out = torch.full((total + GUARD,), 0x5A5A, dtype=torch.int16, device=eng.device)
    else:
        out = torch.full((total + GUARD,), SENTINEL, dtype=torch.int32, device=eng.device).view(torch.float32)
    t = f['clips']
    md5 = 0 if f['as_i16'] else int(((t['n_samples'] * t['channels'] * ((t['bits'] + 7) // 8) + 3) // 4 * 4)[t['md5_set'] != 0].sum())
    need = eng.lib.nisqa_flac_workspace_bytes(f['n_rows'], int(t['block_size'].max()), int(t['channels'].max()), md5)
    ws = torch.full((need + GUARD,), 0xC3, dtype=torch.uint8, device=eng.device)
    got, status = eng.flac_decode(x, t, f['frames_off'], f['n_rows'], total, f['as_i16'], out=out[:total], ws=ws[:need])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert (ws[need:] == 0xC3).all(), 'the workspace guard was written'
    tail = out[total:].cpu().numpy()
    assert (tail == 0x5A5A).all() if f['as_i16'] else (tail.view(np.uint32) == SENTINEL).all(), 'the output guard was written'
    return out[:total].cpu().numpy(), status.cpu().numpy()


def _expected(g, ms_channel=None):
    want = []
    for name in g.names:
        y, _ = wavio.read_wav(name, ms_channel)                    # the host path: int16 (mono 16-bit) or float32 mono
        if y.dtype == np.int16 and not g.flac['as_i16']:
            y = y.astype(np.float32) / np.float32(32768.0)
        want.append(y)
    return want


def _same(got, want, g):
    at = 0
    for name, y in zip(g.names, want):
        part = got[at:at + len(y)]
        assert part.dtype == y.dtype, name
        assert np.array_equal(part.view(np.uint32) if y.dtype == np.float32 else part, y.view(np.uint32) if y.dtype == np.float32 else y), name
        at += len(y)
    assert at == len(got)


@pytest.mark.parametrize('ms_channel', [None, 0, 1])
def test_kernel_equals_the_host_decoder_bit_for_bit(eng, files, ms_channel):
    """All streams in one staged batch (one launch per sample rate, the 16 kHz one with 30 clips and more than 64 frames in one of
    them): every stream is planned for the device, every sample of every clip is written and equals the host decoder's, the status
    words are zero and nothing else is touched."""
    S = fc.streams()
    groups = _stage([files[s.name] for s in S], ms_channel)
    assert sum(len(g.ids) for g, _ in groups) == len(S) > 64 and all(g.kind == 'flac' for g, _ in groups)
    assert max(len(s.sizes) for s in S) > 64 and max(g.flac['n_rows'] for g, _ in groups) > 64
    for g, raw in groups:
        got, status = _launch(eng, g, raw)
        assert not status.any(), (g.names, status)
        _same(got, _expected(g, ms_channel), g)


def test_mono_16_bit_groups_decode_to_int16_and_many_clips_share_a_launch(eng, files):
    """The int16 form: 70 clips x 4 frames at block 192 plus every other mono 16-bit stream, one launch per rate."""
    mono16 = [s for s in fc.streams() if s.bits == 16 and s.channels == 1]
    paths = [files[s.name] for s in mono16] + [files['fixed%d' % (k % 5)] for k in range(70)]
    groups = _stage(paths)
    assert any(len(g.ids) > 64 for g, _ in groups)
    for g, raw in groups:
        assert g.flac['as_i16']
        got, status = _launch(eng, g, raw)
        assert got.dtype == np.int16 and not status.any()
        _same(got, _expected(g), g)


def _shift_row(raw, g):
    rows = raw[g.flac['frames_off']:].view(fc.ROW)
    k = int(g.flac['clips']['n_frames'][:SHIFTED].sum()) + 1        # the second frame of clip SHIFTED
    rows['offset'][k] += 1
    return raw


SHIFTED = 3


def test_refusals_flag_exactly_the_damaged_clip(eng, files, tmp_path):
    """The six fixed mutations (each refused by the host-compiled decoder in test_flac_frame_host first): exactly that clip's status
    word is set, by the check that should see it, and every other clip of the launch is bit-identical."""
    want_bits = {'residual': 1 << 5, 'rice': None, 'warmup': 1 << 5, 'crc16': 1 << 5, 'md5': lib.FLAC_BAD_MD5}
    by_rate = {}
    for s in fc.streams():
        by_rate.setdefault(s.sr, []).append(s)
    for name, stream, mutate in fc.MUTATIONS:
        s = fc.by_name(stream)
        b = bytearray(s.data)
        mutate(b, s)
        bad = str(tmp_path / (name + '.flac'))
        with open(bad, 'wb') as f:
            f.write(bytes(b))
        mates = by_rate[s.sr]
        k = mates.index(s)
        (g, raw), = _stage([bad if m is s else files[m.name] for m in mates])
        got, status = _launch(eng, g, raw)
        # (damaged samples also miss STREAMINFO's MD5, which the device checks whatever the frames said; a damaged CRC-16 alone does not)
        extra = lib.FLAC_BAD_MD5 if name in ('residual', 'rice', 'warmup') else 0
        assert status[k] != 0 and (want_bits[name] is None or status[k] == want_bits[name] | extra), (name, status)
        assert not np.delete(status, k).any(), (name, status)
        good = g.names[:k] + [files[s.name]] + g.names[k + 1:]
        want = [wavio.read_wav(p, None)[0] for p in good]
        at = 0
        for j, y in enumerate(want):
            y = y.astype(np.float32) / np.float32(32768.0) if y.dtype == np.int16 and not g.flac['as_i16'] else y
            if j != k:
                assert np.array_equal(got[at:at + len(y)].view(np.uint32 if y.dtype == np.float32 else y.dtype),
                                      y.view(np.uint32 if y.dtype == np.float32 else y.dtype)), (name, g.names[j])
            at += len(y)
    # a table row whose next offset is off by one: the frame before it no longer ends there, the frame itself starts off its sync
    mates = by_rate[16000]
    (g, raw), = _stage([files[m.name] for m in mates])
    got, status = _launch(eng, g, raw, edit=_shift_row)
    assert status[SHIFTED] == (1 << 6) | (1 << 1) | lib.FLAC_BAD_MD5 and not np.delete(status, SHIFTED).any(), status      # (+ the MD5 of what frame 1 left undecoded)
    want = _expected(g)
    at = 0
    for j, y in enumerate(want):
        if j != SHIFTED:
            assert np.array_equal(got[at:at + len(y)].view(np.uint32), y.view(np.uint32)), g.names[j]
        at += len(y)


def test_tables_outside_the_limits_are_refused_on_the_host(eng, files):
    (g, raw), = _stage([files['fixed2'], files['stereo10']])
    x = torch.from_numpy(raw).to(eng.device)
    f, total = g.flac, int(sum(g.lengths))
    for field, value in (('src_off', 8), ('src_bytes', 1 << 30), ('dst_off', total), ('n_samples', 1 << 31), ('channels', 3), ('bits', 25),
                         ('channel', 2), ('block_size', 0), ('n_frames', 1)):
        bad = f['clips'].copy()
        bad[field][1] = value
        with pytest.raises(ValueError, match='nisqa_flac_decode'):
            eng.flac_decode(x, bad, f['frames_off'], f['n_rows'], total, False)
    for off, rows in ((f['frames_off'] + 16, f['n_rows']), (f['frames_off'] + 2, f['n_rows']), (f['frames_off'], f['n_rows'] + 1)):
        with pytest.raises(ValueError, match='nisqa_flac_decode'):
            eng.flac_decode(x, f['clips'], off, rows, total, False)
    with pytest.raises(ValueError, match='nisqa_flac_decode'):
        eng.flac_decode(x, f['clips'], f['frames_off'], f['n_rows'], total, True)       # a stereo stream has no int16 form
    # rows native code did not write (a clip index outside the table) are caught on the device: the launch's last status word
    raw2 = raw.copy()
    raw2[f['frames_off']:].view(fc.ROW)['clip'][0] = 9
    out, status = eng.flac_decode(torch.from_numpy(raw2).to(eng.device), f['clips'], f['frames_off'], f['n_rows'], total, False)
    assert status.cpu().numpy()[-1] == lib.FLAC_BAD_TABLE


# ---- the loops -----------------------------------------------------------------------------------------------------------------
COLS = ['mos_pred', 'noi_pred', 'dis_pred', 'col_pred', 'loud_pred']


def _checkpoint(tmp_path):
    args = dict(helpers.DIM_ARGS)
    args.update({'pretrained_model': False, 'tr_bs_val': 4, 'tr_num_workers': 0})
    path = str(tmp_path / 'rand.tar')
    torch.save({'args': args, 'model_state_dict': helpers.random_state_dict(7)}, path)
    return path


def _predict(tmp_path, ckpt, names, tag):
    import pandas as pd
    from nisqa_amd.NISQA_model import nisqaModel
    pd.DataFrame({'deg': names}).to_csv(tmp_path / (tag + '.csv'), index=False)
    a = {'mode': 'predict_csv', 'pretrained_model': ckpt, 'deg': None, 'data_dir': str(tmp_path), 'output_dir': None,
         'csv_file': tag + '.csv', 'csv_deg': 'deg', 'num_workers': 2, 'bs': 4, 'ms_channel': None, 'tr_bs_val': 4, 'tr_num_workers': 2}
    return nisqaModel(a).predict()[COLS].to_numpy()


def _write_24bit_wav(path, v, sr):
    import struct
    raw = b''.join(int(x & 0xFFFFFF).to_bytes(3, 'little') for x in v)
    hdr = b'RIFF' + struct.pack('<I', 36 + len(raw)) + b'WAVE' + b'fmt ' + struct.pack('<IHHIIHH', 16, 1, 1, sr, 3 * sr, 3, 24) \
        + b'data' + struct.pack('<I', len(raw))
    with open(path, 'wb') as fh:
        fh.write(hdr + raw)


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """Seven clips (the sizes of test_predict_csv_on_flac_files_equals_...: 0.4-1.6 s) at two rates, as WAV and as FLAC twins: mono
    16-bit, one stereo 16-bit and one mono 24-bit per rate group."""
    d = tmp_path_factory.mktemp('flac_corpus')
    rng = np.random.default_rng(31)
    names = []
    for i in range(7):
        sr = 48000 if i < 4 else 16000
        pcm = synth.synth_pcm16(500 + i, float(rng.uniform(0.4, 1.6)), sr=sr)
        bits, data = 16, pcm
        w, f = str(d / ('c%d.wav' % i)), str(d / ('c%d.flac' % i))
        if i in (3, 6):
            data = np.stack([pcm, np.roll(pcm, 7)], axis=1)
        if i in (2, 5):
            bits, data = 24, pcm.astype(np.int32) * 256 + 37
            _write_24bit_wav(w, data, sr)
        else:
            synth.write_wav(w, data, sr)
        with open(f, 'wb') as fh:
            fh.write(flac_enc.encode(data, sr, bits, blocksize=4096, stereo=10 if np.ndim(data) == 2 else 0,
                                     kinds={'type': 'fixed', 'order': 2, 'porder': 2}))
        names.append('c%d' % i)
    return d, names


def test_predict_rows_equal_the_host_flac_run_and_the_wav_twins(corpus, monkeypatch):
    """predict_csv over a job that mixes WAV files with mono 16-bit, stereo 16-bit and mono 24-bit FLAC streams at two sample rates:
    the device path (the host FLAC decoder must not run), NISQA_HOST_FLAC=1 and the all-WAV twin job give the same five columns."""
    d, names = corpus
    ckpt = _checkpoint(d)
    mixed = [n + ('.wav' if i in (1,) else '.flac') for i, n in enumerate(names)]
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    monkeypatch.delenv('NISQA_HOST_FLAC', raising=False)
    assert ingest.device_flac_default()

    def boom(*a, **k):
        raise AssertionError('the host FLAC decoder ran')
    with monkeypatch.context() as m:
        m.setattr(wavio, '_decode_flac', boom)
        m.setattr(lib.load_ingest(), 'nisqa_ingest_decode_flac', boom)
        dev = _predict(d, ckpt, mixed, 'dev')
    monkeypatch.setenv('NISQA_HOST_FLAC', '1')
    with monkeypatch.context() as m:
        m.setattr(lib.load_ingest(), 'nisqa_ingest_flac_plan', boom)
        host = _predict(d, ckpt, mixed, 'host')
    wav = _predict(d, ckpt, [n + '.wav' for n in names], 'wav')
    assert dev.shape == (7, 5) and np.isfinite(host).all()
    np.testing.assert_array_equal(dev, host)
    np.testing.assert_array_equal(dev, wav)


def test_a_damaged_stream_surfaces_as_could_not_load_file(corpus, tmp_path, monkeypatch):
    d, names = corpus
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    monkeypatch.delenv('NISQA_HOST_FLAC', raising=False)
    data = bytearray(open(str(d / 'c4.flac'), 'rb').read())
    data[-1] ^= 0xFF                                                  # the last frame's CRC-16
    for n in ('c5.flac', 'c6.flac'):
        os.symlink(str(d / n), str(tmp_path / n))
    with open(str(tmp_path / 'c4.flac'), 'wb') as f:
        f.write(bytes(data))
    ckpt = _checkpoint(tmp_path)
    with pytest.raises(ValueError, match='Could not load file .*c4.flac'):
        _predict(tmp_path, ckpt, ['c5.flac', 'c4.flac', 'c6.flac'], 'bad')


def test_group_pcm_with_ms_channel_equals_the_host_path(eng, corpus):
    """What trainloop.train does with a staged batch: ingest.group_pcm per rate group with ms_channel = 1 -- the second channel of the
    stereo streams, channel 0 of the mono ones -- for the device path against the host-decoding Ingest."""
    d, names = corpus
    paths = [str(d / (n + '.flac')) for n in names] + [str(d / 'c1.wav')]
    pcm = {}
    for mode in (True, False):
        ing = ingest.Ingest(_ListDataset(paths, ms_channel=1), [list(range(len(paths)))], pin=True, num_workers=2, device_decode=True,
                            device_flac=mode)
        try:
            staged = next(iter(ing))
            raw = ing.ring.buf[staged.slot]
            pcm[mode] = [(g.kind, g.ids, g.lengths, g.sr, ingest.group_pcm(raw, g, eng, 1)) for g in staged.groups]
            ev = torch.cuda.Event()
            ev.record()
            ing.ring.release_after(staged.slot, ev)
            torch.cuda.synchronize()
        finally:
            ing.close()
    assert [k for k, *_ in pcm[True]] == ['flac', 'flac'] and [k for k, *_ in pcm[False]] == ['raw', 'raw']
    for (_, ids, lengths, sr, got), (_, ids2, lengths2, sr2, want) in zip(pcm[True], pcm[False]):
        assert (ids, lengths, sr) == (ids2, lengths2, sr2) and got.dtype == want.dtype == torch.float32 and got.numel() == sum(lengths)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # and mono 16-bit clips alone, WAV and FLAC side by side: the int16 form either way
    mono = [str(d / 'c0.flac'), str(d / 'c1.wav'), str(d / 'c1.flac')]
    out = {}
    for mode in (True, False):
        ing = ingest.Ingest(_ListDataset(mono), [[0, 1, 2]], pin=True, num_workers=2, device_decode=True, device_flac=mode)
        try:
            staged = next(iter(ing))
            (g,) = staged.groups
            out[mode] = (g.kind, ingest.group_pcm(ing.ring.buf[staged.slot], g, eng))
            torch.cuda.synchronize()
            ing.ring.release_after(staged.slot, None)
        finally:
            ing.close()
    assert out[True][0] == 'flac' and out[False][0] == 'i16' and out[True][1].dtype == torch.int16
    assert torch.equal(out[True][1], out[False][1])
