"""nisqa_wav_decode on the GPU: every WAV encoding the ingest accepts, from the verbatim data chunk to the float32 mono samples
``wavio._decode`` returns -- compared bit for bit --, and the predict and training loops on top of it against their
host-decoding selves (NISQA_HOST_DECODE=1)."""
import numpy as np
import pytest
import torch

import helpers
import wav_cases as wc
from nisqa_amd import ingest, lib, synth, wavio

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF            # a NaN no decoder produces


@pytest.fixture(scope='module')
def eng():
    from nisqa_amd.engine import HipNisqa
    args = dict(helpers.DIM_ARGS)
    args.update({'pretrained_model': False, 'tr_bs_val': 1, 'tr_num_workers': 0})
    return HipNisqa(args, helpers.random_state_dict(7))


def _decode(eng, cases, gap):
    """The cases through ONE launch -> (uint32 view of the whole output, the table)."""
    raw, table, n_out = wc.pack(cases, gap)
    out = torch.full((n_out,), SENTINEL, dtype=torch.int32, device=eng.device).view(torch.float32)
    got = eng.decode(torch.from_numpy(raw).to(eng.device), table, n_out, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy().view(np.uint32), table


def _check(cases, bits, table, gap):
    covered = np.zeros(len(bits), dtype=bool)
    for c, row in zip(cases, table):
        at = int(row['dst_off'])
        want = c.expected()
        got = bits[at:at + c.n]
        assert np.array_equal(got.view(np.float32), want) and np.array_equal(got, want.view(np.uint32)), c      # (the bits too: -0.0)
        covered[at:at + c.n] = True
    assert covered.sum() == sum(c.n for c in cases) and (bits[~covered] == SENTINEL).all()      # between and behind the clips: untouched
    assert (~covered).sum() == gap * len(cases)


@pytest.mark.parametrize('enc', list(wc.ENCODINGS))
def test_kernel_equals_wavio_decode_bit_for_bit(eng, enc):
    """One encoding, little- and big-endian, 1 / 2 / 3 / 7 / 8 / 9 / 32 channels, the mean / the first / the last channel, every
    frame count of wav_cases.FRAMES, the format's extreme values in the first frames: one table, one launch."""
    cases = wc.cases_of(enc, np.random.default_rng(11))
    assert len(cases) == 2 * 19 * 9
    bits, table = _decode(eng, cases, gap=3)
    _check(cases, bits, table, 3)


def test_one_table_mixing_every_encoding_and_tables_of_one_clip(eng):
    rng = np.random.default_rng(12)
    mixed = []
    for k in range(120):
        enc = list(wc.ENCODINGS)[k % len(wc.ENCODINGS)]
        ch = int(rng.choice(wc.CHANNELS))
        mixed.append(wc.Case(enc, int(rng.choice(wc.FRAMES[:-1] + (1025, 1300))), ch, bool(k // 10 % 2), int(rng.choice(wc.channel_modes(ch))), rng))
    mixed += [wc.Case('alaw', 256, 1, False, -1, rng), wc.Case('mulaw', 256, 1, False, -1, rng)]           # all 256 codes each
    order = rng.permutation(len(mixed))
    mixed = [mixed[i] for i in order]
    bits, table = _decode(eng, mixed, gap=1)
    _check(mixed, bits, table, 1)
    for enc in wc.ENCODINGS:                                         # n_clips = 1
        one = [wc.Case(enc, 257, 3, enc in ('pcm24', 'f64'), -1, rng)]
        bits, table = _decode(eng, one, gap=5)
        _check(one, bits, table, 5)


def test_a_buffer_that_ends_with_its_last_sample_is_read_byte_by_byte_there(eng):
    """raw_bytes = the exact end of the last data chunk, no tail pad, poison behind it in the same allocation: the last 16-byte span
    of each clip is fetched byte by byte up to raw_bytes, and the samples are the same."""
    rng = np.random.default_rng(17)
    for enc, n, ch in (('pcm24', 65, 3), ('u8', 1, 1), ('f64', 1, 1), ('pcm16', 63, 1), ('mulaw', 257, 1), ('f32', 255, 7), ('pcm32', 4099, 2)):
        cases = [wc.Case('pcm16', 64, 1, False, -1, rng), wc.Case(enc, n, ch, enc == 'f32', -1, rng)]
        raw, table, n_out = wc.pack(cases)
        exact = int(table['src_off'][-1]) + len(cases[-1].data)
        assert exact % 16 != 0 and exact < len(raw)
        full = torch.from_numpy(np.concatenate([raw[:exact], np.full(64, 0xFF, np.uint8)])).to(eng.device)
        got = eng.decode(full[:exact], table, n_out).cpu().numpy()
        want = np.concatenate([c.expected() for c in cases])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), cases[-1]


def test_bad_sizes_and_tables_are_refused_on_the_host(eng):
    """Nothing is launched for them: the entry returns NISQA_ERR_ARG, the binding raises for a table entry the kernel would skip."""
    case = wc.Case('pcm24', 100, 2, False, -1, np.random.default_rng(13))
    raw, table, n_out = wc.pack([case])
    dev = torch.from_numpy(raw).to(eng.device)
    tab = torch.from_numpy(table.view(np.uint8).copy()).to(eng.device)
    out = torch.zeros(n_out, device=eng.device)
    L, s = eng.lib, eng._stream()
    p = lambda t: lib.c_p(t.data_ptr())
    assert L.nisqa_wav_decode(p(dev), dev.numel(), p(tab), 1, 100, p(out), s) == lib.NISQA_OK
    assert np.array_equal(out.cpu().numpy(), case.expected())
    for args in ((p(dev), dev.numel(), p(tab), 0, 100, p(out), s), (p(dev), dev.numel(), p(tab), 1, 0, p(out), s),
                 (p(dev), 0, p(tab), 1, 100, p(out), s), (p(dev), dev.numel(), p(tab), -1, 100, p(out), s),
                 (None, dev.numel(), p(tab), 1, 100, p(out), s), (lib.c_p(dev.data_ptr() + 4), dev.numel() - 4, p(tab), 1, 100, p(out), s)):
        assert L.nisqa_wav_decode(*args) == lib.NISQA_ERR_ARG
    for field, value in (('src_off', 8), ('src_off', 1 << 40), ('n_frames', 101 + 16), ('dst_off', 1), ('channel', 2), ('container', 5),
                         ('encoding', 2), ('channels', 0)):
        bad = table.copy()
        bad[field] = value
        with pytest.raises(ValueError, match='nisqa_wav_decode'):
            eng.decode(dev, bad, n_out)
    wide = table.copy()
    wide['channels'], wide['n_frames'] = 33, 1                        # a mean over more than 32 channels is the host's
    with pytest.raises(ValueError, match='nisqa_wav_decode'):
        eng.decode(dev, wide, n_out)


# ---- the loops -----------------------------------------------------------------------------------------------------------------
COLS = ['mos_pred', 'noi_pred', 'dis_pred', 'col_pred', 'loud_pred']


def _checkpoint(tmp_path, **over):
    args = dict(helpers.DIM_ARGS)
    args.update({'pretrained_model': False, 'tr_bs_val': 4, 'tr_num_workers': 0})
    args.update(over)
    path = str(tmp_path / 'rand.tar')
    torch.save({'args': args, 'model_state_dict': helpers.random_state_dict(7)}, path)
    return path


def _predict_both_ways(tmp_path, monkeypatch, ckpt, names):
    """predict_csv over ``names`` with the device decoder (wavio._decode must not run) and with NISQA_HOST_DECODE=1 -> both tables."""
    import pandas as pd
    from nisqa_amd.NISQA_model import nisqaModel
    pd.DataFrame({'wav': names}).to_csv(tmp_path / 'l.csv', index=False)
    a = {'mode': 'predict_csv', 'pretrained_model': ckpt, 'deg': None, 'data_dir': str(tmp_path), 'output_dir': None,
         'csv_file': 'l.csv', 'csv_deg': 'wav', 'num_workers': 2, 'bs': 4, 'ms_channel': None, 'tr_bs_val': 4, 'tr_num_workers': 2}

    def boom(*args, **kw):
        raise AssertionError('the host decoder ran')
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    with monkeypatch.context() as m:
        m.setattr(wavio, '_decode', boom)
        dev = nisqaModel(dict(a)).predict()[COLS].to_numpy()
    monkeypatch.setenv('NISQA_HOST_DECODE', '1')
    host = nisqaModel(dict(a)).predict()[COLS].to_numpy()
    return dev, host


def test_predict_rows_equal_the_host_decoding_run(tmp_path, monkeypatch):
    """One file per encoding and channel count (the even ones RIFX) plus mono PCM16 files at the same and at another rate: every
    prediction column of the default run -- data chunks decoded by the kernel -- equals the NISQA_HOST_DECODE=1 run exactly."""
    rng = np.random.default_rng(14)
    names = []
    for k, (enc, ch) in enumerate((e, c) for e in wc.ENCODINGS for c in wc.CHANNELS):
        names.append('%s_%02d.wav' % (enc, ch))
        wc.write_case(str(tmp_path / names[-1]), wc.Case(enc, 2400 + 37 * k, ch, k % 2 == 1, -1, rng, edges=False), 16000)
    for k, sr in enumerate((16000, 16000, 8000, 8000)):
        names.append('mono16_%d.wav' % k)
        synth.write_wav(str(tmp_path / names[-1]), synth.synth_pcm16(80 + k, 0.4, sr=sr), sr)
    dev, host = _predict_both_ways(tmp_path, monkeypatch, _checkpoint(tmp_path), names)
    assert dev.shape == (len(names), 5) and np.isfinite(host).all()
    assert np.array_equal(dev, host)


def test_resampled_rows_equal_the_host_decoding_run(tmp_path, monkeypatch):
    """ms_sr = 48 000 on a 44.1 kHz stereo 24-bit file: nisqa_resample sees the same float32 samples either way."""
    rng = np.random.default_rng(15)
    wc.write_case(str(tmp_path / 'st24.wav'), wc.Case('pcm24', 9000, 2, False, -1, rng, edges=False), 44100)
    synth.write_wav(str(tmp_path / 'mono16.wav'), synth.synth_pcm16(90, 0.3, sr=44100), 44100)
    dev, host = _predict_both_ways(tmp_path, monkeypatch, _checkpoint(tmp_path, ms_sr=48000), ['st24.wav', 'mono16.wav'])
    assert np.isfinite(host).all() and np.array_equal(dev, host)


class _ListDataset(object):
    ms_channel = None

    def __init__(self, paths):
        self.paths = paths

    def file_path(self, i):
        return self.paths[i]


def test_group_pcm_of_a_mixed_rate_training_batch_equals_the_host_path(eng, tmp_path):
    """What trainloop.train does with a staged batch: ingest.group_pcm per rate group, for stereo 24-bit and mono PCM16 files at two
    rates -- the device PCM of the raw groups equals the host-decoded float32, the int16 group is the int16 group."""
    rng = np.random.default_rng(16)
    spec = [('pcm24', 2, 16000, 3001), ('pcm16', 1, 16000, 2500), ('pcm24', 2, 8000, 1777), ('pcm16', 1, 48000, 4000), ('pcm16', 1, 48000, 5000),
            ('pcm16', 1, 8000, 900)]
    paths = [wc.write_case(str(tmp_path / ('t%d.wav' % k)), wc.Case(enc, n, ch, False, -1, rng), sr) for k, (enc, ch, sr, n) in enumerate(spec)]
    pcm = {}
    for mode in (True, False):
        ing = ingest.Ingest(_ListDataset(paths), [list(range(len(paths)))], pin=True, num_workers=2, device_decode=mode)
        try:
            staged = next(iter(ing))
            raw = ing.ring.buf[staged.slot]
            pcm[mode] = [(g.kind, g.ids, g.lengths, g.sr, ingest.group_pcm(raw, g, eng)) for g in staged.groups]
            ev = torch.cuda.Event()
            ev.record()
            ing.ring.release_after(staged.slot, ev)
            torch.cuda.synchronize()
        finally:
            ing.close()
    assert [k for k, *_ in pcm[True]] == ['raw', 'raw', 'i16'] and [k for k, *_ in pcm[False]] == ['f32', 'f32', 'i16']
    for (_, ids, lengths, sr, got), (_, ids2, lengths2, sr2, want) in zip(pcm[True], pcm[False]):
        assert (ids, lengths, sr) == (ids2, lengths2, sr2) and got.dtype == want.dtype and got.numel() == sum(lengths)
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                           want.view(torch.int32) if want.dtype == torch.float32 else want)
