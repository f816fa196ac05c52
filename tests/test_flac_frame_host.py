"""Host side of the device FLAC decoder: the shared frame decoder (csrc/flac_frame.hpp) compiled with g++ against the host decoder
(flac.hpp through nisqa_ingest_decode_flac), the plan / read entries of libnisqa_ingest.so against an independent walk of the files,
what ``Ingest(..., device_flac=True)`` stages, and the ABI of both libraries.  No GPU, no sanitizer (tools/flac_frame_fuzz.cpp is the
sanitizer run, by hand)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import flac_dev_cases as fc
import flac_enc
import wav_cases as wc
from nisqa_amd import ingest, lib, wavio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return fc.build_host_decoder(tmp_path_factory.mktemp('flac_frame_host'))


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    """Every stream of the list as a file -> {name: path}."""
    d = tmp_path_factory.mktemp('flac_streams')
    out = {}
    for s in fc.streams():
        out[s.name] = str(d / (s.name + '.flac'))
        with open(out[s.name], 'wb') as f:
            f.write(s.data)
    return out


def _native_decode(path):
    L = lib.load_ingest()
    info = (lib.WavInfo * 1)()
    paths = (ctypes.c_char_p * 1)(os.fsencode(path))
    if L.nisqa_ingest_probe(paths, 1, info, 1) != 0:
        return None
    v = np.full((info[0].n_frames, info[0].channels), 0x55555555, dtype=np.int32)
    return v if L.nisqa_ingest_decode_flac(os.fsencode(path), info, ctypes.c_void_p(v.ctypes.data)) == 0 else None


def _plan(paths):
    L, n = lib.load_ingest(), len(paths)
    arr = (ctypes.c_char_p * n)(*[os.fsencode(p) for p in paths])
    info = (lib.WavInfo * n)()
    assert L.nisqa_ingest_probe(arr, n, info, 2) == 0
    plans = (lib.FlacPlan * n)()
    good = L.nisqa_ingest_flac_plan(arr, n, info, plans, 2)
    return arr, info, plans, good


# ---- the shared decoder ------------------------------------------------------------------------------------------------------------
def test_shared_decoder_equals_the_host_decoder_sample_for_sample(host, files):
    assert len(fc.streams()) > 64 and sum(len(s.sizes) for s in fc.streams()) > 64
    for s in fc.streams():
        rc, got, rows = fc.host_decode(host, s.data)
        want = _native_decode(files[s.name])
        assert rc == 0 and want is not None, s
        assert np.array_equal(got, want) and np.array_equal(got, s.samples()), s
        assert [tuple(r)[:3] for r in rows.tolist()] == s.rows(), s


def test_mutated_streams_are_refused_or_decode_to_the_host_decoders_result(host):
    """240 single-bit and byte-run mutations per stream: the device path refuses the stream, hands it to the host path, or returns
    exactly the host decoder's samples -- never samples the host decoder would not have produced."""
    rng = np.random.default_rng(21)
    counts = np.zeros(4, dtype=np.int64)
    for s in fc.streams():
        for it in range(240):
            b = bytearray(s.data)
            pos = int(rng.integers(4, len(b)))
            if it % 2 == 0:
                b[pos] ^= 1 << int(rng.integers(0, 8))
            else:
                run = rng.integers(0, 256, int(rng.integers(1, 17)), dtype=np.uint8).tobytes()
                b[pos:pos + len(run)] = run[:len(b) - pos]
            rc = host.nqff_compare(bytes(b), len(b))
            assert rc != 3, (s, it, pos)
            counts[rc] += 1
    print('mutations: accepted %d, refused %d, host path %d' % tuple(counts[:3]))
    assert counts[1] > counts[0]


def test_the_six_fixed_mutations_are_refused(host):
    """The mutations the GPU refusal test repeats: each is refused here first, by the check that should see it."""
    want = {'residual': 1 << 5, 'rice': None, 'warmup': 1 << 5, 'crc16': 1 << 5, 'md5': 0x80}       # (1 << 5: the CRC-16)
    for name, stream, mutate in fc.MUTATIONS:
        s = fc.by_name(stream)
        b = bytearray(s.data)
        mutate(b, s)
        assert bytes(b) != s.data
        rc, _, _ = fc.host_decode(host, bytes(b))
        assert rc != 'host' and rc != 0 and (want[name] is None or rc == want[name]), (name, rc)
        assert host.nqff_compare(bytes(b), len(b)) == 1
    s = fc.by_name('lpc8_12')
    rc, _, _ = fc.host_decode(host, s.data, fc.shift_second_row)
    assert rc == (1 << 6) | (1 << 1), rc                   # frame 0 no longer ends where the table says, frame 1 starts off its sync


# ---- plan / read -------------------------------------------------------------------------------------------------------------------
def test_plan_reports_eligibility_region_and_streaminfo(files, tmp_path):
    S = fc.streams()
    arr, info, plans, good = _plan([files[s.name] for s in S])
    assert good == len(S)
    for s, p in zip(S, plans):
        n = len(s.x)
        assert p.eligible == 1, s
        assert (p.region_off, p.region_bytes) == (s.first_frame, len(s.data) - s.first_frame), s
        assert (p.n_frames, p.block_size, p.bits, p.channels, p.n_samples) == (len(s.sizes), s.blocksize, s.bits, s.channels, n), s
        assert p.md5_set == (0 if s.kw.get('with_md5') is False else 1), s
        assert bytes(p.md5) == s.data[s.first_frame - 16 - sum(4 + len(b) for _, b in s.kw.get('extra_blocks', ())):][:16], s
    # the ineligible cases: exactly these
    x = fc.signal(600, seed=1)
    cases = {'variable': flac_enc.encode(x, 16000, 16, blocksize=192, variable=True),
             'no_total': flac_enc.encode(x, 16000, 16, blocksize=192, with_total=False),
             'short': flac_enc.encode(x[:100], 16000, 16, blocksize=192),
             'three_ch': flac_enc.encode(np.stack([x, x // 2, -x], axis=1), 16000, 16, blocksize=192)}
    paths = []
    for name, data in cases.items():
        paths.append(str(tmp_path / (name + '.flac')))
        with open(paths[-1], 'wb') as f:
            f.write(data)
        assert _native_decode(paths[-1]) is not None, name          # (streams the host decoder reads)
    paths.append(wc.write_case(str(tmp_path / 'a.wav'), wc.Case('pcm16', 100, 1, False, -1, np.random.default_rng(1)), 16000))
    arr, info, plans, good = _plan(paths)
    assert good == 0 and [p.eligible for p in plans] == [0] * 5
    L = lib.load_ingest()
    assert L.nisqa_ingest_flac_plan(None, 3, None, None, 1) == -1 and L.nisqa_ingest_flac_plan(None, 0, None, None, 1) == 0


def _read(paths, clip_ids=None):
    """plan + read of ``paths`` into one buffer -> (plans, status, list of (region bytes, frame rows))."""
    L, n = lib.load_ingest(), len(paths)
    arr, info, plans, good = _plan(paths)
    region_off, table_off, at = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64), 0
    for k, p in enumerate(plans):
        if p.eligible:
            region_off[k] = at
            at = (at + p.region_bytes + 15) // 16 * 16
            table_off[k] = at
            at += 16 * p.n_frames
    buf = np.full(at + 64, 0xA5, dtype=np.uint8)
    ids = np.arange(n, dtype=np.int32) + 7 if clip_ids is None else np.asarray(clip_ids, dtype=np.int32)
    status = np.full(n, -1, dtype=np.int32)
    i64, i32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    bad = L.nisqa_ingest_flac_read(arr, n, plans, buf.ctypes.data, region_off.ctypes.data_as(i64), table_off.ctypes.data_as(i64),
                                   ids.ctypes.data_as(i32), status.ctypes.data_as(i32), 3)
    assert bad == int((status != 0).sum())
    assert (buf[at:] == 0xA5).all()                                 # nothing behind the last table
    out = []
    for k, p in enumerate(plans):
        if not p.eligible:
            out.append(None)
            continue
        rows = buf[table_off[k]:table_off[k] + 16 * p.n_frames].view(fc.ROW)
        out.append((bytes(buf[region_off[k]:region_off[k] + p.region_bytes]), rows))
    return plans, status, out


def test_read_copies_the_region_verbatim_and_indexes_every_frame(files):
    S = fc.streams()
    plans, status, out = _read([files[s.name] for s in S])
    assert (status == 0).all()
    for k, (s, (region, rows)) in enumerate(zip(S, out)):
        assert region == s.data[s.first_frame:], s
        assert [tuple(r) for r in rows.tolist()] == [r + (k + 7,) for r in s.rows()], s


def _header_with_number(stream, number):
    """The six header bytes of the stream's first frame, renumbered, with their CRC-8."""
    h = bytearray(stream.data[stream.first_frame:stream.first_frame + 4]) + flac_enc.utf8_number(number)
    return bytes(h) + bytes([flac_enc.crc_bitwise(bytes(h), 0x07, 8)])


def test_a_false_sync_with_a_valid_crc8_but_the_wrong_number_is_skipped(tmp_path, host):
    x = fc.signal(3 * 192, seed=5)
    plain = fc.Stream('plain', x, 16000, 16, kinds={'type': 'verbatim'}, blocksize=192)
    fake = _header_with_number(plain, 7)                            # a header that parses, CRC-8 and all, for frame 7
    assert len(fake) == 6
    x[20:23] = np.frombuffer(fake, dtype='>i2')                     # verbatim 16-bit samples are byte-aligned behind an 8-bit subframe header
    s = fc.Stream('planted', x, 16000, 16, kinds={'type': 'verbatim', 'wasted': False}, blocksize=192)
    at = s.data.find(fake, s.first_frame + 6)
    assert s.first_frame + 6 < at < s.first_frame + s.sizes[0]      # inside frame 0, before the true second frame
    p = str(tmp_path / 'planted.flac')
    with open(p, 'wb') as f:
        f.write(s.data)
    plans, status, out = _read([p], [0])
    assert status.tolist() == [0] and [tuple(r)[:3] for r in out[0][1].tolist()] == s.rows()
    rc, got, _ = fc.host_decode(host, s.data)
    assert rc == 0 and np.array_equal(got, s.samples())


def _renumbered(x):
    """A stream the host decoder reads (it ignores frame numbers) but whose second frame is numbered 51 behind frame 0."""
    a = fc.Stream('a', x, 16000, 16, kinds={'type': 'fixed', 'order': 2}, blocksize=192)
    b = fc.Stream('b', x, 16000, 16, kinds={'type': 'fixed', 'order': 2}, blocksize=192, first_frame_number=50)
    return a.data[:a.first_frame + a.sizes[0]] + b.data[b.first_frame + b.sizes[0]:]


def test_read_fails_a_stream_it_cannot_index(tmp_path):
    x = fc.signal(3 * 192 + 5, seed=6)
    s = fc.Stream('t', x, 16000, 16, kinds={'type': 'fixed', 'order': 2}, blocksize=192)
    cases = {'truncated': s.data[:s.first_frame + s.sizes[0] + s.sizes[1] + s.sizes[2] // 2],      # the last frame's header is gone
             'renumbered': _renumbered(x), 'whole': s.data}
    paths = []
    for name, data in cases.items():
        paths.append(str(tmp_path / (name + '.flac')))
        with open(paths[-1], 'wb') as f:
            f.write(data)
    plans, status, out = _read(paths)
    assert [p.eligible for p in plans] == [1, 1, 1]
    assert status[0] != 0 and status[1] != 0 and status[2] == 0
    assert _native_decode(paths[0]) is None and np.array_equal(_native_decode(paths[1])[:, 0], x)


# ---- Ingest ------------------------------------------------------------------------------------------------------------------------
class _ListDataset(object):
    def __init__(self, paths, ms_channel=None):
        self.paths, self.ms_channel = paths, ms_channel

    def file_path(self, i):
        return self.paths[i]


def _stage_one(ds, idx, **kw):
    ing = ingest.Ingest(ds, [idx], pin=False, num_workers=2, **kw)
    try:
        staged = next(iter(ing))
        buf = ing.ring.buf[staged.slot].numpy().copy()
        ing.ring.release_after(staged.slot, None)
        return staged.groups, buf
    finally:
        ing.close()


def _boom(*a, **k):
    raise AssertionError('a FLAC entry for the device decoder was called')


def test_device_decode_without_the_flag_stages_flac_as_before(files, monkeypatch):
    names = ['fixed2', 'stereo10', 'bits24', 'id3']
    ds = _ListDataset([files[n] for n in names])
    L = lib.load_ingest()
    with monkeypatch.context() as m:
        m.setattr(L, 'nisqa_ingest_flac_plan', _boom)
        m.setattr(L, 'nisqa_ingest_flac_read', _boom)
        (g,), buf = _stage_one(ds, [0, 1, 2, 3], device_decode=True)
        (h,), _ = _stage_one(ds, [0, 1, 2, 3], device_flac=True)    # (the flag alone, without device decode, changes nothing either)
    assert g.kind == 'raw' and g.flac is None and h.kind == 'f32' and h.flac is None
    t = g.clips
    assert t['container'].tolist() == [2, 4, 4, 2] and t['encoding'].tolist() == [lib.WAVENC_PCM, lib.WAVENC_FLOAT, lib.WAVENC_FLOAT, lib.WAVENC_PCM]
    for k, n in enumerate(names):
        want, _ = wavio.read_wav(files[n], None)
        at = g.offset + int(t['src_off'][k])
        got = buf[at:at + want.nbytes].view(want.dtype)
        assert np.array_equal(got, want), n


def test_an_all_wav_job_plans_and_reads_nothing_new(tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    paths = [wc.write_case(str(tmp_path / ('w%d.wav' % k)), wc.Case(enc, 300 + k, ch, False, -1, rng), 16000)
             for k, (enc, ch) in enumerate((('pcm16', 1), ('pcm24', 2), ('pcm16', 1)))]
    L = lib.load_ingest()
    want, want_buf = _stage_one(_ListDataset(paths), [0, 1, 2], device_decode=True)
    with monkeypatch.context() as m:
        m.setattr(L, 'nisqa_ingest_flac_plan', _boom)
        m.setattr(L, 'nisqa_ingest_flac_read', _boom)
        got, buf = _stage_one(_ListDataset(paths), [0, 1, 2], device_decode=True, device_flac=True)
    assert [(g.kind, g.offset, g.nbytes, g.flac) for g in got] == [(g.kind, g.offset, g.nbytes, None) for g in want]
    g = got[0]
    assert np.array_equal(g.clips, want[0].clips) and bytes(buf[g.offset:g.offset + g.nbytes]) == bytes(want_buf[g.offset:g.offset + g.nbytes])


def test_flac_groups_carry_regions_tables_and_the_other_clips(files, tmp_path):
    rng = np.random.default_rng(3)
    wav = wc.write_case(str(tmp_path / 'st.wav'), wc.Case('pcm24', 123, 2, False, -1, rng), 16000)
    short = str(tmp_path / 'short.flac')                             # not eligible: the reader threads decode it into its int16 slot
    x = fc.signal(100, seed=9)
    with open(short, 'wb') as f:
        f.write(flac_enc.encode(x, 16000, 16, blocksize=192))
    names = ['fixed2', 'stereo10', 'bits24', 'number']
    paths = [files[n] for n in names[:2]] + [wav, short] + [files[n] for n in names[2:]]
    (g,), buf = _stage_one(_ListDataset(paths, ms_channel=1), list(range(6)), device_decode=True, device_flac=True)
    S = [fc.by_name(n) for n in names]
    assert g.kind == 'flac' and not g.flac['as_i16'] and g.flac['pos'].tolist() == [0, 1, 4, 5]
    assert g.lengths == [len(S[0].x), len(S[1].x), 123, 100, len(S[2].x), len(S[3].x)]
    t = g.flac['clips']
    assert t.dtype == ingest.FLAC_CLIP and (t['src_off'] % 16 == 0).all()
    assert t['dst_off'].tolist() == [0, g.lengths[0], sum(g.lengths[:4]), sum(g.lengths[:5])]
    assert t['channel'].tolist() == [0, 1, 0, 0] and t['channels'].tolist() == [1, 2, 1, 1] and t['bits'].tolist() == [16, 16, 24, 16]
    assert g.flac['n_rows'] == sum(len(s.sizes) for s in S) and g.flac['frames_off'] + 16 * g.flac['n_rows'] == g.nbytes
    rows = buf[g.offset + g.flac['frames_off']:g.offset + g.nbytes].view(fc.ROW)
    want_rows = [r + (k,) for k, s in enumerate(S) for r in s.rows()]
    assert [tuple(r) for r in rows.tolist()] == want_rows
    for row, s in zip(t, S):
        at = g.offset + int(row['src_off'])
        assert bytes(buf[at:at + int(row['src_bytes'])]) == s.data[s.first_frame:], s
        assert (row['n_samples'], row['n_frames'], row['block_size']) == (len(s.x), len(s.sizes), s.blocksize)
    w = g.clips                                                     # the other two clips: a verbatim WAV chunk and host-decoded int16
    assert len(w) == 2 and w['channels'].tolist() == [2, 1] and w['container'].tolist() == [3, 2] and w['channel'].tolist() == [1, 0]
    assert w['dst_off'].tolist() == [sum(g.lengths[:2]), sum(g.lengths[:3])]
    at = g.offset + int(w['src_off'][1])
    assert np.array_equal(buf[at:at + 200].view(np.int16), x)
    # a group of mono 16-bit clips alone keeps the int16 form
    (g2,), _ = _stage_one(_ListDataset([files['fixed2'], short, files['number']]), [0, 1, 2], device_decode=True, device_flac=True)
    assert g2.kind == 'flac' and g2.flac['as_i16'] and g2.flac['pos'].tolist() == [0, 2] and len(g2.clips) == 1


def test_a_stream_the_read_refuses_is_restaged_on_the_host_path(files, tmp_path):
    x = fc.signal(3 * 192 + 5, seed=6)
    ren = str(tmp_path / 'renumbered.flac')
    with open(ren, 'wb') as f:
        f.write(_renumbered(x))
    (g,), buf = _stage_one(_ListDataset([files['fixed2'], ren, files['stereo10']]), [0, 1, 2], device_decode=True, device_flac=True)
    assert g.kind == 'flac' and g.flac['pos'].tolist() == [0, 2] and len(g.flac['clips']) == 2
    assert len(g.clips) == 1 and g.clips['container'][0] == 2       # decoded by the reader threads into its int16 slot
    at = g.offset + int(g.clips['src_off'][0])
    assert np.array_equal(buf[at:at + 2 * len(x)].view(np.int16), x)
    s = fc.by_name('fixed2')
    cut = str(tmp_path / 'truncated.flac')
    with open(cut, 'wb') as f:
        f.write(s.data[:s.first_frame + s.sizes[0] + s.sizes[1] // 2])
    with pytest.raises(ValueError, match='Could not load file .*truncated.flac'):
        _stage_one(_ListDataset([files['stereo10'], cut]), [0, 1], device_decode=True, device_flac=True)


def test_byte_cap_is_charged_with_the_compressed_bytes():
    frames = np.full(40, 160000, dtype=np.int64)
    srs = np.full(40, 16000, dtype=np.int64)
    widths = np.full(40, 2, dtype=np.int64)
    sizes = np.full(40, 150000, dtype=np.int64)                      # a frame region with its rows: about half the PCM
    pol = ingest.LengthAware(range(40), 1, lambda f, r: np.maximum(1, f // 1600), min_tokens=1 << 30, byte_cap=1 << 20)
    plain, packed = pol.cut_raw(frames, srs, widths, np.ones(40, bool)), pol.cut_raw(frames, srs, widths, np.ones(40, bool), sizes)
    assert max(len(c) for c in plain) == 3 and max(len(c) for c in packed) == 6
    assert all(len(c) * 150000 <= (1 << 20) + (1 << 19) for c in packed)


def test_switches(monkeypatch):
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    monkeypatch.delenv('NISQA_HOST_FLAC', raising=False)
    default = ingest.device_flac_default()
    monkeypatch.setenv('NISQA_HOST_FLAC', '1')
    assert ingest.device_flac_default() is False and ingest.device_decode_default() is True
    monkeypatch.setenv('NISQA_HOST_FLAC', '0')
    assert ingest.device_flac_default() is default
    monkeypatch.setenv('NISQA_HOST_DECODE', '1')
    assert ingest.device_flac_default() is False


def test_check_flac_status_asks_the_host_decoder(files, tmp_path):
    s = fc.by_name('fixed2')
    bad = str(tmp_path / 'bad.flac')
    b = bytearray(s.data)
    b[s.first_frame + s.sizes[0] - 1] ^= 0xFF
    with open(bad, 'wb') as f:
        f.write(bytes(b))
    g = ingest.Group([0, 1], [1, 1], 16000, 0, 0, False, [files['fixed2'], bad], 'flac', None, {'pos': np.array([0, 1])})
    ingest.check_flac_status(g, np.zeros(3, np.int32))
    with pytest.raises(ValueError, match='Could not load file .*bad.flac'):
        ingest.check_flac_status(g, np.array([0, 32, 0], np.int32))
    with pytest.raises(RuntimeError, match='fixed2.flac.*NISQA_HOST_FLAC=1'):
        ingest.check_flac_status(g, np.array([32, 0, 0], np.int32))
    with pytest.raises(RuntimeError, match='names no clip'):
        ingest.check_flac_status(g, np.array([0, 0, 256], np.int32))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------
def test_structs_mirror_the_headers_and_the_entries_are_exported(tmp_path):
    structs = {'nisqa_flac_clip': (lib.FlacClip, 'nisqa_hip.h', 88), 'nisqa_flac_frame': (lib.FlacFrame, 'nisqa_hip.h', 16),
               'nisqa_flac_plan': (lib.FlacPlan, 'nisqa_ingest.h', 64)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "nisqa_hip.h"', '#include "nisqa_ingest.h"', 'int main(void) {']
    for cname, (cls, _, _) in structs.items():
        lines.append('  printf("%s.size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines.append('  printf("bits %d %d %d %d\\n", NISQA_FLAC_BAD_MD5, NISQA_FLAC_BAD_TABLE, NISQA_INGEST_ABI_VERSION, NISQA_ABI_VERSION);')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines) + '\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)])      # (both headers, one unit)
    out = dict(l.split(None, 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, (cls, _, size) in structs.items():
        assert int(out[cname + '.size']) == ctypes.sizeof(cls) == size, cname
        for fname, _ in cls._fields_:
            assert int(out['%s.%s' % (cname, fname)]) == getattr(cls, fname).offset, (cname, fname)
    assert [int(v) for v in out['bits'].split()] == [lib.FLAC_BAD_MD5, lib.FLAC_BAD_TABLE, 2, 2] == [0x80, 0x100, 2, 2]
    assert ingest.FLAC_CLIP.itemsize == 88 and ingest.FLAC_FRAME.itemsize == 16 and ingest.FLAC_PLAN.itemsize == 64 and fc.ROW.itemsize == 16
    for name, n_args in (('nisqa_flac_decode', 16), ('nisqa_flac_workspace_bytes', 4)):
        assert name in lib.SYMBOLS and len(lib.SYMBOLS[name][1]) == n_args
    for name, n_args in (('nisqa_ingest_flac_plan', 5), ('nisqa_ingest_flac_read', 9)):
        assert name in lib.INGEST_SYMBOLS and len(lib.INGEST_SYMBOLS[name][1]) == n_args
    hip = open(os.path.join(ROOT, 'include', 'nisqa_hip.h')).read()
    ing = open(os.path.join(ROOT, 'include', 'nisqa_ingest.h')).read()
    assert re.search(r'^int nisqa_flac_decode\(', hip, re.M) and re.search(r'^size_t nisqa_flac_workspace_bytes\(', hip, re.M)
    assert set(re.findall(r'^\s*int\s+(nisqa_ingest_flac_[a-z0-9_]+)\s*\(', ing, re.M)) == {'nisqa_ingest_flac_plan', 'nisqa_ingest_flac_read'}
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert {'nisqa_flac_decode', 'nisqa_flac_workspace_bytes'} <= set(lib.exported_symbols(lib.LIB_PATH, 'nisqa_flac_'))
    assert {'nisqa_ingest_flac_plan', 'nisqa_ingest_flac_read'} <= set(lib.exported_symbols(lib.INGEST_PATH, 'nisqa_ingest_flac_'))


def test_argument_checks_reject_before_anything_is_launched():
    """Bad sizes and pointers come back as NISQA_ERR_ARG / NISQA_ERR_WORKSPACE from the host half of the entry: no GPU is touched
    (this test runs without one)."""
    L = lib.load()
    W = L.nisqa_flac_workspace_bytes
    assert W(64, 192, 1, 0) == 64 * 192 * 4 + 256 and W(65, 192, 2, 5) == 128 * 192 * 2 * 4 + 512 + 256
    assert W(0, 192, 1, 0) == 0 and W(1, 0, 1, 0) == 0 and W(1, 65536, 1, 0) == 0 and W(1, 192, 3, 0) == 0 and W(1, 192, 1, -1) == 0
    p = lambda v: lib.c_p(v)                                           # noqa: E731  (addresses that are never dereferenced)
    good = [p(4096), 1000, p(8192), 1, p(4096 + 512), 3, 192, 1, 0, p(16384), 600, 0, p(65536), 1 << 20, p(32768), None]
    for k, v in ((0, None), (0, p(4096 + 8)), (1, 0), (2, None), (3, 0), (4, None), (4, p(4096 + 2)), (5, 0), (6, 0), (6, 65536), (7, 0),
                 (7, 3), (9, None), (9, p(16384 + 2)), (10, 0), (11, -1), (12, None), (12, p(65536 + 16)), (14, None)):
        args = list(good)
        args[k] = v
        assert L.nisqa_flac_decode(*args) == lib.NISQA_ERR_ARG, (k, v)
    args = list(good)
    args[13] = W(3, 192, 1, 0) - 1
    assert L.nisqa_flac_decode(*args) == lib.NISQA_ERR_WORKSPACE
    Li = lib.load_ingest()
    assert Li.nisqa_ingest_flac_read(None, 2, None, None, None, None, None, None, 1) == -1
    assert Li.nisqa_ingest_flac_read(None, 0, None, None, None, None, None, None, 1) == 0
