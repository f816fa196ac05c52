"""Resident spectrograms (tr_ds_to_memory), the part that needs no GPU: the ABI of nisqa_mel_gather, the step-order functions
against what the file-fed paths produce, the flag's way into the datasets, and the arena layout and budget from the headers."""
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import melstore_cases as MC
from nisqa_amd import ingest, lib, melstore, synth, trainloop, wavio
from nisqa_amd.engine import BatchPlan
from nisqa_amd.melbank import resampled_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mel_gather_is_declared_exported_and_validates_without_gpu():
    # include/nisqa_train.h declares it, so its row lives in lib.TRAIN_SYMBOLS: the table lib.load() binds next to lib.SYMBOLS
    # (test_host.py holds each table to its own header)
    table = dict(lib.SYMBOLS, **lib.TRAIN_SYMBOLS)
    assert 'nisqa_mel_gather' in lib.TRAIN_SYMBOLS and len(table['nisqa_mel_gather'][1]) == 12
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_train.h')).read()
    assert re.search(r'^int nisqa_mel_gather\s*\(', hdr, re.M)
    assert int(re.search(r'#define NISQA_MEL_GATHER_LDS_CLIPS (\d+)', hdr).group(1)) == lib.MEL_GATHER_LDS_CLIPS
    L = lib.load()
    out = subprocess.check_output(['nm', '-D', '--defined-only', lib.LIB_PATH]).decode()
    assert ' T nisqa_mel_gather' in out
    P = 4096                                                    # non-NULL, 16-byte aligned, never read: every call returns before a launch
    good = [P, 1, P, P, 1, P, P, 1, 1, P, P, None]              # store, store_rows, clip_row, store_floor, n_store, ids, out_frame_off, n, out_frames, out_mel, out_floor, stream
    bad = [(k, None) for k in (0, 2, 3, 5, 6, 9, 10)]           # NULL pointers
    bad += [(7, 0), (7, -1), (4, 0), (4, -3), (8, 0), (8, -1), (1, 0), (1, -5)]      # n, n_store, out_frames, store_rows <= 0
    for k, v in bad:
        a = list(good)
        a[k] = v
        assert L.nisqa_mel_gather(*a) == lib.NISQA_ERR_ARG, (k, v)


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp('melstore_host')
    return d, MC.write_corpus(d)


# batches of 4 over the 14 files: mixed rates and kinds; in [1, 0, 3, 8] and [4, 6, 0, 10] the first file has the batch's rarer rate
BATCHES = [[0, 1, 2, 3], [1, 0, 3, 8], [4, 6, 0, 10], [5, 7, 9, 2], [13, 12, 11, 10], [7, 5], [2, 4, 5, 7]]


@pytest.mark.parametrize('device_decode', [False, True])
def test_single_ended_step_order_is_the_order_the_file_fed_loop_stages(corpus, device_decode):
    d, names = corpus
    ds = MC.dataset(d, names, synth.MOS_ARGS)
    info = ingest.probe_headers(ds, range(len(ds)))
    srs = info['sample_rate'].astype(np.int64)
    assert set(srs.tolist()) == {16000, 48000}
    ing = ingest.Ingest(ds, BATCHES, pin=False, num_workers=1, device_decode=device_decode, device_flac=device_decode)
    staged_ids = []
    try:
        for staged in ing:
            staged_ids.append([i for g in staged.groups for i in g.ids])
            assert [g.sr for g in staged.groups] == [sr for sr, _ in ingest.rate_groups(srs[[i for g in staged.groups for i in g.ids]])]
            ing.ring.release_after(staged.slot, None)
    finally:
        ing.close()
    assert len(staged_ids) == len(BATCHES)
    for b, got in zip(BATCHES, staged_ids):
        b = np.asarray(b)
        assert np.asarray(b)[ingest.step_order(srs[b])].tolist() == got
        first = srs[b[0]]                                        # written out: the first file's rate group leads, batch order inside
        assert got == [i for i in b if srs[i] == first] + [i for i in b if srs[i] != first]
    assert staged_ids[1] == [1, 8, 0, 3] and staged_ids[2] == [4, 6, 0, 10]


def test_double_ended_step_order_is_stage_pairs_sort_key(corpus):
    d, names = corpus
    refs = names[3:] + names[:3]                                  # pairs whose files differ in rate and kind
    ds = MC.dataset(d, names, synth.MOS_ARGS, ref_names=refs)
    deg, ref = melstore.MelStore(None, ds), melstore.MelStore(None, ds.ref_view())
    deg.plan()
    ref.plan()
    kind = lambda it: (int(it[1]), it[0].dtype.str)              # trainloop.stage_pairs' key, from the samples the host readers return
    seen = set()
    for b in BATCHES:
        items = [(ds.load_audio(i), ds.ref_view().load_audio(i)) for i in b]
        want = sorted(range(len(b)), key=lambda k: kind(items[k][0]) + kind(items[k][1]))
        assert trainloop.pair_order(deg.kinds(b), ref.kinds(b)) == want
        assert deg.kinds(b) == [kind(it[0]) for it in items] and ref.kinds(b) == [kind(it[1]) for it in items]
        seen |= set(deg.kinds(b))
    assert seen == {(16000, '<i2'), (48000, '<i2'), (16000, '<f4'), (48000, '<f4')}
    assert any(trainloop.pair_order(deg.kinds(b), ref.kinds(b)) != list(range(len(b))) for b in BATCHES)


@pytest.mark.parametrize('flag', [True, False])
def test_tr_ds_to_memory_reaches_both_datasets(tmp_path, flag):
    from nisqa_amd.NISQA_model import nisqaModel
    rows = [{'db': 'A' if k < 3 else 'B', 'filepath_deg': 'x%d.wav' % k, 'mos': 3.0} for k in range(5)]
    pd.DataFrame(rows).to_csv(tmp_path / 'files.csv', index=False)
    args = dict(synth.MOS_ARGS, mode='main', pretrained_model=False, tr_device='cpu', data_dir=str(tmp_path), csv_file='files.csv',
                csv_con=None, csv_deg='filepath_deg', csv_mos_train='mos', csv_mos_val='mos', csv_db_train=['A'], csv_db_val=['B'],
                tr_ds_to_memory=flag, tr_ds_to_memory_workers=0, ms_channel=None, output_dir=None)
    nm = nisqaModel(args)
    assert nm.ds_train.to_memory is flag and nm.ds_val.to_memory is flag
    assert nm.ds_train.store is None and nm.ds_val.store is None     # nothing happens at construction
    if not flag:
        nm.load_to_memory()                                          # nothing asks for a store: no engine is built, no file is opened
        assert nm.ds_train.store is None


def _independent_frames(ds, names, d):
    """192 x sum of frames from the plans of the files as the host readers load them (one plan per file)."""
    total, per = 0, []
    ms_sr = int(ds.ms_sr) if ds.ms_sr is not None else None
    for nme in names:
        y, sr = wavio.read_wav(str(d / nme))
        n, rate = len(y), sr
        if ms_sr is not None and sr != ms_sr:
            n, rate = int(resampled_lengths([n], sr, ms_sr)[0][0]), ms_sr
        p = BatchPlan([n], int(rate * ds.ms_hop_length), int(ds.seg_hop_length), ds.max_length)
        per.append((p.total_frames, int(p.n_wins[0])))
        total += p.total_frames
    return total, per


@pytest.mark.parametrize('ms_sr', [None, 32000])
def test_arena_bytes_come_from_the_headers_and_the_budget_is_checked_before_any_allocation(corpus, monkeypatch, ms_sr):
    d, names = corpus
    ds = MC.dataset(d, names, dict(synth.MOS_ARGS, ms_sr=ms_sr))
    total, per = _independent_frames(ds, names, d)
    st = melstore.MelStore(None, ds)
    need = st.plan()
    assert need == 192 * total == st.nbytes
    assert list(zip(st.frames.tolist(), st.n_wins.tolist())) == per
    assert st.clip_row.dtype == np.int64 and st.clip_row.tolist() == np.concatenate(([0], np.cumsum([f for f, _ in per]))).tolist()
    calls = []
    monkeypatch.setattr(melstore, '_alloc', lambda *a, **k: calls.append(a) or (_ for _ in ()).throw(AssertionError('allocated')))
    monkeypatch.setenv('NISQA_DS_MEMORY_BYTES', str(need - 1))
    with pytest.raises(RuntimeError) as e:
        melstore.MelStore(None, ds).fill()
    msg = str(e.value)
    assert str(need) in msg and str(need - 1) in msg and 'tr_ds_to_memory: False' in msg
    assert calls == []


def test_an_unreadable_file_raises_the_reference_error_from_the_plan(corpus, tmp_path):
    d, names = corpus
    for n in names[:3]:
        os.symlink(str(d / n), str(tmp_path / n))
    (tmp_path / 'broken.wav').write_bytes(b'RIFF\x00\x00')
    ds = MC.dataset(tmp_path, names[:2] + ['broken.wav', names[2]], synth.MOS_ARGS)
    with pytest.raises(ValueError, match='Could not load file .*broken.wav'):
        melstore.MelStore(None, ds).plan()


def test_batch_tables_are_checked_on_the_host(corpus):
    d, names = corpus
    st = melstore.MelStore(None, MC.dataset(d, names, synth.MOS_ARGS))
    st.plan()
    ids, off = st.offsets([3, 0, 3])
    st.check_table(ids, off)
    with pytest.raises(ValueError, match='entry 1: id 14 is outside'):
        st.offsets([0, 14])
    with pytest.raises(ValueError, match='entry 2: id -1 is outside'):
        st.check_table([3, 0, -1], off)
    bad = off.copy()
    bad[2:] += 1
    with pytest.raises(ValueError, match='entry 1: output span'):
        st.check_table(ids, bad)
    with pytest.raises(ValueError):
        st.check_table([], [0])
