"""Resident spectrograms (tr_ds_to_memory) on the GPU: nisqa_mel_gather against numpy, the fill against the mel front end clip by
clip, the step inputs against what the file-fed loops stage, training without files, validation rows, and the whole loop against
the file-fed loop."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import de_oracle as DO
import lstm_train_oracle as LT
import melstore_cases as MC
from nisqa_amd import NISQA_lib as NL
from nisqa_amd import ingest, lib, melstore, synth, trainloop
from nisqa_amd.engine import HipNisqa
from nisqa_amd.train import HipTrainer

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = np.float32(-7.25)                                        # what output buffers hold before a launch
GUARD = 8                                                       # rows / floors behind the output that must stay as they were

# nisqa_mel_gather runs 256-thread workgroups, one 16-byte unit per thread and trip, twelve units per row: in id order 4, 5, 6 the
# clips of 21, 22 and 21 rows end at units 252 (one row-unit group before the workgroup edge 256), 516 (just behind the edge 512) and
# 768 (exactly on an edge)
FRAMES = [1, 15, 16, 17, 21, 22, 21, 1000, 2]


def _store_arrays(seed=5):
    rng = np.random.default_rng(seed)
    rows = np.concatenate(([0], np.cumsum(FRAMES))).astype(np.int64)
    arena = rng.standard_normal((int(rows[-1]), 48)).astype(np.float32)
    arena[3, 7], arena[40, 0] = np.float32('inf'), np.float32(-0.0)              # bit patterns a copy must keep
    floors = rng.standard_normal(len(FRAMES)).astype(np.float32)
    return arena, rows, floors


def _launch(dev, ids, off, n=None, out_frames=None):
    """nisqa_mel_gather through the raw ABI on sentinel-filled outputs with guard rows -> (out_mel, out_floor) on the host."""
    arena, rows, floors = dev
    L = lib.load()
    n = len(ids) if n is None else n
    out_frames = int(off[-1]) if out_frames is None else out_frames
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    ids_d, off_d = t(np.asarray(ids, np.int32)), t(np.asarray(off, np.int32))
    out = torch.full((out_frames + GUARD, 48), float(SENT), dtype=torch.float32, device=DEV)
    fl = torch.full((n + GUARD,), float(SENT), dtype=torch.float32, device=DEV)
    rc = L.nisqa_mel_gather(arena.data_ptr(), arena.shape[0], rows.data_ptr(), floors.data_ptr(), len(FRAMES), ids_d.data_ptr(),
                            off_d.data_ptr(), n, out_frames, out.data_ptr(), fl.data_ptr(),
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == lib.NISQA_OK
    torch.cuda.synchronize()
    return out.cpu().numpy(), fl.cpu().numpy()


@pytest.fixture(scope='module')
def dev_store():
    arena, rows, floors = _store_arrays()
    return (torch.from_numpy(arena).to(DEV), torch.from_numpy(rows).to(DEV), torch.from_numpy(floors).to(DEV)), (arena, rows, floors)


_rng = np.random.default_rng(9)
ID_LISTS = {'one': [0], 'reverse': list(range(8, -1, -1)), 'edges': [4, 5, 6, 0, 1, 2, 3, 7, 8], 'repeat': [2, 7, 2, 8, 2, 0, 0],
            'over_lds_cap': _rng.integers(0, 9, lib.MEL_GATHER_LDS_CLIPS + 1).tolist()}


@pytest.mark.parametrize('case', list(ID_LISTS))
def test_gather_kernel_equals_numpy_bit_for_bit(dev_store, case):
    dev, (arena, rows, floors) = dev_store
    ids = ID_LISTS[case]
    off = np.concatenate(([0], np.cumsum([FRAMES[i] for i in ids]))).astype(np.int64)
    if case == 'edges':
        assert [int(o) * 12 for o in off[1:4]] == [252, 516, 768]
    if case == 'over_lds_cap':
        assert int(off[-1]) * 12 > 2048 * 256                     # more units than one trip of the largest grid
    out, fl = _launch(dev, ids, off)
    want = np.concatenate([arena[rows[i]:rows[i + 1]] for i in ids])
    total = int(off[-1])
    assert out[:total].view(np.uint32).tobytes() == want.view(np.uint32).tobytes()
    assert fl[:len(ids)].view(np.uint32).tobytes() == floors[ids].view(np.uint32).tobytes()
    assert (out[total:] == SENT).all() and (fl[len(ids):] == SENT).all()      # nothing behind the spans is touched


def test_gather_kernel_skips_what_it_cannot_trust(dev_store):
    dev, (arena, rows, floors) = dev_store
    ids = [1, 9, 3, 2, 8]                                         # entry 1: id out of range; entry 3: a span one row short of clip 2
    spans = [FRAMES[1], 5, FRAMES[3], FRAMES[2] - 1, FRAMES[8]]
    off = np.concatenate(([0], np.cumsum(spans))).astype(np.int64)
    out, fl = _launch(dev, ids, off)
    for c, i in enumerate(ids):
        got = out[off[c]:off[c + 1]]
        if c in (1, 3):
            assert (got == SENT).all() and np.isnan(fl[c])
        else:
            assert got.view(np.uint32).tobytes() == arena[rows[i]:rows[i + 1]].view(np.uint32).tobytes() and fl[c] == floors[i]
    assert (out[int(off[-1]):] == SENT).all() and (fl[len(ids):] == SENT).all()
    out, fl = _launch(dev, [-1, 0], [0, 4, 4 + FRAMES[0]])
    assert (out[:4] == SENT).all() and np.isnan(fl[0]) and fl[1] == floors[0] and (out[4] == arena[0]).all()


# ---- the fill ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp('melstore_gpu')
    return d, MC.write_corpus(d)


@pytest.fixture(scope='module')
def sd_mos():
    return synth.random_state_dict(7, 'NISQA')


def _alone(eng, ds, i):
    """(mel, floor, n_wins) of item i computed on its own from the samples the host readers return"""
    y, sr = ds.load_audio(i)
    plan = eng.audio_plan([len(y)], sr)
    pcm = eng.resample(torch.from_numpy(y).to(eng.device), [len(y)], sr)
    mel, floor = eng.mel(pcm, plan, eng.rate(sr), clamp=False)
    return mel.cpu().numpy(), floor.cpu().numpy(), int(plan.n_wins[0])


@pytest.mark.parametrize('ms_sr', [None, 32000])
def test_fill_holds_every_clip_as_the_front_end_computes_it_alone(corpus, sd_mos, ms_sr, capsys, monkeypatch):
    d, names = corpus
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    monkeypatch.delenv('NISQA_HOST_FLAC', raising=False)
    monkeypatch.delenv('NISQA_DS_MEMORY_BYTES', raising=False)
    args = dict(synth.MOS_ARGS, ms_sr=ms_sr)
    eng = HipNisqa(args, sd_mos, DEV)
    ds = MC.dataset(d, names, args)
    st = melstore.MelStore(eng, ds).fill()
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('tr_ds_to_memory:')]
    assert len(line) == 1 and '%d clips' % len(names) in line[0] and '%d bytes' % st.nbytes in line[0]
    assert st.arena.shape == (int(st.clip_row[-1]), 48) and st.arena.dtype == torch.float32 and st.floor.shape == (len(names),)
    assert st.clip_row_dev.cpu().numpy().tolist() == st.clip_row.tolist()
    arena, floors = st.arena.cpu().numpy(), st.floor.cpu().numpy()
    for i in range(len(names)):
        mel, floor, n_wins = _alone(eng, ds, i)
        got = arena[st.clip_row[i]:st.clip_row[i + 1]]
        assert got.shape == mel.shape and got.view(np.uint32).tobytes() == mel.view(np.uint32).tobytes(), names[i]
        assert floors[i:i + 1].view(np.uint32).tobytes() == floor.view(np.uint32).tobytes(), names[i]
        assert int(st.n_wins[i]) == n_wins
    # an item served from the store is the item the file path gives
    ds.bind_engine(lambda: eng)
    x_file = ds[4]
    ds.store = st
    x_res = ds[4]
    assert torch.equal(x_file[0], x_res[0]) and int(x_file[2][1]) == int(x_res[2][1])


# ---- step inputs --------------------------------------------------------------------------------------------------------
def _same(a, b):
    (m0, o0, n0, f0), (m1, o1, n1, f1) = a, b
    assert torch.equal(m0.view(torch.int32), m1.view(torch.int32)) and torch.equal(f0.view(torch.int32), f1.view(torch.int32))
    assert o0.dtype == o1.dtype == torch.int32 and torch.equal(o0, o1)
    assert np.asarray(n0).tolist() == np.asarray(n1).tolist()


def test_store_batches_are_the_step_inputs_of_the_file_fed_loops(corpus, sd_mos, monkeypatch):
    d, names = corpus
    monkeypatch.delenv('NISQA_HOST_DECODE', raising=False)
    monkeypatch.delenv('NISQA_HOST_FLAC', raising=False)
    tr = HipTrainer(dict(synth.MOS_ARGS), sd_mos, DEV)
    refs = names[3:] + names[:3]                                   # pairs that differ in rate and kind
    ds = MC.dataset(d, names, synth.MOS_ARGS)
    ds2 = MC.dataset(d, names, synth.MOS_ARGS, ref_names=refs)
    deg, ref = melstore.MelStore(tr.eng, ds).fill(), melstore.MelStore(tr.eng, ds2.ref_view()).fill()
    rng = np.random.default_rng(17)
    n_batches = 0
    for _ in range(2):
        perm = rng.permutation(len(names))
        batches = [perm[s:s + 4].tolist() for s in range(0, len(perm), 4)]
        # single-ended: what trainloop.train stages for these batches
        ing = ingest.Ingest(ds, batches, pin=True, num_workers=2, device_decode=True, device_flac=True)
        try:
            for b, staged in zip(batches, ing):
                ids, groups = trainloop.stage_groups(tr, ds, ing, staged)
                mine = np.asarray(b)[ingest.step_order(deg.sr[b])]
                assert mine.tolist() == ids.tolist()
                _same(deg.batch(mine), tr._mel_groups(groups))
                n_batches += 1
        finally:
            ing.close()
        # double-ended: both sides of what stage_pairs stages
        for b in batches:
            ids, g_deg, g_ref = trainloop.stage_pairs(tr, ds2, b)
            mine = np.asarray(b)[trainloop.pair_order(deg.kinds(b), ref.kinds(b))]
            assert mine.tolist() == ids.tolist()
            _same(deg.batch(mine), tr._mel_groups(g_deg))
            _same(ref.batch(mine), tr._mel_groups(g_ref))
    assert n_batches == 8
    with pytest.raises(ValueError, match='entry 1: id 99'):
        deg.batch([0, 99])


# ---- the loops ------------------------------------------------------------------------------------------------------------
_LOOP = {'tr_epochs': 2, 'tr_early_stop': 20, 'tr_bs': 4, 'tr_bs_val': 4, 'tr_lr': 1e-3, 'tr_lr_patience': 15, 'tr_num_workers': 2,
         'tr_parallel': False, 'tr_ds_to_memory_workers': 0, 'tr_device': None, 'tr_checkpoint': 'every_epoch', 'tr_verbose': 0,
         'tr_bias_mapping': None, 'tr_bias_min_r': None, 'tr_bias_anchor_db': None, 'ms_channel': None, 'pretrained_model': False,
         'csv_con': None, 'csv_deg': 'filepath_deg', 'csv_mos_train': 'mos', 'csv_mos_val': 'mos', 'csv_file': 'files.csv'}


def _tiny_corpus(d, seed, double_ended=False, mixed=False):
    """The tiny-corpus recipe of the training-loop tests (7 + 6 training files, 5 validation files of 0.5-1.6 s; with ``mixed`` every
    third file at 16 kHz), as (deg, ref) pairs when double_ended -> the audio files written."""
    rng = np.random.default_rng(seed)
    d.mkdir()
    rows, files = [], []
    for db, n in (('TRAIN_A', 7), ('TRAIN_B', 6), ('VAL_A', 5)):
        for i in range(n):
            row = {'db': db, **{t: float(rng.uniform(1, 5)) for t in ('mos', 'noi', 'dis', 'col', 'loud')}}
            for col, base in (('filepath_deg', 100), ('filepath_ref', 300))[:2 if double_ended else 1]:
                name = '%s_%s_%d.wav' % (col[-3:], db, i)
                sr = 16000 if mixed and len(rows) % 3 == 1 else 48000
                synth.write_wav(str(d / name), synth.synth_pcm16(base + len(rows), float(rng.uniform(0.5, 1.6)), sr=sr), sr)
                row[col] = name
                files.append(d / name)
            rows.append(row)
    pd.DataFrame(rows).to_csv(d / 'files.csv', index=False)
    return files


def _loop_args(kind, d, out, to_memory):
    base = {'dim': synth.DIM_ARGS, 'mos': synth.MOS_ARGS, 'lstm': LT.AVG_ARGS, 'de': DO.DE_ARGS}[kind]
    args = dict(base, **_LOOP)
    args.update({'name': 'tiny_' + kind, 'mode': 'main', 'data_dir': str(d), 'output_dir': str(out), 'tr_ds_to_memory': to_memory,
                 'csv_db_train': ['TRAIN_A', 'TRAIN_B'], 'csv_db_val': ['VAL_A']})
    if kind == 'de':
        args['csv_ref'] = 'filepath_ref'
    return args


@pytest.mark.parametrize('kind', ['dim', 'lstm', 'de'])
def test_training_opens_no_file_after_load_to_memory(tmp_path, capsys, kind):
    from nisqa_amd.NISQA_model import nisqaModel
    d = tmp_path / 'corpus'
    files = _tiny_corpus(d, 12, double_ended=kind == 'de')
    torch.manual_seed(3)
    nm = nisqaModel(_loop_args(kind, d, tmp_path / 'out', True))
    assert nm.ds_train.to_memory and nm.ds_val.to_memory and nm.ds_train.store is None
    nm.load_to_memory()
    assert nm.ds_train.store.filled and nm.ds_val.store.filled and (nm.ds_train.ref_store is not None) == (kind == 'de')
    for f in files:
        os.unlink(str(f))
    nm.train()
    out = capsys.readouterr().out
    assert len(re.findall(r'^tr_ds_to_memory: \d+ clips', out, re.M)) == (4 if kind == 'de' else 2)     # one fill per store, none by train()
    assert '--> Training done.' in out and out.count('ep 1 sec') == 1 and out.count('ep 2 sec') == 1
    run_dir = tmp_path / 'out' / nm.runname
    hist = pd.read_csv(run_dir / (nm.runname + '__results.csv'))
    assert len(hist) == 2 and np.isfinite(hist['loss'].astype(float)).all()
    c = torch.load(str(run_dir / (nm.runname + '__ep_002.tar')), map_location='cpu', weights_only=False)
    assert c['epoch'] == 2 and int(c['model_state_dict']['cnn.model.bn1.num_batches_tracked']) == (16 if kind == 'de' else 8)
    cls = {'dim': NL.NISQA_DIM, 'lstm': NL.NISQA, 'de': NL.NISQA_DE}[kind]
    cls(**c['model_args']).load_state_dict(c['model_state_dict'], strict=True)       # loadable
    assert np.isfinite(nm.ds_val.df['mos_pred'].to_numpy(dtype=np.float64)).all()


@pytest.mark.parametrize('kind', ['mos', 'dim', 'lstm', 'de'])
def test_resident_validation_rows_equal_the_file_fed_rows(corpus, kind, monkeypatch):
    d, names = corpus
    monkeypatch.delenv('NISQA_EXACT_BS', raising=False)
    args = dict({'dim': synth.DIM_ARGS, 'mos': synth.MOS_ARGS, 'lstm': LT.AVG_ARGS, 'de': DO.DE_ARGS}[kind])
    sd = {'de': lambda: DO.random_de_state_dict(3), 'dim': lambda: synth.random_state_dict(11, 'NISQA_DIM'),
          'mos': lambda: synth.random_state_dict(11, 'NISQA'), 'lstm': lambda: None}[kind]()
    model = {'dim': NL.NISQA_DIM, 'mos': NL.NISQA, 'lstm': NL.NISQA, 'de': NL.NISQA_DE}[kind](
        **{k: v for k, v in args.items() if k not in ('model', 'name')})
    if sd is None:
        torch.manual_seed(5)
        NL.init_parameters_(model)
    else:
        model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.bind_args(args)
    refs = (names[3:] + names[:3]) if kind == 'de' else None
    predict = NL.predict_dim if kind == 'dim' else NL.predict_mos
    cols = ['mos_pred', 'noi_pred', 'dis_pred', 'col_pred', 'loud_pred'] if kind == 'dim' else ['mos_pred']
    ds_file = MC.dataset(d, names, args, ref_names=refs, dim=kind == 'dim')
    seen_file, seen_res = [], []
    y_file, _ = predict(model, ds_file, 4, DEV, num_workers=2, on_rows=lambda ids, rows: seen_file.extend(int(i) for i in ids))
    ds_res = MC.dataset(d, names, args, ref_names=refs, dim=kind == 'dim', to_memory=True)
    eng = model.engine(DEV)
    eng = getattr(eng, 'base', eng)
    ds_res.store = melstore.MelStore(eng, ds_res).fill()
    if kind == 'de':
        ds_res.ref_store = melstore.MelStore(eng, ds_res.ref_view()).fill()
    monkeypatch.setattr(ingest, 'Ingest', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the file feed ran')))
    monkeypatch.setattr(ds_res, 'load_audio', lambda *a, **k: (_ for _ in ()).throw(AssertionError('a file was read')))
    y_res, _ = predict(model, ds_res, 4, DEV, num_workers=2, on_rows=lambda ids, rows: seen_res.extend(int(i) for i in ids))
    assert y_res.shape == y_file.shape == (len(names), len(cols)) and np.isfinite(y_res).all()
    assert y_res.view(np.uint32).tobytes() == y_file.view(np.uint32).tobytes()
    assert sorted(seen_res) == sorted(seen_file) == list(range(len(names)))
    for c in cols:
        assert list(ds_res.df.columns) == list(ds_file.df.columns)
        assert ds_res.df[c].to_numpy().tobytes() == ds_file.df[c].to_numpy().tobytes()
    monkeypatch.setenv('NISQA_EXACT_BS', '1')                      # other batches, the same rows
    y_exact, _ = predict(model, ds_res, 4, DEV)
    assert y_exact.view(np.uint32).tobytes() == y_file.view(np.uint32).tobytes()


def test_resident_loop_trains_what_the_file_fed_loop_trains(tmp_path):
    """The same corpus (two rates) and seed three times: file-fed, file-fed again, resident.  The resident run may differ from a
    file-fed run by no more than the two file-fed runs differ from each other: exactly equal where they are equal, and within
    4 x their largest difference per tensor (one more draw from the same noise) where they are not.  Both spreads are printed.

    MEASURED, AND NOT HELD: the step is not run-to-run deterministic on the MI355X (atomic reductions in the weight
    gradients; Adam turns noise-level gradients into +-lr steps), and the per-tensor 4 x bound does not hold between FILE-FED runs
    either.  Three file-fed runs differed pairwise by 2.8e-3 / 9.8e-4 / 3.8e-3 at most over the state_dict (epoch loss 1.5e-8 ..
    2.2e-7), three resident runs by 4.6e-3 / 3.4e-3 / 1.2e-3, resident against file-fed by 3.9e-4 .. 5.4e-3 (loss 6e-8 .. 7e-6);
    the third file-fed run missed the bound against the first two on 2 of 78 tensors (tensors the first two agreed on bit for
    bit), the resident runs on 6 / 59 / 7 of 78.  In this test's own runs: pool.model.linear1.bias 5.1e-7 against 4 x 6.7e-8;
    cnn.model.bn2.weight 6.0e-8 and time_dependency.model.layers.0.norm2.weight 1.2e-7 against 4 x 0 (tensors on which the two
    file-fed runs happened to agree); in a run where the file-fed pair was 3.4e-3 apart overall and the resident run 2.1e-3.
    Four trainers fed the same eight batches (file-staged, store, file-staged, store) are bit-identical in loss and y_hat at step
    0 and 1e-7 apart in y_hat from step 1 on, whichever feed.  What pins the feed: every step's inputs and the validation rows are
    bit for bit the file-fed ones (the tests above)."""
    from nisqa_amd.NISQA_model import nisqaModel
    d = tmp_path / 'corpus'
    _tiny_corpus(d, 12, mixed=True)
    runs = []
    for tag, to_memory in (('file_a', False), ('file_b', False), ('resident', True)):
        torch.manual_seed(3)
        nm = nisqaModel(_loop_args('mos', d, tmp_path / ('out_' + tag), to_memory))
        nm.train()
        run_dir = tmp_path / ('out_' + tag) / nm.runname
        hist = pd.read_csv(run_dir / (nm.runname + '__results.csv'))
        c = torch.load(str(run_dir / (nm.runname + '__ep_002.tar')), map_location='cpu', weights_only=False)
        sd = {k: v.double().numpy() for k, v in c['model_state_dict'].items()}
        sd['loss per epoch'] = hist['loss'].to_numpy(dtype=np.float64)
        sd['validation rows'] = nm.ds_val.df['mos_pred'].to_numpy(dtype=np.float64)
        runs.append(sd)
    a, b, r = runs
    spread_files = {k: float(np.abs(a[k] - b[k]).max()) for k in a}
    spread_res = {k: max(float(np.abs(r[k] - a[k]).max()), float(np.abs(r[k] - b[k]).max())) for k in a}
    print('file-fed vs file-fed: max over tensors %.3g (loss %.3g); resident vs file-fed: max over tensors %.3g (loss %.3g)' % (
        max(spread_files.values()), spread_files['loss per epoch'], max(spread_res.values()), spread_res['loss per epoch']))
    for k in a:
        assert float(np.abs(r[k] - a[k]).max()) <= 4 * spread_files[k], (k, spread_res[k], spread_files[k])
