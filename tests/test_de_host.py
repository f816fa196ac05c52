"""NISQA_DE (double-ended) host surface without a GPU: checkpoint loading with strict keys, the refusals of every configuration the
engine does not run, the (degraded, reference) dataset, pair work in the shard planner, the new C entry, and the restatement the GPU
tests use checked against the reference's own Alignment / Fusion / NISQA_DE modules."""
import os
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import de_oracle as DO
from nisqa_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference():
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip('reference tree not staged')
    return ref_shim.import_reference_lib()


def _write_pairs(d, n=3, secs=(1.0, 2.0, 0.6)):
    rows = []
    for k in range(n):
        deg, ref = 'deg_%d.wav' % k, 'ref_%d.wav' % k
        synth.write_wav(os.path.join(d, deg), synth.synth_pcm16(10 + k, secs[k % len(secs)]))
        synth.write_wav(os.path.join(d, ref), synth.synth_pcm16(20 + k, secs[(k + 1) % len(secs)] + 0.5))
        rows.append({'filepath_deg': deg, 'filepath_ref': ref, 'mos': 1.0 + k, 'db': 'x'})
    pd.DataFrame(rows).to_csv(os.path.join(d, 'pairs.csv'), index=False)
    return rows


def _checkpoint(d, args=None, seed=3):
    args = dict(args or DO.DE_ARGS)
    args.update({'pretrained_model': False, 'tr_bs_val': 1, 'tr_num_workers': 0, 'csv_ref': 'filepath_ref'})
    path = os.path.join(str(d), 'rand_de.tar')
    torch.save({'args': args, 'model_state_dict': DO.random_de_state_dict(seed, args['de_fuse'])}, path)
    return path


def _predict_args(d, ckpt, **kw):
    a = {'mode': 'predict_csv', 'pretrained_model': ckpt, 'data_dir': str(d), 'csv_file': 'pairs.csv', 'csv_deg': 'filepath_deg',
         'output_dir': None, 'tr_bs_val': 1, 'tr_num_workers': 0, 'ms_channel': None, 'tr_device': 'cpu'}
    a.update(kw)
    return a


@pytest.mark.parametrize('fuse', DO.FUSES)
def test_de_checkpoint_loads_with_strict_keys(tmp_path, fuse):
    from nisqa_amd.NISQA_model import nisqaModel
    _write_pairs(str(tmp_path))
    m = nisqaModel(_predict_args(tmp_path, _checkpoint(tmp_path, DO.de_args(fuse=fuse))))
    assert m.model.name == 'NISQA_DE' and m.args['double_ended'] is True
    keys = set(m.model.state_dict())
    assert keys == set(DO.random_de_state_dict(3, fuse))
    assert not any(k.startswith(('align.', 'fuse.')) for k in keys)
    assert tuple(m.model.state_dict()['time_dependency_2.model.linear.weight'].shape) == (64, DO.FUSE_WIDTH[fuse])
    for k in ('de_align', 'de_align_apply', 'de_fuse_dim', 'de_fuse'):
        assert k in m.model_args
    # the dataset pairs each row's degraded file with its reference file from csv_ref
    ds = m.ds_val
    assert ds.double_ended and ds.filename_column_ref == 'filepath_ref'
    assert [os.path.basename(ds.file_path(i)) for i in range(3)] == ['deg_0.wav', 'deg_1.wav', 'deg_2.wav']
    assert [os.path.basename(ds.ref_view().file_path(i)) for i in range(3)] == ['ref_0.wav', 'ref_1.wav', 'ref_2.wav']
    y, sr = ds.ref_view().load_audio(1)
    assert sr == 48000 and len(y) == int(1.1 * 48000)


def test_csv_ref_from_the_command_line_wins(tmp_path):
    from nisqa_amd.NISQA_model import nisqaModel
    sys.path.insert(0, ROOT)
    import run_predict
    d = str(tmp_path)
    _write_pairs(d)
    pd.read_csv(os.path.join(d, 'pairs.csv')).rename(columns={'filepath_ref': 'clean'}).to_csv(os.path.join(d, 'pairs.csv'), index=False)
    a = run_predict.build_args(['--mode', 'predict_csv', '--pretrained_model', _checkpoint(d), '--data_dir', d, '--csv_file', 'pairs.csv',
                                '--csv_deg', 'filepath_deg', '--csv_ref', 'clean'])
    assert a['csv_ref'] == 'clean'
    a['tr_device'] = 'cpu'
    assert os.path.basename(nisqaModel(a).ds_val.ref_view().file_path(0)) == 'ref_0.wav'
    b = run_predict.build_args(['--mode', 'predict_csv', '--pretrained_model', 'x.tar', '--csv_file', 'a.csv', '--csv_deg', 'f'])
    assert 'csv_ref' not in b                                   # absent: the checkpoint's own csv_ref is kept


@pytest.mark.parametrize('key,value,word', [
    ('de_align', 'bahd', 'bahd'), ('de_align', 'luong', 'luong'), ('de_align', 'distance', 'distance'), ('de_align', 'none', 'none'),
    ('de_fuse_dim', 32, 'de_fuse_dim'), ('td_2', 'lstm', 'td_2'), ('td_2', 'skip', 'td_2'), ('td', 'lstm', 'td'),
    ('pool', 'avg', 'pool'), ('cnn_model', 'standard', 'cnn_model'), ('td_2_sa_nhead', 2, 'td_2_sa_nhead'),
    ('td_sa_pos_enc', True, 'td_sa_pos_enc'), ('cnn_pool_3', [6, 4], 'CNN geometry'), ('de_align_apply', 'sharp', 'sharp'),
    ('de_fuse', 'x*y', 'x\\*y')])
def test_out_of_scope_de_options_raise_naming_the_option(key, value, word):
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import check_de_args
    args = dict(DO.DE_ARGS, **{key: value})
    with pytest.raises(NotImplementedError, match=word):
        check_de_args(args)
    with pytest.raises(NotImplementedError, match=word):
        NL.NISQA_DE(**DO.model_kwargs(args))
    with pytest.raises(NotImplementedError, match='bf16x3'):
        check_de_args(DO.DE_ARGS, 'bf16x3')
    check_de_args(DO.DE_ARGS, 'f16x4')                          # in scope: no exception


def test_de_checkpoint_out_of_scope_option_refused_at_load(tmp_path):
    from nisqa_amd.NISQA_model import nisqaModel
    _write_pairs(str(tmp_path))
    with pytest.raises(NotImplementedError, match='luong'):
        nisqaModel(_predict_args(tmp_path, _checkpoint(tmp_path, DO.de_args(align='luong'))))


def test_de_training_and_single_file_modes_refuse(tmp_path):
    from nisqa_amd.NISQA_model import nisqaModel
    args = dict(DO.DE_ARGS, mode='main', pretrained_model=False, tr_device='cpu')
    with pytest.raises(NotImplementedError, match='training'):
        nisqaModel(args)
    from nisqa_amd.train import HipTrainer
    with pytest.raises(NotImplementedError):
        HipTrainer(DO.DE_ARGS, DO.random_de_state_dict(1), "cpu")
    _write_pairs(str(tmp_path))
    ck = _checkpoint(tmp_path)
    with pytest.raises(NotImplementedError, match='predict_file'):
        nisqaModel({'mode': 'predict_file', 'pretrained_model': ck, 'deg': os.path.join(str(tmp_path), 'deg_0.wav'),
                    'output_dir': None, 'tr_bs_val': 1, 'tr_num_workers': 0, 'ms_channel': None, 'tr_device': 'cpu'})
    with pytest.raises(NotImplementedError, match='predict_dir'):
        nisqaModel({'mode': 'predict_dir', 'pretrained_model': ck, 'data_dir': str(tmp_path), 'output_dir': None, 'tr_bs_val': 1,
                    'tr_num_workers': 0, 'ms_channel': None, 'tr_device': 'cpu'})
    with pytest.raises(ValueError, match='csv_ref'):
        a = _predict_args(tmp_path, ck)
        torch.save(dict(torch.load(ck, weights_only=False), args=dict(torch.load(ck, weights_only=False)['args'], csv_ref=None)), ck)
        nisqaModel(a)


def test_pair_work_counts_both_files_in_the_shard_planner(tmp_path):
    from nisqa_amd import NISQA_lib as NL, dist
    d = str(tmp_path)
    _write_pairs(d, n=3, secs=(1.0, 2.0, 0.6))
    df = pd.read_csv(os.path.join(d, 'pairs.csv'))
    ds = NL.SpeechQualityDataset(df, data_dir=d, filename_column='filepath_deg', mos_column='predict_only', max_length=1300,
                                 seg_hop_length=4, ms_hop_length=0.01, ms_win_length=0.02, ms_n_mels=48, ms_sr=None,
                                 double_ended=True, filename_column_ref='filepath_ref')
    tok = NL.pair_tokens(ds, range(3))
    deg = NL.tokens_of(ds, [48000, 96000, int(0.6 * 48000)], [48000] * 3)
    ref = NL.tokens_of(ds, [120000, int(1.1 * 48000), 72000], [48000] * 3)
    assert list(tok) == list(deg + ref)
    assert dist.balanced_bounds(tok, 2) == dist.balanced_bounds(deg + ref, 2)
    with pytest.raises(ValueError, match='filename_column_ref'):
        NL.SpeechQualityDataset(df, data_dir=d, filename_column='filepath_deg', double_ended=True)


def test_de_align_entry_is_declared_and_exported():
    from nisqa_amd import lib
    assert 'nisqa_de_align_fuse' in lib.SYMBOLS
    assert 'nisqa_de_align_fuse' in open(os.path.join(ROOT, 'include', 'nisqa_hip.h')).read()
    if not os.path.isfile(lib.LIB_PATH):
        pytest.skip('library not built')
    assert 'nisqa_de_align_fuse' in lib.exported_symbols(lib.LIB_PATH, 'nisqa_')


@pytest.mark.parametrize('in_features', [192, 128])
def test_narrow_projection_packs_as_zero_extended_384(in_features):
    from nisqa_amd import weights as W
    sd = DO.random_de_state_dict(5, 'x/y/-' if in_features == 192 else 'x/y')
    pfx = 'time_dependency_2.model.'
    wide = dict(sd)
    w = torch.zeros(64, 384)
    w[:, :in_features] = sd[pfx + 'linear.weight']
    wide[pfx + 'linear.weight'] = w
    assert np.array_equal(W.pack_self_att(sd, 2, pfx, in_features=in_features), W.pack_self_att(wide, 2, pfx))
    assert np.array_equal(W.pack_self_att_bf16(sd, 2, pfx, terms=3, in_features=in_features),
                          W.pack_self_att_bf16(wide, 2, pfx, terms=3))
    with pytest.raises(NotImplementedError, match='Linear'):
        W.pack_self_att(sd, 2, pfx)                              # the 384 default refuses a narrower checkpoint


@pytest.mark.parametrize('align', DO.ALIGNS)
@pytest.mark.parametrize('apply', DO.APPLIES)
@pytest.mark.parametrize('fuse', DO.FUSES)
def test_numpy_restatement_equals_reference_alignment_and_fusion(align, apply, fuse):
    NL = _reference()
    rng = np.random.RandomState(1)
    B, Lx, Ly = 3, 40, 50
    x = rng.standard_normal((B, Lx, 64)).astype(np.float32)
    y = rng.standard_normal((B, Ly, 64)).astype(np.float32)
    x[1, 3] = 0.0                                               # a zero row (cosine: the 1e-8 clamp)
    ny = np.array([50, 1, 17])
    al = NL.Alignment(align, apply, q_dim=64, y_dim=64).eval()
    fu = NL.Fusion(in_feat=64, fuse_dim=None, fuse=fuse).eval()
    with torch.no_grad():
        ref = fu(torch.from_numpy(x), al(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(ny))).numpy()
    for b in range(B):
        got, idx, gap = DO.align_fuse(x[b].astype(np.float64), y[b, :ny[b]].astype(np.float64), align, apply, fuse)
        assert np.abs(got - ref[b]).max() < 1e-5, (b, np.abs(got - ref[b]).max())
        if apply == 'hard':
            ridx = al.apply_att.idx[b].numpy()
            sure = gap > 1e-5
            assert (idx[sure] == ridx[sure]).all()


@pytest.mark.parametrize('align,apply,fuse', [('cosine', 'hard', 'x/y/-'), ('dot', 'soft', '+/-'), ('cosine', 'soft', 'x/y')])
def test_restated_forward_equals_reference_nisqa_de(align, apply, fuse):
    """The whole double-ended forward of de_oracle (float32) against the reference's NISQA_DE on padded batches of random segments."""
    NL = _reference()
    args = DO.de_args(align, apply, fuse)
    sd = DO.random_de_state_dict(4, fuse)
    model = NL.NISQA_DE(**DO.model_kwargs(args))
    model.load_state_dict(sd, strict=True)
    model.eval()
    rng = np.random.RandomState(2)
    n = [(9, 12), (12, 1), (1, 7)]
    L = 12
    x = np.zeros((3, L, 2, 48, 15), np.float32)
    for b, (nx, ny) in enumerate(n):
        x[b, :nx, 0] = rng.standard_normal((nx, 48, 15)) * 10 - 40
        x[b, :ny, 1] = rng.standard_normal((ny, 48, 15)) * 10 - 40
    with torch.no_grad():
        ref = model(torch.from_numpy(x), torch.tensor(n)).numpy().reshape(-1)
    for b, (nx, ny) in enumerate(n):
        got = DO.forward_segments(sd, args, x[b, :nx, 0:1], x[b, :ny, 1:2], dtype=torch.float32)
        assert abs(got - ref[b]) < 1e-4, (b, got, ref[b])
