"""NISQA_DE training, host side without a GPU: the float64 restatement of the step (tests/de_train_oracle.py) against the
reference's own modules in train mode, the trainer dispatch, the argument check and the C entries."""
import os
import re

import numpy as np
import pytest
import torch

import de_oracle as DO
import de_train_oracle as DT
import lstm_train_oracle as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference():
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip('reference tree not staged')
    return ref_shim.import_reference_lib()


@pytest.mark.parametrize('align,fuse', [('cosine', 'x/y/-'), ('dot', '+/-'), ('cosine', 'x/y')])
def test_oracle_step_matches_the_reference_modules_in_train_mode(align, fuse):
    """Dropout 0, float64 on both sides: loss, y_hat and every gradient to 1e-9 of the tensor's largest entry (the conv biases'
    gradients are zero in exact arithmetic under train-mode BatchNorm, and so is that of the pooling score's bias, which the
    softmax cancels: rounding noise on both sides, held below 1e-12), the
    BatchNorm buffers after the step's TWO updates, num_batches_tracked + 2."""
    from oracle import net as onet
    NL = _reference()
    import pandas as pd
    args = DT.de_train_args(align, fuse)
    sd0 = DO.random_de_state_dict(33, fuse)
    fd, fr = [15, 97, 40], [40, 97, 15]
    specs_d, y = LT.batch(93, fd)
    specs_r, _ = LT.batch(1093, fr)
    model = NL.NISQA_DE(**DO.model_kwargs(args))
    model.load_state_dict(sd0, strict=True)
    model.double().train()
    seg = lambda s, L: onet.segment_specs(s, args['ms_seg_length'], args['ms_seg_hop_length'], L)
    nw = np.array([[seg(d, None)[1], seg(r, None)[1]] for d, r in zip(specs_d, specs_r)])
    L = int(nw.max())
    x = torch.stack([torch.cat([torch.as_tensor(seg(d, L)[0]), torch.as_tensor(seg(r, L)[0])], 1) for d, r in zip(specs_d, specs_r)])
    y_hat = model(x.double(), torch.as_tensor(nw))
    loss = NL.biasLoss(pd.Series(['db'] * 3), anchor_db=None, mapping=None, min_r=None, do_print=False).get_loss(
        torch.as_tensor(y).double(), y_hat, np.arange(3))
    loss.backward()

    segs_d, nw_d = DT.segments(specs_d, args)
    segs_r, nw_r = DT.segments(specs_r, args)
    assert nw_d.tolist() == nw[:, 0].tolist() and nw_r.tolist() == nw[:, 1].tolist()
    got = DT.train_step(sd0, args, segs_d, nw_d, segs_r, nw_r, y)
    assert got['gap'] > 1e-6                                       # no argmax of this batch sits on a tie
    assert abs(got['loss'] - float(loss.detach())) <= 1e-9 * abs(float(loss.detach()))
    np.testing.assert_allclose(got['y_hat'], y_hat.detach().numpy(), rtol=1e-9, atol=0)
    for k, p in model.named_parameters():
        want, g = p.grad.numpy(), got['grads'][k]
        if re.match(r'cnn\.model\.conv\d\.bias', k) or k == 'pool.model.linear2.bias':
            assert np.abs(want).max() < 1e-12 and np.abs(g).max() < 1e-12, k
        else:
            assert np.abs(g - want).max() <= 1e-9 * np.abs(want).max(), (k, np.abs(g - want).max(), np.abs(want).max())
    sd1 = model.state_dict()
    for k, v in got['bufs'].items():
        np.testing.assert_allclose(v, sd1[k].numpy(), rtol=1e-10, atol=1e-12, err_msg=k)
    for i in range(1, 7):
        k = 'cnn.model.bn%d.num_batches_tracked' % i
        assert int(sd1[k]) == int(sd0[k]) + 2


def test_pooled_batchnorm_is_a_different_model():
    """the oracle's wrong-on-purpose variant (one CNN pass over all 2B clips) is far from the step: the GPU test that guards the
    two-call semantics has something to tell apart"""
    args = DT.de_train_args()
    sd0 = DO.random_de_state_dict(33)
    specs_d, y = LT.batch(93, [15, 97])
    specs_r, _ = LT.batch(1093, [40, 97])
    segs_d, nw_d = DT.segments(specs_d, args)
    segs_r, nw_r = DT.segments(specs_r, args)
    a = DT.train_step(sd0, args, segs_d, nw_d, segs_r, nw_r, y)
    b = DT.train_step(sd0, args, segs_d, nw_d, segs_r, nw_r, y, pooled_bn=True)
    k = 'cnn.model.bn3.weight'
    assert np.abs(a['grads'][k] - b['grads'][k]).max() > 0.05 * np.abs(a['grads'][k]).max()


def test_trainer_dispatch_returns_the_double_ended_trainer():
    from nisqa_amd import trainloop
    from nisqa_amd.train import HipTrainer
    from nisqa_amd.train_de import HipTrainerDE
    from nisqa_amd import synth
    assert trainloop.trainer_class(DO.de_args()) is HipTrainerDE
    assert trainloop.trainer_class(dict(synth.MOS_ARGS)) is HipTrainer


@pytest.mark.parametrize('align', ['dot', 'cosine'])
@pytest.mark.parametrize('fuse', DO.FUSES)
def test_argument_check_accepts_what_trains(align, fuse):
    from nisqa_amd.train_de import check_de_train_args
    assert check_de_train_args(DO.de_args(align, 'hard', fuse)) in ('f32', 'mixed', 'bf16x3', 'bf16x6', 'f16x4')
    assert check_de_train_args(DO.de_args(align, 'hard', fuse), 'f32') == 'f32'


@pytest.mark.parametrize('key,value,word', [('de_align_apply', 'soft', 'soft'), ('de_align', 'bahd', 'bahd'),
                                            ('de_fuse_dim', 64, 'de_fuse_dim'), ('td_2', 'lstm', 'td_2'),
                                            ('pool_att_dropout', 0.1, 'pool_att_dropout')])
def test_argument_check_refuses_naming_the_option(key, value, word):
    from nisqa_amd.train_de import check_de_train_args
    with pytest.raises(NotImplementedError, match=word):
        check_de_train_args(dict(DO.DE_ARGS, **{key: value}))


def test_refusal_reaches_the_user_before_any_gpu_work():
    from nisqa_amd.NISQA_model import nisqaModel
    with pytest.raises(NotImplementedError, match='de_align_apply=soft'):
        nisqaModel(dict(DO.DE_ARGS, mode='main', pretrained_model=False, tr_device='cpu', de_align_apply='soft'))


def test_training_on_a_cpu_device_is_refused_after_the_argument_check():
    """no CPU path: the shipped recipe on device cpu is refused when the model is loaded, and an option that is not built is named first"""
    from nisqa_amd.NISQA_model import nisqaModel
    with pytest.raises(NotImplementedError, match='training runs as HIP kernels on a GPU'):
        nisqaModel(dict(DO.DE_ARGS, mode='main', pretrained_model=False, tr_device='cpu'))
    with pytest.raises(NotImplementedError, match='bahd'):
        nisqaModel(dict(DO.DE_ARGS, mode='main', pretrained_model=False, tr_device='cpu', de_align='bahd'))


def test_training_tables_without_csv_ref_name_it(tmp_path):
    """_loadDatasets in training mode (reached on a GPU only: called here on its own)"""
    import pandas as pd
    from nisqa_amd.NISQA_model import nisqaModel
    pd.DataFrame([{'db': 'A', 'filepath_deg': 'a.wav', 'mos': 1.0}]).to_csv(tmp_path / 'f.csv', index=False)
    nm = object.__new__(nisqaModel)
    nm.args = dict(DO.DE_ARGS, mode='main', double_ended=True, dim=False, data_dir=str(tmp_path), csv_file='f.csv', csv_con=None,
                   csv_deg='filepath_deg', csv_ref=None, csv_mos_train='mos', csv_mos_val='mos', csv_db_train=['A'], csv_db_val=['A'])
    nm.runinfos = {}
    with pytest.raises(ValueError, match='NISQA_DE needs csv_ref'):
        nm._loadDatasets()


def test_alignment_training_entries_are_declared_bound_and_exported():
    from nisqa_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_train.h')).read()
    declared = set(re.findall(r'^\s*(?:int|int64_t)\s+(nisqa_[a-z0-9_]+)\s*\(', hdr, re.M))
    for name in ('nisqa_de_align_fuse_bwd', 'nisqa_de_align_fuse_packed'):
        assert name in declared and name in lib.TRAIN_SYMBOLS
    assert len(lib.TRAIN_SYMBOLS['nisqa_de_align_fuse_bwd'][1]) == 13 and len(lib.TRAIN_SYMBOLS['nisqa_de_align_fuse_packed'][1]) == 14
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exported = lib.exported_symbols(lib.LIB_PATH, 'nisqa_de_')
    assert {'nisqa_de_align_fuse', 'nisqa_de_align_fuse_bwd', 'nisqa_de_align_fuse_packed'} <= set(exported)
    assert lib.exported_symbols(lib.LIB_PATH, 'nisqa_debug_') == []
    L = lib.load()
    assert L.nisqa_de_align_fuse_bwd(None, 192, None, None, None, None, None, 1, 1, 0, None, None, None) == lib.NISQA_ERR_ARG
    assert L.nisqa_de_align_fuse_packed(None, None, None, None, None, None, 1, 1, 0, 0, 192, None, None, None) == lib.NISQA_ERR_ARG


def test_stage_pairs_keeps_both_sides_on_the_same_rows_across_sample_rates(tmp_path):
    """Rows whose files differ in rate (between rows and within a pair): each side falls into groups of one rate, and clip k of the
    degraded side and clip k of the reference side, counted through the groups, are the two files of row ids[k]."""
    import types
    import pandas as pd
    from nisqa_amd import NISQA_lib as NL, synth, trainloop
    rates = [(48000, 48000), (16000, 48000), (48000, 16000), (16000, 16000), (48000, 48000)]
    rows = []
    for k, (rd, rr) in enumerate(rates):                       # every file has its own length: a clip is recognised by it
        synth.write_wav(str(tmp_path / ('d%d.wav' % k)), synth.synth_pcm16(k, 0.2 + 0.01 * k, rd), rd)
        synth.write_wav(str(tmp_path / ('r%d.wav' % k)), synth.synth_pcm16(10 + k, 0.3 + 0.01 * k, rr), rr)
        rows.append({'deg': 'd%d.wav' % k, 'ref': 'r%d.wav' % k, 'mos': 3.0, 'db': 'x'})
    ds = NL.SpeechQualityDataset(pd.DataFrame(rows), data_dir=str(tmp_path), filename_column='deg', mos_column='mos',
                                 double_ended=True, filename_column_ref='ref')
    eng = types.SimpleNamespace(device=torch.device('cpu'), rate=lambda sr: int(sr), resample=lambda pcm, lengths, sr: pcm,
                                pcm16_to_f32=lambda pcm: pcm.float(),
                                audio_plan=lambda lengths, sr, names=None: types.SimpleNamespace(lengths=list(lengths), sr=sr, names=names))
    ids, g_deg, g_ref = trainloop.stage_pairs(types.SimpleNamespace(eng=eng), ds, [4, 2, 0, 3, 1])
    assert sorted(ids.tolist()) == [0, 1, 2, 3, 4]
    for groups, view, col in ((g_deg, ds, 0), (g_ref, ds.ref_view(), 1)):
        lengths = [n for _, plan, _ in groups for n in plan.lengths]
        assert lengths == [len(view.load_audio(int(i))[0]) for i in ids]                       # row by row, in the step's order
        for pcm, plan, sr in groups:
            assert sr == plan.sr and pcm.numel() == sum(plan.lengths) and pcm.dtype == torch.float32
            assert all(rates[int(n[1:-4])][col] == sr for n in (os.path.basename(p) for p in plan.names))
    assert len(g_deg) >= 2 and len(g_ref) >= 2
