"""The inner operator model(x, n_wins) for StandardCNN + BiLSTM and NISQA_DE checkpoints, the part that needs no GPU: the argument
checks of the segment-fed StandardCNN entries, their rows in the engine's precision table, and the refusals of malformed segment
tensors before any engine is built."""
import numpy as np
import pandas as pd
import pytest
import torch

import de_oracle as DO
import helpers
from nisqa_amd import engine, lib

HIP_NISQA, HIP_NISQA_DE = engine.HipNisqa, engine.HipNisqaDE   # the classes themselves (_no_gpu_work replaces the module's names)
P = 0x1000                                       # a pointer that only has to be non-NULL: a rejected call never reads it
ENTRIES = {'f32': 'nisqa_cnn_standard_segments', 'bf16x3': 'nisqa_cnn_standard_segments_bf16', 'bf16x6': 'nisqa_cnn_standard_segments_bf16x6',
           'f16x3': 'nisqa_cnn_standard_segments_f16', 'f16x4': 'nisqa_cnn_standard_segments_f16'}


def _args(precision, x=P, seg_len=90, n_clips=3, total=192, products=None):
    """the entry's argument list: the AdaptCNN segments head, then the tail of the `standard` entry of the precision"""
    head = [x, seg_len, P, P, n_clips, total, P]
    if precision == 'f32':
        return head + [P, P, None]               # p3_ws, feat20, stream
    if precision in ('bf16x3', 'bf16x6'):
        return head + [P, P, None]               # cnn_wb, feat20, stream
    return head + [P, int(precision[-1]) if products is None else products, P, None]


@pytest.mark.parametrize('precision', list(ENTRIES))
def test_segment_fed_standard_entries_reject_bad_arguments_before_launching(precision):
    L = lib.load()
    f = getattr(L, ENTRIES[precision])
    ERR = lib.NISQA_ERR_ARG
    assert f(*_args(precision, x=None)) == ERR
    for seg_len in (0, -1):
        assert f(*_args(precision, seg_len=seg_len)) == ERR
    for total in (0, -32, 16, 33, 95, 191):
        assert f(*_args(precision, total=total)) == ERR
    for n_clips in (0, -1):
        assert f(*_args(precision, n_clips=n_clips)) == ERR
    if precision.startswith('f16'):
        for products in (-1, 0, 2, 5, 6):
            assert f(*_args(precision, products=products)) == ERR
    assert L.nisqa_abi_version() == 2            # additive: the ABI version stays


@pytest.mark.parametrize('precision', list(ENTRIES))
def test_precision_table_names_the_segment_fed_standard_entry(precision):
    row = engine.PRECISION[precision]
    assert row._fields[-1] == 'standard_segments'
    name, tail = row.standard_segments
    assert name == ENTRIES[precision] and name in lib.SYMBOLS
    assert tail == row.standard[1]               # the tail of the `standard` entry of the same precision
    head7 = ['x', 90, 'tok_off', 'n_wins', 3, 192, 'cnn_w']
    got, what, args = engine.cnn_call(precision, 'standard_segments', head7, 'WB', 'P3', 'FEAT', 'STREAM')
    restype, argtypes = lib.SYMBOLS[name]
    assert got == name and len(args) == len(argtypes) and args[:7] == head7 and args[-1] == 'STREAM' and args[-2] == 'FEAT'
    assert what == ('nisqa_cnn_standard_segments_bf16x3' if precision == 'bf16x3' else name)
    # the head is the AdaptCNN segments head; the tail is the `standard` entry's own
    seg_types, std_types = lib.SYMBOLS[row.segments[0]][1], lib.SYMBOLS[row.standard[0]][1]
    assert argtypes[:7] == seg_types[:7] and argtypes[7:] == std_types[9:]
    if precision.startswith('f16'):
        pos = argtypes.index(lib.c_i32, 7)       # the only int32 behind cnn_w: the term count
        assert args[pos] == int(precision[-1]) and args[pos - 1] == 'WB'
    elif precision == 'f32':
        assert args[7] == 'P3'
    else:
        assert args[7] == 'WB'


def _no_gpu_work(monkeypatch):
    """Any attempt to build an engine fails the test."""
    def boom(*a, **k):
        raise AssertionError('GPU work started before the refusal')
    monkeypatch.setattr(engine, 'HipNisqa', boom)
    monkeypatch.setattr(engine, 'HipNisqaDE', boom)


BAD_SINGLE = [
    (torch.zeros(2, 8, 48, 15), [3, 8], 'shape'),
    (torch.zeros(2, 8, 2, 48, 15), [3, 8], 'shape'),
    (torch.zeros(2, 8, 1, 48, 14), [3, 8], 'shape'),
    (torch.zeros(2, 8, 1, 40, 15), [3, 8], 'shape'),
    (torch.zeros(2, 8, 1, 48, 15), [3], 'n_wins'),
    (torch.zeros(2, 8, 1, 48, 15), [3, 8, 1], 'n_wins'),
    (torch.zeros(2, 8, 1, 48, 15), [0, 8], 'n_wins'),
    (torch.zeros(2, 8, 1, 48, 15), [3, 9], 'n_wins'),
    (torch.zeros(2, 8, 1, 48, 15), torch.tensor([-1, 2]), 'n_wins'),
]


@pytest.mark.parametrize('model', ['NISQA_TTS', 'NISQA'])
@pytest.mark.parametrize('case', range(len(BAD_SINGLE)))
def test_single_ended_forward_refuses_malformed_segments_before_any_engine(monkeypatch, model, case):
    from nisqa_amd import NISQA_lib as NL
    _no_gpu_work(monkeypatch)
    x, n, word = BAD_SINGLE[case]
    args = dict(helpers.TTS_ARGS if model == 'NISQA_TTS' else helpers.MOS_ARGS)
    m = NL.NISQA(**{k: v for k, v in args.items() if k.startswith(('cnn_', 'td', 'pool', 'ms_seg_length', 'ms_n_mels'))}).bind_args(args)
    with pytest.raises(ValueError, match=word):
        m(x, n)
    # the engine's own method: an instance whose construction was skipped must refuse before it touches any of its state
    eng = object.__new__(HIP_NISQA)
    eng.arch = 1 if model == 'NISQA_TTS' else 0
    with pytest.raises(ValueError, match=word):
        eng.forward_segments(x, n)


BAD_DE = [
    (torch.zeros(2, 8, 1, 48, 15), [[3, 8], [1, 1]], 'shape'),
    (torch.zeros(2, 8, 3, 48, 15), [[3, 8], [1, 1]], 'shape'),
    (torch.zeros(2, 8, 2, 48), [[3, 8], [1, 1]], 'shape'),
    (torch.zeros(2, 8, 2, 48, 16), [[3, 8], [1, 1]], 'shape'),
    (torch.zeros(2, 8, 2, 48, 15), [3, 8], r'\[B, 2\]'),
    (torch.zeros(2, 8, 2, 48, 15), [[3, 8, 1], [1, 1, 1]], r'\[B, 2\]'),
    (torch.zeros(2, 8, 2, 48, 15), [[3, 8]], r'\[B, 2\]'),
    (torch.zeros(2, 8, 2, 48, 15), [[3, 8], [0, 1]], 'n_wins'),
    (torch.zeros(2, 8, 2, 48, 15), [[3, 9], [1, 1]], 'n_wins'),
    (torch.zeros(2, 8, 2, 48, 15), torch.tensor([[3, 8], [1, -1]]), 'n_wins'),
]


@pytest.mark.parametrize('case', range(len(BAD_DE)))
def test_double_ended_forward_refuses_malformed_segments_before_any_engine(monkeypatch, case):
    from nisqa_amd import NISQA_lib as NL
    _no_gpu_work(monkeypatch)
    x, n, word = BAD_DE[case]
    args = DO.de_args()
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    with pytest.raises(ValueError, match=word):
        m(x, n)
    eng = object.__new__(HIP_NISQA_DE)
    with pytest.raises(ValueError, match=word):
        eng.forward_segments(x, n)


def test_check_segments_returns_the_counts():
    n = engine.check_segments(torch.zeros(3, 8, 1, 48, 15), torch.tensor([1, 8, 4]), 1)
    assert n.dtype == np.int64 and n.tolist() == [1, 8, 4]
    n = engine.check_segments(torch.zeros(2, 8, 2, 48, 15), np.array([[1, 8], [4, 2]]), 2)
    assert n.dtype == np.int64 and n.tolist() == [[1, 8], [4, 2]]


def test_double_ended_dataset_item_needs_a_bound_engine(tmp_path):
    from nisqa_amd import NISQA_lib as NL
    df = pd.DataFrame([{'deg': 'd.wav', 'ref': 'r.wav'}])
    ds = NL.SpeechQualityDataset(df, data_dir=str(tmp_path), filename_column='deg', mos_column='predict_only', seg_length=15,
                                 max_length=1300, seg_hop_length=4, ms_n_fft=4096, ms_hop_length=0.01, ms_win_length=0.02, ms_n_mels=48,
                                 ms_sr=None, ms_fmax=20000, double_ended=True, filename_column_ref='ref')
    single = ds.ref_view()
    for d in (ds, single):
        with pytest.raises(RuntimeError, match='bind_engine'):
            d[0]
