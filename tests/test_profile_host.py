"""Per-segment score profile, host surface without a GPU: the float64 restatement the GPU tests use (tests/profile_oracle.py) against
the reference's own PoolAttFF / PoolAvg modules, the new C entry (declared, bound, exported, guarded), the weight packer's layout, the
refusals of profile_audio before any GPU work, and the segment times."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import helpers
import lstm_pool_oracle as LO
import profile_oracle as PO
from nisqa_amd import synth

ROOT = helpers.ROOT


def _reference():
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip('reference tree not staged')
    return ref_shim.import_reference_lib()


@pytest.mark.parametrize('n_heads', [1, 5])
def test_restatement_is_the_references_pool_att_ff(n_heads):
    """sum_t weights * local is PoolAttFF.forward's output, and the weights are its masked softmax (recomputed from the module's own
    linear1 / linear2), in float64 to 1e-12 -- on a padded batch, so the reference's mask is exercised."""
    ref = _reference()
    torch.manual_seed(11 + n_heads)
    heads = PO.DIM_HEADS if n_heads == 5 else PO.MOS_HEADS
    mods = [ref.PoolAttFF(64, 1, 128).double().eval() for _ in heads]
    sd = {p + k: v for p, m in zip(heads, mods) for k, v in m.state_dict().items()}
    n_wins = torch.tensor([1, 63, 64, 65, 130, 7])
    L = int(n_wins.max())
    x = torch.randn(len(n_wins), L, 64, dtype=torch.float64)
    with torch.no_grad():
        outs = torch.cat([m(x.clone(), n_wins) for m in mods], 1).numpy()                    # [B, H]
        logits = [m.linear2(torch.relu(m.linear1(x))).squeeze(2) for m in mods]             # [B, L] per head
    for b, n in enumerate(n_wins.tolist()):
        w, loc = PO.profile(sd, x[b, :n].numpy(), heads, torch.float64)
        assert w.shape == (n, n_heads) and loc.shape == (n, n_heads)
        assert np.abs((w * loc).sum(0) - outs[b]).max() <= 1e-12
        assert np.abs(w.sum(0) - 1.0).max() <= 1e-12
        for h in range(n_heads):
            masked = logits[h][b].clone()
            masked[n:] = float('-inf')
            soft = torch.softmax(masked, 0).numpy()
            assert np.abs(w[:, h] - soft[:n]).max() <= 1e-12 and (soft[n:] == 0).all()


def test_restatement_is_the_references_pool_avg():
    ref = _reference()
    torch.manual_seed(5)
    mod = ref.PoolAvg(256, 1).double().eval()
    sd = {'pool.model.' + k: v for k, v in mod.state_dict().items()}
    n_wins = torch.tensor([1, 64, 65, 700])
    x = torch.randn(len(n_wins), int(n_wins.max()), 256, dtype=torch.float64)
    with torch.no_grad():
        out = mod(x.clone(), n_wins).numpy()                       # (PoolAvg zeroes its input's padding in place: a copy)
    for b, n in enumerate(n_wins.tolist()):
        w, loc = PO.profile(sd, x[b, :n].numpy(), 'avg', torch.float64)
        assert w.shape == (n, 1) and (w == 1.0 / n).all()
        assert abs(float((w * loc).sum()) - float(out[b, 0])) <= 1e-12


def test_restatement_sums_to_the_oracle_networks_pooling():
    """... and to oracle.net.pool_att_ff, the pooling of the network oracle every other GPU test is held to (no reference needed)"""
    from oracle import net as onet
    sd = {k: v.double() for k, v in synth.random_state_dict(7, 'NISQA_DIM').items() if k.startswith('pool')}
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((130, 64)))
    w, loc = PO.profile(sd, x.numpy(), PO.DIM_HEADS, torch.float64)
    for h, p in enumerate(PO.DIM_HEADS):
        assert abs(float((w[:, h] * loc[:, h]).sum()) - float(onet.pool_att_ff(sd, x, p)[0])) <= 1e-12


def test_entry_is_declared_bound_exported_and_guarded():
    from nisqa_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_hip.h')).read()
    decl = re.search(r'^int nisqa_pool_profile\(([^;]*)\);', hdr, re.M | re.S)
    assert decl is not None
    params = [' '.join(p.split()) for p in decl.group(1).split(',')]
    assert params == ['const float* x', 'int32_t ld', 'const int32_t* tok_off', 'const int32_t* n_wins', 'int32_t n_clips',
                      'int32_t total_tok_padded', 'int32_t n_heads', 'int32_t mode', 'const float* w', 'float* weights_out',
                      'float* local_out', 'void* stream']
    restype, argtypes = lib.SYMBOLS['nisqa_pool_profile']
    import ctypes
    assert restype is ctypes.c_int
    assert argtypes == [lib.c_p if '*' in p else lib.c_i32 for p in params]
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert 'nisqa_pool_profile' in lib.exported_symbols(lib.LIB_PATH, 'nisqa_pool_')
    L = lib.load()
    one, E = 16, lib.NISQA_ERR_ARG                                  # a non-NULL pointer that is never followed: the guards come first
    call = lambda x=one, ld=64, to=one, nw=one, b=3, np_=192, h=5, mode=0, w=one, wo=one, lo=one: \
        L.nisqa_pool_profile(x, ld, to, nw, b, np_, h, mode, w, wo, lo, None)
    for kw in ('x', 'to', 'nw', 'w', 'wo', 'lo'):
        assert call(**{kw: None}) == E, kw
    assert call(b=0) == E and call(b=-2) == E and call(np_=0) == E
    assert call(h=0) == E and call(h=6) == E and call(h=-1) == E
    assert call(mode=2) == E and call(mode=-1) == E
    assert call(ld=256) == E and call(ld=63) == E and call(mode=1, ld=64, h=1) == E and call(mode=1, ld=256, h=5) == E


def test_weight_packer_layout_round_trips_against_the_state_dict():
    from nisqa_amd import weights as W
    assert (W.PP_W1, W.PP_B1, W.PP_W2, W.PP_B2, W.PP_W3, W.PP_B3, W.PP_FLOATS) == (0, 8192, 8320, 8448, 8449, 8513, 8514)
    # the offsets the kernel reads the blob at are these
    src = open(os.path.join(ROOT, 'nisqa_amd', 'csrc', 'pool_profile.hip')).read()
    consts = dict(re.findall(r'constexpr int (PP_\w+) = ([^;]+);', src))
    env = {}
    for k, v in consts.items():
        env[k] = eval(v, {}, env)
    for k in ('PP_W1', 'PP_B1', 'PP_W2', 'PP_B2', 'PP_W3', 'PP_B3', 'PP_FLOATS'):
        assert env[k] == getattr(W, k), k
    sd = synth.random_state_dict(7, 'NISQA_DIM')
    blob = W.pack_pool_profile(sd, PO.DIM_HEADS)
    assert blob.dtype == np.float32 and blob.shape == (5 * W.PP_FLOATS,)
    for h, p in enumerate(PO.DIM_HEADS):
        head = blob[h * W.PP_FLOATS:(h + 1) * W.PP_FLOATS]
        f = lambda k: sd[p + k].numpy().reshape(-1)
        assert np.array_equal(head[W.PP_W1:W.PP_B1].reshape(128, 64), sd[p + 'linear1.weight'].numpy())
        assert np.array_equal(head[W.PP_B1:W.PP_W2], f('linear1.bias')) and np.array_equal(head[W.PP_W2:W.PP_B2], f('linear2.weight'))
        assert head[W.PP_B2] == f('linear2.bias')[0] and head[W.PP_B3] == f('linear3.bias')[0]
        assert np.array_equal(head[W.PP_W3:W.PP_B3], f('linear3.weight'))
    one = W.pack_pool_profile(synth.random_state_dict(8, 'NISQA'), PO.MOS_HEADS)
    assert one.shape == (W.PP_FLOATS,)
    lsd = LO.state_dict()
    avg = W.pack_pool_profile_avg(lsd)
    assert avg.dtype == np.float32 and avg.shape == (W.PP_AVG_FLOATS,) == (257,)
    assert np.array_equal(avg[:256], lsd['pool.model.linear.weight'].numpy().reshape(-1))
    assert avg[256] == lsd['pool.model.linear.bias'].numpy()[0]
    with pytest.raises(NotImplementedError):
        W.pack_pool_profile({k: (v[:64] if k.endswith('linear1.weight') else v) for k, v in sd.items()}, PO.DIM_HEADS)


def _model(model, args):
    from nisqa_amd import NISQA_lib as NL
    from oracle import ref_shim
    m = getattr(NL, model)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
    m.eval()
    return m


def test_profile_audio_refuses_what_forward_audio_refuses_before_any_gpu_work():
    m = _model('NISQA_DIM', dict(synth.DIM_ARGS))
    y = torch.zeros(2, 9600)
    bad = [(torch.zeros(2, 9600, dtype=torch.int16), None), (torch.zeros(2, 3, 9600), None), (torch.zeros(()), None),
           (torch.zeros(0, 9600), None), (torch.zeros(2, 0), None), (y.numpy(), None),
           (y, [9600]), (y, [9600, 0]), (y, [9600, 9601]), (y, [9600.5, 9600]), (y, torch.tensor([-1, 9600]))]
    for yy, lengths in bad:
        with pytest.raises(ValueError) as mine:
            m.profile_audio(yy, 48000, lengths)
        with pytest.raises(ValueError) as theirs:
            m.forward_audio(yy, 48000, lengths)
        assert str(mine.value) == str(theirs.value) and m._engine is None
    with pytest.raises(ValueError):
        m.profile_audio(y, 48000.5)
    with pytest.raises(ValueError, match='Sample too short'):
        m.profile_audio(torch.zeros(2, 9600), 48000, [9600, 6000])
    m2 = _model('NISQA_DIM', dict(synth.DIM_ARGS, ms_max_segments=2))
    with pytest.raises(ValueError, match='ms_max_segments'):
        m2.profile_audio(torch.zeros(30 * 480), 48000)
    assert m._engine is None and m2._engine is None


def test_double_ended_profile_audio_refuses_what_forward_audio_refuses_before_any_gpu_work():
    import de_oracle as DO
    from nisqa_amd import NISQA_lib as NL
    args = DO.de_args()
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    y = torch.zeros(2, 9600)
    for a, b, kw in ((y, torch.zeros(3, 9600), {}), (y, torch.zeros(9600), {}), (y, y, {'lengths_ref': [9600, 9601]}),
                     (y, y.long(), {}), (y, y, {'lengths_deg': [9600, 6000]})):
        with pytest.raises(ValueError) as mine:
            m.profile_audio(a, b, 48000, **kw)
        with pytest.raises(ValueError) as theirs:
            m.forward_audio(a, b, 48000, **kw)
        assert str(mine.value) == str(theirs.value) and m._engine is None


@pytest.mark.parametrize('pool', ['last_step_bi', 'max'])
def test_pools_without_a_decomposition_are_refused_by_name_before_any_gpu_work(pool):
    from nisqa_amd import engine
    args = dict(LO.LSTM_AVG_ARGS, pool=pool)
    with pytest.raises(NotImplementedError, match='pool=' + pool):
        engine.check_profile_args(args)
    engine.check_profile_args(LO.LSTM_AVG_ARGS)
    engine.check_profile_args(synth.DIM_ARGS)
    m = _model('NISQA', args)
    with pytest.raises(NotImplementedError, match='pool=' + pool):
        m.profile_audio(torch.zeros(9600), 48000)
    assert m._engine is None


def test_segment_times_for_hop_4_and_hop_1():
    from nisqa_amd import NISQA_lib as NL
    a4 = dict(synth.DIM_ARGS)
    assert a4['ms_seg_hop_length'] == 4 and a4['ms_seg_length'] == 15 and a4['ms_hop_length'] == 0.01
    t0, t1 = NL.segment_times(a4, 4)
    assert t0.dtype == np.float64 and np.allclose(t0, [0.0, 0.04, 0.08, 0.12], atol=1e-15)
    assert np.allclose(t1, [0.15, 0.19, 0.23, 0.27], atol=1e-15)
    a1 = dict(synth.TTS_ARGS)
    assert a1['ms_seg_hop_length'] == 1
    t0, t1 = NL.segment_times(a1, 3)
    assert np.allclose(t0, [0.0, 0.01, 0.02], atol=1e-15) and np.allclose(t1, [0.15, 0.16, 0.17], atol=1e-15)
    assert NL.segment_times(a1, 0)[0].shape == (0,)


def test_run_profile_takes_run_predicts_command_line():
    sys.path.insert(0, ROOT)
    import run_predict
    src = open(os.path.join(ROOT, 'run_profile.py')).read()
    assert 'from run_predict import build_args' in src and '.profile()' in src
    a = run_predict.build_args(['--mode', 'predict_dir', '--pretrained_model', 'x.tar', '--data_dir', 'd', '--bs', '4'])
    assert a['tr_bs_val'] == 4 and a['output_dir'] is None
