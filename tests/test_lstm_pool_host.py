"""CNN-LSTM-AVG / CNN-LSTM-MAX checkpoints (config/train_nisqa_cnn_lstm_avg.yaml and its pool: max variant) on the host side: model
construction and strict loading, the options the engine refuses, the oracle restatement against the reference's modules and the committed
fixtures, the segment count at hop 3, the batch policy and the new ABI entry point's argument checks.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import helpers
import lstm_pool_oracle as LO
from nisqa_amd import synth
from oracle import ref_shim

POOLS = ['avg', 'max']


def _ref_lib():
    return ref_shim.import_reference_lib() if ref_shim.reference_available() else None


@pytest.mark.parametrize('pool', POOLS)
def test_recipe_model_constructs_with_the_reference_key_set(pool):
    from nisqa_amd import NISQA_lib as NL
    kw = LO.model_kwargs(LO.POOL_ARGS[pool])
    m = NL.NISQA(**kw)
    keys = set(m.state_dict())
    RL = _ref_lib()
    if RL is not None:
        want = set(RL.NISQA(**kw).state_dict())
    else:                                        # the tts parameter tree: PoolAvg / PoolMax hold the same linear layer
        want = set(NL.NISQA(**dict(kw, pool='last_step_bi')).state_dict())
    assert keys == want
    assert keys == set(LO.state_dict())
    assert m.state_dict()['pool.model.linear.weight'].shape == (1, 256)


@pytest.mark.parametrize('pool', POOLS)
def test_checkpoint_loads_with_strict_keys_through_nisqaModel(tmp_path, pool):
    from nisqa_amd.NISQA_model import nisqaModel
    args = dict(LO.POOL_ARGS[pool], pretrained_model=False)
    sd = LO.state_dict()
    ck = str(tmp_path / ('lstm_%s.tar' % pool))
    torch.save({'args': args, 'model_state_dict': sd}, ck)
    wav = str(tmp_path / 'a.wav')
    synth.write_wav(wav, synth.synth_pcm16(3, 1.0), 48000)
    m = nisqaModel({'mode': 'predict_file', 'pretrained_model': ck, 'deg': wav, 'data_dir': None, 'output_dir': None,
                    'csv_file': None, 'csv_deg': None, 'num_workers': 0, 'bs': 1, 'ms_channel': None, 'tr_bs_val': 1,
                    'tr_num_workers': 0})
    got = m.model.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    assert m.args['pool'] == pool and m.args['ms_seg_hop_length'] == 3


REFUSED = [
    ({'td_lstm_bidirectional': False}, 'td_lstm_bidirectional'),
    ({'pool': 'last_step'}, 'pool=last_step'),
    ({'td_lstm_num_layers': 2}, 'td_lstm_num_layers=2'),
    ({'td_lstm_h': 64}, 'td_lstm_h=64'),
    ({'pool': 'att', 'pool_att_h': 128}, 'pool=att'),
    ({'td_2': 'self_att'}, 'td_2=self_att'),
    ({'cnn_fc_out_h': 32}, 'cnn_fc_out_h=32'),
]


@pytest.mark.parametrize('change,option', REFUSED, ids=[o for _, o in REFUSED])
def test_unsupported_lstm_options_are_refused_by_name(change, option):
    """Each option outside the supported set raises NotImplementedError naming it: at model construction and in the engine's
    constructor before any GPU work (no GPU is needed to see it)."""
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import HipNisqa
    args = dict(LO.LSTM_AVG_ARGS, **change)
    with pytest.raises(NotImplementedError, match=option):
        NL.NISQA(**LO.model_kwargs(args))
    with pytest.raises(NotImplementedError, match=option):
        HipNisqa(args, LO.state_dict())


@pytest.mark.parametrize('pool', POOLS)
def test_avg_and_max_behind_self_attention_and_with_NISQA_DIM_are_refused(pool):
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import HipNisqa
    with pytest.raises(NotImplementedError, match='pool=%s' % pool):
        NL.NISQA(**LO.model_kwargs(dict(synth.MOS_ARGS, pool=pool)))
    with pytest.raises(NotImplementedError, match='pool=%s' % pool):
        HipNisqa(dict(synth.MOS_ARGS, pool=pool), synth.random_state_dict(8, 'NISQA'))
    with pytest.raises(NotImplementedError):
        NL.NISQA_DIM(**LO.model_kwargs(LO.POOL_ARGS[pool]))
    with pytest.raises(NotImplementedError, match='model=NISQA_DIM'):
        HipNisqa(dict(LO.POOL_ARGS[pool], model='NISQA_DIM'), LO.state_dict())


def _gamma(n):
    """Higham's bound on the relative rounding error of an n-term fp32 sum, in any order"""
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def test_oracle_pooling_matches_the_reference_modules():
    """lstm_pool_oracle.pool_vector on each clip's valid rows against the reference's PoolAvg / PoolMax on the padded batch.  What is
    compared is the pooled vector, captured at the input of the reference's linear layer: max bit for bit; avg within the rounding
    bound of an fp32 sum against float64, and within 1e-5 of the reference (a wrong mask or divisor is off by 1e-2 and more).  The
    linear layer runs as a matrix-vector product here and as a GEMM there, in a summation order the CPU's BLAS picks, so each output is
    held to the rounding bound of its 257-term dot product against float64 rather than to the other's bits."""
    RL = _ref_lib()
    g = torch.Generator().manual_seed(5)
    n_wins = torch.tensor([1, 7, 64, 33, 1300])
    x = torch.tanh(torch.randn(len(n_wins), int(n_wins.max()), 256, generator=g) * 2)
    lin = torch.nn.Linear(256, 1)
    sd = {'pool.model.linear.weight': lin.weight.detach(), 'pool.model.linear.bias': lin.bias.detach()}
    w64, b64 = lin.weight.detach().double().reshape(-1), float(lin.bias.detach().double())
    with torch.no_grad():
        for pool in POOLS:
            mine_v = torch.stack([LO.pool_vector(x[b, :n], pool) for b, n in enumerate(n_wins.tolist())])
            mine = torch.stack([LO.pool_linear(sd, v) for v in mine_v]).reshape(-1)
            mask = torch.arange(x.shape[1])[None, :, None] < n_wins[:, None, None]
            if RL is None:                        # the reference's formula, restated: masked fill, sum or max over the padded axis
                ref_v = x.masked_fill(~mask, 0).sum(1) / n_wins[:, None] if pool == 'avg' else \
                    x.masked_fill(~mask, float('-inf')).max(1)[0]
                ref = lin(ref_v).reshape(-1)
            else:
                mod = (RL.PoolAvg if pool == 'avg' else RL.PoolMax)(256, 1)
                mod.linear.load_state_dict(lin.state_dict())
                seen = []
                hook = mod.linear.register_forward_hook(lambda m, inp, out: seen.append(inp[0].detach().clone()))
                ref = mod(x.clone(), n_wins).reshape(-1)
                hook.remove()
                ref_v = seen[0]
            if pool == 'max':
                assert torch.equal(mine_v, ref_v)
            else:
                x64 = x.double().masked_fill(~mask, 0)
                exact = x64.sum(1) / n_wins[:, None].double()
                bound = torch.tensor([_gamma(int(x.shape[1])) for _ in n_wins])[:, None] * (x64.abs().sum(1) / n_wins[:, None]) \
                    + 2.0 ** -24 * exact.abs()
                for v in (mine_v, ref_v):
                    assert ((v.double() - exact).abs() <= bound).all()
                assert (mine_v - ref_v).abs().max() <= 1e-5
            for out, v in ((mine, mine_v), (ref, ref_v)):
                v64 = v.double()
                exact = v64 @ w64 + b64
                scale = v64.abs() @ w64.abs() + abs(b64)
                assert ((out.double() - exact).abs() <= _gamma(257) * scale).all(), (pool, out, exact)


@pytest.mark.parametrize('pool', POOLS)
def test_oracle_matches_the_reference_fixture(pool):
    g = helpers.golden('net_lstm_%s_rand.npz' % pool)
    args, sd = LO.POOL_ARGS[pool], LO.state_dict()
    assert list(g['clip_samples']) == [c[1] for c in LO.CLIPS]
    for i in range(len(LO.CLIPS)):
        import zlib
        p = LO.clip_pcm(i)
        assert zlib.crc32(p.tobytes()) == int(g['pcm_crc32'][i])
        out, st = LO.predict(sd, args, LO.clip_spec(p, args), return_stages=True)
        assert st['feat'].shape[0] == int(g['n_wins'][i])
        if i in list(g['stage_clips']):
            np.testing.assert_allclose(st['feat'].numpy(), g['feat_%d' % i], rtol=0, atol=2e-5)
        np.testing.assert_allclose(st['pooled'].numpy(), g['pooled'][i], rtol=0, atol=2e-5)
        np.testing.assert_allclose(out, g['out'][i], rtol=0, atol=1e-4)
    assert int(g['n_wins'][-1]) == 1300


def test_segment_count_at_hop_3_matches_segment_specs_up_to_the_cap():
    """tokens_of (the predict loop's batching, from WAV headers) and BatchPlan (the engine's layout) against segment_specs at the recipe's
    segment hop 3, including a clip at ms_max_segments = 1300 (runs) and one segment past it (the reference's ValueError)."""
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import BatchPlan
    from oracle import net as onet
    RL = _ref_lib()

    class Ds(object):
        seg_length, seg_hop_length, max_length = 15, 3, 1300
        ms_hop_length, ms_sr = 0.01, None

    lengths = np.array([6720, 7200, 7679, 7680, 8160, 17760, 48000, 480000, LO.CAP_SAMPLES - 1, LO.CAP_SAMPLES, LO.CAP_SAMPLES + 479])
    got = NL.tokens_of(Ds(), lengths, np.full(len(lengths), 48000))
    plan = BatchPlan(lengths, LO.HOP, 3, 1300)
    for k, n in enumerate(lengths):
        T = 1 + int(n) // LO.HOP
        spec = np.zeros((48, T), np.float32)
        if RL is not None:
            _, want = RL.segment_specs('f', spec, 15, 3, 1300)
        else:
            _, want = onet.segment_specs(spec, 15, 3, 1300)
        assert int(got[k]) == int(want) == int(plan.n_wins[k]), (n, got[k], want, plan.n_wins[k])
    assert int(plan.n_wins[-1]) == 1300 and int(plan.n_wins[0]) == 1
    over = LO.OVER_CAP_SAMPLES
    assert int(NL.tokens_of(Ds(), np.array([over]), np.array([48000]))[0]) == 1301
    with pytest.raises(ValueError, match='n_wins 1301 > max_length 1300'):
        BatchPlan([48000, over], LO.HOP, 3, 1300, names=['a.wav', 'long.wav'])
    if RL is not None:
        with pytest.raises(ValueError, match='n_wins 1301 > max_length 1300'):
            RL.segment_specs('long.wav', np.zeros((48, 1 + over // LO.HOP), np.float32), 15, 3, 1300)


def test_batch_policy_treats_every_lstm_arch_as_lstm():
    from nisqa_amd import NISQA_lib as NL

    class Eng(object):
        arch = 0

    class Ds(object):
        seg_length, seg_hop_length, max_length = 15, 3, 1300
        ms_n_fft, ms_hop_length, ms_sr = 4096, 0.01, None
    for arch in (1, 2, 3):
        e = Eng()
        e.arch = arch
        pol = NL.batch_policy(e, Ds(), range(1000), 8)
        assert pol.min_tokens == 0 and pol.min_clips == NL.MIN_CLIPS_LSTM, arch
    pol = NL.batch_policy(Eng(), Ds(), range(1000), 8)
    assert pol.min_tokens == NL.MIN_TOKENS_SA and pol.min_clips == 1


def test_lstm_pool_and_arch_argument_validation_without_gpu():
    """nisqa_lstm_pool refuses an unknown pool_mode and an empty batch, and nisqa_predict_batch an arch outside 0..3, before any launch."""
    from nisqa_amd import lib
    L = lib.load()
    assert (lib.LSTM_POOL_LAST_STEP_BI, lib.LSTM_POOL_AVG, lib.LSTM_POOL_MAX) == (0, 1, 2)
    for mode in (3, -1, 7):
        assert L.nisqa_lstm_pool(None, None, None, 4, None, mode, None, None, None, None) == lib.NISQA_ERR_ARG
    for mode in (0, 1, 2):
        assert L.nisqa_lstm_pool(None, None, None, 0, None, mode, None, None, None, None) == lib.NISQA_ERR_ARG
        assert L.nisqa_lstm_pool(None, None, None, -3, None, mode, None, None, None, None) == lib.NISQA_ERR_ARG
    cfg = lib.MelCfg(4096, 480, 960, 48, 1707, 4032, 1e-8, 80.0)
    fake = ctypes.c_void_p(256)                   # never dereferenced: the arch check comes first
    for arch in (4, -1, 99):
        model = lib.ModelDev()
        model.arch = arch
        model.seg_hop = 3
        for fn in (L.nisqa_predict_batch, L.nisqa_predict_batch_pcm16):
            rc = fn(fake, fake, fake, fake, fake, 2, 100, 64, ctypes.byref(cfg), ctypes.byref(model), fake, 1 << 30, fake, None)
            assert rc == lib.NISQA_ERR_ARG, (arch, rc)
