"""Self-attention blocks of 1, 3 and 4 layers on the CPU: the weight helper (tests/sa_layers.py), the float64 oracle at those
depths against torch's own encoder layers, how far a wrong depth, a wrong layer order or a wrong layer stride moves the float64
output compared with what the GPU tests of tests/test_gpu_layer_count.py allow, and the guard of the training step's sum rows."""
import types

import numpy as np
import pytest
import torch

import de_oracle as DO
import helpers
import sa_layers as SL
import test_gpu_stage_width as SW           # _sample, _oracle_sa, _heads, _per_clip: the harness the GPU tests judge with
from nisqa_amd import synth
from oracle import mel as omel, net as onet

COUNTS = [1, 31, 32, 33, 63, 64, 65, 129, 257]                      # the token counts of tests/test_gpu_layer_count.py
SETS = [('NISQA_DIM', 7, 1), ('NISQA_DIM', 7, 3), ('NISQA_DIM', 7, 4), ('NISQA', 8, 3)]
SEPARATION = 100.0                                                   # x the float32 CPU oracle's own distance from float64


def _bits(a, b):
    a, b = (np.asarray(v.detach().cpu() if torch.is_tensor(v) else v) for v in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('model,seed', [('NISQA_DIM', 7), ('NISQA', 8)])
def test_two_layers_is_the_state_dict_itself(model, seed):
    sd = synth.random_state_dict(seed, model)
    out = SL.with_layers(sd, 2)
    assert list(out) == list(sd)
    assert all(_bits(out[k], sd[k]) for k in sd)
    assert all(out[k] is not sd[k] for k in sd)                      # a copy: nothing aliases a seeded fixture
    de = DO.random_de_state_dict(5, 'x/y/-', n_layers2=3)
    assert list(SL.with_layers(de, 3, SL.TD2)) == list(de) and list(SL.with_layers(de, 2)) == list(de)
    assert SL.args_with_layers(synth.DIM_ARGS, 3)['td_sa_num_layers'] == 3 and synth.DIM_ARGS['td_sa_num_layers'] == 2
    assert SL.args_with_layers(DO.DE_ARGS, 1, 'td_2_sa_num_layers')['td_2_sa_num_layers'] == 1


def test_other_depths_keep_drop_and_draw_whole_layers():
    sd = synth.random_state_dict(7, 'NISQA_DIM')
    one, four = SL.with_layers(sd, 1), SL.with_layers(sd, 4)
    assert SL.depth(one) == 1 and SL.depth(four) == 4
    assert all(_bits(one[k], sd[k]) for k in one) and all(_bits(four[k], sd[k]) for k in sd)
    assert all(_bits(SL.with_layers(sd, 3)[k], four[k]) for k in SL.with_layers(sd, 3))          # layer 2 does not depend on n
    keys = lambda d, l: [k[len(SL.TD + 'layers.%d.' % l):] for k in d if SL.layer_of(k) == l]
    for l in (2, 3):
        assert keys(four, l) == keys(sd, 0)
        for k in keys(four, l):
            a, b = four[SL.TD + 'layers.%d.%s' % (l, k)], sd[SL.TD + 'layers.0.' + k]
            assert a.shape == b.shape and a.dtype == b.dtype
            assert 0.6 < float(a.std()) / float(b.std()) < 1.6, (l, k)
    assert not _bits(four[SL.TD + 'layers.2.norm1.weight'], four[SL.TD + 'layers.3.norm1.weight'])
    assert not _bits(four[SL.TD + 'layers.2.norm1.weight'], SL.with_layers(sd, 4, seed=1)[SL.TD + 'layers.2.norm1.weight'])
    order = list(four)
    assert order.index(SL.TD + 'layers.3.norm2.bias') + 1 == order.index('pool_layers.0.model.linear1.weight')
    de = SL.with_layers(DO.random_de_state_dict(5, '+/-'), 3)        # the first block of a double-ended model: the second stays
    assert SL.depth(de) == 3 and SL.depth(de, SL.TD2) == 2
    assert SL.depth(SL.with_layers(de, 1, SL.TD2), SL.TD2) == 1 and SL.depth(SL.with_layers(de, 1, SL.TD2)) == 3


def _torch_stack(sd, n, pfx=SL.TD):
    """n of torch's own post-norm encoder layers (nn.TransformerEncoderLayer: MultiheadAttention, LayerNorm, ReLU feed-forward --
    the modules, and the parameter names, the reference's SelfAttentionLayer is made of) in float64, each loaded strict"""
    layers = []
    for l in range(n):
        m = torch.nn.TransformerEncoderLayer(64, 1, 64, dropout=0.0, activation='relu', batch_first=True, norm_first=False).double()
        p = pfx + 'layers.%d.' % l
        m.load_state_dict({k[len(p):]: v.double() for k, v in sd.items() if k.startswith(p)}, strict=True)
        layers.append(m.eval())
    return layers


@pytest.mark.parametrize('model,seed,n', [s for s in SETS if s[2] != 2] + [('NISQA_DIM', 7, 5)])
def test_other_depths_load_strict_and_the_oracle_is_the_module_stack(model, seed, n):
    """The package's module built from the matching args takes the state dict with strict=True (it holds parameters only: its
    forward is the HIP engine), and the float64 oracle at depth n equals n of torch's own encoder layers on top of the block's
    projection and LayerNorm."""
    from nisqa_amd import NISQA_lib as NL
    from oracle import ref_shim
    base = synth.DIM_ARGS if model == 'NISQA_DIM' else synth.MOS_ARGS
    sd, args = SL.with_layers(synth.random_state_dict(seed, model), n), SL.args_with_layers(base, n)
    m = getattr(NL, model)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS})
    m.load_state_dict(sd, strict=True)
    assert len(m.time_dependency.model.layers) == n
    assert list(m.state_dict()) == list(sd) and all(_bits(v, sd[k]) for k, v in m.state_dict().items())
    with pytest.raises(RuntimeError):
        getattr(NL, model)(**{k: base[k] for k in ref_shim.MODEL_ARG_KEYS}).load_state_dict(sd, strict=True)
    s = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    feat = torch.from_numpy(np.random.default_rng(n).standard_normal((37, 384)))
    with torch.no_grad():
        got = onet.self_attention(s, feat, n)
        x = torch.nn.functional.layer_norm(torch.nn.functional.linear(feat, s[SL.TD + 'linear.weight'], s[SL.TD + 'linear.bias']),
                                           (64,), s[SL.TD + 'norm1.weight'], s[SL.TD + 'norm1.bias'], onet.LN_EPS)
        for layer in _torch_stack(sd, n):
            x = layer(x[None])[0]
        short = onet.self_attention(s, feat, n - 1)
    assert float((got - x).abs().max()) < 1e-12
    assert float((got - short).abs().max()) > 1e-2                   # ... and the depth is not a no-op


# ---- (iii) what a wrong stack does to the float64 output, against what the GPU bound lets through ------------------------------
def feature_rows():
    """rows of AdaptCNN features: the float32 oracle CNN (the weights of seed 7; the CNN is not under test) on two synthetic clips"""
    sd = {k: v for k, v in synth.random_state_dict(7, 'NISQA_DIM').items() if k.startswith('cnn.')}
    rows = []
    for i in range(2):
        spec = omel.melspec_db_from_audio(synth.synth_pcm16(900 + i, 2.0).astype(np.float32) / np.float32(32768.0), 48000)
        with torch.no_grad():
            rows.append(onet.adapt_cnn(sd, onet.segment_specs(spec, 15, 4)[0]).numpy())
    return np.concatenate(rows)


def _wrong_stacks(sd, n):
    """(name, state dict, depth) of the mistakes a launcher can make at depth n"""
    def relayered(order):
        """layer l holds sd's layer order[l]"""
        out = dict(sd)
        for l, src in enumerate(order):
            for k, _, _, _ in SL.LAYER:
                out[SL.TD + 'layers.%d.%s' % (l, k)] = sd[SL.TD + 'layers.%d.%s' % (src, k)]
        return out
    out = [('one layer fewer', sd, n - 1)]
    if n >= 2:
        ident = list(range(n))
        out.append(('last two layers swapped', relayered(ident[:-2] + [n - 1, n - 2]), n))
        out += [('layer %d also as layer %d' % (l, l + 1), relayered(ident[:l + 1] + [l] + ident[l + 2:]), n) for l in range(n - 1)]
    return out


@pytest.mark.parametrize('model,seed,n', SETS)
def test_a_wrong_stack_is_far_outside_the_float32_floor(model, seed, n):
    base = synth.DIM_ARGS if model == 'NISQA_DIM' else synth.MOS_ARGS
    sd, args = SL.with_layers(synth.random_state_dict(seed, model), n), SL.args_with_layers(base, n)
    feats = SW._sample(feature_rows(), COUNTS, 1)
    heads = SW._heads(args)
    td64, chain64 = SW._oracle_sa(sd, feats, n, torch.float64, heads)
    td32, chain32 = SW._oracle_sa(sd, feats, n, torch.float32, heads)
    cpu_td, cpu_chain = float(SW._per_clip(td32, td64).max()), float(SW._per_clip(chain32, chain64).max())
    print('%s x%d: float32 CPU oracle from float64: self-attention %.3g, pooled %.3g' % (model, n, cpu_td, cpu_chain))
    for name, wrong, depth in _wrong_stacks(sd, n):
        td, chain = SW._oracle_sa(wrong, feats, depth, torch.float64, heads)
        d_td, d_chain = SW._per_clip([t.astype(np.float32) for t in td], td64), SW._per_clip([c.astype(np.float32) for c in chain], chain64)
        print('   %-28s self-attention x%.3g .. x%.3g of the floor, pooled x%.3g .. x%.3g' % (
            name, d_td.min() / cpu_td, d_td.max() / cpu_td, d_chain.min() / cpu_chain, d_chain.max() / cpu_chain))
        assert (d_td > SEPARATION * cpu_td).all(), (name, d_td, cpu_td)
        assert (d_chain > SEPARATION * cpu_chain).all(), (name, d_chain, cpu_chain)


# ---- the float64 sum rows of a training step ------------------------------------------------------------------------------------
def test_sum_rows_past_the_end_raise_instead_of_handing_out_a_short_view():
    from nisqa_amd.train import _FlatTrainer
    tr = types.SimpleNamespace(_sums=torch.zeros((5, 512), dtype=torch.float64), _sum_i=0)
    take = lambda n=1: _FlatTrainer._sum_rows(tr, n)
    assert take().numel() == 512 and take(3).numel() == 3 * 512 and tr._sum_i == 4
    with pytest.raises(RuntimeError, match='sum rows'):
        take(2)                                                      # one row left: torch would slice a 512-element view
    assert tr._sum_i == 4
    assert take().data_ptr() == tr._sums[4].data_ptr()
    with pytest.raises(RuntimeError, match='sum rows'):
        take()                                                       # none left: an empty view


def test_helpers_module_still_hands_out_two_layers():
    assert SL.depth(helpers.random_state_dict(7, 'NISQA_DIM')) == 2 and SL.depth(DO.random_de_state_dict(1), SL.TD2) == 2
