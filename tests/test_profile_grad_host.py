"""The gradient of the per-segment profile, host side without a GPU: the new C entry (declared, bound, exported, guarded), the
refusals of profile_audio(..., differentiable=True) before any GPU work, and the float64 restatement the GPU tests are held to
(tests/profile_grad_oracle.py) against the reference's own modules and against the score's gradient oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import helpers
import input_grad_oracle as IG
import lstm_pool_oracle as LO
import profile_grad_oracle as PG
import profile_oracle as PO
from nisqa_amd import synth

ROOT = helpers.ROOT
PARAMS = ['const float* x', 'int32_t ld', 'const int32_t* tok_off', 'const int32_t* n_wins', 'int32_t n_clips',
          'int32_t total_tok_padded', 'int32_t n_heads', 'int32_t mode', 'const float* w', 'const float* d_weights',
          'const float* d_local', 'const float* d_embed', 'float* dx', 'void* stream']


def test_entry_is_declared_bound_exported_and_guarded():
    from nisqa_amd import lib
    hdr = open(os.path.join(ROOT, 'include', 'nisqa_hip.h')).read()
    decl = re.search(r'^int nisqa_pool_profile_bwd\(([^;]*)\);', hdr, re.M | re.S)
    assert decl is not None
    assert [' '.join(p.split()) for p in decl.group(1).split(',')] == PARAMS
    restype, argtypes = lib.SYMBOLS['nisqa_pool_profile_bwd']
    assert restype is ctypes.c_int and argtypes == [lib.c_p if '*' in p else lib.c_i32 for p in PARAMS]
    if not os.path.isfile(lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert 'nisqa_pool_profile_bwd' in lib.exported_symbols(lib.LIB_PATH, 'nisqa_pool_')
    L = lib.load()
    one, E = 16, lib.NISQA_ERR_ARG                                  # a non-NULL pointer that is never followed: the guards come first
    call = lambda x=one, ld=64, to=one, nw=one, b=3, np_=192, h=5, mode=0, w=one, dw=one, dl=one, de=one, dx=one: \
        L.nisqa_pool_profile_bwd(x, ld, to, nw, b, np_, h, mode, w, dw, dl, de, dx, None)
    for kw in ('x', 'to', 'nw', 'w', 'dx'):
        assert call(**{kw: None}) == E, kw
    assert call(b=0) == E and call(b=-2) == E and call(np_=0) == E and call(np_=-64) == E
    assert call(h=0) == E and call(h=6) == E and call(h=-1) == E
    assert call(mode=1) == E and call(mode=1, ld=256, h=1) == E and call(mode=2) == E and call(mode=-1) == E      # PoolAvg: no entry
    assert call(ld=256) == E and call(ld=63) == E and call(ld=0) == E
    # the absent cotangents do not make a call malformed: it is still refused for what is malformed
    assert call(dw=None, dl=None, de=None, dx=None) == E and call(dw=None, b=0) == E


def _model(model, args):
    from nisqa_amd import NISQA_lib as NL
    from oracle import ref_shim
    m = getattr(NL, model)(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
    m.eval()
    return m


def _model_de(**extra):
    import de_oracle as DO
    from nisqa_amd import NISQA_lib as NL
    args = dict(DO.de_args(), **extra)
    return NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)


def _y():
    return torch.zeros(2, 9600).requires_grad_(True)


@pytest.mark.parametrize('precision', ['f16x4', 'f16x3', 'bf16x3'])
def test_fast_precisions_refuse_a_differentiable_profile_before_any_gpu_work(monkeypatch, precision):
    """by name, as forward_audio refuses a gradient, single-ended and double-ended; the engine is never built"""
    monkeypatch.setenv('NISQA_HIP_PRECISION', precision)
    m = _model('NISQA_DIM', dict(synth.DIM_ARGS))
    with pytest.raises(NotImplementedError, match=precision) as mine:
        m.profile_audio(_y(), 48000, differentiable=True)
    with pytest.raises(NotImplementedError, match=precision) as theirs:
        m.forward_audio(_y(), 48000)
    assert str(mine.value) == str(theirs.value) and m._engine is None
    d = _model_de()
    for a, b in ((_y(), torch.zeros(2, 9600)), (torch.zeros(2, 9600), _y()), (_y(), _y())):
        with pytest.raises(NotImplementedError, match=precision) as mine:
            d.profile_audio(a, b, 48000, differentiable=True)
        with pytest.raises(NotImplementedError, match=precision) as theirs:
            d.forward_audio(a, b, 48000)
        assert str(mine.value) == str(theirs.value) and d._engine is None


def test_a_resampling_checkpoint_refuses_a_differentiable_profile_before_any_gpu_work(monkeypatch):
    monkeypatch.delenv('NISQA_HIP_PRECISION', raising=False)
    m = _model('NISQA', dict(synth.MOS_ARGS, ms_sr=16000))
    with pytest.raises(NotImplementedError, match='resampler') as mine:
        m.profile_audio(_y(), 48000, differentiable=True)
    with pytest.raises(NotImplementedError, match='resampler') as theirs:
        m.forward_audio(_y(), 48000)
    assert str(mine.value) == str(theirs.value) and '48000 != 16000' in str(mine.value) and m._engine is None
    d = _model_de(ms_sr=16000)
    with pytest.raises(NotImplementedError, match='resampler') as mine:
        d.profile_audio(torch.zeros(2, 9600), _y(), 48000, differentiable=True)
    with pytest.raises(NotImplementedError, match='resampler') as theirs:
        d.forward_audio(torch.zeros(2, 9600), _y(), 48000)
    assert str(mine.value) == str(theirs.value) and d._engine is None


def test_the_bilstm_with_pool_avg_refuses_a_differentiable_profile_by_name(monkeypatch):
    """its backward through time takes a pooled gradient, not one per step; pools without a profile keep their own refusal"""
    from nisqa_amd import engine
    monkeypatch.delenv('NISQA_HIP_PRECISION', raising=False)
    m = _model('NISQA', dict(LO.LSTM_AVG_ARGS))
    with pytest.raises(NotImplementedError, match=r'BiLSTM.*pool=avg'):
        m.profile_audio(_y(), 48000, differentiable=True)
    assert m._engine is None
    with pytest.raises(NotImplementedError, match=r'BiLSTM.*pool=avg'):
        engine.check_profile_grad_args(LO.LSTM_AVG_ARGS)
    with pytest.raises(NotImplementedError, match='pool=max'):
        engine.check_profile_grad_args(dict(LO.LSTM_AVG_ARGS, pool='max'))
    engine.check_profile_grad_args(synth.DIM_ARGS)
    engine.check_profile_args(LO.LSTM_AVG_ARGS)                      # the plain profile of that family keeps working


@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_restatement_obeys_the_identity_with_the_score_gradient(model):
    """score = sum_t weights_t local_t: with c_w = g * local and c_l = g * weights the profile's gradient in x is
    input_grad_oracle.oracle's for g, in float64 to 1e-9 of each clip's largest entry; the score is that oracle's"""
    sd, args, x, n_wins, g = IG.case(model)
    at = PG.oracle(sd, args, x, n_wins, [])
    got = PG.oracle(sd, args, x, n_wins, [PG.identity_cotangents(at['weights'], at['local'], g), {'g': g}])
    want = IG.oracle(sd, args, x, n_wins, [g])
    assert np.abs(got['y'] - want['y']).max() <= 1e-12 and np.array_equal(got['margin'], want['margin'])
    assert np.abs((at['weights'] * at['local']).sum(1) - want['y']).max() <= 1e-12
    for dx in got['dx']:
        err = IG.clip_error(dx, want['dx'][0])
        print(model, 'relative distance per clip', err)
        assert (err <= 1e-9).all()
        for b, n in enumerate(n_wins):
            assert (dx[b, n:] == 0).all()
    # and the rows the pooling read are what profile_oracle's forward restatement is evaluated on
    for b, n in enumerate(n_wins):
        w, l = PO.profile(sd, at['embed'][b, :n], IG.heads_of(model), torch.float64)
        assert np.array_equal(w, at['weights'][b, :n]) and np.array_equal(l, at['local'][b, :n])


@pytest.mark.parametrize('model', ['NISQA_DIM', 'NISQA'])
def test_restatement_against_the_reference_modules_hooked_at_the_pooling(model):
    """The reference's module tree in float64, eval mode, with a forward hook on every pooling module (model.pool; NISQA_DIM:
    model.pool_layers[h]) that takes the hooked module's input and n_wins and forms the profile with the module's OWN linear layers and
    mask; the scalar sum c_w * weights + sum c_l * local + sum c_e * embed + sum g * score backpropagates to x through the
    reference's CNN and self-attention.  Against the restatement to 1e-9 of each clip's largest entry; padding rows hold NaN
    cotangents on the restatement's side."""
    from oracle import ref_shim
    if not ref_shim.reference_available():
        pytest.skip('reference tree not staged')
    sd, args, x, n_wins, g = IG.case(model)
    B, L, H = x.shape[0], x.shape[1], len(IG.heads_of(model))
    cot = PG.random_cotangents(3, B, L, H)
    ref = ref_shim.build_reference_model(args, sd)[0].double()
    seen = []

    def hook(mod, inputs, output):
        xin, nw = inputs
        att = mod.model.linear2(torch.relu(mod.model.linear1(xin))).squeeze(2)                  # [B, L]
        mask = torch.arange(xin.shape[1])[None, :] < nw[:, None]          # (the reference drops the rows behind the longest clip)
        seen.append((torch.softmax(att.masked_fill(~mask, float('-inf')), 1), mod.model.linear3(xin).squeeze(2), xin, mask))
    pools = list(ref.pool_layers) if model == 'NISQA_DIM' else [ref.pool]
    handles = [p.register_forward_hook(hook) for p in pools]
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y = ref(xt, torch.as_tensor(n_wins))
    for h_ in handles:
        h_.remove()
    assert len(seen) == H
    scalar = (torch.from_numpy(cot['g'].astype(np.float64)) * y).sum()
    f = lambda a: torch.from_numpy(a[:, :seen[0][2].shape[1]].astype(np.float64))
    for h, (w, l, xin, mask) in enumerate(seen):
        scalar = scalar + (f(cot['w'][:, :, h]) * w)[mask].sum() + (f(cot['l'][:, :, h]) * l)[mask].sum()
    scalar = scalar + (f(cot['e']) * seen[0][2])[seen[0][3]].sum()
    scalar.backward()
    nan_pad = {k: v.copy() for k, v in cot.items()}
    for b, n in enumerate(n_wins):
        for k in 'wle':
            nan_pad[k][b, n:] = np.nan
    want = PG.oracle(sd, args, x, n_wins, [nan_pad])
    assert np.abs(y.detach().numpy() - want['y']).max() <= 1e-10
    for h, (w, l, _, _) in enumerate(seen):
        for b, n in enumerate(n_wins):
            assert np.abs(w[b, :n].detach().numpy() - want['weights'][b, :n, h]).max() <= 1e-12
            assert np.abs(l[b, :n].detach().numpy() - want['local'][b, :n, h]).max() <= 1e-10
    err = IG.clip_error(xt.grad.numpy(), want['dx'][0])
    print(model, 'relative distance per clip', err)
    assert np.isfinite(want['dx'][0]).all() and (err <= 1e-9).all()


def test_pool_level_restatement_is_the_network_level_one():
    """pool_grad (what the kernel is held to) on the rows the network oracle's pooling read gives the cotangent that, pushed through
    nothing else, reproduces the identity at the pooling's input: its gradient for c_w = g * local, c_l = g * weights is autograd's of
    oracle.net.pool_att_ff for g"""
    sd = {k: v.double() for k, v in synth.random_state_dict(7, 'NISQA_DIM').items() if k.startswith('pool')}
    rows = np.random.default_rng(2).standard_normal((70, 64))
    w, l = PO.profile(sd, rows, PO.DIM_HEADS, torch.float64)
    g = np.random.default_rng(3).standard_normal(5)
    got = PG.pool_grad(sd, rows, PO.DIM_HEADS, cw=g[None] * l, cl=g[None] * w)
    from oracle import net as onet
    xt = torch.from_numpy(rows).requires_grad_(True)
    y = torch.cat([onet.pool_att_ff(sd, xt, p) for p in PO.DIM_HEADS])
    want, = torch.autograd.grad((y * torch.from_numpy(g)).sum(), xt)
    assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
    ce = np.random.default_rng(4).standard_normal((70, 64))
    assert np.array_equal(PG.pool_grad(sd, rows, PO.DIM_HEADS, ce=ce), ce)
    one = PG.pool_grad(sd, rows[:1], PO.DIM_HEADS, cw=np.ones((1, 5)))
    assert (one == 0).all()                                        # one token: its weight is 1 whatever x is
