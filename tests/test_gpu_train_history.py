"""The three training steps on dirty workspaces and after shape changes, on the MI355X (run with -m gpu).  Shapes, data and oracle:
tests/train_history_cases.py; their conditioning: tests/test_train_history_host.py.

1. a clean step (fresh trainer, one shape) of HipTrainer against the float64 oracle -- the anchor;
2. one HipTrainer walking BIG -> TINY -> EDGE -> PERM -> TINY -> BIG with its state restored before every step, so that every step
   must reproduce the clean step of its shape: as is, with every float of reused and fresh scratch set to NaN (byte 0xFF) before
   each step, and with 3.39e38 (byte 0x7F).  Differential: same code, same inputs, only the order of atomics differs;
3. the same walk and poison for HipTrainerLSTM and HipTrainerDE;
4. three steps without restoring: Adam moments, parameters and BatchNorm buffers against a float64 recurrence fed with the
   trainer's own gradients.

What is poisoned: the fused block's workspace and fragment buffer (pre-set larger than BIG needs, so they are never reallocated),
the flat gradient buffer(s), the float64 sums, the convolutions' weight fragments, and everything _FlatTrainer._new hands out
(replaced on the instance by a function that allocates and byte-fills) -- deterministically, not through the caching allocator.
Only floating-point memory: int32 scratch holds indices, and a stale index is an address, not a value."""
import numpy as np
import pytest
import torch

import train_history_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LR = 1e-3
PRECISIONS = ['f32', 'bf16x6', 'f16x4']
POISONS = [None, 0xFF, 0x7F]
_CLEAN = {}


# ---- one step's results, and the differential bars ---------------------------------------------------------------------------
def _capture(tr, loss):
    torch.cuda.synchronize()
    sd = tr.state_dict()
    out = dict(loss=float(loss), y_hat=tr.last['y_hat'].cpu().numpy().copy(), grads={k: v.numpy() for k, v in tr.grads().items()},
               params={k: v.numpy() for k, v in sd.items() if k in tr.keys},
               bufs={k: v.numpy() for k, v in sd.items() if 'running' in k},
               nbt={k: int(v) for k, v in sd.items() if k.endswith('num_batches_tracked')})
    if getattr(tr, 'last_idx', None) is not None:
        out['idx'] = tr.last_idx.cpu().numpy().copy()
    return out


def _restore(tr, sd):
    tr.load_state_dict(sd)
    tr.m.zero_()
    tr.v.zero_()
    tr.t = 0


def _same_step(clean, got, what, worst):
    """the bars for "same arithmetic, other summation order" (test_training_step_at_other_depths, fused against operator path; the
    Adam rule of test_training_step_matches_reference_fixture); worst: {quantity: largest figure so far}, updated"""
    def note(q, v):
        worst[q] = max(worst.get(q, 0.0), float(v))
        return float(v)

    assert np.isfinite(got['loss']) and np.isfinite(got['y_hat']).all(), what
    for part in ('grads', 'params', 'bufs'):
        assert set(got[part]) == set(clean[part])
        for k, v in got[part].items():
            assert np.isfinite(v).all(), (what, part, k)
    assert note('loss', abs(got['loss'] - clean['loss']) / abs(clean['loss'])) < 1e-5, what
    assert note('y_hat', np.abs(got['y_hat'] - clean['y_hat']).max()) < 1e-5, what
    if 'idx' in clean:
        assert np.array_equal(got['idx'], clean['idx']), what
    for k, g0 in clean['grads'].items():
        g1, top = got['grads'][k], float(np.abs(g0).max())
        if top < 1e-4:                   # analytically zero (conv biases, the score bias under the softmax): stays rounding noise
            assert note('zero grad', np.abs(g1).max()) < 1e-4, (what, k)
            continue
        assert note('grad', np.abs(g1 - g0).max() / max(1e-3, top)) < 2e-5, (what, k)
        solid = (np.abs(g0) > 1e-3 * max(1e-3, top)) & (not C.conv_bias(k))
        d = np.abs(got['params'][k] - clean['params'][k])
        assert note('param (solid)', d[solid].max(initial=0)) < 1e-4, (what, k)
    for k, p0 in clean['params'].items():
        assert note('param', np.abs(got['params'][k] - p0).max()) <= 2.002 * LR, (what, k)
    for k, b0 in clean['bufs'].items():
        assert note('buffer', np.abs(got['bufs'][k] - b0).max() / max(1.0, float(np.abs(b0).max()))) < 1e-6, (what, k)
    assert got['nbt'] == clean['nbt'], what


# ---- poison ------------------------------------------------------------------------------------------------------------------
def _fill(t, byte):
    if t is not None and t.numel():
        t.view(-1).view(torch.uint8).fill_(byte)


def _persistent(tr):
    """the float memory a trainer keeps from step to step and must clear or overwrite itself"""
    out = [tr.gflat, tr._sums, getattr(tr, 'gflat2', None), getattr(tr, '_td_ws', None), getattr(tr, '_td_frags', None)]
    out += list(getattr(tr, '_sc_frags', {}).values()) + list(getattr(tr, '_sc32_frags', {}).values())
    return [t for t in out if t is not None]


def _poison_new(tr, byte, count):
    def new(*shape, dtype=torch.float32):
        t = torch.empty(shape, dtype=dtype, device=tr.device)
        if dtype != torch.int32:         # float32 scratch and the 16-bit weight fragments; indices are left alone
            _fill(t, byte)
        count[0] += 1
        return t
    tr._new = new


def _walk(tr, sd, steps, clean_of, byte, what):
    """steps: [(name, run(tr) -> loss)]; every step from the restored initial state against clean_of(name) -> (worst figures,
    patched allocations)"""
    count, worst, ws = [0], {}, set()
    if byte is not None:
        _poison_new(tr, byte, count)
        ws.add(tr._td_ws.data_ptr() if getattr(tr, '_td_ws', None) is not None else None)
    for i, (name, run) in enumerate(steps):
        _restore(tr, sd)
        if byte is not None:
            for t in _persistent(tr):
                _fill(t, byte)
        got = _capture(tr, run(tr))
        _same_step(clean_of(name), got, '%s, step %d (%s)' % (what, i, name), worst)
        ws.add(tr._td_ws.data_ptr() if getattr(tr, '_td_ws', None) is not None else None)
    assert len(ws) == 1, ws                                          # one workspace (or none) from the first step to the last
    if byte is not None:
        assert count[0] > 10 * len(steps), count[0]                  # the patched _new is the one the step allocates through
    print('%s, byte %s, %d patched allocations: worst clean-vs-walk ' % (what, 'none' if byte is None else hex(byte), count[0])
          + ', '.join('%s %.2e' % kv for kv in sorted(worst.items())))
    return worst, count[0]


# ---- HipTrainer ----------------------------------------------------------------------------------------------------------------
def _trainer(model, path, precision, monkeypatch):
    from nisqa_amd.train import HipTrainer
    monkeypatch.setenv('NISQA_HIP_TRAIN_FUSED_TD', '1' if path == 'fused' else '0')
    tr = HipTrainer(C.model_args(model), C.state_dict(model), DEV, lr=LR, precision=precision)
    assert tr.fused_td == (path == 'fused') and tr.precision == precision
    return tr


def _run(model, shape):
    specs, y = C.data(model, shape)
    return lambda tr: tr.step_spec(specs, y)


def _clean(model, shape, path, precision, monkeypatch):
    """one step of a fresh trainer, cached"""
    key = (model, shape, path, precision)
    if key not in _CLEAN:
        tr = _trainer(model, path, precision, monkeypatch)
        _CLEAN[key] = _capture(tr, _run(model, shape)(tr))
        assert list(tr.L) == C.SHAPES[shape]
        if path == 'fused':
            assert tr._td_plan_cur['NP'] == C.TABLE[shape][1]
    return _CLEAN[key]


@pytest.mark.parametrize('path', ['fused', 'operator'])
@pytest.mark.parametrize('model,shape', C.CASES)
def test_clean_step_against_float64(model, shape, path, monkeypatch):
    """Loss to 1e-4 relative, y_hat to 1e-4, running buffers to 2e-4 max(1, max |want|), every gradient tensor to max(3e-3, twice
    what torch's float32 evaluation of the oracle is off by) of max(1e-3, max |want|): the bars of the masked-step and layer-count
    tests; the second term is below 6e-4 at every case (tests/test_train_history_host.py), so it can hide nothing."""
    got, ref = _clean(model, shape, path, 'f32', monkeypatch), C.oracle_step(model, shape)
    f32 = C.f32_oracle_margin(model, shape)[2]
    assert max(f32.values()) < C.F32_ORACLE_BAR
    ge = C.grad_errors(got['grads'], ref['grads'])
    for k in got['grads']:
        if C.conv_bias(k):
            assert np.abs(got['grads'][k]).max() == 0.0, k           # kept at the cleared value
    wk = max(ge, key=ge.get)
    dl = abs(got['loss'] - ref['loss']) / abs(ref['loss'])
    dy = float(np.abs(got['y_hat'] - ref['y_hat']).max())
    db = max(float(np.abs(got['bufs'][k] - w).max()) / max(1.0, float(np.abs(w).max())) for k, w in ref['bufs'].items())
    print('%s %s %s: clean step against float64: loss %.2e relative, y_hat %.2e, buffers %.2e, worst gradient tensor %.2e (%s; the '
          'float32 oracle there: %.2e)' % (model, shape, path, dl, dy, db, ge[wk], wk, f32[wk]))
    assert dl < 1e-4
    assert dy < 1e-4
    assert db < 2e-4
    assert got['nbt'] == {k: int(v) + 1 for k, v in C.state_dict(model).items() if k.endswith('num_batches_tracked')}
    assert len(got['nbt']) == 6
    for k, e in ge.items():
        assert e < max(3e-3, 2 * f32[k]), (k, e, f32[k])


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('path', ['fused', 'operator'])
@pytest.mark.parametrize('model', sorted(C.MODELS))
def test_walk_over_shapes_reproduces_the_clean_steps_on_poisoned_memory(model, path, precision, monkeypatch):
    sd = C.state_dict(model)
    clean_of = lambda shape: _clean(model, shape, path, precision, monkeypatch)
    steps = [(shape, _run(model, shape)) for shape in C.WALK]
    tr = _trainer(model, path, precision, monkeypatch)
    for byte in POISONS:
        if byte is not None and path == 'fused':
            # larger than BIG needs, so that the walk never reallocates them and every later step runs inside these very bytes
            pl = tr._td_plan(np.asarray(C.SHAPES['BIG']))[1]
            tr._td_ws = torch.empty(pl['ws'] + pl['ws'] // 4 + 4096, dtype=torch.float32, device=DEV)
            tr._td_frags = torch.empty(pl['frags'] + pl['frags'] // 4 + 4096, dtype=torch.float32, device=DEV)
        _walk(tr, sd, steps, clean_of, byte, '%s %s %s' % (model, path, precision))
        assert (tr._td_ws is not None) == (path == 'fused')
    assert tr.t == 1 and tr._prep_key == np.asarray(C.SHAPES['BIG'], np.int64).tobytes()


# ---- the other two trainers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pool', ['avg', 'max', 'last_step_bi'])
def test_lstm_walk_reproduces_the_clean_steps_on_poisoned_memory(pool):
    from nisqa_amd.train_lstm import HipTrainerLSTM
    args, sd, batches = C.lstm_case(pool)
    clean = {}
    for name, (specs, y) in batches.items():
        tr = HipTrainerLSTM(args, sd, DEV, lr=LR)
        clean[name] = _capture(tr, tr.step_spec(specs, y))
    steps = [(name, (lambda tr, b=batches[name]: tr.step_spec(*b))) for name in C.LSTM_WALK]
    tr = HipTrainerLSTM(args, sd, DEV, lr=LR)
    for byte in POISONS:
        _walk(tr, sd, steps, clean.__getitem__, byte, 'LSTM ' + pool)


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
@pytest.mark.parametrize('name', sorted(C.DE_CASES))
def test_double_ended_walk_reproduces_the_clean_steps_on_poisoned_memory(name, precision):
    from nisqa_amd.train_de import HipTrainerDE
    args, sd, batches = C.de_case(name)
    run = lambda b: (lambda tr: tr.step_spec(b[0], b[1], b[2], masks=b[3], bias=b[4]))
    clean = {}
    for which, b in batches.items():
        tr = HipTrainerDE(args, sd, DEV, lr=LR, precision=precision)
        clean[which] = _capture(tr, run(b)(tr))
        assert clean[which]['nbt'] == {k: int(v) + 2 for k, v in sd.items() if k.endswith('num_batches_tracked')}
    steps = [(which, run(batches[which])) for which in C.DE_WALK]
    tr = HipTrainerDE(args, sd, DEV, lr=LR, precision=precision)
    for byte in POISONS:
        _walk(tr, sd, steps, clean.__getitem__, byte, 'DE %s %s' % (name, precision))


# ---- carried state ---------------------------------------------------------------------------------------------------------------
def test_three_steps_without_restoring_carry_adam_and_batchnorm_state(monkeypatch):
    """BIG -> TINY -> EDGE on one trainer.  The Adam recurrence in float64 on the host, fed with the trainer's own gradient buffer
    of each step (what grads() returns, in the flat layout, the padding between tensors included), so that gradient conditioning
    plays no part: moments to 2e-6 of the tensor's largest entry (a few fp32 ulps of a two-term recurrence over three steps),
    parameters to 1e-6 (test_layernorm_softmax_elementwise_loss_adam); running buffers against the float64 oracle's batch
    statistics at the trainer's own weights, carried by the momentum-0.1 recurrence from the trainer's own previous buffers.

    The moments are held twice: tr.m and tr.v each as the one flat tensor it is, to 2e-6 of its largest entry, and every
    parameter's slice of them to 2e-6 of the slice's largest recurrence TERM, 0.9 |m| + 0.1 |g| (0.999 v + 0.001 g^2: v itself).
    Rounding is a few ulps of the terms, not of their sum: pool_layers.3.model.linear3.bias is one number whose gradient changes
    sign between BIG and TINY (3.4757, then -3.1060), so m = 0.31282 - 0.31060 = 2.2218e-3 after step 2, and the fp32 moment's
    1.4e-8 (half an ulp of 0.31) is 6.4e-6 of that remainder -- measured; no fp32 recurrence can do better there."""
    model = 'NISQA_DIM'
    tr = _trainer(model, 'fused', 'f32', monkeypatch)
    args = C.model_args(model)
    p = tr.flat.cpu().numpy().astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    worst = {}
    for t, shape in enumerate(['BIG', 'TINY', 'EDGE'], 1):
        specs, y = C.data(model, shape)
        before = tr.state_dict()
        loss = tr.step_spec(specs, y)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss))
        g = tr.gflat.cpu().numpy()
        for k, gk in tr.grads().items():
            assert np.array_equal(tr._to_kernel(k, gk).reshape(-1).numpy(), g[tr.off[k]:tr.off[k] + int(np.prod(tr.kshape[k]))]), k
        terms = {'m': 0.9 * np.abs(m) + 0.1 * np.abs(g), 'v': 0.999 * v + 0.001 * g.astype(np.float64) ** 2}
        p, m, v = C.adam_f64(p, g, m, v, t, LR)
        got = {'m': tr.m.cpu().numpy(), 'v': tr.v.cpu().numpy(), 'p': tr.flat.cpu().numpy()}
        for q, want in (('m', m), ('v', v)):                           # tr.m and tr.v, each as the one tensor it is
            e = float(np.abs(got[q] - want).max()) / float(np.abs(want).max())
            worst[q + ' (flat)'] = max(worst.get(q + ' (flat)', 0.0), e)
            assert e < 2e-6, (t, q, e)
        for k in tr.keys:
            sl = slice(tr.off[k], tr.off[k] + int(np.prod(tr.kshape[k])))
            for q, want in (('m', m), ('v', v)):
                e = float(np.abs(got[q][sl] - want[sl]).max()) / max(float(terms[q][sl].max()), 1e-30)
                worst[q] = max(worst.get(q, 0.0), e)
                assert e < 2e-6, (t, q, k, e)
            e = float(np.abs(got['p'][sl] - p[sl]).max())
            worst['p'] = max(worst.get('p', 0.0), e)
            assert e < 1e-6, (t, k, e)
        after = tr.state_dict()
        want = C.next_buffers({k: b.numpy() for k, b in before.items() if 'running' in k}, C.batch_stats(before, args, specs))
        for k, w in want.items():
            e = float(np.abs(after[k].numpy() - w).max()) / max(1.0, float(np.abs(w).max()))
            worst['buffer'] = max(worst.get('buffer', 0.0), e)
            assert e < 2e-4, (t, k, e)
        assert all(int(after[k]) == int(C.state_dict(model)[k]) + t for k in after if k.endswith('num_batches_tracked'))
    assert tr.t == 3
    print('carried state over BIG -> TINY -> EDGE: worst ' + ', '.join('%s %.2e' % kv for kv in sorted(worst.items())))
