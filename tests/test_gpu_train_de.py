"""NISQA_DE training on the MI355X (nisqa_amd/train_de.py, csrc/de_align.hip): the backward of alignment + fusion bit for bit
against a sequential fp32 restatement, the packed forward against tests/de_oracle.py, the whole step against fixtures written by
the reference's own modules in train mode (tests/golden/make_golden_train_de.py) and against the float64 restatement with explicit
dropout masks and a bias mapping (tests/de_train_oracle.py), the two-call BatchNorm semantics, and the loop."""
import functools
import os

import numpy as np
import pytest
import torch

import de_oracle as DO
import de_train_oracle as DT
import helpers
import lstm_train_oracle as LT
from nisqa_amd import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAIRS = [(1, 1), (1, 7), (7, 1), (65, 3), (64, 64), (130, 97)]
FUSE_ID = {'x/y/-': 0, '+/-': 1, 'x/y': 2}


def _p(t):
    return t.data_ptr() if t is not None else None


def _st():
    return torch.cuda.current_stream().cuda_stream


def _layout():
    """packed rows of the six pairs in ONE token buffer, degraded clips first: the trainer's layout"""
    Lx, Ly = np.array([p[0] for p in PAIRS]), np.array([p[1] for p in PAIRS])
    off = np.concatenate(([0], np.cumsum(np.concatenate([Lx, Ly])))).astype(np.int32)
    return Lx, Ly, off


def _crafted_idx(Lx, Ly):
    rng = np.random.RandomState(5)
    idx = [np.zeros(1, np.int64), np.array([5]), np.zeros(7, np.int64), np.arange(65) % 3, rng.permutation(64),
           (np.arange(130) * 37) % 50]                       # (130, 97): not monotone, reference rows 50 .. 96 chosen by nobody
    assert all(len(i) == n and i.max() < m for i, n, m in zip(idx, Lx, Ly))
    return idx


def _bwd_restated(dF, idx, Lx, Ly, fuse):
    """fp32, one reference row's sum in ascending order of the degraded token, starting from +0"""
    g = [dF[:, 64 * k:64 * k + 64] for k in range(dF.shape[1] // 64)]
    if fuse == 'x/y/-':
        dx, dya = g[0] + g[2], g[1] - g[2]
    elif fuse == '+/-':
        dx, dya = g[0] + g[1], g[0] - g[1]
    else:
        dx, dya = g[0].copy(), g[1].copy()
    out, o = [], 0
    for i_b, nx, ny in zip(idx, Lx, Ly):
        acc = np.zeros((ny, 64), np.float32)
        for i in range(nx):
            acc[i_b[i]] = acc[i_b[i]] + dya[o + i]
        out.append(acc)
        o += nx
    return dx.astype(np.float32), np.concatenate(out)


@pytest.mark.parametrize('fuse', DO.FUSES)
def test_align_fuse_backward_kernel_bit_for_bit(fuse):
    from nisqa_amd import lib
    L = lib.load()
    Lx, Ly, off = _layout()
    B, Sx, Sy, F = len(PAIRS), int(Lx.sum()), int(Ly.sum()), DO.FUSE_WIDTH[fuse]
    ld = F + 8
    rng = np.random.RandomState(7)
    dF = np.full((Sx, ld), np.nan, np.float32)               # the columns behind F are never read
    dF[:, :F] = rng.standard_normal((Sx, F)).astype(np.float32)
    idx = _crafted_idx(Lx, Ly)
    want_dx, want_dref = _bwd_restated(dF[:, :F], idx, Lx, Ly, fuse)
    d_dF, d_idx = torch.from_numpy(dF).to(DEV), torch.from_numpy(np.concatenate(idx).astype(np.int32)).to(DEV)
    d_off, d_n = torch.from_numpy(off).to(DEV), torch.from_numpy(np.concatenate([Lx, Ly]).astype(np.int32)).to(DEV)
    runs = []
    for _ in range(2):
        out = torch.full((Sx + Sy + 3, 64), float('nan'), dtype=torch.float32, device=DEV)      # three guard rows behind the last token
        lib.check(L.nisqa_de_align_fuse_bwd(_p(d_dF), ld, _p(d_idx), _p(d_off), _p(d_n), _p(d_off) + 4 * B, _p(d_n) + 4 * B, B,
                                            int(max(Lx.max(), Ly.max())), FUSE_ID[fuse], _p(out), _p(out), _st()), 'bwd')
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy())
    got = runs[0]
    assert np.isnan(got[Sx + Sy:]).all()                      # nothing behind the last token is touched
    assert not np.isnan(got[:Sx + Sy]).any()                  # every row of every token of both sides is written
    assert np.array_equal(got[:Sx].view(np.uint32), want_dx.view(np.uint32))
    assert np.array_equal(got[Sx:Sx + Sy].view(np.uint32), want_dref.view(np.uint32))
    chosen = np.zeros(97, bool)
    chosen[idx[5]] = True
    r0 = Sx + int(Ly[:5].sum())
    assert (got[r0:r0 + 97][~chosen] == 0).all() and (~chosen).sum() == 47
    assert np.array_equal(runs[0][:Sx + Sy].view(np.uint32), runs[1][:Sx + Sy].view(np.uint32))
    # two output buffers, each addressed by its own side's offsets, give the same rows
    a = torch.full((Sx, 64), float('nan'), dtype=torch.float32, device=DEV)
    b = torch.full((Sy, 64), float('nan'), dtype=torch.float32, device=DEV)
    r_off = torch.from_numpy((off[B:] - off[B]).astype(np.int32)).to(DEV)
    lib.check(L.nisqa_de_align_fuse_bwd(_p(d_dF), ld, _p(d_idx), _p(d_off), _p(d_n), _p(r_off), _p(d_n) + 4 * B, B,
                                        int(max(Lx.max(), Ly.max())), FUSE_ID[fuse], _p(a), _p(b), _st()), 'bwd')
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), want_dx.view(np.uint32))
    assert np.array_equal(b.cpu().numpy().view(np.uint32), want_dref.view(np.uint32))


@pytest.mark.parametrize('align', DO.ALIGNS)
@pytest.mark.parametrize('fuse', DO.FUSES)
def test_packed_forward_matches_the_oracle_and_feeds_the_backward(align, fuse):
    """The forward alignment the trainer calls, on random first-self-attention outputs: indices where the top-2 gap exceeds 1e-5 and
    fused rows to 1e-5 (the bounds of DESIGN.md 4.8 / tests/test_gpu_de.py), nothing outside the valid rows written; the backward
    of the indices the forward wrote equals the restatement fed with the same indices."""
    from nisqa_amd import lib
    L = lib.load()
    Lx, Ly, off = _layout()
    B, Sx, Sy, F = len(PAIRS), int(Lx.sum()), int(Ly.sum()), DO.FUSE_WIDTH[fuse]
    rng = np.random.RandomState(11)
    x = rng.standard_normal((Sx + Sy, 64)).astype(np.float32)
    d_x = torch.from_numpy(x).to(DEV)
    d_off, d_n = torch.from_numpy(off).to(DEV), torch.from_numpy(np.concatenate([Lx, Ly]).astype(np.int32)).to(DEV)
    tiles = np.concatenate(([0], np.cumsum((Lx + 63) // 64))).astype(np.int32)
    d_tiles = torch.from_numpy(tiles).to(DEV)
    fused = torch.full((Sx + 2, F), float('nan'), dtype=torch.float32, device=DEV)
    idx = torch.full((Sx + 2,), -7, dtype=torch.int32, device=DEV)
    lib.check(L.nisqa_de_align_fuse_packed(_p(d_x), _p(d_off), _p(d_n), _p(d_off) + 4 * B, _p(d_n) + 4 * B, _p(d_tiles), B,
                                           int(tiles[-1]), {'dot': 0, 'cosine': 1}[align], FUSE_ID[fuse], F, _p(fused), _p(idx),
                                           _st()), 'fwd')
    torch.cuda.synchronize()
    f, k = fused.cpu().numpy(), idx.cpu().numpy()
    assert np.isnan(f[Sx:]).all() and (k[Sx:] == -7).all() and np.isfinite(f[:Sx]).all()
    per_pair = []
    for b, (nx, ny) in enumerate(PAIRS):
        r0, c0 = off[b], off[B + b]
        xd, xr = x[r0:r0 + nx].astype(np.float64), x[c0:c0 + ny].astype(np.float64)
        _, widx, gap = DO.align_fuse(xd, xr, align, 'hard', fuse)
        kb = k[r0:r0 + nx]
        assert ((kb >= 0) & (kb < ny)).all()
        sure = gap > 1e-5
        assert (kb[sure] == widx[sure]).all(), b
        assert np.abs(f[r0:r0 + nx] - DO.fuse_rows(xd, xr[kb], fuse)).max() <= 1e-5
        per_pair.append(kb.astype(np.int64))
    dF = rng.standard_normal((Sx, F)).astype(np.float32)
    want_dx, want_dref = _bwd_restated(dF, per_pair, Lx, Ly, fuse)
    out = torch.full((Sx + Sy, 64), float('nan'), dtype=torch.float32, device=DEV)
    lib.check(L.nisqa_de_align_fuse_bwd(_p(torch.from_numpy(dF).to(DEV)), F, _p(idx), _p(d_off), _p(d_n), _p(d_off) + 4 * B,
                                        _p(d_n) + 4 * B, B, 130, FUSE_ID[fuse], _p(out), _p(out), _st()), 'bwd')
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:Sx].view(np.uint32), want_dx.view(np.uint32))
    assert np.array_equal(got[Sx:].view(np.uint32), want_dref.view(np.uint32))


# ---- the whole step --------------------------------------------------------------------------------------------
def _conv_bias(k):
    return k.startswith('cnn.model.conv') and k.endswith('.bias')


def _grad_errors(grads, want):
    """worst max |err| / max(1e-3, max |want|) over the tensors (the bar of tests/test_gpu_train.py); the conv biases' gradients,
    zero under train-mode BatchNorm, must stay at the cleared value"""
    worst, wk = 0.0, None
    assert set(grads) == set(want)
    for k, gr in grads.items():
        assert tuple(gr.shape) == tuple(want[k].shape), k
        if _conv_bias(k):
            assert np.abs(gr.numpy()).max() == 0.0, k
            continue
        e = float(np.abs(gr.numpy() - want[k]).max()) / max(1e-3, float(np.abs(want[k]).max()))
        if e > worst:
            worst, wk = e, k
    return worst, wk


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
@pytest.mark.parametrize('name', ['cos_xym', 'dot_pm'])
def test_training_step_matches_reference_fixture(name, precision):
    """Bars: those tests/test_gpu_train.py holds HipTrainer to against train_mos.npz -- loss to 1e-4 relative, y_hat to 1e-4,
    gradients to 1e-3 of max(1e-3, the tensor's largest entry) -- with, after step 1, the running mean to 1e-5 and the running
    variance to 1e-4 of max(1, the buffer's largest entry) (that test: 2e-4 for both).
    Step 2 follows one Adam update, which moves a parameter by lr g / (|g| + 1e-8): about lr whatever the gradient's size.  The
    conv biases' gradients are zero under train-mode BatchNorm; the trainer keeps them at exactly zero, the reference's autograd
    leaves rounding noise (fixture cos_xym: up to 7e-6 in conv1.bias), which Adam turns into moves of up to 0.9986e-3.  A conv
    bias shifts its BatchNorm's batch mean one to one and nothing else, so the fixture's running means after step 2 carry up
    to 0.19 lr = 1.9e-4 of that noise from their own bias alone, more through the layers in front (measured distance to the
    trainer: 7.3e-5 in bn1.running_mean, at most 4.2e-4 in bn4 / bn5 of cos_xym, the same to three digits in 'f32' and 'bf16x6':
    it is the fixture's side that moved), and no step that keeps those gradients at zero can meet 1e-5 there.  Step 2 is therefore held to what that test holds it to: loss2 (and here
    y_hat2) to 2e-2, the running buffers to 1e-3 of max(1, the buffer's largest entry)."""
    from nisqa_amd.train_de import HipTrainerDE
    g, gc = helpers.golden('train_de_%s.npz' % name), helpers.golden('train_de_%s_cnn.npz' % name)
    assert min(float(g['gap1']), float(g['gap2'])) >= 1e-4
    args = DT.de_train_args(str(g['align']), str(g['fuse']))
    sd = DO.random_de_state_dict(int(g['seed_sd']), args['de_fuse'])
    specs_d, y = LT.batch(int(g['seed_deg']), DT.FRAMES_DEG)
    specs_r, _ = LT.batch(int(g['seed_ref']), DT.FRAMES_REF)
    tr = HipTrainerDE(args, sd, DEV, lr=float(g['lr']), precision=precision)
    loss = tr.step_spec(specs_d, specs_r, y)
    torch.cuda.synchronize()
    assert np.array_equal(tr.last_idx.cpu().numpy(), g['idx1'])              # every hard index, no exclusions
    want = {k[5:]: (g if k in g.files else gc)[k] for k in list(g.files) + list(gc.files) if k.startswith('grad/')}
    worst, wk = _grad_errors(tr.grads(), want)
    dy1 = float(np.abs(tr.last['y_hat'].cpu().numpy() - g['y_hat1']).max())
    print(name, precision, 'loss1', float(loss), float(g['loss1']), 'y_hat1 err', dy1, 'worst relative gradient error', worst, wk)
    assert float(loss) == pytest.approx(float(g['loss1']), rel=1e-4)
    assert dy1 < 1e-4
    assert worst < 1e-3, (worst, wk)

    def buffers(step):
        for k, v in tr.state_dict().items():
            w = g['sd%d/%s' % (step, k)] if 'running' in k or k.endswith('num_batches_tracked') else None
            if k.endswith('num_batches_tracked'):
                assert int(v) == int(w) == int(g['nbt0']) + 2 * step, k
            elif 'running' in k:
                e = float(np.abs(v.numpy() - w).max()) / max(1.0, float(np.abs(w).max()))
                print(name, precision, 'step', step, k, 'error %.3g' % e)
                assert e < (1e-3 if step == 2 else 1e-5 if k.endswith('running_mean') else 1e-4), (step, k, e)
    buffers(1)
    loss2 = tr.step_spec(specs_d, specs_r, y)
    torch.cuda.synchronize()
    dy2 = float(np.abs(tr.last['y_hat'].cpu().numpy() - g['y_hat2']).max())
    print(name, precision, 'loss2', float(loss2), float(g['loss2']), 'y_hat2 err', dy2)
    assert float(loss2) == pytest.approx(float(g['loss2']), rel=2e-2)
    assert dy2 < 2e-2 * max(1.0, float(np.abs(g['y_hat2']).max()))
    buffers(2)


def test_trained_weights_round_trip_into_the_mirror_and_the_engine():
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import HipNisqaDE
    from nisqa_amd.train_de import HipTrainerDE
    args = DT.de_train_args()
    sd = DO.random_de_state_dict(33)
    specs_d, y = LT.batch(93, [15, 97])
    specs_r, _ = LT.batch(1093, [40, 97])
    tr = HipTrainerDE(args, sd, DEV, lr=1e-3)
    tr.step_spec(specs_d, specs_r, y)
    new = tr.state_dict()
    assert list(new) == list(sd) and all(tuple(new[k].shape) == tuple(sd[k].shape) for k in sd)
    assert any(not torch.equal(new[k], sd[k]) for k in sd if k.startswith('time_dependency_2.'))
    mirror = NL.NISQA_DE(**DO.model_kwargs(args))
    mirror.load_state_dict(new, strict=True)
    tr2 = HipTrainerDE(args, mirror.state_dict(), DEV)        # and back, strict in the other direction
    assert all(torch.equal(tr2.state_dict()[k], new[k]) for k in new)
    eng = HipNisqaDE(args, new, DEV)
    out = eng.forward_items([(synth.synth_pcm16(1, 1.0), 48000), (synth.synth_pcm16(2, 1.5), 48000)])
    assert np.isfinite(out.cpu().numpy()).all()


# masks on every site (the two CNN calls' differ), a cubic bias mapping per clip, one NaN label: three pairs (1,7), (21,21), (72,62).
# Weight / batch seeds found on the CPU so that no argmax of the float64 step sits within 1e-4 of a tie (asserted below).
MASK_CASES = {'dot_pm': ('dot', '+/-', 41), 'cos_xy': ('cosine', 'x/y', 51)}


@functools.lru_cache(maxsize=None)
def _mask_case(name):
    """(the float64 step, the HIP step in 'f32', the oracle's inputs) -- computed once, shared by the tests below"""
    from nisqa_amd.train_de import HipTrainerDE
    align, fuse, seed = MASK_CASES[name]
    args = DT.de_train_args(align, fuse, cnn_dropout=0.2, td_sa_dropout=0.1, td_2_sa_dropout=0.1)
    sd = DO.random_de_state_dict(seed, fuse)
    specs_d, y = LT.batch(100 + seed, [15, 97, 300])
    specs_r, _ = LT.batch(1100 + seed, [40, 97, 260])
    y[1, 0], y[2, 0] = 3.0, np.nan
    segs_d, nw_d = DT.segments(specs_d, args)
    segs_r, nw_r = DT.segments(specs_r, args)
    assert nw_d.tolist() == [1, 21, 72] and nw_r.tolist() == [7, 21, 62]
    masks = DT.random_masks(seed, nw_d, nw_r, 2, 2, 0.2)
    assert not np.array_equal(masks['cnn_d2'][:20], masks['ref_cnn_d2'][:20])
    bias = np.array([[0.1, 0.9, 0.02, -0.003], [-0.2, 1.1, -0.01, 0.002], [0.05, 1.0, 0.0, 0.001]], np.float32)
    ref = DT.train_step(sd, args, segs_d, nw_d, segs_r, nw_r, y, masks=masks, bias=bias)
    tr = HipTrainerDE(args, sd, DEV, lr=1e-3, precision='f32')
    loss = tr.step_spec(specs_d, specs_r, y, masks=masks, bias=bias)
    torch.cuda.synchronize()
    got = dict(loss=float(loss), y_hat=tr.last['y_hat'].cpu().numpy(), grads=tr.grads(), idx=tr.last_idx.cpu().numpy(),
               bufs={k: v.numpy() for k, v in tr.state_dict().items() if 'running' in k})
    return ref, got, (sd, args, segs_d, nw_d, segs_r, nw_r, y, masks, bias)


@pytest.mark.parametrize('name', sorted(MASK_CASES))
def test_step_with_masks_and_bias_mapping_matches_the_float64_oracle(name):
    ref, got, _ = _mask_case(name)
    assert ref['gap'] >= 1e-4
    assert np.array_equal(got['idx'], np.concatenate(ref['idx']))
    worst, wk = _grad_errors(got['grads'], ref['grads'])
    dy = float(np.abs(got['y_hat'] - ref['y_hat']).max())
    print(name, 'loss', got['loss'], ref['loss'], 'y_hat err', dy, 'worst relative gradient error', worst, wk)
    assert got['loss'] == pytest.approx(ref['loss'], rel=1e-4)
    assert dy < 1e-4
    assert worst < 1e-3, (worst, wk)
    for k, w in ref['bufs'].items():
        e = float(np.abs(got['bufs'][k] - w).max()) / max(1.0, float(np.abs(w).max()))
        assert e < (1e-5 if k.endswith('running_mean') else 1e-4), (k, e)


def test_batchnorm_statistics_are_per_cnn_call():
    """One CNN pass over all 2B clips with pooled statistics -- the obvious shortcut -- is another model: the step is within the
    bar of the two-call oracle (the test above) and more than a hundred bars from the pooled one."""
    ref, got, (sd, args, segs_d, nw_d, segs_r, nw_r, y, masks, bias) = _mask_case('dot_pm')
    pooled = DT.train_step(sd, args, segs_d, nw_d, segs_r, nw_r, y, masks=masks, bias=bias, pooled_bn=True)
    far = max(float(np.abs(got['grads'][k].numpy() - pooled['grads'][k]).max()) / max(1e-3, float(np.abs(pooled['grads'][k]).max()))
              for k in ('cnn.model.bn2.weight', 'cnn.model.bn4.weight', 'cnn.model.conv3.weight'))
    near, _ = _grad_errors(got['grads'], ref['grads'])
    print('pooled-statistics model: relative gradient distance', far, 'two-call oracle:', near)
    assert far > 0.1 and near < 1e-3
    assert np.abs(got['bufs']['cnn.model.bn2.running_mean'] - pooled['bufs']['cnn.model.bn2.running_mean']).max() > 1e-3


# ---- the loop ---------------------------------------------------------------------------------------------------
def test_train_loop_on_pairs_writes_a_checkpoint_that_predicts(tmp_path, capsys):
    """nisqaModel(args).train() as run_train.py drives the double-ended recipe: six synthetic pairs of 1-2 s, tr_bs 4, two epochs,
    from scratch; the checkpoint then drives predict_csv with csv_ref."""
    import pandas as pd
    from nisqa_amd.NISQA_model import nisqaModel
    rng = np.random.default_rng(21)
    d = tmp_path / 'corpus'
    d.mkdir()
    rows = []
    for k in range(6):
        deg, ref = 'deg_%d.wav' % k, 'ref_%d.wav' % k
        synth.write_wav(str(d / deg), synth.synth_pcm16(200 + k, float(rng.uniform(1.0, 2.0))), 48000)
        synth.write_wav(str(d / ref), synth.synth_pcm16(300 + k, float(rng.uniform(1.0, 2.0))), 48000)
        rows.append({'db': 'A' if k < 3 else 'B', 'filepath_deg': deg, 'filepath_ref': ref, 'mos': float(rng.uniform(1, 5))})
    pd.DataFrame(rows).to_csv(d / 'pairs.csv', index=False)
    args = dict(DO.DE_ARGS)
    args.update({'name': 'tiny_de', 'mode': 'main', 'data_dir': str(d), 'output_dir': str(tmp_path / 'out'), 'pretrained_model': False,
                 'csv_file': 'pairs.csv', 'csv_con': None, 'csv_deg': 'filepath_deg', 'csv_ref': 'filepath_ref',
                 'csv_mos_train': 'mos', 'csv_mos_val': 'mos', 'csv_db_train': ['A', 'B'], 'csv_db_val': ['B'], 'tr_epochs': 2,
                 'tr_early_stop': 20, 'tr_bs': 4, 'tr_bs_val': 4, 'tr_lr': 1e-3, 'tr_lr_patience': 15, 'tr_num_workers': 0,
                 'tr_parallel': False, 'tr_ds_to_memory': False, 'tr_ds_to_memory_workers': 0, 'tr_device': None,
                 'tr_checkpoint': 'every_epoch', 'tr_verbose': 1, 'tr_bias_mapping': None, 'tr_bias_min_r': None,
                 'tr_bias_anchor_db': None, 'ms_channel': None})
    torch.manual_seed(3)
    nm = nisqaModel(args)
    nm.train()
    out = capsys.readouterr().out
    assert 'Training size: 6, Validation size: 3' in out and '--> start training' in out and '--> Training done.' in out
    assert out.count('ep 1 sec') == 1 and out.count('ep 2 sec') == 1
    run_dir = tmp_path / 'out' / nm.runname
    hist = pd.read_csv(run_dir / (nm.runname + '__results.csv'))
    assert len(hist) == 2 and np.isfinite(hist['loss'].astype(float)).all()
    ck = run_dir / (nm.runname + '__ep_002.tar')
    assert ck.exists()
    c = torch.load(str(ck), map_location='cpu', weights_only=False)
    assert c['epoch'] == 2 and c['model_name'] == 'NISQA_DE'
    assert int(c['model_state_dict']['cnn.model.bn1.num_batches_tracked']) == 8      # 2 epochs x 2 batches x 2 CNN calls
    assert set(c['model_state_dict']) == set(DO.random_de_state_dict(1))
    p = nisqaModel({'mode': 'predict_csv', 'pretrained_model': str(ck), 'data_dir': str(d), 'csv_file': 'pairs.csv',
                    'csv_deg': 'filepath_deg', 'csv_ref': 'filepath_ref', 'output_dir': None, 'ms_channel': None, 'tr_bs_val': 4,
                    'tr_num_workers': 0})
    df = p.predict()
    assert np.isfinite(df['mos_pred'].to_numpy(dtype=np.float64)).all() and len(df) == 6
    # ... and rows 3..5 are the validation predictions the loop made with the same weights
    assert df['mos_pred'].to_numpy(dtype=np.float64)[3:] == pytest.approx(nm.ds_val.df['mos_pred'].to_numpy(dtype=np.float64), abs=1e-4)


def test_unsupported_option_is_refused_before_any_gpu_work():
    from nisqa_amd.NISQA_model import nisqaModel
    with pytest.raises(NotImplementedError, match='de_align_apply=soft'):
        nisqaModel(dict(DO.DE_ARGS, mode='main', pretrained_model=False, tr_device='cpu', de_align_apply='soft'))
