"""Self-attention stacks of 1, 3 and 4 layers on the MI355X (run with -m gpu).  Every shipped checkpoint and every seeded fixture
has two layers; the launchers loop over n_layers, ping-pong two Q/K/V buffers on the layer's parity and change the shape of the
last layer's launch, and the double-ended engine keeps two independent counts.  Here the depth is what varies: the stage harness
and the bound of tests/test_gpu_stage_width.py (float64 yardstick, calibrated on the float32 CPU oracle) at small token counts,
the whole forward through the C ABI, the double-ended model with blocks of different depth, and the gradient with respect to the
input.  tests/test_sa_layers_host.py shows on the CPU that a stack one layer short, with its last layers swapped or with one
layer's weights used twice sits about 10^6 floors from float64: none of these passes a bound of 1.5 floors.  The training steps
are in tests/test_gpu_layer_count_train.py.

What the cases can see, from the launch code (csrc/td.hip, td_bf16.hip, td16_bf16x6.hip: qb[l & 1] / lbuf[l & 1]).  A launcher
that used buffer 0 for every layer would, at three and four layers, let a layer's tiles overwrite the K / V of their clip's
other tiles while those are still being read and feed layer l + 1 from a half-written buffer: wrong rows in every clip of more
than one tile (33 tokens and up here), at any depth with a next layer; one layer has no next layer and stays right, which is
why depth 1 alone would not do.  A last layer that read the buffer it did not own shows against the NaN workspaces of the
harness and against the fresh engine of the stale-buffer test.  HipNisqaDE passing the first block's count for the second runs
that block at 1 layer for 3 or at 3 for 1 -- a layer short, or a layer read past the packed blob -- and the score moves by
10^5 floors against a bound of 1e-4."""
import numpy as np
import pytest
import torch

import de_oracle as DO
import helpers
import input_grad_de_oracle as IGD
import input_grad_oracle as IG
import sa_layers as SL
import test_gpu_stage_width as SW
from nisqa_amd import synth
from oracle import mel as omel, net as onet
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
# the 32-token tile of the exact-fp32 and two-term kernels, the 64-token workgroup of csrc/td16_bf16x6.hip, a clip of one token,
# several key tiles per clip
COUNTS = [1, 31, 32, 33, 63, 64, 65, 129, 257]
SMALL = [1, 33, 65]
STACKS = [(1, 'NISQA_DIM'), (3, 'NISQA_DIM'), (4, 'NISQA_DIM'), (3, 'NISQA')]


def _set(model, L):
    """(tag, args, state dict, tag / args / state dict of the two-layer set the CNN rows come from)"""
    def make():
        seed, base, name = (7, helpers.DIM_ARGS, 'dim') if model == 'NISQA_DIM' else (8, helpers.MOS_ARGS, 'mos')
        sd = helpers.random_state_dict(seed, model)
        return ('%s_x%d' % (name, L), SL.args_with_layers(base, L), SL.with_layers(sd, L)), (name + '_rand', dict(base), sd)
    return SW._cached(('layers', model, L), make)


def _inputs(model, L, counts, seed):
    def make():
        (tag, args, sd), two = _set(model, L)
        feats = SW._sample(SW._cnn_rows(*two, 0), counts, seed)       # the CNN's weights do not depend on L
        heads = SW._heads(args)
        td64, chain64 = SW._oracle_sa(sd, feats, L, torch.float64, heads)
        td32, chain32 = SW._oracle_sa(sd, feats, L, torch.float32, heads)
        return {'feat': feats, 'td64': td64, 'td32': td32, 'chain64': chain64, 'chain32': chain32}
    return SW._cached(('layers-in', model, L, tuple(counts), seed), make)


# =============================================================================================================================
# 1. stage level
# =============================================================================================================================
@pytest.mark.parametrize('L,model', STACKS)
def test_stack_against_float64(L, model):
    (tag, args, sd), _ = _set(model, L)
    inp = _inputs(model, L, COUNTS, 1)
    plan = SW._plan(COUNTS)
    feat = SW._upload_rows(inp['feat'], plan)
    td, chain = {}, {}
    for m in SW.ALL_MODES:
        eng = SW._engine(tag, args, sd, m)
        assert eng.n_layers == L
        td[m] = SW._valid(SW.run_td(eng, feat, plan), plan)
        if eng.td_precision == 'bf16x6':
            chain[m] = list(SW.run_td_pool(eng, feat, plan).cpu().numpy())
    f32 = SW._engine(tag, args, sd, 'f32')
    chain['f32'] = list(SW.run_pool(f32, SW.run_td(f32, feat, plan), plan).cpu().numpy())
    for m in ('f16x4', 'f16x3'):                           # the same three-term kernels as 'bf16x6'
        SW._same_bits('td ' + m, td[m], td['bf16x6'])
        SW._same_bits('td_pool ' + m, chain[m], chain['bf16x6'])
    SW.judge('self-attention x%d [%s]' % (L, tag), COUNTS, {m: td[m] for m in ('f32', 'bf16x6', 'bf16x3')}, inp['td64'], inp['td32'])
    SW.judge('self-attention x%d + pooling, fused [%s]' % (L, tag), COUNTS, {m: chain[m] for m in ('f32', 'bf16x6')},
             inp['chain64'], inp['chain32'])


def _rows_of(eng, feats, counts):
    """what eng.td and eng.td_pool give for one batch: per clip the self-attention rows followed by the pooled outputs"""
    plan = SW._plan(counts)
    feat = SW._upload_rows(feats, plan)
    x = SW._valid(eng.td(feat, plan), plan)
    out = eng.td_pool(feat, plan).cpu().numpy()
    return [np.concatenate([r.reshape(-1), o]) for r, o in zip(x, out)]


@pytest.mark.parametrize('L', [1, 3])
def test_stale_buffers_do_not_reach_an_odd_stack(L):
    """An odd stack ends on the other ping-pong buffer: a last layer that read the buffer an earlier, larger call filled would
    show here.  The engine that has seen the larger batch and one that has not must agree bit for bit on the small one -- and with
    the direct calls of the harness, whose workspaces hold NaN wherever the kernels did not write."""
    from nisqa_amd.engine import HipNisqa
    (tag, args, sd), _ = _set('NISQA_DIM', L)
    big, small = _inputs('NISQA_DIM', L, COUNTS, 2)['feat'], _inputs('NISQA_DIM', L, SMALL, 3)['feat']
    plan = SW._plan(SMALL)
    for m in ('f32', 'bf16x3', 'bf16x6'):
        used = SW._engine(tag, args, sd, m)
        _rows_of(used, big, COUNTS)
        first, second = _rows_of(used, small, SMALL), _rows_of(used, small, SMALL)
        fresh = _rows_of(HipNisqa(args, sd, DEV, precision=m), small, SMALL)
        assert all(np.isfinite(r).all() for r in fresh)
        SW._same_bits('x%d %s: after a larger batch' % (L, m), first, fresh)
        SW._same_bits('x%d %s: twice' % (L, m), second, first)
        direct = SW._valid(SW.run_td(used, SW._upload_rows(small, plan), plan), plan)
        SW._same_bits('x%d %s: workspace of NaN' % (L, m), direct, [r[:-used.n_heads].reshape(-1, 64) for r in fresh])


# =============================================================================================================================
# 2. the whole forward through the C ABI (nisqa_predict_batch_pcm16 -> model->n_layers)
# =============================================================================================================================
@pytest.mark.parametrize('precision', ['f32', 'bf16x6', 'bf16x3'])
@pytest.mark.parametrize('L', [1, 3, 4])
def test_forward_pcm_at_other_depths(L, precision):
    """Three clips of 0.2 s, 1.0 s and 2.6 s against oracle/net.py in float64 on the engine's own spectrogram, at the output bars
    of tests/test_gpu_parity.py."""
    (tag, args, sd), _ = _set('NISQA_DIM', L)
    eng = SW._engine(tag, args, sd, precision)
    pcm = [synth.synth_pcm16(970 + i, s) for i, s in enumerate((0.2, 1.0, 2.6))]
    plan = eng.plan([len(p) for p in pcm], 48000)
    dev = torch.from_numpy(np.concatenate(pcm)).to(eng.device)
    eng.forward_pcm(dev, plan, 48000)
    ws = eng._ws[torch.cuda.current_stream(eng.device).cuda_stream]
    ws.zero_()
    out = eng.forward_pcm(dev, plan, 48000).cpu().numpy()
    ws.fill_(0xFF)                                         # every float of the engine's workspace NaN: the same bits
    SW._same_bits('forward_pcm x%d %s, workspace 0xFF' % (L, precision), list(eng.forward_pcm(dev, plan, 48000).cpu().numpy()), list(out))
    mel = eng.mel(dev, plan, 48000, clamp=True)[0].cpu().numpy()

    def refs():
        specs = [mel[plan.frame_off[n]:plan.frame_off[n + 1]].T for n in range(plan.n_clips)]
        return ([onet.predict_from_melspec(sd, args, s, dtype=torch.float64) for s in specs],
                [onet.predict_from_melspec(sd, args, s) for s in specs])
    ref64, ref32 = SW._cached(('layers-pcm', L), refs)             # (the mel stage is the same kernel in every mode)
    err = np.array([np.abs(o.astype(np.float64) - r).max() for o, r in zip(out, ref64)])
    cpu = np.array([np.abs(a.astype(np.float64) - r).max() for a, r in zip(ref32, ref64)])
    print('forward_pcm x%d %s: segments %s, max |out - float64| per clip %s (float32 CPU oracle %s), bar %.0e' % (
        L, precision, list(plan.n_wins), err, cpu, TOL[precision][1]))
    assert np.isfinite(out).all() and out.shape == (3, 5)
    assert (err <= TOL[precision][1]).all(), (L, precision, err)


# =============================================================================================================================
# 3. double-ended: the two counts differ
# =============================================================================================================================
DE_PAIRS = [(65, 33), (1, 7), (130, 97)]
# Random self-attention layers pull the tokens of a clip together, and under cosine scores the float64 top-2 gap of most tokens
# then falls under 1e-5 (lstm_train_oracle.batch clips: 13 .. 92 % of the tokens for seeds 60 .. 65).  The clips are therefore
# synthetic audio through the oracle's mel front end, and the weight seeds were searched on the CPU (60 .. 199) for the widest
# smallest gap: 1.1e-4 at (1, 3), 6.1e-5 at (3, 1) -- no token under 1e-5 (asserted in the test as a share of at most 1 %).
DE_SEEDS = {(1, 3): 99, (3, 1): 107}
TIE = 1e-5


def _de_specs(seed, frames):
    out = []
    for i, T in enumerate(frames):
        n = (T - 1) * 480
        pcm = synth.synth_pcm16(seed * 10 + i, n / 48000.0 + 0.1)[:n]
        out.append(omel.melspec_db_from_audio(pcm.astype(np.float32) / np.float32(32768.0), 48000)[:, :T])
    return out


def de_case(layers, align, apply, fuse):
    """-> (args, state dict, x [B, L, 2, 48, 15] with NaN in the padding rows, n_wins [B, 2], float64 results per pair): blocks of
    layers = (td, td_2) layers; also run on the CPU when a seed is chosen (the share of near-tie tokens is asserted in the test)"""
    def make():
        seed = DE_SEEDS[layers]
        args = DO.de_args(align, apply, fuse, td_sa_num_layers=layers[0], td_2_sa_num_layers=layers[1])
        sd = SL.with_layers(DO.random_de_state_dict(seed, fuse, n_layers2=layers[1]), layers[0], seed=seed)
        frames = lambda side: [15 + 4 * (p[side] - 1) for p in DE_PAIRS]
        L = max(max(p) for p in DE_PAIRS)
        xd, nd = IG.segment_tensor(_de_specs(seed + 500, frames(0)), args, L, np.nan)
        xr, nr = IG.segment_tensor(_de_specs(seed + 1500, frames(1)), args, L, np.nan)
        n_wins = np.stack([nd, nr], 1).astype(np.int64)
        assert n_wins.tolist() == [list(p) for p in DE_PAIRS]
        res = [DO.forward_segments(sd, args, xd[b, :p[0]], xr[b, :p[1]], torch.float64, stages=True) for b, p in enumerate(DE_PAIRS)]
        return args, sd, np.concatenate([xd, xr], 2), n_wins, res
    return SW._cached(('layers-de', layers, align, apply, fuse), make)


def near_tie_share(res):
    """the share of degraded tokens (with at least two reference tokens to choose from) whose float64 top-2 score gap is under TIE"""
    gap = np.concatenate([st['gap'] for _, st in res])
    gap = gap[np.isfinite(gap)]
    return float((gap < TIE).mean())


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
@pytest.mark.parametrize('align,apply,fuse', [('cosine', 'hard', 'x/y/-'), ('dot', 'soft', '+/-')])
@pytest.mark.parametrize('layers', [(1, 3), (3, 1)])
def test_double_ended_blocks_of_different_depth(layers, align, apply, fuse, precision):
    """HipNisqaDE.forward_segments against tests/de_oracle.py in float64 at the bound of tests/test_gpu_de.py (1e-4 on the score);
    hard indices must be float64's wherever its top-2 gap is at least 1e-5, and at most 1 % of the tokens may fall under that gap,
    so that the tie rule cannot hide a wrong index."""
    from nisqa_amd.engine import BatchPlan, HipNisqaDE
    args, sd, x, n_wins, res = de_case(layers, align, apply, fuse)
    share = near_tie_share(res)
    assert share <= 0.01, share
    eng = SW._cached(('layers-de-eng', layers, align, apply, fuse, precision), lambda: HipNisqaDE(args, sd, DEV, precision=precision))
    assert (eng.base.n_layers, eng.n_layers2) == layers
    got = eng.forward_segments(torch.from_numpy(x), n_wins).cpu().numpy().reshape(-1)
    want = np.array([m for m, _ in res])
    err = np.abs(got - want)
    print('DE x%d / x%d %s/%s/%s %s: hip %s oracle %s |d| %s, near-tie share %.3g' % (
        layers + (align, apply, fuse, precision, got, want, err, share)))
    assert np.isfinite(got).all()
    assert err.max() <= 1e-4, err
    if apply == 'hard':                                   # the same chain once more, with the indices it chose
        xd = torch.from_numpy(x).to(DEV)
        x2 = torch.cat([xd[:, :, 0:1], xd[:, :, 1:2]], 0).contiguous()
        plan = BatchPlan.from_n_wins(np.concatenate([n_wins[:, 0], n_wins[:, 1]]))
        out, idx = eng.forward_features(eng.base.cnn_segments(x2, plan), plan, want_idx=True)
        assert np.array_equal(out.cpu().numpy().reshape(-1), got)
        idx = idx.cpu().numpy()
        for b, (nx, ny) in enumerate(DE_PAIRS):
            k, st = idx[plan.tok_off[b]:plan.tok_off[b] + nx], res[b][1]
            sure = st['gap'] >= TIE
            assert ((k >= 0) & (k < ny)).all()
            assert (k[sure] == st['idx'][sure]).all(), (b, np.nonzero(k[sure] != st['idx'][sure]))


# =============================================================================================================================
# 5. gradients with respect to the input
# =============================================================================================================================
IG_BAR, IG_TIE = 1e-3, 1e-5                  # tests/test_gpu_input_grad.py's BAR and TIE


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
@pytest.mark.parametrize('model,L', [('NISQA_DIM', 3), ('NISQA', 1)])
def test_input_gradient_at_other_depths(model, L, precision):
    """grad_segments on the small case of tests/test_gpu_input_grad.py (1, 3 and 2 segments padded to four with NaN) against
    tests/input_grad_oracle.py in float64, which reads the depth from args: a random g and, for NISQA_DIM, every one-hot head."""
    from nisqa_amd.engine import HipNisqa
    sd2, args2, x, n_wins, g = IG.case(model, IG.SMALL, fill=np.nan)
    sd, args = SL.with_layers(sd2, L), SL.args_with_layers(args2, L)
    B, H = g.shape
    gs = [g] + ([IG.one_hot(B, H, h) for h in range(H)] if H > 1 else [])
    want = SW._cached(('layers-ig', model, L), lambda: IG.oracle(sd, args, x, n_wins, gs))
    assert want['margin'][np.isfinite(want['margin'])].min() >= IG_TIE       # nothing sits on a tie: nothing is excluded
    eng = HipNisqa(args, sd, DEV, precision=precision)
    xd = torch.from_numpy(x).to(DEV)
    y = eng.forward_segments(xd, n_wins).cpu().numpy()
    np.testing.assert_allclose(y, want['y'], rtol=0, atol=1e-3)
    for k, gk in enumerate(gs):
        dx = eng.grad_segments(xd, n_wins, torch.from_numpy(gk).to(DEV))
        assert dx.shape == xd.shape and dx.dtype == torch.float32
        got, w = dx.cpu().numpy(), want['dx'][k]
        assert np.isfinite(got).all() and (np.abs(w).reshape(B, -1).max(1) > 0).all()
        for b, n in enumerate(n_wins):
            assert (got[b, n:] == 0).all()
        err = IG.clip_error(got, w)
        print(model, 'x%d' % L, precision, 'random g' if k == 0 else 'head %d' % (k - 1), 'relative distance per clip', err)
        assert (err <= IG_BAR).all(), (k, err)
    again = eng.grad_segments(xd, n_wins, torch.from_numpy(g).to(DEV))
    assert torch.equal(again, eng.grad_segments(xd, n_wins, torch.from_numpy(g).to(DEV)))



@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
def test_input_gradient_at_other_depths_double_ended(precision):
    """NISQA_DE with three layers in the first block and one in the second, dot / soft / '+/-', on the small case of
    tests/test_gpu_input_grad_de.py against tests/input_grad_de_oracle.py, at that test's bar for dot / soft: per clip and channel
    max(1e-3, 2 x the distance of the oracle chain's own float32 run from float64) of the channel's largest entry."""
    from nisqa_amd.engine import HipNisqaDE
    config = ('dot', 'soft', '+/-')
    sd2, args2, x, n_wins, g = IGD.case(config, IGD.SMALL, fill=np.nan)
    sd = SL.with_layers(SL.with_layers(sd2, 3), 1, SL.TD2)
    args = SL.args_with_layers(SL.args_with_layers(args2, 3), 1, 'td_2_sa_num_layers')

    def oracle():
        w = IGD.oracle(sd, args, x, n_wins, [g])
        w['dx32'] = IGD.oracle(sd, args, x, n_wins, [g], dtype=torch.float32, margins=False)['dx'][0]
        return w
    want = SW._cached(('layers-igde',), oracle)
    valid = np.isfinite(want['margin'])
    assert valid.sum() == 12 and (want['margin'][valid] >= IG_TIE).all()
    eng = HipNisqaDE(args, sd, DEV, precision=precision)
    assert (eng.base.n_layers, eng.n_layers2) == (3, 1)
    xd = torch.from_numpy(x).to(DEV)
    y = eng.forward_segments(xd, n_wins).cpu().numpy()
    np.testing.assert_allclose(y, want['y'], rtol=0, atol=1e-3)
    dx = eng.grad_segments(xd, n_wins, torch.from_numpy(g).to(DEV))
    got = dx.cpu().numpy()
    assert dx.shape == xd.shape and dx.dtype == torch.float32 and np.isfinite(got).all()
    for b in range(len(n_wins)):
        for c in range(2):
            assert (got[b, n_wins[b, c]:, c] == 0).all()
    err = IGD.channel_error(got, want['dx'][0])
    e32 = IGD.channel_error(want['dx32'], want['dx'][0])
    bar = max(IG_BAR, 2.0 * float(e32.max()))
    print('DE x3 / x1 dot_soft', precision, 'relative distance per clip and channel', err.ravel(), 'float32 CPU chain', e32.ravel(), 'bar', bar)
    assert (err <= bar).all(), err
    assert torch.equal(dx, eng.grad_segments(xd, n_wins, torch.from_numpy(g).to(DEV)))
