"""The 'bf16x6' AdaptCNN kernel with layers in the transposed form (output channels on the rows, pixels on the columns of
16x16x32 MFMA tiles): the pixel <-> column map, the tap masks and the row-indexed shifts against a float64 evaluation of the
network at the workgroup edges, the rounding width against the exact-fp32 kernels, every wave slot against every other, and
determinism.  Seeded random weights throughout."""
import numpy as np
import pytest
import torch

import helpers
from nisqa_amd import synth
from oracle import net as onet
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
HOP = 480                                           # 10 ms at 48 kHz
N_WINS = [1, 3, 4, 5, 9]                            # one to four valid waves, workgroups of padding waves, a second and a third workgroup

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sd():
    return _cached('sd', lambda: helpers.random_state_dict(7, 'NISQA_DIM'))


def _engine(precision):
    from nisqa_amd.engine import HipNisqa
    return _cached(('eng', precision), lambda: HipNisqa(dict(helpers.DIM_ARGS), _sd(), 'cuda:0', precision=precision))


def _clip_of(seed, n_wins):
    """int16 PCM whose spectrogram has exactly n_wins segments at the segment hop of 4 (the last one ragged)"""
    t = 14 + 1 + 4 * (n_wins - 1)
    return synth.synth_pcm16(seed, (t - 1) * HOP / 48000.0 + 0.1)[:(t - 1) * HOP]


def _feat64(spec):
    """float64 AdaptCNN features of one clip's [48, T] spectrogram"""
    sd64 = _cached('sd64', lambda: {k: torch.as_tensor(np.asarray(v)).to(torch.float64) for k, v in _sd().items()
                                    if k.split('.')[-1] != 'num_batches_tracked'})
    with torch.no_grad():
        x, n = onet.segment_specs(spec)
        return onet.adapt_cnn(sd64, x.to(torch.float64)).numpy(), n


def _mel_batch(key, pcm):
    """GPU spectrogram (clamped at each clip's floor) of the clips -> (mel, floor, plan, float64 features per clip); computed once"""
    def make():
        eng = _engine('f32')                        # the mel kernel is the same in every mode
        plan = eng.plan([len(p) for p in pcm], 48000)
        mel, floor = eng.mel(torch.from_numpy(np.concatenate(pcm)).to(eng.device), plan, 48000, clamp=True)
        torch.cuda.synchronize()
        mel_h = mel.cpu().numpy()
        ref = []
        for b in range(plan.n_clips):
            f, n = _feat64(mel_h[plan.frame_off[b]:plan.frame_off[b + 1]].T)
            assert n == plan.n_wins[b]
            ref.append(f)
        return mel, floor, plan, ref
    return _cached(key, make)


def _edge_batch():
    return _mel_batch('edge', [_clip_of(900 + i, n) for i, n in enumerate(N_WINS)])


def _distance(feat, plan, ref):
    fh = feat.cpu().numpy().astype(np.float64)
    return max(float(np.abs(fh[int(plan.tok_off[b]):int(plan.tok_off[b]) + int(plan.n_wins[b])] - ref[b]).max())
               for b in range(plan.n_clips))


def test_features_against_float64_at_workgroup_edges():
    """Clips of 1, 3, 4, 5 and 9 segments in one batch: a wrong pixel map, tap mask, shift row or pooling window is an error of order
    one; the bound is the one tests/test_gpu_parity.py holds the fp32-grade precisions' features to.  Rows k >= n_wins stay zero."""
    mel, floor, plan, ref = _edge_batch()
    assert list(plan.n_wins) == N_WINS
    eng = _engine('bf16x6')
    feat, _ = eng.cnn(mel, floor, plan)
    torch.cuda.synchronize()
    assert torch.isfinite(feat).all()
    fh = feat.cpu().numpy().astype(np.float64)
    for b, n in enumerate(N_WINS):
        t0 = int(plan.tok_off[b])
        err = float(np.abs(fh[t0:t0 + n] - ref[b]).max())
        print('n_wins', n, 'max |feat - float64|', err, 'max |feat|', float(np.abs(ref[b]).max()))
        assert np.abs(ref[b]).max() > 0.1
        assert err < TOL['bf16x6'][0], (n, err)
        assert (fh[t0 + n:int(plan.tok_off[b + 1])] == 0).all()


def test_rounding_width_is_that_of_fp32_arithmetic():
    """One 10 s clip: the distance of 'bf16x6' from float64 against that of the exact-fp32 kernels and of the float32 torch operators,
    in the relation test_rounding_error_of_the_precision_modes_against_float64 asserts."""
    mel, floor, plan, ref = _mel_batch('ten', [synth.synth_pcm16(2, 10.0)])
    dist = {}
    for prec in ('f32', 'bf16x6'):
        feat, _ = _engine(prec).cnn(mel, floor, plan)
        torch.cuda.synchronize()
        dist[prec] = _distance(feat, plan, ref)
    sd32 = {k: torch.as_tensor(np.asarray(v)) for k, v in _sd().items()}
    with torch.no_grad():
        x, _ = onet.segment_specs(mel.cpu().numpy().T)
        dist['float32 torch'] = float(np.abs(onet.adapt_cnn(sd32, x).numpy().astype(np.float64) - ref[0]).max())
    print('max |feat - float64|:', {k: '%.3g' % v for k, v in dist.items()})
    assert dist['bf16x6'] <= 1.5 * max(dist['f32'], dist['float32 torch'])


def test_every_wave_slot_computes_the_same_thing():
    """One window repeated 8 times as the segments of a clip, through the segment-fed kernel (the CNN stage of forward_segments): the
    eight feature rows are the same bits -- the four LDS regions, the S4 slot offsets and the column map under each wave index, two
    workgroups -- and so is the row of the window alone with n_wins = 1."""
    from nisqa_amd.engine import BatchPlan
    mel, floor, plan, _ = _edge_batch()
    eng = _engine('bf16x6')
    win = mel[int(plan.frame_off[4]) + 3:int(plan.frame_off[4]) + 18].T.contiguous()          # [48, 15]
    x = torch.zeros((2, 8, 1, 48, 15), dtype=torch.float32, device=eng.device)
    x[0, :, 0] = win
    x[1, 0, 0] = win
    splan = BatchPlan.from_n_wins([8, 1])
    feat = eng.cnn_segments(x, splan)
    out = eng.forward_segments(x, [8, 1])
    torch.cuda.synchronize()
    rows = feat[int(splan.tok_off[0]):int(splan.tok_off[0]) + 8]
    assert torch.isfinite(rows).all() and float(rows.abs().max()) > 0.1
    for k in range(1, 8):
        assert torch.equal(rows[k], rows[0]), (k, float((rows[k] - rows[0]).abs().max()))
    assert torch.equal(feat[int(splan.tok_off[1])], rows[0])
    assert torch.isfinite(out).all()


def test_two_runs_give_the_same_bits():
    mel, floor, plan, _ = _edge_batch()
    eng = _engine('bf16x6')
    a, _ = eng.cnn(mel, floor, plan)
    b, _ = eng.cnn(mel, floor, plan)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
