"""The pooling epilogues of the 'bf16x6' AdaptCNN kernel that store a layer's term planes as 32-bit words of a channel pair (conv1's
A1, conv2's A2; csrc/conv_bf16.hpp lds_store_terms2_cpair): after the exchange with the neighbouring lane every pooled pixel and
every channel must land where the next layer reads it.  Impulse windows walk the pooling windows, the lane halves and the six conv1
iterations; one random window holds every channel apart from its pair partner.  All against a float64 evaluation of the network
(oracle.net.adapt_cnn), with seeded random weights, through the segment-fed kernel (eng.cnn_segments)."""
import numpy as np
import pytest
import torch

import helpers
from oracle import net as onet
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu
BOUND = TOL['bf16x6'][0]
FLOOR, PEAK = -70.0, 10.0                           # dB: the level of a silent window and of the one pixel that is not

# (mel, frame) of the one pixel of each segment; five segments per clip (two workgroups: four waves + one wave and three padding waves)
POSITIONS = (
    [(0, 0), (0, 14), (47, 0), (47, 14)]                                  # the corners
    + [(0, 7), (23, 7), (24, 7), (47, 7)]                                 # mel 0, 23 | 24, 47: the lane-half boundary of conv1
    + [(10, f) for f in (0, 1, 2, 12, 13, 14)]                            # the first and the last pooling windows over the frames
    + [(10, 7), (11, 7)]                                                  # both members of a mel pair
    + [(4 * g + 1, 5) for g in range(6)]                                  # one pixel in each of conv1's six iterations, lower half
    + [(24 + 4 * g + 2, 9) for g in range(6)]                             # ... and upper half
    + [(36, 3), (30, 11)])
assert len(POSITIONS) == 30 and len(set(POSITIONS)) == 30

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _sd(alive=False):
    """seeded random weights; alive: BatchNorm shifts of conv1 / conv2 drawn positive, so that the ReLU leaves no channel of A1 / A2 dead
    (two dead channels are equal maps)"""
    def make():
        sd = helpers.random_state_dict(11, 'NISQA_DIM')
        if alive:
            sd['cnn.model.bn1.bias'] = sd['cnn.model.bn1.bias'].abs() + 0.5
            sd['cnn.model.bn2.bias'] = sd['cnn.model.bn2.bias'].abs() + 3.0
        return sd
    return _cached(('sd', alive), make)


def _sd64(alive=False):
    return _cached(('sd64', alive), lambda: {k: torch.as_tensor(np.asarray(v)).to(torch.float64) for k, v in _sd(alive).items()
                                             if k.split('.')[-1] != 'num_batches_tracked'})


def _engine(alive=False):
    from nisqa_amd.engine import HipNisqa
    return _cached(('eng', alive), lambda: HipNisqa(dict(helpers.DIM_ARGS), _sd(alive), 'cuda:0', precision='bf16x6'))


def _feat64(windows, stages=False, alive=False):
    """float64 AdaptCNN features [N, 384] of the windows [N, 48, 15] (and the layer outputs)"""
    with torch.no_grad():
        out = onet.adapt_cnn(_sd64(alive), torch.as_tensor(windows).to(torch.float64).unsqueeze(1), return_stages=stages)
    return (out[0].numpy(), {k: v.numpy() for k, v in out[1].items()}) if stages else out.numpy()


def impulse_windows():
    """[30, 48, 15] float32: window q is FLOOR everywhere but PEAK at POSITIONS[q]"""
    w = np.full((len(POSITIONS), 48, 15), FLOOR, np.float32)
    for q, (m, f) in enumerate(POSITIONS):
        w[q, m, f] = PEAK
    return w


def _impulse_batch():
    """(windows, float64 features, GPU features of the six 5-segment clips in one batch, its plan) -- computed once"""
    def make():
        from nisqa_amd.engine import BatchPlan
        eng = _engine()
        w = impulse_windows()
        x = torch.from_numpy(w).reshape(6, 5, 1, 48, 15).contiguous().to(eng.device)
        plan = BatchPlan.from_n_wins([5] * 6)
        feat = eng.cnn_segments(x, plan)
        torch.cuda.synchronize()
        return w, _feat64(w), x, feat, plan
    return _cached('impulse', make)


def _rows(feat, plan, b, n):
    t0 = int(plan.tok_off[b])
    return feat[t0:t0 + n]


def test_impulse_windows_against_float64():
    """One pixel per segment: a pooled pixel stored one place off, a channel pair in swapped order or a word of the wrong iteration moves
    the features by far more than the bound -- the float64 features of any two impulse positions differ by over 100 bounds."""
    w, ref, x, feat, plan = _impulse_batch()
    d = np.abs(ref[:, None, :] - ref[None, :, :]).max(-1)
    d[np.arange(len(ref)), np.arange(len(ref))] = np.inf
    print('smallest max |feat64(p) - feat64(q)| over position pairs', float(d.min()), 'max |feat64|', float(np.abs(ref).max()))
    assert d.min() > 100 * BOUND
    assert torch.isfinite(feat).all()
    for b in range(6):
        got = _rows(feat, plan, b, 5).cpu().numpy().astype(np.float64)
        err = np.abs(got - ref[5 * b:5 * b + 5]).max(-1)
        print('clip', b, 'positions', POSITIONS[5 * b:5 * b + 5], 'max |feat - float64|', err)
        assert err.max() < BOUND, (b, err)


def test_channels_that_differ_from_their_pair_partner():
    """One random window, weights whose conv1 and conv2 output channels are all different maps (checked on the float64 pooled tensors):
    a channel pair stored in swapped order cannot hide."""
    from nisqa_amd.engine import BatchPlan
    eng = _engine(alive=True)
    win = (np.random.default_rng(5).uniform(FLOOR, PEAK, (1, 48, 15))).astype(np.float32)
    ref, st = _feat64(win, stages=True, alive=True)
    for name in ('p1', 'p2'):
        p = st[name][0]                                                  # [C, H, W]
        gap = min(float(np.abs(p[c] - p[e]).max()) for c in range(len(p)) for e in range(c))
        print(name, 'smallest max |channel c - channel e|', gap)
        assert gap > 0.5
    feat = eng.cnn_segments(torch.from_numpy(win).reshape(1, 1, 1, 48, 15).to(eng.device), BatchPlan.from_n_wins([1]))
    torch.cuda.synchronize()
    err = float(np.abs(feat[0].cpu().numpy().astype(np.float64) - ref[0]).max())
    print('max |feat - float64|', err, 'max |feat64|', float(np.abs(ref).max()))
    assert err < BOUND


@pytest.mark.parametrize('n', [1, 4])
def test_a_short_clip_alone_carries_the_bits_of_the_batch(n):
    """The first n segments of a 5-segment clip, alone in a batch (n_wins = 1: three padding waves; 4: a full workgroup): the same bits as
    the same windows inside the batch of six clips."""
    from nisqa_amd.engine import BatchPlan
    w, ref, x, feat, plan = _impulse_batch()
    eng = _engine()
    for b in (0, 3):
        alone = eng.cnn_segments(x[b:b + 1, :n].contiguous(), BatchPlan.from_n_wins([n]))
        torch.cuda.synchronize()
        assert torch.equal(alone[:n], _rows(feat, plan, b, n)), (b, float((alone[:n] - _rows(feat, plan, b, n)).abs().max()))
