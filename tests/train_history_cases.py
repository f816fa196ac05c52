"""Training steps on dirty workspaces and after shape changes: test support (not a test module) -- the batch shapes, the seeded data,
the float64 / float32 oracle steps and the comparisons shared by tests/test_train_history_host.py (CPU) and
tests/test_gpu_train_history.py (MI355X).

The three trainers keep state between steps that no one-shape, fresh-trainer test exercises: HipTrainer's fused-block workspace
and fragment buffer (kept while large enough), the padded token rows and empty share planes of csrc/train_td.hip (which must hold
zeros: the one weight-gradient GEMM and the column sums run over all NP padded rows), the index tables cached by the segment
counts, the cast table, the gradient buffer / float64 sums / loss slot / split-K tiles that atomics add into, the per-step weight
maximum of 'f16x4', and scratch that is torch.empty.  The shapes below cross every class boundary of the fused block.

Gradients of this network at random weights are ill-conditioned against float64 at most data seeds (ReLU / max-pool gate flips:
torch's own float32 evaluation of the oracle operators is off by per cent), so the GPU anchor uses only the seeds of SEEDS, at
which float32 stays within 3e-4 of float64 on every gradient tensor -- tests/test_train_history_host.py holds that on the CPU.
"""
import numpy as np
import torch

import de_oracle as DO
import de_train_oracle as DT
import lstm_train_oracle as LT
from nisqa_amd import synth
from oracle import net as onet, train as otrain

# segments per clip; TABLE: S, NP (32 padded rows per tile), split-K chunks of the one weight-gradient GEMM, blocks per job of the
# column-sum launch (csrc/train_td.hip, nisqa_tdtrain_step: classes at NP = 256 / 1024 / 4096 and 256 / 2048)
SHAPES = {'BIG': [200, 130, 257, 96, 1, 64, 300], 'EDGE': [65, 1, 64, 33, 32, 31], 'PERM': [31, 32, 33, 64, 1, 65],
          'TINY': [31, 1, 32, 33, 5, 17]}
TABLE = {'BIG': (1048, 1184, 16, 4), 'EDGE': (226, 320, 4, 4), 'PERM': (226, 320, 4, 4), 'TINY': (119, 224, 1, 1)}
WALK = ['BIG', 'TINY', 'EDGE', 'PERM', 'TINY', 'BIG']       # TINY returns after two other keys; BIG returns into a workspace of its size
MODELS = {'NISQA_DIM': (synth.DIM_ARGS, 7), 'NISQA': (synth.MOS_ARGS, 8)}
# data seeds at which float32 stays close to float64 on every gradient tensor (found on the CPU; worst tensor relative to
# max(1e-3, max |g|), conv biases left out):
#              BIG          EDGE         PERM         TINY
#   NISQA_DIM  4 (7.8e-5)   1 (1.2e-4)   0 (8.8e-5)   11 (4.2e-5)
#   NISQA      65 (1.5e-4)  2 (8.5e-6)   3 (3.4e-5)   0 (1.1e-5)
# Two seeds were replaced after the clean HIP step missed the 3e-3 gradient bar against float64 with loss, y_hat and buffers in
# place (<= 3e-6), the same on both paths, torch's float32 within 2e-4 -- each one gate that fp32 rounding decides:
#   NISQA BIG, seed 0: conv4.weight 7.7e-3, all of it in output channel 32 (the next channel 5.6e-6), bn4.weight / bn4.bias and
#     conv5..6 at 7e-6, conv1..3 diffusely 1e-3: an arg-max tie of the pool behind conv4 -- segment 361, channel 32, window
#     (2, 1) holds 0.5479609379 and 0.5479594689 in float64 (gap 1.5e-6; torch's float32 puts both 1e-6 lower);
#   NISQA PERM, seed 2: bn2.bias 4.1e-3, conv2.weight 3.1e-3, bn2.weight 8e-4, all in channel 5 (the next 6e-6), conv3..6 at
#     5e-6: a ReLU gate of layer 2 -- one BatchNorm output of channel 5 is 8.3e-8 in float64 (3.7e-7 in torch's float32).
# The replacements are the first seeds that pass the host test and whose float64 gradients also move by less than 1e-3 when the
# spectrograms are scaled by 1 + 2e-7 N(0, 1), ten draws (65: 3.1e-4, 3: 6.5e-6; seed 0 moved by 3.1e-2 and seed 2 by 4.1e-3
# under 1e-6, and at that size no seed of 40 tried per shape stayed below 3e-3).
SEEDS = {('NISQA_DIM', 'BIG'): 4, ('NISQA_DIM', 'EDGE'): 1, ('NISQA_DIM', 'PERM'): 0, ('NISQA_DIM', 'TINY'): 11,
         ('NISQA', 'BIG'): 65, ('NISQA', 'EDGE'): 2, ('NISQA', 'PERM'): 3, ('NISQA', 'TINY'): 0}
CASES = sorted(SEEDS)
F32_ORACLE_BAR = 3e-4                         # a tenth of the 3e-3 the GPU step is held to
_CACHE = {}


def conv_bias(k):
    return k.startswith('cnn.model.conv') and k.endswith('.bias')


def padded_tokens(shape):
    return int(sum((n + 31) // 32 * 32 for n in shape))


def td_classes(NP):
    """(split-K chunks, column-sum blocks per job) the fused block launches with at NP padded rows"""
    return (64 if NP >= 4096 else 16 if NP >= 1024 else 4 if NP >= 256 else 1), (32 if NP >= 2048 else 4 if NP >= 256 else 1)


def model_args(model):
    return dict(MODELS[model][0], cnn_dropout=0.0, td_sa_dropout=0.0)


def state_dict(model):
    if ('sd', model) not in _CACHE:
        _CACHE[('sd', model)] = synth.random_state_dict(MODELS[model][1], model)
    return _CACHE[('sd', model)]


def data(model, shape):
    """-> (specs: one [48, T] spectrogram per clip, y [B, heads] with one NaN) -- the recipe of test_gpu_layer_count_train._case"""
    key = ('data', model, shape)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + SEEDS[(model, shape)])
        specs = [(-40 + 18 * rng.standard_normal((48, 15 + 4 * (n - 1)))).astype(np.float32) for n in SHAPES[shape]]
        y = rng.uniform(1, 5, (len(specs), 5 if model == 'NISQA_DIM' else 1)).astype(np.float32)
        y[1, 0] = np.nan
        _CACHE[key] = (specs, y)
    return _CACHE[key]


def segments(specs):
    segs, n_wins = zip(*[onet.segment_specs(s, 15, 4, None) for s in specs])
    return torch.cat([torch.as_tensor(x)[:n] for x, n in zip(segs, n_wins)]), [int(n) for n in n_wins]


def batch_stats(sd, args, specs, dtype=torch.float64):
    """BatchNorm batch statistics of one train-mode forward at the weights sd -> {'bn<i>': (mean, biased variance, count)}"""
    s = {k: (torch.as_tensor(np.asarray(v)).to(dtype) if torch.as_tensor(np.asarray(v)).is_floating_point()
             else torch.as_tensor(np.asarray(v))) for k, v in sd.items()}
    segs, n_wins = segments(specs)
    with torch.no_grad():
        _, stats = otrain.forward_train(s, args, segs.to(dtype), n_wins, None)
    return stats


def next_buffers(prev, stats):
    """the momentum-0.1 update of the running buffers prev {key: array} by the batch statistics -> {key: float64 array}"""
    out = {}
    for i in range(1, 7):
        mean, var, cnt = stats['bn%d' % i]
        p = 'cnn.model.bn%d.' % i
        out[p + 'running_mean'] = 0.9 * np.asarray(prev[p + 'running_mean'], np.float64) + 0.1 * mean.double().numpy()
        out[p + 'running_var'] = (0.9 * np.asarray(prev[p + 'running_var'], np.float64)
                                  + 0.1 * var.double().numpy() * (cnt / (cnt - 1)))
    return out


def oracle_step(model, shape, dtype=torch.float64):
    """one step of oracle.train's operators in ``dtype`` (oracle.train.train_step itself computes in float32) -> dict(loss, y_hat,
    grads {key: array}, bufs {running buffer: array after the step}); computed once per process"""
    key = ('oracle', model, shape, dtype)
    if key in _CACHE:
        return _CACHE[key]
    args, sd = model_args(model), state_dict(model)
    specs, y = data(model, shape)
    segs, n_wins = segments(specs)
    assert n_wins == SHAPES[shape]
    s = {k: (v.to(dtype, copy=True) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    keys = otrain.param_keys(s)
    for k in keys:
        s[k].requires_grad_(True)
    y_hat, stats = otrain.forward_train(s, args, segs.to(dtype), n_wins, None)
    loss = otrain.nan_mse_loss(y_hat, torch.from_numpy(y).to(dtype))
    grads = torch.autograd.grad(loss, [s[k] for k in keys])
    _CACHE[key] = {'loss': float(loss.detach()), 'y_hat': y_hat.detach().double().numpy(),
                   'grads': {k: g.double().numpy() for k, g in zip(keys, grads)},
                   'bufs': next_buffers({k: v.numpy() for k, v in sd.items() if 'running' in k}, stats)}
    return _CACHE[key]


def grad_errors(got, want):
    """{key: max |got - want| / max(1e-3, max |want|)} over the gradient tensors, conv biases (zero under train-mode BatchNorm)
    left out as everywhere in the suite; a missing or misshapen tensor is noticed"""
    assert set(got) == set(want)
    out = {}
    for k, w in want.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == np.asarray(w).shape, k
        if not conv_bias(k):
            out[k] = float(np.abs(g - w).max()) / max(1e-3, float(np.abs(w).max()))
    return out


def f32_oracle_margin(model, shape):
    """how far torch's float32 evaluation of the oracle operators is from the float64 one -> (loss, relative; y_hat; {key: gradient
    error as grad_errors measures it})"""
    w, g = oracle_step(model, shape, torch.float64), oracle_step(model, shape, torch.float32)
    return (abs(g['loss'] - w['loss']) / abs(w['loss']), float(np.abs(g['y_hat'] - w['y_hat']).max()),
            grad_errors(g['grads'], w['grads']))


def adam_f64(p, g, m, v, t, lr):
    """torch.optim.Adam's update number t (default hyper-parameters) in float64 -> (p, m, v)"""
    g = np.asarray(g, np.float64)
    m = 0.9 * np.asarray(m, np.float64) + 0.1 * g
    v = 0.999 * np.asarray(v, np.float64) + 0.001 * g * g
    p = np.asarray(p, np.float64) - (lr / (1 - 0.9 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8)
    return p, m, v


# ---- StandardCNN + BiLSTM: a large batch, then lstm_train_oracle.batch()'s own clips -----------------------------------------------
LSTM_FRAMES_BIG = [1001, 700, 260, 513, 97]
LSTM_ARGS = {'avg': LT.AVG_ARGS, 'max': LT.MAX_ARGS, 'last_step_bi': synth.TTS_ARGS}
LSTM_WALK = ['big', 'own', 'big']


def lstm_case(pool):
    """-> (args, state dict, {'big' / 'own': (specs, y)})"""
    args = dict(LSTM_ARGS[pool], cnn_dropout=0.0)
    return args, synth.random_state_dict(31, 'NISQA_TTS'), {'big': LT.batch(73, LSTM_FRAMES_BIG), 'own': LT.batch(71)}


# ---- NISQA_DE: a large pair batch, then the pairs, masks and bias mapping of test_gpu_train_de's masked step -------------------------
# (align, fuse, seed of the weights and of the masked step's batch, seed of the large batch): 'dot_pm' is that test's own case, seed
# kept (chosen away from argmax ties); 'cos_xym' takes tests/test_gpu_layer_count_train.py's double-ended seed; the large batches'
# seeds are the first from 200 on at which the float64 step's smallest top-2 gap reaches 1e-4 (cos_xym: 3.0e-5, 3.8e-5, 1.4e-5 at
# 200..202, 1.2e-4 at 203; dot_pm: 1.5e-3 at 200).  tests/test_train_history_host.py holds all four batches to that gap, so that no
# rounding difference between two runs flips a hard index
DE_CASES = {'cos_xym': ('cosine', 'x/y/-', 70, 203), 'dot_pm': ('dot', '+/-', 41, 200)}
DE_FRAMES = {'big': ([300, 15, 520, 97, 260, 180], [260, 40, 400, 97, 300, 131]), 'own': ([15, 97, 300], [40, 97, 260])}
DE_BIAS = np.array([[0.1, 0.9, 0.02, -0.003], [-0.2, 1.1, -0.01, 0.002], [0.05, 1.0, 0.0, 0.001]], np.float32)
DE_WALK = ['big', 'own', 'big']


def de_case(name):
    """-> (args, state dict, {'big' / 'own': (specs_deg, specs_ref, y, masks, bias)}): explicit masks on every dropout site, so
    that a step does not depend on how many masks were drawn before it"""
    if ('de', name) in _CACHE:
        return _CACHE[('de', name)]
    align, fuse, seed, seed_big = DE_CASES[name]
    args = DT.de_train_args(align, fuse, cnn_dropout=0.2, td_sa_dropout=0.1, td_2_sa_dropout=0.1)
    sd = DO.random_de_state_dict(seed, fuse)
    batches = {}
    for which, (fd, fr) in DE_FRAMES.items():
        bs = seed_big if which == 'big' else seed
        specs_d, y = LT.batch(100 + bs, fd)
        specs_r, _ = LT.batch(1100 + bs, fr)
        y[1, 0], y[2, 0] = 3.0, np.nan
        nw_d, nw_r = DT.segments(specs_d, args)[1], DT.segments(specs_r, args)[1]
        masks = DT.random_masks(bs, nw_d, nw_r, 2, 2, 0.2)
        bias = np.tile(DE_BIAS, (len(fd) // 3, 1))
        batches[which] = (specs_d, specs_r, y, masks, bias)
    _CACHE[('de', name)] = (args, sd, batches)
    return _CACHE[('de', name)]


def de_gap(name, which):
    """smallest top-2 score gap of the alignment in the float64 step of one batch"""
    args, sd, batches = de_case(name)
    specs_d, specs_r, y, masks, bias = batches[which]
    segs_d, nw_d = DT.segments(specs_d, args)
    segs_r, nw_r = DT.segments(specs_r, args)
    return float(DT.train_step(sd, args, segs_d, nw_d, segs_r, nw_r, y, masks=masks, bias=bias)['gap'])
