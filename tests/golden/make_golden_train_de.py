"""Golden vectors for HipTrainerDE (double-ended NISQA_DE training), produced by the REFERENCE's own modules in train mode
(nisqa/NISQA_lib.py NISQA_DE; biasLoss.get_loss; torch.optim.Adam as at NISQA_model.py:96, 131-152).

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_de.py [case ...]
The reference is imported through oracle/ref_shim.py.  Dropout probabilities are set to 0 (the reference draws its masks inside
its modules; tests/de_train_oracle.py takes them as inputs instead).  Weights: tests/de_oracle.random_de_state_dict(seed_sd, fuse).
Inputs: five pairs, the degraded spectrograms tests/lstm_train_oracle.batch(seed_deg, 15 / 40 / 97 / 300 / 260 frames) with its
labels (one NaN), the reference spectrograms batch(seed_ref, 40 / 15 / 97 / 260 / 300 frames): at hop 4 n_wins (1,7), (7,1),
(21,21), (72,62), (62,72) -- a single token on either side (a one-token reference is chosen by every degraded token), more than
64 tokens on either side.

Condition on the inputs: a hard index is only comparable where its argmax is no near-tie.  The seeds are searched (seed_sd + k,
seed_deg + k, seed_ref + k for k = 0, 1, ...) until the smallest fp32 top-2 score gap over every degraded token with at least two
reference tokens is >= 1e-4 in BOTH steps -- ten times the 1e-5 band inside which the inference tests accept either index -- and the
stored case asserts it.  The scores are those of the reference's own first self-attention outputs (forward hooks), restated by
de_oracle.scores.

Stored per case: the seeds, n_wins of both sides, the hard indices of step 1 (pair after pair) and the smallest gap of each step,
loss and y_hat of two consecutive steps, every gradient of the first step (the CNN's in a second file, train_de_<name>_cnn.npz, so
that each file stays under 1 MiB), the BatchNorm buffers and num_batches_tracked after each step.
Cases: cos_xym (cosine, hard, x/y/-: the shipped recipe) and dot_pm (dot, hard, +/-).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shim, net as onet                       # noqa: E402
import de_oracle as DO                                         # noqa: E402
import de_train_oracle as DT                                   # noqa: E402
import lstm_train_oracle as LT                                 # noqa: E402

MIN_GAP = 1e-4


def attempt(NL, args, seed_sd, seed_deg, seed_ref, lr):
    """two steps of the reference on one choice of seeds -> the case's arrays (with the smallest gap of each step)"""
    import pandas as pd
    model = NL.NISQA_DE(**DO.model_kwargs(args))
    sd0 = DO.random_de_state_dict(seed_sd, args['de_fuse'], args['td_2_sa_num_layers'])
    model.load_state_dict(sd0, strict=True)
    model.train()
    specs_d, y = LT.batch(seed_deg, DT.FRAMES_DEG)
    specs_r, _ = LT.batch(seed_ref, DT.FRAMES_REF)
    n = len(specs_d)
    seg = lambda s, L: onet.segment_specs(s, args['ms_seg_length'], args['ms_seg_hop_length'], L)
    nw = np.array([[seg(d, None)[1], seg(r, None)[1]] for d, r in zip(specs_d, specs_r)])
    L = int(nw.max())
    x = torch.stack([torch.cat([torch.as_tensor(seg(d, L)[0]), torch.as_tensor(seg(r, L)[0])], 1) for d, r in zip(specs_d, specs_r)])
    n_wins = torch.as_tensor(nw)
    td_out = []
    hook = model.time_dependency.register_forward_hook(lambda m, i, o: td_out.append(o[0].detach().numpy().copy()))
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loss_fn = NL.biasLoss(pd.Series(['db'] * n), anchor_db=None, mapping=None, min_r=None, do_print=False)
    out = {'n_wins': nw, 'seed_sd': seed_sd, 'seed_deg': seed_deg, 'seed_ref': seed_ref, 'lr': lr,
           'nbt0': int(sd0['cnn.model.bn1.num_batches_tracked']), 'hop': int(args['ms_seg_hop_length']),
           'align': str(args['de_align']), 'fuse': str(args['de_fuse'])}
    yt = torch.as_tensor(y)
    for step in (1, 2):
        del td_out[:]
        y_hat = model(x, n_wins)
        loss = loss_fn.get_loss(yt, y_hat, np.arange(n))
        loss.backward()
        tx, ty = td_out                                             # [B, L, 64] of the degraded, then of the reference clips
        idx, gap = [], np.inf
        for b in range(n):
            _, i_b, g_b = DO.align_fuse(tx[b, :nw[b, 0]], ty[b, :nw[b, 1]], args['de_align'], 'hard', args['de_fuse'])
            idx.append(i_b)
            gap = min(gap, float(g_b.min()))
        out['gap%d' % step] = gap
        out['loss%d' % step] = float(loss.detach())
        out['y_hat%d' % step] = y_hat.detach().numpy()
        if step == 1:
            out['idx1'] = np.concatenate(idx).astype(np.int32)
            for k, p in model.named_parameters():
                out['grad/' + k] = p.grad.detach().numpy().copy()
        for k, v in model.state_dict().items():                    # BatchNorm buffers after this step's two CNN calls
            if k.split('.')[-1].startswith(('running', 'num_batches')):
                out['sd%d/%s' % (step, k)] = v.detach().numpy().copy()
        opt.step()
        opt.zero_grad()
    hook.remove()
    return out


def run(name, align, fuse, seed_sd, seed_deg, seed_ref, lr=1e-3, tries=40):
    NL = ref_shim.import_reference_lib()
    args = DT.de_train_args(align, fuse)
    for k in range(tries):
        out = attempt(NL, args, seed_sd + k, seed_deg + k, seed_ref + k, lr)
        print(name, 'seeds', seed_sd + k, seed_deg + k, seed_ref + k, 'gaps %.3g %.3g' % (out['gap1'], out['gap2']))
        if min(out['gap1'], out['gap2']) >= MIN_GAP:
            break
    assert min(out['gap1'], out['gap2']) >= MIN_GAP, 'no seeds with a top-2 gap >= %g' % MIN_GAP
    k = 'cnn.model.bn1.num_batches_tracked'                                  # two CNN calls per step
    assert int(out['sd1/' + k]) == out['nbt0'] + 2 and int(out['sd2/' + k]) == out['nbt0'] + 4
    cnn = {k: v for k, v in out.items() if k.startswith('grad/cnn.')}
    np.savez_compressed(os.path.join(HERE, 'train_de_%s.npz' % name), **{k: v for k, v in out.items() if k not in cnn})
    np.savez_compressed(os.path.join(HERE, 'train_de_%s_cnn.npz' % name), **cnn)
    print(name, 'loss', out['loss1'], out['loss2'], 'n_wins', out['n_wins'].tolist())


if __name__ == '__main__':
    torch.manual_seed(0)
    want = set(sys.argv[1:])
    cases = [('cos_xym', lambda: run('cos_xym', 'cosine', 'x/y/-', 33, 93, 1093)),
             ('dot_pm', lambda: run('dot_pm', 'dot', '+/-', 34, 94, 1094))]
    for name, fn in cases:
        if not want or name in want:
            fn()
