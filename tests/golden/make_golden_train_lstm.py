"""Golden vectors for HipTrainerLSTM (StandardCNN + BiLSTM training), produced by the REFERENCE's own modules in train mode
(nisqa/NISQA_lib.py NISQA with cnn_model=standard, td=lstm; biasLoss.get_loss; torch.optim.Adam as at NISQA_model.py:96,
131-152).

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_lstm.py [case ...]
The reference is imported through oracle/ref_shim.py.  Dropout probabilities are set to 0 (the reference draws its masks inside
its modules; tests/lstm_train_oracle.py takes them as inputs instead).  Inputs: tests/lstm_train_oracle.batch(seed_batch), so
clips of 15 (one segment), 40, 97, 260 and 1001 frames, one NaN label.
Stored per case: seeds, loss and y_hat of two consecutive steps, every gradient of the first step (the CNN's in a second file,
train_lstm_<name>_cnn.npz, so that each file stays under 1 MiB) and the BatchNorm buffers after each step.  The post-Adam weights are not stored: tests recompute them with torch.optim.Adam from the stored gradients.
Cases: avg (the recipe, hop 3) and max from synth.random_state_dict(seed, 'NISQA_TTS'); last_step_bi at hop 1 from the
published nisqa_tts.tar (a fine-tuning step: first-step gradients only).
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
from nisqa_amd import synth                                    # noqa: E402
import lstm_train_oracle as LT                                 # noqa: E402


def run(name, args, seed_sd, seed_batch, lr, checkpoint=None):
    NL = ref_shim.import_reference_lib()
    if checkpoint is not None:
        ck = torch.load(checkpoint, map_location='cpu', weights_only=False)
        args = dict(ck['args'])
        sd0 = {k: v.numpy() for k, v in ck['model_state_dict'].items()}
    else:
        args = dict(args)
        sd0 = synth.random_state_dict(seed_sd, 'NISQA_TTS')
    args['cnn_dropout'] = 0.0
    margs = {k: args[k] for k in ref_shim.MODEL_ARG_KEYS}
    model = NL.NISQA(**margs)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd0.items()}, strict=True)
    model.train()
    specs, y = LT.batch(seed_batch)
    n = len(specs)
    L = args['ms_max_segments']
    xs, nw = zip(*[onet.segment_specs(s, args['ms_seg_length'], args['ms_seg_hop_length'], L) for s in specs])
    x, n_wins = torch.stack(xs), torch.tensor(nw)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    import pandas as pd
    loss_fn = NL.biasLoss(pd.Series(['db'] * n), anchor_db=None, mapping=None, min_r=None, do_print=False)
    out = {'n_wins': np.array(nw), 'seed_sd': seed_sd, 'seed_batch': seed_batch, 'lr': lr,
           'hop': int(args['ms_seg_hop_length']), 'pool': str(args['pool'])}
    yt = torch.as_tensor(y)
    for step in (1, 2):
        y_hat = model(x, n_wins)
        loss = loss_fn.get_loss(yt, y_hat, np.arange(n))
        loss.backward()
        out['loss%d' % step] = float(loss)
        out['y_hat%d' % step] = y_hat.detach().numpy()
        if step == 1:
            for k, p in model.named_parameters():
                out['grad/' + k] = p.grad.detach().numpy().copy()
        for k, v in model.state_dict().items():                    # BatchNorm buffers after this step's forward
            if k.split('.')[-1].startswith(('running', 'num_batches')):
                out['sd%d/%s' % (step, k)] = v.detach().numpy().copy()
        if checkpoint is not None:
            break
        opt.step()
        opt.zero_grad()
    # two files per case (each under 1 MiB): the CNN's gradients in train_lstm_<name>_cnn.npz, everything else here
    cnn = {k: v for k, v in out.items() if k.startswith('grad/cnn.')}
    np.savez_compressed(os.path.join(HERE, 'train_lstm_%s.npz' % name), **{k: v for k, v in out.items() if k not in cnn})
    np.savez_compressed(os.path.join(HERE, 'train_lstm_%s_cnn.npz' % name), **cnn)
    print(name, 'loss', out['loss1'], out.get('loss2'), 'segments', int(sum(nw)))


if __name__ == '__main__':
    torch.manual_seed(0)
    want = set(sys.argv[1:])
    tts = os.path.join(ref_shim.REFERENCE_ROOT, 'weights', 'nisqa_tts.tar')
    cases = [('avg', lambda: run('avg', LT.AVG_ARGS, 21, 51, 1e-3)),
             ('max', lambda: run('max', LT.MAX_ARGS, 22, 52, 1e-3)),
             ('last_step_bi', lambda: run('last_step_bi', None, -1, 53, 1e-3, checkpoint=tts))]
    for name, fn in cases:
        if not want or name in want:
            fn()
