"""Golden vectors for the gradient of model(x, n_wins) with respect to x of the StandardCNN + BiLSTM models, produced by the
REFERENCE's own NISQA module (nisqa/NISQA_lib.py; cnn_model=standard, td=lstm, pool=last_step_bi / avg / max) in eval mode, in
its own float32 arithmetic: ``y = model(x, n_wins); y.backward(g); x.grad``.

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grad_lstm.py
The reference is imported through oracle/ref_shim.py.  Input: the small case of tests/input_grad_lstm_oracle.py (weights
synth.random_state_dict(30, 'NISQA_TTS'), clips lstm_train_oracle.batch(530, [15, 17, 16]) -> 1, 3 and 2 segments at hop 1 padded
with zeros to L = 4, g drawn from seed 31).  Stored per pooling in input_grad_lstm_{last_step_bi,avg,max}.npz: the seeds and frame
counts (x is rebuilt from them), n_wins, g [B, 1], y [B, 1] and dx [B, L, 1, 48, 15].
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shim                                     # noqa: E402
import input_grad_lstm_oracle as IL                             # noqa: E402


def run(pool):
    sd, args, x, n_wins, g = IL.case(pool)
    ref, _ = ref_shim.build_reference_model(args, sd)
    xt = torch.from_numpy(x).requires_grad_(True)
    y = ref(xt, torch.as_tensor(n_wins))
    y.backward(torch.from_numpy(g))
    spec = IL.SMALL
    out = os.path.join(HERE, 'input_grad_lstm_%s.npz' % pool)
    np.savez_compressed(out, seed_sd=spec['seed_sd'], seed_batch=spec['seed_batch'], frames=np.array(spec['frames']), L=spec['L'],
                        n_wins=n_wins, g=g, y=y.detach().numpy(), dx=xt.grad.numpy())
    print(out, os.path.getsize(out), 'bytes; max |dx| per clip', np.abs(xt.grad.numpy()).reshape(len(n_wins), -1).max(1))


if __name__ == '__main__':
    for pool in IL.POOLS:
        run(pool)
