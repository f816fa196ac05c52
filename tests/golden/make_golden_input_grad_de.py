"""Golden vectors for the gradient of NISQA_DE's model(x, n_wins) with respect to x, produced by the REFERENCE's own NISQA_DE module
(nisqa/NISQA_lib.py) in eval mode, in its own float32 arithmetic: ``y = model(x, n_wins); y.backward(g); x.grad``.

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_input_grad_de.py
The reference is imported through oracle/ref_shim.py.  Input: the small case of tests/input_grad_de_oracle.py with zero padding
(weights de_oracle.random_de_state_dict(41, fuse); pairs of (1, 3), (3, 1) and (2, 2) segments padded to L = 4, the degraded clips
lstm_train_oracle.batch(541, .), the reference clips batch(1541, .); g drawn from seed 42), for the three configurations
(cosine, hard, x/y/-), (dot, soft, +/-) and (cosine, soft, x/y).  Stored per configuration in input_grad_de_{cos_hard,dot_soft,
cos_soft}.npz: the seeds and pairs (x is rebuilt from them), n_wins [B, 2], g [B, 1], y [B, 1] and dx [B, L, 2, 48, 15].
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
import de_oracle as DO                                          # noqa: E402
import input_grad_de_oracle as IGD                              # noqa: E402


def run(config):
    NL = ref_shim.import_reference_lib()
    sd, args, x, n_wins, g = IGD.case(config)
    model = NL.NISQA_DE(**DO.model_kwargs(args))
    model.load_state_dict(sd, strict=True)
    model.eval()
    xt = torch.from_numpy(x).requires_grad_(True)
    y = model(xt, torch.as_tensor(n_wins))
    y.backward(torch.from_numpy(g))
    spec = IGD.SMALL
    out = os.path.join(HERE, 'input_grad_de_%s.npz' % IGD.NAMES[config])
    np.savez_compressed(out, seed_sd=spec['seed_sd'], seed_batch=spec['seed_batch'], pairs=np.array(spec['pairs']), L=spec['L'],
                        align=config[0], apply=config[1], fuse=config[2], n_wins=n_wins, g=g, y=y.detach().numpy(),
                        dx=xt.grad.numpy())
    print(out, os.path.getsize(out), 'bytes; max |dx| per clip', np.abs(xt.grad.numpy()).reshape(len(n_wins), -1).max(1))


if __name__ == '__main__':
    for config in IGD.CONFIGS:
        run(config)
