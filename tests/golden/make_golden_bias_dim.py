"""Golden vectors for the bias-aware loss of NISQA_DIM training, produced by the REFERENCE's own ``biasLoss``
(nisqa/NISQA_lib.py:1856-1938), five objects, one per dimension, driven as nisqa/NISQA_model.py:256-371 drives them: after each of
two epochs every object's ``update_bias`` sees its own dimension's labels and predictions; then one batch's loss is the sum of the
five ``get_loss`` values, and autograd gives d loss / d y_hat.

The table (tests/bias_dim_case.py, seeded): 60 files in 3 databases, one of them the anchor (its rows stay the identity), one
with an unlabelled value in one dimension (that dimension's line is skipped for that database).

Run where the reference tree is present:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bias_dim.py
Writes tests/golden/bias_dim.npz: b [2 epochs][5 heads][n][4] (float64, each head's table after each update), idx, loss (fp32),
dy_hat [B][5] (fp32).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref_shim                                    # noqa: E402
import bias_dim_case as case                                   # noqa: E402


def main():
    NL = ref_shim.import_reference_lib()
    db, y, y_hat, idx = case.table()
    losses = [NL.biasLoss(db, anchor_db=case.ANCHOR, mapping='first_order', min_r=case.MIN_R, do_print=False)
              for _ in range(case.HEADS)]
    b = []
    for epoch in range(2):
        for h, bl in enumerate(losses):
            bl.update_bias(y[:, h].reshape(-1, 1), y_hat[epoch][:, h].reshape(-1, 1))
        b.append(np.stack([bl.b.copy() for bl in losses]))
    yb = torch.tensor(y[idx], dtype=torch.float)
    yb_hat = torch.tensor(y_hat[1][idx], dtype=torch.float, requires_grad=True)
    loss = sum(bl.get_loss(yb[:, h].view(-1, 1), yb_hat[:, h].view(-1, 1), idx) for h, bl in enumerate(losses))
    loss.backward()
    np.savez_compressed(os.path.join(HERE, 'bias_dim.npz'), b=np.stack(b), idx=idx, loss=np.float32(loss.item()),
                        dy_hat=yb_hat.grad.numpy())
    print('wrote bias_dim.npz: loss', loss.item(), 'updated heads per epoch', [[bool(bl_b[:, :2].std() > 0) for bl_b in e] for e in b])


if __name__ == '__main__':
    main()
