"""Bias-aware loss of NISQA_DIM training, test support (not a test module): the seeded table behind tests/golden/bias_dim.npz
(tests/golden/make_golden_bias_dim.py runs the reference's five ``biasLoss`` objects on it) and a restatement of the loss with
one cubic mapping per clip AND head (reference nisqa/NISQA_model.py:341-347 with NISQA_lib.py:1879-1894, 1934-1938):

    loss = sum_h mean over {b : y[b,h] not NaN} of (map_bh(y_hat[b,h]) - y[b,h])^2,   map_bh(v) = q0 + q1 v + q2 v^2 + q3 v^3,
    q = bias[b,h,:]

as a torch function of any dtype, so autograd gives d loss / d y_hat (and, through a model, every parameter gradient).
"""
import numpy as np
import pandas as pd
import torch

HEADS = 5
MIN_R = 0.5
ANCHOR = 'DB_ANCHOR'
DBS = (('DB_ANCHOR', 22), ('DB_PLAIN', 20), ('DB_GAP', 18))       # 60 files; DB_GAP has one unlabelled value in head 2
SEED = 2024


def table(seed=SEED):
    """-> (db: pandas Series [n], y float64 [n,5] with one NaN, y_hat float64 [2 epochs][n,5], idx: the batch's indices).
    Every database sees the labels through its own line (what the bias loss is about).  Head 3's predictions of the first epoch
    are noise, so that head's correlation stays below MIN_R and its table is first written after the second epoch."""
    rng = np.random.default_rng(seed)
    db = pd.Series([name for name, n in DBS for _ in range(n)], name='db')
    n = len(db)
    y = rng.uniform(1.0, 5.0, (n, HEADS))
    slope = {name: rng.uniform(0.6, 1.3, HEADS) for name, _ in DBS}
    shift = {name: rng.uniform(-0.8, 0.8, HEADS) for name, _ in DBS}
    y_hat = []
    for epoch in range(2):
        e = np.stack([(y[i] - shift[d]) / slope[d] for i, d in enumerate(db)]) + (0.5 - 0.2 * epoch) * rng.standard_normal((n, HEADS))
        if epoch == 0:
            e[:, 3] = rng.uniform(1.0, 5.0, n)
        y_hat.append(e)
    gap = int(np.flatnonzero((db == 'DB_GAP').to_numpy())[4])
    y[gap, 2] = np.nan
    idx = np.concatenate(([gap], rng.permutation(np.delete(np.arange(n), gap))[:11])).astype(np.int64)     # all three databases
    return db, y, np.stack(y_hat), idx


def per_head_loss(y_hat, y, bias=None):
    """y_hat, y [B,H] (NaN = unlabelled), bias [B,H,4] or None -> the scalar loss (a head without a label contributes 0)."""
    loss = y_hat.sum() * 0
    for h in range(y_hat.shape[1]):
        v = y_hat[:, h]
        if bias is not None:
            q = bias[:, h]
            v = q[:, 0] + q[:, 1] * v + q[:, 2] * v ** 2 + q[:, 3] * v ** 3
        ok = ~torch.isnan(y[:, h])
        if bool(ok.any()):
            loss = loss + torch.mean((v[ok] - y[ok, h]) ** 2)
    return loss
