"""CPU side of NISQA_DIM's bias-aware loss and of training batches that mix sample rates (no GPU is used):

* ``trainloop.biasLoss`` x 5 against the reference's five objects (tests/golden/bias_dim.npz, written by
  tests/golden/make_golden_bias_dim.py), and the ``[B, 5, 4]`` rows it hands to the step against the reference's loss and autograd
  gradient, through the per-head loss restatement (tests/bias_dim_case.py) the GPU tests reuse;
* the two forms of the coefficients the trainers accept (``train.bias_rows``);
* the bookkeeping of a batch staged as several groups (``train.concat_groups``);
* the argument checks of nisqa_mse_loss_heads and nisqa_tdtrain_step_heads (rejected before any launch)."""
import numpy as np
import pytest
import torch

import bias_dim_case as case
import helpers


def _five_losses(db, y, y_hat, epochs=2):
    from nisqa_amd.trainloop import biasLoss
    losses = [biasLoss(db, anchor_db=case.ANCHOR, mapping='first_order', min_r=case.MIN_R, do_print=False) for _ in range(case.HEADS)]
    tables = []
    for epoch in range(epochs):
        for h, bl in enumerate(losses):
            bl.update_bias(y[:, h].reshape(-1, 1), y_hat[epoch][:, h].reshape(-1, 1))
        tables.append(np.stack([bl.b.copy() for bl in losses]))
    return losses, np.stack(tables)


def test_five_bias_losses_reproduce_the_reference_tables_loss_and_gradient():
    g = helpers.golden('bias_dim.npz')
    db, y, y_hat, idx = case.table()
    assert np.array_equal(idx, g['idx']) and len(db) == 60 and int(np.isnan(y).sum()) == 1
    losses, b = _five_losses(db, y, y_hat)
    assert b.shape == g['b'].shape == (2, 5, 60, 4)
    assert np.abs(b - g['b']).max() < 1e-12
    # what the fixture is about: the anchor keeps the identity, the database with an unlabelled value in head 2 keeps it in that
    # head only, head 3 starts one epoch late, and the heads' lines differ
    ident = np.array([0.0, 1.0, 0.0, 0.0])
    anchor, gap = (db == case.ANCHOR).to_numpy(), (db == 'DB_GAP').to_numpy()
    assert (b[:, :, anchor] == ident).all() and (b[:, 2, gap] == ident).all() and (b[0, 3] == ident).all()
    assert not (b[1, 3, ~anchor] == ident).all(-1).any() and not (b[1, 0, gap] == ident).all(-1).any()
    assert np.abs(b[1, 0, ~anchor] - b[1, 1, ~anchor]).max() > 0.1
    rows = np.stack([bl.rows(idx) for bl in losses], 1)
    assert rows.shape == (len(idx), 5, 4) and rows.dtype == np.float32
    yb = torch.tensor(y[idx], dtype=torch.float)
    yb_hat = torch.tensor(y_hat[1][idx], dtype=torch.float, requires_grad=True)
    loss = case.per_head_loss(yb_hat, yb, torch.from_numpy(rows))
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(g['loss']), rel=1e-6)
    assert np.abs(yb_hat.grad.numpy() - g['dy_hat']).max() < 1e-6
    assert np.abs(g['dy_hat'][0, 2]) == 0 and np.abs(g['dy_hat']).min(0).max() > 0          # the unlabelled value: no gradient


def test_bias_losses_that_are_switched_off_hand_out_no_rows():
    from nisqa_amd.trainloop import biasLoss
    db, y, y_hat, idx = case.table()
    bl = biasLoss(db, mapping=None, min_r=None)
    bl.update_bias(y[:, 0], y_hat[0][:, 0])
    assert bl.rows(idx) is None and not bl.apply_bias_loss


def test_bias_rows_accepts_one_mapping_per_clip_or_per_clip_and_head():
    from nisqa_amd.train import bias_rows
    rng = np.random.default_rng(0)
    shared = rng.standard_normal((6, 4))
    rows, per_head = bias_rows(shared, 6, 5)
    assert rows.shape == (6, 4) and rows.dtype == np.float32 and not per_head and np.array_equal(rows, shared.astype(np.float32))
    each = rng.standard_normal((6, 5, 4)).astype(np.float32)
    rows, per_head = bias_rows(each, 6, 5)
    assert rows.shape == (6, 20) and per_head and rows.flags['C_CONTIGUOUS']
    assert np.array_equal(rows.reshape(6, 5, 4), each)                    # [clip][head][4], head-major inside a clip
    one = rng.standard_normal((6, 1, 4)).astype(np.float32)               # one head: the two forms are the same thing
    rows, per_head = bias_rows(one, 6, 1)
    assert rows.shape == (6, 4) and not per_head and np.array_equal(rows, one[:, 0])
    rows, per_head = bias_rows(one[:, 0], 6, 1)
    assert rows.shape == (6, 4) and not per_head
    for bad, h in ((each, 4), (each[:5], 5), (shared[:, :3], 5), (each.reshape(6, 20), 5), (one, 5)):
        with pytest.raises(ValueError):
            bias_rows(bad, 6, h)


def _group(frames, n_wins):
    return np.concatenate(([0], np.cumsum(frames))).astype(np.int32), np.asarray(n_wins, np.int32)


def test_groups_of_one_batch_concatenate_frame_offsets_segment_counts_and_clip_order():
    from nisqa_amd.train import concat_groups
    f0, n0 = _group([17, 71, 131], [1, 15, 30])               # three clips, the first a single segment
    f1, n1 = _group([41, 101], [7, 22])
    f2, n2 = _group([15], [1])                                # a group of ONE single-segment clip
    off, n, order = concat_groups([f0, f1], [n0, n1])
    assert off.dtype == np.int32 and n.dtype == np.int32
    assert off.tolist() == [0, 17, 88, 219, 219 + 41, 219 + 142]
    assert n.tolist() == [1, 15, 30, 7, 22]
    assert order.tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1]]
    off, n, order = concat_groups([f2, f0, f1], [n2, n0, n1])
    assert off.tolist() == [0, 15, 15 + 17, 15 + 88, 15 + 219, 234 + 41, 234 + 142]
    assert n.tolist() == [1, 1, 15, 30, 7, 22]
    assert order.tolist() == [[0, 0], [1, 0], [1, 1], [1, 2], [2, 0], [2, 1]]
    assert f0.tolist() == [0, 17, 88, 219] and f1.tolist() == [0, 41, 142] and f2.tolist() == [0, 15]     # inputs untouched
    # every clip's frames are where its group's spectrogram lands in the concatenation
    for gi, (f, base) in enumerate(zip((f2, f0, f1), (0, 15, 234))):
        for ci in range(len(f) - 1):
            b = order.tolist().index([gi, ci])
            assert off[b] == base + f[ci] and off[b + 1] - off[b] == f[ci + 1] - f[ci]
    with pytest.raises(ValueError):
        concat_groups([f0, f1], [n0, n1[:1]])
    with pytest.raises(ValueError):
        concat_groups([f0, f1 + 1], [n0, n1])


def test_one_group_comes_back_untouched():
    from nisqa_amd.train import concat_groups
    f0, n0 = _group([17, 71, 131], [1, 15, 30])
    off, n, order = concat_groups([f0], [n0])
    assert off is f0 and n is n0
    assert order.tolist() == [[0, 0], [0, 1], [0, 2]]


def test_per_head_entries_validate_without_gpu():
    """nisqa_mse_loss_heads and nisqa_tdtrain_step_heads reject NULL pointers and bad counts before any launch; pointers that only
    have to be non-NULL are the integer P, which a rejected call never reads."""
    import ctypes
    from nisqa_amd import lib
    L, ERR, P = lib.load(), lib.NISQA_ERR_ARG, 0x1000
    assert L.nisqa_mse_loss_heads(None, None, None, 6, 5, None, None, None) == ERR
    for hole in range(4):
        ptrs = [P, P, P, P]
        ptrs[hole] = None
        assert L.nisqa_mse_loss_heads(ptrs[0], ptrs[1], P, 6, 5, ptrs[2], ptrs[3], None) == ERR, hole
    for n_clips, n_heads in ((0, 5), (-1, 5), (6, 0), (6, -2), (6, 65)):
        assert L.nisqa_mse_loss_heads(P, P, P, n_clips, n_heads, P, P, None) == ERR, (n_clips, n_heads)
        assert L.nisqa_mse_loss(P, P, P, n_clips, n_heads, P, P, None) == ERR, (n_clips, n_heads)          # like its twin
    assert L.nisqa_tdtrain_step_heads(None, None) == ERR

    def args(**kw):
        a = lib.TdTrainArgs()
        a.n_clips, a.n_tokens, a.n_tokens_padded, a.n_layers, a.n_heads = 2, 40, 64, 2, 5
        a.n_wgrad_groups, a.n_wgrad_tiles, a.n_colsum_jobs = 1, 1, 1
        for f in ('seg_off', 'ptok_off', 'tile_clip', 'sq_off', 'params', 'grads', 'poff', 'ws', 'frags', 'labels', 'bias_map',
                  'inv_count', 'wgrad_desc', 'colsum_jobs'):
            setattr(a, f, P)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for entry in (L.nisqa_tdtrain_step_heads, L.nisqa_tdtrain_step):
        assert entry(ctypes.byref(lib.TdTrainArgs()), None) == ERR                                      # all zero
        for f in ('seg_off', 'ptok_off', 'tile_clip', 'sq_off', 'params', 'grads', 'poff', 'ws', 'frags', 'labels', 'inv_count',
                  'wgrad_desc', 'colsum_jobs'):
            assert entry(ctypes.byref(args(**{f: None})), None) == ERR, f
        for f, v in (('n_clips', 0), ('n_tokens', 0), ('n_heads', 0), ('n_heads', 9), ('n_layers', 0), ('n_layers', 5),
                     ('n_tokens_padded', 40), ('n_tokens_padded', 0)):
            assert entry(ctypes.byref(args(**{f: v})), None) == ERR, (f, v)
