"""Per-segment score profile test support (not a test module): a torch restatement, in any dtype, of what nisqa_pool_profile computes
-- PoolAttFF (reference nisqa/NISQA_lib.py:1171-1183) taken apart into the masked softmax of its logits and the per-token output of
linear3, PoolAvg (:1196-1204) into 1 / n and the per-token output of its linear layer -- written with the operators of oracle.net's
pool_att_ff, on ONE clip's valid rows (the mask is then a no-op, as everywhere in oracle.net).  tests/test_profile_host.py checks it
against the reference's own modules; the GPU tests check the kernel and the engine against it in float64, with a bar taken from its
own float32 evaluation."""
import numpy as np
import torch
import torch.nn.functional as F

DIM_HEADS = ['pool_layers.%d.model.' % h for h in range(5)]        # NISQA_DIM: mos, noi, dis, col, loud
MOS_HEADS = ['pool.model.']


def att_profile(sd, x, pfx):
    """x [n, 64] (the clip's valid rows) -> (weights [n], local [n], logits [n]) of the PoolAttFF head at pfx, in x's dtype"""
    logits = F.linear(F.relu(F.linear(x, sd[pfx + 'linear1.weight'], sd[pfx + 'linear1.bias'])),
                      sd[pfx + 'linear2.weight'], sd[pfx + 'linear2.bias']).reshape(-1)
    local = F.linear(x, sd[pfx + 'linear3.weight'], sd[pfx + 'linear3.bias']).reshape(-1)
    return torch.softmax(logits, 0), local, logits


def avg_profile(sd, x, pfx='pool.model.'):
    """x [n, 256] (the clip's valid BiLSTM rows) -> (weights [n] = 1 / n, local [n]) of PoolAvg's linear layer, in x's dtype"""
    n = x.shape[0]
    local = F.linear(x, sd[pfx + 'linear.weight'], sd[pfx + 'linear.bias']).reshape(-1)
    return torch.full((n,), 1.0, dtype=x.dtype) / n, local


def profile(sd, rows, heads, dtype=torch.float64):
    """rows: numpy [n, D], one clip's valid rows; heads: the PoolAttFF prefixes, or 'avg' -> (weights [n, H], local [n, H]) as numpy
    arrays of ``dtype``, every operator evaluated in that dtype (float64: the yardstick; float32: what sets the tests' bars)"""
    s = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items() if k.startswith('pool') and 'num_batches' not in k}
    x = torch.from_numpy(np.ascontiguousarray(rows)).to(dtype)
    with torch.no_grad():
        parts = [avg_profile(s, x)] if heads == 'avg' else [att_profile(s, x, p)[:2] for p in heads]
    return torch.stack([p[0] for p in parts], 1).numpy(), torch.stack([p[1] for p in parts], 1).numpy()


def bars(sd, rows, heads):
    """The float64 profile of one clip and the bars of the tests, each max(1e-5, 2 x how far the float32 evaluation of the same
    restatement is from the float64 one): -> (weights64, local64, bar_weights, bar_local, score64 [H], bar_score), the score being
    sum_t weights * local per head."""
    w64, l64 = profile(sd, rows, heads, torch.float64)
    w32, l32 = profile(sd, rows, heads, torch.float32)
    s64, s32 = (w64 * l64).sum(0), (w32 * l32).sum(0, dtype=np.float32)
    bar = lambda a32, a64: max(1e-5, 2.0 * float(np.abs(a32.astype(np.float64) - a64).max()))
    return w64, l64, bar(w32, w64), bar(l32, l64), s64, bar(s32, s64)
