"""Self-attention blocks of another depth (test support, not a test module): a state dict whose block has exactly n encoder
layers, and the matching args.  synth.random_state_dict and de_oracle.random_de_state_dict draw two layers from ONE generator
stream, so a third layer drawn there would move every tensor behind it; here the layers a block lacks come from generators of
their own, (seed, layer), and everything the state dict already holds keeps its bits."""
import numpy as np
import torch

# (key behind 'layers.<l>.', shape, standard deviation, offset): the key set, shapes and magnitudes of one layer in
# synth.random_state_dict -- LayerNorm gammas 1 + 0.1 N(0, 1) and betas 0.1 N(0, 1), so no two layers are alike
LAYER = (('self_attn.in_proj_weight', (192, 64), 0.25, 0.0), ('self_attn.in_proj_bias', (192,), 0.1, 0.0),
         ('self_attn.out_proj.weight', (64, 64), 0.125, 0.0), ('self_attn.out_proj.bias', (64,), 0.1, 0.0),
         ('linear1.weight', (64, 64), 0.125, 0.0), ('linear1.bias', (64,), 0.1, 0.0),
         ('linear2.weight', (64, 64), 0.125, 0.0), ('linear2.bias', (64,), 0.1, 0.0),
         ('norm1.weight', (64,), 0.1, 1.0), ('norm1.bias', (64,), 0.1, 0.0),
         ('norm2.weight', (64,), 0.1, 1.0), ('norm2.bias', (64,), 0.1, 0.0))
TD, TD2 = 'time_dependency.model.', 'time_dependency_2.model.'


def layer_of(key, pfx=TD):
    """the layer index of a key of the block at pfx, None for every other key"""
    head = pfx + 'layers.'
    return int(key[len(head):].split('.')[0]) if key.startswith(head) else None


def depth(sd, pfx=TD):
    ls = [layer_of(k, pfx) for k in sd]
    return 1 + max([l for l in ls if l is not None], default=-1)


def random_layer(seed, l):
    rng = np.random.default_rng((int(seed), int(l)))
    return {k: torch.from_numpy((off + std * rng.standard_normal(shape)).astype(np.float32)) for k, shape, std, off in LAYER}


def with_layers(sd, n, pfx=TD, seed=0):
    """A copy of sd whose block at pfx has layers 0 .. n-1: the layers sd has are kept bit for bit, those >= n are dropped, the
    missing ones are random_layer(seed, l); they stand where the block's layers stand, so the key order stays a checkpoint's."""
    assert n >= 1
    have = depth(sd, pfx)
    new = [(pfx + 'layers.%d.%s' % (l, k), v) for l in range(have, n) for k, v in random_layer(seed, l).items()]
    items, behind_layers, behind_block = [], None, None
    for k, v in sd.items():
        l = layer_of(k, pfx)
        if l is not None and l >= n:
            continue
        items.append((k, v.clone() if torch.is_tensor(v) else np.array(v)))
        if l is not None:
            behind_layers = len(items)
        if k.startswith(pfx):
            behind_block = len(items)
    if new:
        at = behind_layers if behind_layers is not None else behind_block
        assert at is not None, 'no block at ' + pfx
        items[at:at] = new
    out = dict(items)
    assert depth(out, pfx) == n and len(out) == len(sd) + (n - have) * len(LAYER)
    return out


def args_with_layers(args, n, key='td_sa_num_layers'):
    out = dict(args)
    out[key] = int(n)
    return out
