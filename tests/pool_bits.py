"""Inputs and direct C-ABI runs of the bit-identity fixture tests/golden/pool_bits.npz (tests/test_gpu_pool_bits.py compares,
tests/golden/make_golden_pool_bits.py wrote it from a build of the commit BEFORE the two pool-score sources were merged).

One plan of six clips of 1, 31, 32, 33, 64 and 97 tokens, each padded to whole 64-token workgroups, with 64 slack rows behind the
first clip: 512 rows = 16 tiles of 32.  That holds tiles that are all padding (rows 32 .. 127 of clip 0), a tile with ONE valid
token (clip 0, and the last tile of the 33- and 97-token clips), exact tile edges (32, 64), and a tile count that is a multiple of
8 and larger than 8, so xcd_tile (csrc/common.hpp) permutes the blocks.  Weights: synth.random_state_dict through weights.pack_*;
one head (NISQA) and five (NISQA_DIM).  Everything is returned as uint32 views over the valid rows.
"""
import ctypes

import numpy as np
import torch

import helpers
from nisqa_amd import lib as _lib
from nisqa_amd import weights as W

FIXTURE = 'pool_bits.npz'
N_WINS = [1, 31, 32, 33, 64, 97]
TOK_OFF = [0, 128, 192, 256, 320, 384, 512]
HEADS = {1: ('NISQA', 8), 5: ('NISQA_DIM', 7)}              # n_heads -> (model, weight seed)
N_LAYERS = 2
FORMATS = {'bf16': 2, 'bf16x6': 3}                          # entry suffix -> terms per packed fragment


def plan():
    return helpers.plan_with_layout(N_WINS, TOK_OFF)


def _rows(seed, width):
    """[NP, width] float32: standard-normal valid rows, zero padding rows"""
    p = plan()
    a = np.zeros((p.total_tok, width), np.float32)
    idx = p.token_index()
    a[idx] = np.random.default_rng(seed).standard_normal((len(idx), width)).astype(np.float32)
    return a


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t, rows=None):
    h = t.cpu().numpy()
    return np.ascontiguousarray(h if rows is None else h[rows]).view(np.uint32)


def run_pool(n_heads, dev='cuda:0'):
    """-> {'sc_F_hN', 'yv_F_hN': [valid rows, N], 'out_F_hN': [B, N]} for F in FORMATS: what nisqa_pool_score_F leaves in ws, and the
    output of nisqa_pool_att_F"""
    lib = _lib.load()
    model, seed = HEADS[n_heads]
    sd = helpers.random_state_dict(seed, model)
    heads = ['pool_layers.%d.model.' % h for h in range(5)] if n_heads == 5 else ['pool.model.']
    p = plan()
    d = p.to(torch.device(dev))
    np_, idx = p.total_tok, p.token_index()
    x = _up(_rows(31, 64), dev)
    pw = _up(W.pack_pool_att(sd, heads), dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(torch.device(dev)).cuda_stream)
    out = {}
    for fmt, terms in FORMATS.items():
        pwb = _up(W.pack_pool_att_bf16(sd, heads, terms=terms).view(np.int16), dev)
        a = (_p(x), _p(d['tok_off']), _p(d['n_wins']), p.n_clips, np_, n_heads, _p(pw), _p(pwb))
        ws = torch.zeros(np_ * 16, dtype=torch.float32, device=dev)
        _lib.check(getattr(lib, 'nisqa_pool_score_' + fmt)(*a, _p(ws), st), 'nisqa_pool_score_' + fmt)
        out['sc_%s_h%d' % (fmt, n_heads)] = _bits(ws[:np_ * 8].view(np_, 8)[:, :n_heads], idx)
        out['yv_%s_h%d' % (fmt, n_heads)] = _bits(ws[np_ * 8:].view(np_, 8)[:, :n_heads], idx)
        ws2 = torch.zeros(np_ * 16, dtype=torch.float32, device=dev)
        res = torch.zeros((p.n_clips, n_heads), dtype=torch.float32, device=dev)
        _lib.check(getattr(lib, 'nisqa_pool_att_' + fmt)(*a, _p(ws2), _p(res), st), 'nisqa_pool_att_' + fmt)
        out['out_%s_h%d' % (fmt, n_heads)] = _bits(res)
    return out


def run_td(dev='cuda:0'):
    """-> {'td_x': [valid rows, 64]}: the x rows of nisqa_td_selfatt_bf16 (two layers, the NISQA_DIM weights)"""
    lib = _lib.load()
    sd = helpers.random_state_dict(HEADS[5][1], HEADS[5][0])
    p = plan()
    d = p.to(torch.device(dev))
    np_ = p.total_tok
    feat = _up(_rows(32, 384), dev)
    tw = _up(W.pack_self_att(sd, N_LAYERS), dev)
    twb = _up(W.pack_self_att_bf16(sd, N_LAYERS).view(np.int16), dev)
    ws = torch.zeros(np_ * 64 * 9, dtype=torch.float32, device=dev)
    x = torch.zeros((np_, 64), dtype=torch.float32, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(torch.device(dev)).cuda_stream)
    _lib.check(lib.nisqa_td_selfatt_bf16(_p(feat), _p(d['tok_off']), _p(d['n_wins']), p.n_clips, np_, N_LAYERS, _p(tw), _p(twb),
                                         _p(ws), _p(x), st), 'nisqa_td_selfatt_bf16')
    return {'td_x': _bits(x, p.token_index())}
