"""Support of the NISQA_DE audio-gradient tests (not a test module): the float64 double-ended network gradient
(tests/input_grad_de_oracle.py) composed with the float64 restatement of the mel front end (tests/audio_grad_oracle.py), side by
side -- what d model(y_deg, y_ref) / d y_deg and / d y_ref are held to -- and the seeded signals the CPU and the GPU tests share."""
import numpy as np
import torch

import audio_grad_oracle as AG
import input_grad_de_oracle as IGD

SR = 48000
FRAMES_DEG, FRAMES_REF = (15, 23, 19), (19, 15, 27)       # at seg_hop 4: (1, 2), (3, 1) and (2, 4) segments
PAIRS = [(1, 2), (3, 1), (2, 4)]
SEED_G = 77
# seeds of audio_grad_oracle.smooth_signal, (degraded clips, reference clips), one set for every config (the CNN and the first
# self-attention carry SMALL's weights in all of them): per clip the first seed, counting up from 100 b + 11 (reference:
# 1000 + 100 b + 11), for which, at the float64 restatement's own clamped rows, the float64 CNN tie margin of every segment is
# >= 1e-4 = 10 TIE (the engine's rows differ from the restatement's by up to 1e-3 dB), the mel margin >= audio_grad_oracle.MARGIN_DB
# and, for a reference clip, the top-2 gap of the dot and of the cosine scores of every degraded token >= 1e-4.  Such margins
# are rare (one clip in a few hundred); tests/test_de_audio_grad_host.py re-checks the chosen ones: margin 1.03e-4, gap 2.0e-4
# (cosine) / 8.3e-3 (dot), mel margin 28 dB.
SEEDS = ((17, 1226, 758), (1027, 1237, 15948))
E2E_SEEDS = {name: SEEDS for name in ('cos_hard', 'dot_soft', 'cos_soft')}
SEED_MARGIN = 1e-4


def compose_de(sd, args, rows_deg, rows_ref, ys_deg, ys_ref, sr, gs, idx=None):
    """The wanted d (sum g * model) / d y_deg and / d y_ref of a batch of B pairs: rows_* the clamped dB rows [T_b, 48] per clip
    (the engine's float32 rows: the point the network's ReLU, max-pool and argmax choices are compared at; float64 rows keep
    their width), ys_* the samples per clip, gs a list of g [B, 1]; idx: per pair the hard indices to gather at near-ties
    (input_grad_de_oracle's rule).  The float64 network gradient is evaluated at x [B, L, 2, 48, 15] cut from those rows with
    audio_grad_oracle.segments_of, and each channel is pulled back through segments_adjoint and the float64 restatement's
    vector-Jacobian product at its own samples.
    -> dict(dy_deg, dy_ref: per g a list of [L_b] arrays; y [B, 1]; margin [B, L, 2]; gap, own, idx: the oracle's, per pair;
    mel_margin, mel_gap [B, 2]; n_wins [B, 2]; x)"""
    seg_hop = args['ms_seg_hop_length']
    B = len(rows_deg)
    segs = [[AG.segments_of(np.asarray(r), seg_hop) for r in rows] for rows in (rows_deg, rows_ref)]
    n_wins = np.array([[len(segs[0][b]), len(segs[1][b])] for b in range(B)], dtype=np.int64)
    L = int(n_wins.max())
    x = np.zeros((B, L, 2, 48, 15), dtype=np.result_type(*[s.dtype for s in segs[0] + segs[1]]))
    for c in range(2):
        for b, s in enumerate(segs[c]):
            x[b, :len(s), c:c + 1] = s
    net = IGD.oracle(sd, args, x, n_wins, gs, idx=idx)
    dy = [[[] for _ in gs], [[] for _ in gs]]
    mm, mg = np.zeros((B, 2)), np.zeros((B, 2))
    for c, (rows, ys) in enumerate(((rows_deg, ys_deg), (rows_ref, ys_ref))):
        for b, yb in enumerate(ys):
            T = rows[b].shape[0]
            for k in range(len(gs)):
                grow = AG.segments_adjoint(net['dx'][k][b, :n_wins[b, c], c:c + 1], T, seg_hop)
                d, _, _, mm[b, c], mg[b, c] = AG.mel_vjp(yb, sr, grow, args['ms_fmax'])
                dy[c][k].append(d)
    return {'dy_deg': dy[0], 'dy_ref': dy[1], 'y': net['y'], 'margin': net['margin'], 'gap': net['gap'], 'own': net['own'],
            'idx': net['idx'], 'mel_margin': mm, 'mel_gap': mg, 'n_wins': n_wins, 'x': x}


def signals(config_name, seeds=None):
    """the three pairs at 48 kHz -> (ys_deg, ys_ref: lists of float32 sample arrays, lengths_deg, lengths_ref)"""
    sd_, sr_ = seeds or E2E_SEEDS[config_name]
    ld, lr = AG.lengths_of(SR, FRAMES_DEG), AG.lengths_of(SR, FRAMES_REF)
    return ([AG.smooth_signal(SR, n, s) for n, s in zip(ld, sd_)], [AG.smooth_signal(SR, n, s) for n, s in zip(lr, sr_)],
            np.asarray(ld), np.asarray(lr))


def restatement_rows(ys, sr, fmax):
    """the float64 restatement's clamped rows of each clip, rounded to float32: where the seeds are chosen"""
    out = []
    for y in ys:
        with torch.no_grad():
            out.append(AG.mel_forward(torch.from_numpy(y), sr, fmax)[0].numpy().astype(np.float32))
    return out


def case(config):
    """-> (state_dict, args, g [3, 1]) of a config of input_grad_de_oracle.CONFIGS: SMALL's weights"""
    sd, args = IGD.case(config)[:2]
    g = np.random.default_rng(SEED_G).standard_normal((3, 1)).astype(np.float32)
    return sd, args, g


def seed_margins(config, seeds=None):
    """the smallest float64 CNN tie margin, the smallest top-2 score gap and the smallest mel margin of a config's signals at the
    restatement's rows -> (margin, gap, mel margin, n_wins)"""
    sd, args, g = case(config)
    ys_d, ys_r, _, _ = signals(IGD.NAMES[config], seeds)
    want = compose_de(sd, args, restatement_rows(ys_d, SR, args['ms_fmax']), restatement_rows(ys_r, SR, args['ms_fmax']),
                      ys_d, ys_r, SR, [g])
    m = want['margin'][np.isfinite(want['margin'])]
    return float(m.min()), min(float(gp.min()) for gp in want['gap']), float(want['mel_margin'].min()), want['n_wins']
