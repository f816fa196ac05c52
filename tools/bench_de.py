"""NISQA_DE (double-ended) rate on one MI355X, HBM-resident like bench.py's main leg: bs 64 pairs of 10 s clips at 48 kHz (int16 PCM
already on the device), pairs/s over timed steps after warm-up, plus the alignment + fusion kernel's own time against its roofline.
Prints one JSON line.

  python tools/bench_de.py [--steps 50] [--warmup 10] [--precision bf16x6] [--align cosine --apply hard --fuse x/y/-]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

HBM_TBS = 8.0           # MI355X HBM3E peak, TB/s
F32_MATRIX_TFS = 157.3  # fp32 matrix peak, TFLOP/s (the kernel runs fp32 VALU: its own ceiling is the vector rate below)
F32_VECTOR_TFS = 157.3 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--precision', default=None)
    ap.add_argument('--align', default='cosine')
    ap.add_argument('--apply', default='hard')
    ap.add_argument('--fuse', default='x/y/-')
    a = ap.parse_args()
    import de_oracle as DO
    from nisqa_amd import synth
    from nisqa_amd.engine import HipNisqaDE
    args = DO.de_args(a.align, a.apply, a.fuse)
    eng = HipNisqaDE(args, DO.random_de_state_dict(1, a.fuse), 'cuda:0', precision=a.precision)
    B = a.pairs
    deg = [synth.synth_pcm16(i, a.seconds) for i in range(B)]
    ref = [synth.synth_pcm16(1000 + i, a.seconds) for i in range(B)]
    plan = eng.plan([len(p) for p in deg], [len(p) for p in ref], 48000)
    pcm = torch.from_numpy(np.concatenate(deg + ref)).to(eng.device)
    for _ in range(a.warmup):
        eng.forward_pcm(pcm, plan, 48000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        out = eng.forward_pcm(pcm, plan, 48000)
    e1.record()
    torch.cuda.synchronize()
    step_ms = e0.elapsed_time(e1) / a.steps
    # the alignment kernel alone, on the first self-attention output of this batch
    feat = eng.features(pcm, plan, 48000)
    x = eng.base.td(feat, plan)
    for _ in range(5):
        eng.align_fuse(x, plan)
    torch.cuda.synchronize()
    n_al = 200
    e0.record()
    for _ in range(n_al):
        eng.align_fuse(x, plan)
    e1.record()
    torch.cuda.synchronize()
    align_us = e0.elapsed_time(e1) / n_al * 1e3          # includes the zero-fill of the 384-wide output the engine allocates
    nx = plan.n_wins[:B].astype(np.float64)
    ny = plan.n_wins[B:].astype(np.float64)
    flop = float((nx * ny).sum()) * 64 * 2 * (2 if a.apply == 'soft' else 1)
    F = DO.FUSE_WIDTH[a.fuse]
    traffic = float(plan.total_tok * 64 * 4 + plan.tok_off[B] * (F * 4))   # read both clips' rows, write the fused rows
    roof_us = max(flop / (F32_VECTOR_TFS * 1e12), traffic / (HBM_TBS * 1e12)) * 1e6
    print(json.dumps({
        'workload': 'nisqa_de_hbm_resident', 'precision': eng.precision, 'align': a.align, 'apply': a.apply, 'fuse': a.fuse,
        'pairs_per_step': B, 'seconds_per_clip': a.seconds, 'steps': a.steps, 'warmup': a.warmup,
        'step_ms': round(step_ms, 4), 'pairs_per_s': round(B / (step_ms * 1e-3), 1),
        'align_fuse_us': round(align_us, 2), 'align_fuse_gflop': round(flop * 1e-9, 4), 'align_fuse_mb': round(traffic * 1e-6, 2),
        'align_fuse_roofline_us': round(roof_us, 2), 'mos_first': float(out[0, 0].item())}))


if __name__ == '__main__':
    main()
