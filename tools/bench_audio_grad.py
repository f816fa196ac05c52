#!/usr/bin/env python3
"""d scores / d audio samples on one GPU at the contract batch: 64 clips x 10 s at 48 kHz, NISQA_DIM, samples and g
resident in HBM.  Three calls, 3 warm-up and 20 timed calls of each alternating in one process, device events around each call,
median (min-max):
  audio_plain     model.forward_audio(y, sr) under no_grad                    (pack + forward_pcm)
  audio_fwd_bwd   model.forward_audio(y, sr) with y.requires_grad; backward   (+ mel recomputed, segments, grad_segments, adjoints)
  segments_fwd_bwd  model(x, n_wins) with x.requires_grad; backward, on the same clips' segments: the path that existed before the
                  audio gradient, the yardstick.

    python tools/bench_audio_grad.py [--clips 64] [--seconds 10] [--precision bf16x6] [--calls 20] [--json OUT]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python tools/bench_audio_grad.py --trace --calls 5
                                                   (audio_fwd_bwd only: the per-kernel split, a run of its own)
    python tools/bench_audio_grad.py --split DIR/ks_kernel_stats.csv --calls 9       (sums that CSV per call: mel backward, segment
                                                   adjoint, mel forward, everything else; calls = warm-up + timed calls of the trace run + 1)

Prints one JSON line.  No CPU fallback: without a GPU the engine raises."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEL_BWD = ('mel_db_bwd_gate_kernel', 'mel_frame_bwd_kernel', 'mel_overlap_add_bwd_kernel')
SEG_ADJ = ('segments_to_mel_bwd_kernel',)
MEL_FWD = ('mel_frame_kernel', 'mel_floor_kernel', 'mel_clamp_kernel')


def split(path, calls):
    """per-call milliseconds of a rocprofv3 kernel_stats CSV by group, and the largest kernels"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((r['Name'], int(r['Calls']), float(r['TotalDurationNs']) / 1e6))
    group = lambda names: sum(ms for n, _, ms in rows if any(k in n for k in names)) / calls
    total = sum(ms for _, _, ms in rows) / calls
    out = {'calls': calls, 'all_kernels_ms': total, 'mel_backward_ms': group(MEL_BWD), 'segment_adjoint_ms': group(SEG_ADJ),
           'mel_forward_ms': group(MEL_FWD),
           'per_kernel_ms': {k: group((k,)) for k in MEL_BWD + SEG_ADJ + MEL_FWD},
           'largest': [(n[:80], c, ms / calls) for n, c, ms in sorted(rows, key=lambda r: -r[2])[:12]]}
    return out


def timed(fns, warmup, calls):
    """the calls of ``fns`` alternating: {name: [ms]}"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--precision', default='bf16x6')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trace', action='store_true', help='audio_fwd_bwd only (for a kernel trace run)')
    ap.add_argument('--split', default=None, metavar='KERNEL_STATS_CSV')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if a.split:
        out = split(a.split, a.calls)
    else:
        from nisqa_amd import NISQA_lib as NL, synth
        from nisqa_amd.engine import HipNisqa
        from oracle import ref_shim
        dev, sr = 'cuda:0', 48000
        args, sd = dict(synth.DIM_ARGS), synth.random_state_dict(7, 'NISQA_DIM')
        m = NL.NISQA_DIM(**{k: args[k] for k in ref_shim.MODEL_ARG_KEYS}).bind_args(args)
        m.load_state_dict(sd, strict=True)
        m.eval()
        eng = m._engine = HipNisqa(args, m.state_dict(), dev, precision=a.precision)
        n = int(a.seconds * sr)
        y = torch.from_numpy(np.stack([synth.synth_pcm16(c, a.seconds).astype(np.float32) / 32768.0 for c in range(a.clips)])).to(dev)
        assert tuple(y.shape) == (a.clips, n)
        g = torch.ones((a.clips, 5), dtype=torch.float32, device=dev)
        plan = eng.plan([n] * a.clips, sr)
        x = eng.segments_from_mel(eng.mel(y.reshape(-1), plan, sr, clamp=True)[0], plan)         # the same clips' segments
        n_wins = torch.from_numpy(plan.n_wins.astype(np.int64))

        def audio_plain():
            with torch.no_grad():
                return m.forward_audio(y, sr)

        def audio_fwd_bwd():
            yg = y.detach().requires_grad_(True)
            m.forward_audio(yg, sr).backward(g)
            return yg.grad

        def segments_fwd_bwd():
            xg = x.detach().requires_grad_(True)
            m(xg, n_wins).backward(g)
            return xg.grad

        fns = {'audio_fwd_bwd': audio_fwd_bwd} if a.trace else \
            {'audio_plain': audio_plain, 'audio_fwd_bwd': audio_fwd_bwd, 'segments_fwd_bwd': segments_fwd_bwd}
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = timed(fns, a.warmup, a.calls)
        dy = audio_fwd_bwd()
        torch.cuda.synchronize()
        out = {'clips': a.clips, 'seconds': a.seconds, 'precision': a.precision, 'frames': plan.total_frames,
               'segments': int(plan.n_wins.sum()), 'calls': a.calls, 'warmup': a.warmup,
               'peak_mb_above_resident': (torch.cuda.max_memory_allocated() - base) / 2 ** 20,
               'grad_finite': bool(torch.isfinite(dy).all()), 'grad_abs_max': float(dy.abs().max()),
               'ms': {k: stats(v) for k, v in ms.items()}}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
