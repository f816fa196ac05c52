#!/usr/bin/env python3
"""d NISQA_DE score / d (degraded samples, reference samples) on one GPU: 32 pairs x 10 s at 48 kHz, the shipped
recipe's cosine / hard alignment, bf16x6, samples and g resident in HBM.  3 warm-up and 20 timed calls of each kind alternating in
one process, device events around each call, median (min-max):
  audio_plain         model.forward_audio(y_deg, y_ref, sr) under no_grad              (pack + forward_pcm on the 64 clips)
  audio_fwd_bwd_both  forward_audio with both sides requiring a gradient; backward
  audio_fwd_bwd_deg   forward_audio with y_deg alone requiring a gradient; backward     (no reference-side CNN / mel backward)
  segments_fwd_bwd    model(x, n_wins) with x.requires_grad; backward, on the same pairs' segments: the path that existed before
                      the audio gradient, the yardstick
  segments_kernel     HipNisqa.segments_from_mel_db on the 64-clip plan                 (nisqa_mel_segments_fwd, one launch)
  segments_indexing   torch.maximum with the per-frame floors + HipNisqa.segments_from_mel: the path the kernel replaces
  mel_bwd_both / mel_bwd_deg   HipNisqa.mel_bwd on the 64-clip plan / on the 32 degraded clips' plan

    python tools/bench_de_audio_grad.py [--pairs 32] [--seconds 10] [--precision bf16x6] [--apply hard] [--calls 20] [--json OUT]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python tools/bench_de_audio_grad.py --trace --calls 5
                                                   (audio_fwd_bwd_both only: the per-kernel split, a run of its own)
    python tools/bench_de_audio_grad.py --split DIR/ks_kernel_stats.csv --calls 9    (sums that CSV per call; calls = 1 + warm-up
                                                   + timed calls of the trace run, as it prints)
The device-event time of segments_kernel is a CALL time: at 64 clips the launch is shorter than the host work in front of it, so the
kernel's own time and rate come from the trace run (segments_kernel_avg_us) over segments_kernel_bytes.

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
sys.path.insert(0, os.path.join(ROOT, 'tests'))


GROUPS = {'segments_kernel': ('mel_segments_fwd_kernel',),
          'mel_backward': ('mel_db_bwd_gate_kernel', 'mel_frame_bwd_kernel', 'mel_overlap_add_bwd_kernel'),
          'segment_adjoint': ('segments_to_mel_bwd_kernel',), 'mel_forward': ('mel_frame_kernel', 'mel_floor_kernel', 'mel_clamp_kernel')}
X_BYTES_PER_SEGMENT = 2 * 48 * 15 * 4          # nisqa_mel_segments_fwd: a segment's 2880 bytes read and 2880 bytes written


def split(path, calls):
    """per-call milliseconds of a rocprofv3 kernel_stats CSV by group; the segment kernel's own launches and average time"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((r['Name'], int(r['Calls']), float(r['TotalDurationNs']) / 1e6))
    group = lambda names: sum(ms for n, _, ms in rows if any(k in n for k in names)) / calls
    out = {'calls': calls, 'all_kernels_ms': sum(ms for _, _, ms in rows) / calls}
    out.update({k + '_ms': group(v) for k, v in GROUPS.items()})
    seg = [(c, ms) for n, c, ms in rows if 'mel_segments_fwd_kernel' in n]
    if seg:
        out['segments_kernel_launches'] = sum(c for c, _ in seg)
        out['segments_kernel_avg_us'] = 1e3 * sum(ms for _, ms in seg) / sum(c for c, _ in seg)
    out['largest'] = [(n[:80], c, ms / calls) for n, c, ms in sorted(rows, key=lambda r: -r[2])[:10]]
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
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--precision', default='bf16x6')
    ap.add_argument('--apply', default='hard', choices=('hard', 'soft'))
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trace', action='store_true', help='audio_fwd_bwd_both only (for a kernel trace run)')
    ap.add_argument('--split', default=None, metavar='KERNEL_STATS_CSV')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    if a.split:
        print(json.dumps(split(a.split, a.calls)))
        return
    import de_oracle as DO
    from nisqa_amd import NISQA_lib as NL, synth
    from nisqa_amd.engine import HipNisqaDE
    dev, sr, B = 'cuda:0', 48000, a.pairs
    args = DO.de_args('cosine', a.apply, 'x/y/-')                 # the shipped recipe's alignment and fusion
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    m.load_state_dict(DO.random_de_state_dict(1, 'x/y/-'), strict=True)
    m.eval()
    eng = m._engine = HipNisqaDE(args, m.state_dict(), dev, precision=a.precision)
    base_eng = eng.base
    n = int(a.seconds * sr)
    clips = lambda first: torch.from_numpy(np.stack([synth.synth_pcm16(first + c, a.seconds).astype(np.float32) / 32768.0
                                                     for c in range(B)])).to(dev)
    y_deg, y_ref = clips(0), clips(1000)
    assert tuple(y_deg.shape) == (B, n)
    g = torch.ones((B, 1), dtype=torch.float32, device=dev)
    plan = eng.plan([n] * B, [n] * B, sr)
    pcm = torch.cat([y_deg.reshape(-1), y_ref.reshape(-1)])
    mel_db, floor = base_eng.mel(pcm, plan, sr, clamp=False)
    clip_of_frame = torch.from_numpy(np.repeat(np.arange(plan.n_clips), plan.T)).to(dev)
    indexing = lambda: base_eng.segments_from_mel(torch.maximum(mel_db, floor[clip_of_frame][:, None]), plan)
    kernel = lambda: base_eng.segments_from_mel_db(mel_db, floor, plan)
    x2 = kernel()
    same_bits = bool(torch.equal(x2, indexing()))
    x = torch.cat([x2[:B], x2[B:]], 2).contiguous()               # [B, L, 2, 48, 15]: the same pairs' segments
    n_wins = torch.from_numpy(np.stack([plan.n_wins[:B], plan.n_wins[B:]], 1).astype(np.int64))
    gm = torch.ones_like(mel_db)
    sub = eng._side_plan(plan, sr, 0)
    f_deg, s_deg = int(plan.frame_off[B]), int(plan.clip_off[B])

    def audio_plain():
        with torch.no_grad():
            return m.forward_audio(y_deg, y_ref, sr)

    def audio_fwd_bwd(both):
        yd, yr = y_deg.detach().requires_grad_(True), y_ref.detach().requires_grad_(both)
        m.forward_audio(yd, yr, sr).backward(g)
        return yd.grad, yr.grad

    def segments_fwd_bwd():
        xg = x.detach().requires_grad_(True)
        m(xg, n_wins).backward(g)
        return xg.grad

    fns = {'audio_plain': audio_plain, 'audio_fwd_bwd_both': lambda: audio_fwd_bwd(True), 'audio_fwd_bwd_deg': lambda: audio_fwd_bwd(False),
           'segments_fwd_bwd': segments_fwd_bwd, 'segments_kernel': kernel, 'segments_indexing': indexing,
           'mel_bwd_both': lambda: base_eng.mel_bwd(pcm, plan, sr, gm, mel_db, floor),
           'mel_bwd_deg': lambda: base_eng.mel_bwd(pcm[:s_deg], sub, sr, gm[:f_deg], mel_db[:f_deg], floor[:B])}
    audio_fwd_bwd(True)                                           # builds the operator chain and packs the weight fragments
    torch.cuda.synchronize()
    if a.trace:
        timed({'audio_fwd_bwd_both': fns['audio_fwd_bwd_both']}, a.warmup, a.calls)
        print(json.dumps({'trace': True, 'calls_of_audio_fwd_bwd_both': 1 + a.warmup + a.calls}))
        return
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    audio_fwd_bwd(True)
    torch.cuda.synchronize()
    peak_both = torch.cuda.max_memory_allocated() - base
    ms = timed(fns, a.warmup, a.calls)
    d_deg, d_ref = audio_fwd_bwd(True)
    d_only = audio_fwd_bwd(False)[0]
    torch.cuda.synchronize()
    # nisqa_mel_segments_fwd: every row of x written, every segment's 15 source rows read (overlapping reads counted per segment)
    seg_bytes = int(x2.numel() * 4 + int(plan.n_wins.sum()) * X_BYTES_PER_SEGMENT // 2)
    out = {'pairs': B, 'seconds': a.seconds, 'precision': a.precision, 'apply': a.apply, 'frames': plan.total_frames,
           'segments': int(plan.n_wins.sum()), 'calls': a.calls, 'warmup': a.warmup,
           'peak_mb_above_resident_fwd_bwd_both': peak_both / 2 ** 20,
           'grad_finite': bool(torch.isfinite(d_deg).all() and torch.isfinite(d_ref).all()),
           'grad_abs_max': [float(d_deg.abs().max()), float(d_ref.abs().max())],
           'deg_only_same_bits': bool(torch.equal(d_only, d_deg)), 'segments_kernel_same_bits_as_indexing': same_bits,
           'segments_kernel_bytes': seg_bytes, 'segments_kernel_unique_bytes': int(x2.numel() * 4 + mel_db.numel() * 4),
           'ms': {k: stats(v) for k, v in ms.items()}}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
