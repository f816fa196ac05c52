"""CNN-LSTM-AVG (config/train_nisqa_cnn_lstm_avg.yaml: StandardCNN + BiLSTM + average pooling, segment hop 3) on one MI355X,
HBM-resident like bench.py's main leg: bs 64 clips of 10 s at 48 kHz (int16 PCM already on the device), clips/s over timed steps after
warm-up, in each precision asked for.  Then the BiLSTM alone on the batch's features in the three pooling modes (nisqa_lstm_laststep,
nisqa_lstm_pool avg / max), us per launch and per recurrence step from events.  Prints one JSON line.

  python tools/bench_lstm_pool.py [--steps 30] [--warmup 5] [--precisions bf16x6,f32] [--pool avg]

Per-kernel times of lstm_dir_kernel against lstm_dir_avg_kernel / lstm_dir_max_kernel come from a separate profiler run of the LSTM
leg alone (--lstm-only): rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_lstm_pool.py --lstm-only
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


def _time(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--seconds', type=float, default=10.0)
    ap.add_argument('--precisions', default='bf16x6,f32')
    ap.add_argument('--pool', default='avg', choices=['avg', 'max'])
    ap.add_argument('--lstm-only', action='store_true', help='only the BiLSTM leg (for a profiler run)')
    ap.add_argument('--lstm-reps', type=int, default=20)
    a = ap.parse_args()
    import lstm_pool_oracle as LO
    from nisqa_amd import synth
    from nisqa_amd.engine import HipNisqa
    args, sd = LO.POOL_ARGS[a.pool], LO.state_dict()
    B = a.clips
    pcm = [synth.synth_pcm16(i, a.seconds) for i in range(B)]
    res = {'workload': 'nisqa_cnn_lstm_%s_hbm_resident' % a.pool, 'clips_per_step': B, 'seconds_per_clip': a.seconds,
           'seg_hop': args['ms_seg_hop_length'], 'steps': a.steps, 'warmup': a.warmup}
    eng = None
    for prec in a.precisions.split(','):
        eng = HipNisqa(args, sd, 'cuda:0', precision=prec)
        plan = eng.plan([len(p) for p in pcm], 48000)
        dev = torch.from_numpy(np.concatenate(pcm)).to(eng.device)
        if a.lstm_only:
            break
        step_ms = _time(lambda: eng.forward_pcm(dev, plan, 48000), a.steps, a.warmup)
        res['step_ms_' + prec] = round(step_ms, 4)
        res['clips_per_s_' + prec] = round(B / (step_ms * 1e-3), 1)
        res['mos_first_' + prec] = float(eng.forward_pcm(dev, plan, 48000)[0, 0].item())
    # the BiLSTM + pooling alone on this batch's features: one (clip, direction) workgroup each, max(n_wins) sequential steps
    mel, floor = eng.mel(dev, plan, 48000, clamp=False)
    feat = eng.cnn_std(mel, floor, plan)
    n_steps = int(plan.n_wins.max())
    res['lstm_steps'] = n_steps
    for arch, name in ((1, 'laststep'), (2, 'avg'), (3, 'max')):
        ms = _time(lambda: eng.lstm(feat, plan, arch=arch), a.lstm_reps)
        res['lstm_us_' + name] = round(ms * 1e3, 2)
        res['lstm_us_per_step_' + name] = round(ms * 1e3 / n_steps, 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
