"""CNN-LSTM-AVG training step (config/train_nisqa_cnn_lstm_avg.yaml: StandardCNN + BiLSTM + PoolAvg, hop 3) from PCM at the recipe's
own batch, 40 ten-second 48 kHz clips (~13 160 segments), on one GPU: HipTrainerLSTM.step_pcm, median over the timed steps after
warm-up; then the reference's own CPU step on the same clips (oracle.ref_shim.reference_train_step, the second of two steps, as
bench.py's train leg takes it).  Side measurement quoted in DESIGN.md 4.9; the driver's bench contract is bench.py.

    python tools/bench_train_lstm.py [--bs 40] [--steps 50] [--warmup 5] [--pool avg] [--no-ref]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np
import torch

from nisqa_amd import synth
from nisqa_amd.train_lstm import HipTrainerLSTM


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bs', type=int, default=40)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--pool', default='avg', choices=['avg', 'max'])
    ap.add_argument('--no-ref', action='store_true')
    o = ap.parse_args()
    import lstm_train_oracle as LT
    args = dict(LT.AVG_ARGS if o.pool == 'avg' else LT.MAX_ARGS)      # cnn_dropout 0.2 as in the yaml
    sd = synth.random_state_dict(11, 'NISQA_TTS')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    tr = HipTrainerLSTM(args, sd, dev, lr=1e-3)
    clips = [synth.synth_pcm16(i % 8, 10.0) for i in range(o.bs)]
    plan = tr.eng.plan([len(c) for c in clips], 48000)
    x = tr.eng.pcm16_to_f32(torch.from_numpy(np.concatenate(clips)).to(dev))
    y = np.random.default_rng(0).uniform(1, 5, (o.bs, 1)).astype(np.float32)
    for _ in range(o.warmup):
        tr.step_pcm(x, plan, 48000, y)
    torch.cuda.synchronize()
    times = []
    for _ in range(o.steps):
        t0 = time.perf_counter()
        loss = tr.step_pcm(x, plan, 48000, y)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out = {'config': 'train_nisqa_cnn_lstm_avg pool=%s bs=%d x 10 s' % (o.pool, o.bs), 'precision': tr.precision,
           'segments': int(plan.n_wins.sum()), 'steps_per_clip': int(plan.n_wins.max()),
           'ms_per_step_median': round(1e3 * float(np.median(times)), 3), 'ms_per_step_min': round(1e3 * min(times), 3),
           'clips_per_s': round(o.bs / float(np.median(times)), 1), 'loss': float(loss),
           'peak_mem_GB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    if not o.no_ref:
        from oracle import ref_shim
        if ref_shim.reference_available():
            with tempfile.TemporaryDirectory() as d:
                files = []
                for i, c in enumerate(clips):
                    files.append('c%03d.wav' % i)
                    synth.write_wav(os.path.join(d, files[-1]), c, 48000)
                r = ref_shim.reference_train_step(args, sd, d, files, y[:, 0], o.bs, lr=1e-3, steps=2)
            out['reference_cpu_s_per_step'] = round(float(r['seconds'][-1]), 3)
            out['reference_segments'] = int(r['segments'])
            out['speedup_vs_reference_cpu'] = round(float(r['seconds'][-1]) / float(np.median(times)), 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
