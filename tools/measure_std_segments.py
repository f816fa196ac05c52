"""The StandardCNN fed from the segment tensor against the frame-fed kernel, on the 256 mixed 3-30 s clips of `side.tts_mixed`
(bench.py side_tts: durations rng(7).uniform(3, 30), length-sorted batches of the predict loop's policy), quoted in DESIGN.md 4.6.
Both forms run on the same spectrograms in one process; feat20 of the two must be the same bits.

    python tools/measure_std_segments.py [precision ...]                 (default: bf16x6 f32; prints one JSON line, stage times
                                                                           from HIP events)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python tools/measure_std_segments.py
                                                                          (per-kernel durations: cnn_std_bf16x6_kernel against
                                                                           cnn_std_seg_bf16x6_kernel, cnn_std_front_kernel<false>
                                                                           against <true>)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from nisqa_amd import NISQA_lib as NL, synth
from nisqa_amd.engine import BatchPlan, HipNisqa

SR, REPS = 48000, 5
dev = torch.device('cuda:0')
precisions = sys.argv[1:] or ['bf16x6', 'f32']
args = dict(synth.TTS_ARGS)
sd = synth.random_state_dict(9, 'NISQA_TTS')
n_clips = 256
frames = (np.random.default_rng(7).uniform(3, 30, n_clips) * SR).astype(np.int64)
base = synth.synth_pcm16(5, 30.0)
res = {}
for prec in precisions:
    eng = HipNisqa(args, sd, dev, precision=prec)

    class _DS(object):
        ms_hop_length, seg_length, seg_hop_length = args['ms_hop_length'], args['ms_seg_length'], args['ms_seg_hop_length']
    cuts = NL.batch_policy(eng, _DS, range(n_clips), 1).cut(frames, np.full(n_clips, SR, np.int64), np.full(n_clips, 2, np.int64))
    ms = {'frame_fed': 0.0, 'segment_fed': 0.0}
    segs = x_bytes = 0
    for c in cuts:
        plan = eng.plan([int(frames[k]) for k in c], SR)
        pcm = torch.from_numpy(np.concatenate([base[:int(frames[k])] for k in c])).to(dev)
        mel, floor = eng.mel(pcm, plan, SR, clamp=False)
        # the segment tensor of the batch, gathered on the device from the floored spectrogram (SpeechQualityDataset.__getitem__'s gather)
        L = int(plan.n_wins.max())
        x = torch.zeros((plan.n_clips, L, 1, 48, 15), dtype=torch.float32, device=dev)
        win = torch.arange(15, device=dev)[None, :]
        for b in range(plan.n_clips):
            n = int(plan.n_wins[b])
            spec = torch.maximum(mel[int(plan.frame_off[b]):int(plan.frame_off[b + 1])], floor[b])
            x[b, :n, 0] = spec[eng.seg_hop * torch.arange(n, device=dev)[:, None] + win].permute(0, 2, 1)
        splan = BatchPlan.from_n_wins(plan.n_wins)
        valid = torch.from_numpy(plan.token_index()).to(dev)
        runs = {'frame_fed': lambda: eng.cnn_std(mel, floor, plan), 'segment_fed': lambda: eng.cnn_std_segments(x, splan)}
        feats = {}
        for name, run in runs.items():
            feats[name] = run()                                        # warm-up, and the result to compare
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(REPS + 1)]
            ev[0].record()
            for r in range(REPS):
                run()
                ev[r + 1].record()
            torch.cuda.synchronize()
            ms[name] += float(np.median([ev[r].elapsed_time(ev[r + 1]) for r in range(REPS)]))
        assert torch.equal(feats['frame_fed'][valid], feats['segment_fed'][valid]), 'segment-fed feat20 differs from frame-fed'
        segs += int(plan.n_wins.sum())
        x_bytes += int(plan.n_wins.sum()) * 2880
        del x, feats
    res[prec] = {'batches': len(cuts), 'segments': segs, 'segment_tensor_GB_read': round(x_bytes / 1e9, 3),
                 'frame_fed_ms_per_job': round(ms['frame_fed'], 3), 'segment_fed_ms_per_job': round(ms['segment_fed'], 3),
                 'ratio': round(ms['segment_fed'] / ms['frame_fed'], 4), 'same_bits': True}
print(json.dumps(res))
