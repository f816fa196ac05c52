"""config/train_nisqa_double_ended.yaml forward + backward + Adam: 32 pairs of ten-second 48 kHz clips, HBM-resident, one GPU (mel
front end inside the step), in 'f32' and 'bf16x6'; then nisqa_de_align_fuse_bwd alone on the step's shapes next to its byte
roofline.  Side measurement quoted in DESIGN.md 4.8.1 (compare tools/bench_train.py at the same clip count); the driver's bench
contract is bench.py."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np, torch
from nisqa_amd import synth
from nisqa_amd.train import _ptr
from nisqa_amd.train_de import HipTrainerDE
import de_oracle as DO

bs = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
profile = len(sys.argv) > 3 and sys.argv[3] == 'profile'      # under a kernel trace: 'bf16x6' only, 4 + steps steps and nothing else
dev = torch.device('cuda:0')
args = DO.de_args()                                # cosine / hard / x/y/-, cnn_dropout 0.2, td_sa_dropout 0.1, td_2_sa_dropout 0.1
for precision in (('bf16x6',) if profile else ('f32', 'bf16x6')):
    tr = HipTrainerDE(args, DO.random_de_state_dict(8), dev, lr=1e-3, precision=precision)
    plan = tr.eng.plan([480000] * bs, 48000)
    side = lambda s0: (tr.eng.pcm16_to_f32(torch.from_numpy(np.concatenate([synth.synth_pcm16(s0 + i % 8, 10.0) for i in range(bs)])).to(dev)),
                       plan, 48000)
    deg, ref = side(0), side(8)
    y = np.random.default_rng(0).uniform(1, 5, (bs, 1)).astype(np.float32)
    for _ in range(3):
        tr.step_pcm(deg, ref, y)
    torch.cuda.synchronize()
    calls, ck = [0], tr._ck
    tr._ck = lambda rc, what: (calls.__setitem__(0, calls[0] + 1), ck(rc, what))[1]      # C entries of one step (most are one launch)
    tr.step_pcm(deg, ref, y)
    tr._ck = ck
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = tr.step_pcm(deg, ref, y)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    if profile:
        print(json.dumps({'precision': precision, 'steps_run': 4 + steps, 'ms_per_step': round(dt * 1e3, 2), 'c_entries_per_step': calls[0]}))
        break
    # the backward of alignment + fusion alone, on this step's tables
    Sx, Sy, F, B, tv = tr.Sx, tr.Sy, tr.fuse_width, tr.B, tr._tv
    dF, dx = torch.randn(Sx, F, device=dev), torch.empty(Sx + Sy, 64, device=dev)
    off, nw = tv['a_seg_off'], tv['n_wins']
    run = lambda: tr._ck(tr.lib.nisqa_de_align_fuse_bwd(_ptr(dF), F, _ptr(tr.last_idx), _ptr(off), _ptr(nw), _ptr(off, B), _ptr(nw, B), B,
                                                        int(max(tr.Lx.max(), tr.Ly.max())), tr.fuse, _ptr(dx), _ptr(dx), tr._st()), 'bwd')
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        run()
    e1.record()
    torch.cuda.synchronize()
    nbytes = Sx * F * 4 + (Sx + Sy) * 64 * 4
    print(json.dumps({'config': 'train_nisqa_double_ended bs=%d pairs x 10 s' % bs, 'precision': precision,
                      'segments_deg': Sx, 'segments_ref': Sy, 'ms_per_step': round(dt * 1e3, 2), 'pairs_per_s': round(bs / dt, 1),
                      'c_entries_per_step': calls[0], 'loss': float(loss),
                      'align_bwd_us': round(e0.elapsed_time(e1) / 50 * 1e3, 2), 'align_bwd_bytes': nbytes,
                      'align_bwd_roofline_us_at_8TBs': round(nbytes / 8e12 * 1e6, 3),
                      'peak_mem_GB': round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}))
    del tr
