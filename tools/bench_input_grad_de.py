#!/usr/bin/env python3
"""d model(x, n_wins) / d x of NISQA_DE on one GPU: 32 pairs x 10 s = x [32, 247, 2, 48, 15], x and g resident
in HBM, hard and soft alignment in precisions f32 and bf16x6.  Per case: the plain forward under no_grad (the parent commit's call)
and forward + backward (y = model(x, n_wins); y.backward(g)), device events around each call, 3 warm-up and 20 timed calls of each
kind alternating in one process, median (min-max), and the peak allocated above what is resident before the calls.

    python tools/bench_input_grad_de.py [--pairs 32] [--segments 247] [--calls 20] [--json OUT]
    python tools/bench_input_grad_de.py --trace-case soft:f32 --calls 5      # one case only, for a kernel trace run on its own

Prints one JSON line.  No CPU fallback: without a GPU the engine raises."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def model_for(apply, precision, dev):
    import de_oracle as DO
    from nisqa_amd import NISQA_lib as NL
    from nisqa_amd.engine import HipNisqaDE
    args = DO.de_args('cosine', apply, 'x/y/-')                 # the shipped recipe's alignment and fusion
    m = NL.NISQA_DE(**DO.model_kwargs(args)).bind_args(args)
    m.load_state_dict(DO.random_de_state_dict(1, 'x/y/-'), strict=True)
    m.eval()
    m._engine = HipNisqaDE(args, m.state_dict(), dev, precision=precision)
    return m


def timed(fn, warmup, calls):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--segments', type=int, default=247)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--trace-case', default=None, metavar='APPLY:PRECISION')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev = 'cuda:0'
    rng = np.random.default_rng(0)
    x = torch.from_numpy((20 * rng.standard_normal((a.pairs, a.segments, 2, 48, 15)) - 40).astype(np.float32)).to(dev)
    n_wins = torch.full((a.pairs, 2), a.segments, dtype=torch.int64)
    g = torch.ones((a.pairs, 1), dtype=torch.float32, device=dev)
    cases = [tuple(a.trace_case.split(':'))] if a.trace_case else [(ap_, p) for ap_ in ('hard', 'soft') for p in ('f32', 'bf16x6')]
    out = {'pairs': a.pairs, 'segments': a.segments, 'calls': a.calls, 'cases': {}}
    for apply, precision in cases:
        m = model_for(apply, precision, dev)

        def fwd():
            with torch.no_grad():
                return m(x, n_wins)

        def fwd_bwd():
            xg = x.detach().requires_grad_(True)
            m(xg, n_wins).backward(g)
            return xg.grad

        fwd_bwd()                                               # builds the operator chain and packs the weight fragments
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        f_ms, b_ms = [], []
        for fn, ms in ((fwd, f_ms), (fwd_bwd, b_ms)):
            timed(fn, a.warmup, 0)
        for _ in range(a.calls):                                # alternating
            f_ms += timed(fwd, 0, 1)
            b_ms += timed(fwd_bwd, 0, 1)
        out['cases']['%s:%s' % (apply, precision)] = {'forward': stats(f_ms), 'forward_backward': stats(b_ms),
                                                     'peak_allocated_gb': (torch.cuda.max_memory_allocated() - base) / 1e9}
        del m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
