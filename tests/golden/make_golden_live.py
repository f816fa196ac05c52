"""Stored outputs of the reference's own code for the live-reference tests (tests/golden/live_reference.npz).

Those tests run the reference live where ``__graft_entry__.build()`` staged it under oracle/_ref; everywhere else they
compare against what this script recorded from the same code on the same seeded inputs:
  eval_*      eval_results (NISQA_lib.py) of synth.eval_corpus(23, n_db=4, n_con=9, per_con=5), per-file block
  net_live    the reference modules (random NISQA_DIM weights, seed 11) on a seeded random spectrogram
  loop_*      the reference's predict loop through the functional librosa stand-in (random nisqa.tar architecture)
  gpu_*       the same loop on the six clips of the -m gpu live-loop test, fixed seed, each checkpoint's architecture

Run where the reference is staged:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_live.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import helpers                                                 # noqa: E402
from oracle import ref_shim                                    # noqa: E402
from nisqa_amd import synth                                    # noqa: E402

EVAL_MAPPINGS = [None, 'first_order', 'second_order']
GPU_SEEDS = {'nisqa.tar': 20261015, 'nisqa_mos_only.tar': 20261016, 'nisqa_tts.tar': 20261017}


def main():
    assert ref_shim.reference_available(), 'needs the reference (staged under oracle/_ref by build())'
    out = {'provenance': np.array('reference NISQA_lib.py via oracle.ref_shim, CPU fp32; random weights: '
                                  'tests/helpers.py random_checkpoint')}
    RL = ref_shim.import_reference_lib()
    for mapping in EVAL_MAPPINGS:
        df, _ = synth.eval_corpus(23, n_db=4, n_con=9, per_con=5)
        want, ow = RL.eval_results(df, dcon=None, mapping=mapping)
        pre = 'eval_%s_' % mapping
        out.update(helpers.eval_frame_to_arrays(pre, want))
        out[pre + 'overall_keys'] = np.array(list(ow))
        out[pre + 'overall'] = np.array(list(ow.values()), dtype=np.float64)

    args, sd = dict(helpers.DIM_ARGS), helpers.random_state_dict(11, 'NISQA_DIM')
    model, NL = ref_shim.build_reference_model(args, sd)
    spec = (np.random.default_rng(3).standard_normal((48, 123)) * 20 - 40).astype(np.float32)
    x, n = NL.segment_specs('t', spec, 15, 4, 1300)
    with torch.no_grad():
        out['net_live'] = model(x.unsqueeze(0), torch.tensor([int(n)])).numpy()[0]

    with tempfile.TemporaryDirectory() as d:
        path = helpers.random_checkpoint('nisqa.tar', d)
        helpers.functional_loop_clips(d)
        out['loop_y'] = ref_shim.reference_predict(path, d, ['a.wav', 'b_stereo.wav'], bs=2)
        out['loop_y1'] = ref_shim.reference_predict(path, d, ['b_stereo.wav'], bs=1, ms_channel=1)
    for ckpt, seed in GPU_SEEDS.items():
        with tempfile.TemporaryDirectory() as d:
            path = helpers.random_checkpoint(ckpt, d)
            names = helpers.live_loop_clips(seed, d)
            tag = 'gpu_' + ckpt.replace('.tar', '')
            out[tag + '_seed'] = np.array(seed)
            out[tag + '_ref'] = ref_shim.reference_predict(path, d, names, bs=4)
            print(ckpt, out[tag + '_ref'])
    np.savez_compressed(os.path.join(HERE, helpers.LIVE_FIXTURE), **out)


if __name__ == '__main__':
    main()
