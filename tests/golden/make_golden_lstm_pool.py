"""Golden-vector generator of the CNN-LSTM-AVG / CNN-LSTM-MAX fixtures -- runs ONLY where the reference tree is present.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lstm_pool.py

Writes tests/golden/net_lstm_{avg,max}_rand.npz:
* network : the REFERENCE'S OWN torch modules (NISQA with cnn_model=standard, td=lstm, pool=avg | max; segment_specs), imported
            through oracle.ref_shim, run on CPU fp32 in ONE padded batch as predict_mos does (NL:1420-1467);
* weights : nisqa_amd.synth.random_state_dict(lstm_pool_oracle.SEED, 'NISQA_TTS') (the key set of the recipe's checkpoints);
* input   : oracle.mel spectrograms (fmax 20000) of the seeded clips of lstm_pool_oracle.CLIPS: one segment, ragged lengths,
            10 s and one clip at the 1300-segment cap (segment hop 3).
Stored: n_wins, feat20 of lstm_pool_oracle.STAGE_CLIPS, the pooled vectors (the input of the pooling's linear layer, captured with a
forward hook) and out.  A CRC of each PCM clip is stored; the clips are regenerated from seeds at test time.
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import ref_shim                       # noqa: E402
import lstm_pool_oracle as LO                     # noqa: E402


def main():
    assert ref_shim.reference_available(), 'needs the reference tree'
    pcm = [LO.clip_pcm(i) for i in range(len(LO.CLIPS))]
    sd = LO.state_dict()
    for pool, args in sorted(LO.POOL_ARGS.items()):
        specs = [LO.clip_spec(p, args) for p in pcm]
        model, NL = ref_shim.build_reference_model(args, sd)
        xs, nw = [], []
        for s in specs:
            x, n = NL.segment_specs('golden', s, args['ms_seg_length'], args['ms_seg_hop_length'], args['ms_max_segments'])
            xs.append(x)
            nw.append(int(n))
        pooled = []
        hook = model.pool.model.linear.register_forward_hook(lambda mod, inp, out: pooled.append(inp[0].detach().clone()))
        with torch.no_grad():
            out = model(torch.stack(xs, 0), torch.tensor(nw)).numpy()
            stages = {}
            for i in LO.STAGE_CLIPS:
                stages['feat_%d' % i] = model.cnn.model(xs[i][:nw[i]]).numpy()
        hook.remove()
        fix = {
            'provenance': np.array('network: reference torch modules (StandardCNN, LSTM, Pool%s) via oracle.ref_shim, CPU fp32, one '
                                   'padded batch; input mel: oracle.mel restatement, fmax 20000, segment hop 3; weights: '
                                   'synth.random_state_dict(%d, NISQA_TTS)' % (pool.capitalize(), LO.SEED)),
            'clip_seed': np.array([c[0] for c in LO.CLIPS]),
            'clip_samples': np.array([c[1] for c in LO.CLIPS], dtype=np.int64),
            'pcm_crc32': np.array([zlib.crc32(p.tobytes()) for p in pcm], dtype=np.uint64),
            'stage_clips': np.array(LO.STAGE_CLIPS),
            'n_wins': np.array(nw),
            'pooled': pooled[0].numpy(),
            'out': out.astype(np.float32),
        }
        fix.update(stages)
        np.savez_compressed(os.path.join(HERE, 'net_lstm_%s_rand.npz' % pool), **fix)
        print(pool, nw, '\n', out.reshape(-1))


if __name__ == '__main__':
    main()
