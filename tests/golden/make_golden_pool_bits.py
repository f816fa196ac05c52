"""Generator of tests/golden/pool_bits.npz -- runs on an MI355X, against a library built from the commit whose bits are to be kept:

    NISQA_HIP_LIB=/path/to/that/libnisqa_hip.so PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pool_bits.py [out.npz]

Stored (uint32 views, valid rows only; inputs and weights are regenerated from seeds at test time, tests/pool_bits.py): the per-token
scores and values nisqa_pool_score_bf16 / nisqa_pool_score_bf16x6 leave in ws, the outputs of nisqa_pool_att_bf16 /
nisqa_pool_att_bf16x6, for one head and five, and the x rows of nisqa_td_selfatt_bf16.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import pool_bits as PB                            # noqa: E402
from nisqa_amd import lib as _lib                 # noqa: E402


def main():
    fix = {'provenance': np.array('nisqa_pool_score_*, nisqa_pool_att_* (bf16, bf16x6) and nisqa_td_selfatt_bf16 of the library '
                                  'built from the parent of the commit that merged td_bf16x6.hip into td_bf16.hip; gfx950')}
    for nh in sorted(PB.HEADS):
        fix.update(PB.run_pool(nh))
    fix.update(PB.run_td())
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, PB.FIXTURE)
    np.savez_compressed(out, **fix)
    print(_lib.LIB_PATH, '->', out, {k: v.shape for k, v in fix.items()})


if __name__ == '__main__':
    main()
