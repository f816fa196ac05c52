"""The two-term and three-term pooling entries and the two-term self-attention give the bits they gave before their chain helpers and
the pool-score kernel were merged into one source over the number of terms (csrc/td_bf16.hip): tests/golden/pool_bits.npz was
written from a build of the parent commit (tests/golden/make_golden_pool_bits.py); inputs, plan and weights: tests/pool_bits.py.
Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import helpers
import pool_bits as PB

pytestmark = pytest.mark.gpu


def _same(got, gold):
    for k, v in sorted(got.items()):
        assert v.dtype == np.uint32 and v.shape == gold[k].shape, (k, v.shape, gold[k].shape)
        bad = np.argwhere(v != gold[k])
        assert len(bad) == 0, (k, len(bad), 'differing words, first at', bad[0])


@pytest.mark.parametrize('n_heads', sorted(PB.HEADS))
def test_pool_score_and_pool_att_entries_keep_their_bits(n_heads):
    got = PB.run_pool(n_heads)
    assert sorted(got) == sorted('%s_%s_h%d' % (w, f, n_heads) for w in ('sc', 'yv', 'out') for f in PB.FORMATS)
    _same(got, helpers.golden(PB.FIXTURE))


def test_two_term_self_attention_keeps_its_bits():
    _same(PB.run_td(), helpers.golden(PB.FIXTURE))
