"""ISA checks of the shipped mel front end (no GPU needed): the real-input recombination pairs bins without lane shuffles,
and the instantiations the shipped 48 kHz front ends run (PCM16 and float input, both filter-bank forms) do not spill."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _kernels(prefix):
    """-> {symbol: [instruction lines]} of every gfx950 kernel in the built library whose name starts with prefix"""
    import isa_lint
    from nisqa_amd import lib
    objdump = os.path.join(isa_lint.LLVM, 'llvm-objdump')
    if not os.path.isfile(objdump):
        pytest.skip('llvm-objdump not on this machine')
    tmp = tempfile.mkdtemp(prefix='nq_mel_isa_')
    try:
        so = os.path.join(tmp, os.path.basename(lib.LIB_PATH))
        shutil.copyfile(lib.LIB_PATH, so)
        subprocess.run([objdump, '--offloading', so], cwd=tmp, check=True, capture_output=True)
        out, cur = {}, None
        for o in sorted(glob.glob(so + '.*gfx950*')):
            txt = subprocess.run([objdump, '-d', o], check=True, capture_output=True, text=True).stdout
            for line in txt.split('\n'):
                m = re.match(r'^[0-9a-f]+ <(\w+)>:', line)
                if m:
                    cur = m.group(1) if m.group(1).startswith(prefix) else None
                    if cur:
                        out.setdefault(cur, [])
                elif cur and line.strip():
                    out[cur].append(line.strip())
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_mel_recombination_has_no_lane_shuffle_and_shipped_instantiations_do_not_spill():
    ks = _kernels('_Z16mel_frame_kernel')
    assert len(ks) == 10, sorted(ks)
    for name, ins in ks.items():
        # the only ds_bpermute left is the per-clip wave maximum (one __shfl_xor per halving step, once per clip);
        # the recombination used to shuffle 56 values per frame
        n_bp = sum('ds_bpermute' in i for i in ins)
        assert n_bp <= 6, (name, n_bp)
    # <1, short, 1 | 2>: the shipped 48 kHz front ends on PCM16 input (bench.py, predict on WAV files)
    for tag in ('ILi1EsLi1E', 'ILi1EsLi2E', 'ILi1EfLi2E'):
        (name,) = [n for n in ks if tag in n]
        spills = [i for i in ks[name] if re.search(r'\bscratch_(load|store)', i)]
        assert not spills, (name, spills[:4])
