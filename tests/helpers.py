"""Shared test helpers: checkpoint lookup, seeded random state dicts, fixture loading."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import sys
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

from nisqa_amd.synth import DIM_ARGS, MOS_ARGS, TTS_ARGS, random_state_dict  # noqa: E402,F401


def find_weights(name='nisqa.tar'):
    """Real checkpoint if one is staged in this tree, else None.

    ``__graft_entry__.build()`` stages the published checkpoints under oracle/_ref/weights/ (git-ignored) where the
    reference tree is present; $NISQA_WEIGHTS_DIR points elsewhere explicitly.
    """
    cands = [os.environ.get('NISQA_WEIGHTS_DIR', ''), os.path.join(ROOT, 'oracle', '_ref', 'weights')]
    for d in cands:
        p = os.path.join(d, name) if d else ''
        if p and os.path.isfile(p):
            return p
    return None


def load_checkpoint(path):
    ck = torch.load(path, map_location='cpu')
    return ck['args'], ck['model_state_dict']


def golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# ---- stored outputs of the reference (tests/golden/live_reference.npz, tests/golden/make_golden_live.py) ----------------------
# The live-reference tests run the reference's own code where build() staged it (oracle/_ref); elsewhere they compare against
# what that code computed on the same seeded inputs, with seeded random weights of each checkpoint's architecture.
LIVE_FIXTURE = 'live_reference.npz'
RANDOM_CHECKPOINTS = {'nisqa.tar': (DIM_ARGS, 'NISQA_DIM', 7), 'nisqa_mos_only.tar': (MOS_ARGS, 'NISQA', 8),
                      'nisqa_tts.tar': (TTS_ARGS, 'NISQA_TTS', 9)}


def random_checkpoint(name, dst_dir):
    """A checkpoint file with seeded random weights of the architecture of the published ``name`` -> its path."""
    args, model, seed = RANDOM_CHECKPOINTS[name]
    args = dict(args)
    args.update({'pretrained_model': False, 'tr_bs_val': 1, 'tr_num_workers': 0})
    path = os.path.join(str(dst_dir), 'rand_' + name)
    torch.save({'args': args, 'model_state_dict': random_state_dict(seed, model)}, path)
    return path


def live_loop_clips(seed, d):
    """The six WAV files of the live-reference loop test (0.5 .. 9 s, one stereo) drawn from ``seed`` into d -> names."""
    from nisqa_amd import synth
    rng = np.random.default_rng(seed)
    names = []
    for i in range(6):
        dur = float(rng.uniform(0.5, 9.0))
        pcm = synth.synth_pcm16(int(rng.integers(1 << 30)), dur)
        if i == 4:                                               # one stereo file: lb.load averages the channels
            pcm = np.stack([pcm, synth.synth_pcm16(int(rng.integers(1 << 30)), dur)], 1)
        synth.write_wav(os.path.join(str(d), 'f%d.wav' % i), pcm, 48000)
        names.append('f%d.wav' % i)
    return names


def functional_loop_clips(d):
    """The files of the functional-librosa loop test: a.wav (mono, 1.6 s), b_stereo.wav (1.1 s) -> the stereo PCM."""
    from nisqa_amd import synth
    st = np.stack([synth.synth_pcm16(61, 1.1), synth.synth_pcm16(62, 1.1)], 1)
    synth.write_wav(os.path.join(str(d), 'a.wav'), synth.synth_pcm16(60, 1.6), 48000)
    synth.write_wav(os.path.join(str(d), 'b_stereo.wav'), st, 48000)
    return st


def tok_offsets(n_wins, gran=64, slack=0):
    """tok_off of ``n_wins`` with every clip padded to a multiple of ``gran`` tokens, plus ``slack`` extra rows for every
    other clip (clips 1, 3, 5, ...)."""
    n = np.asarray(n_wins, np.int64).reshape(-1)
    pad = -(-n // gran) * gran + slack * (np.arange(len(n)) % 2)
    return np.concatenate([[0], np.cumsum(pad)]).astype(np.int32)


def plan_with_layout(n_wins, tok_off, frame_off=None):
    """A BatchPlan over ``n_wins`` with a caller-chosen token layout (and frame layout, for the CNN entries that read mel_tm)."""
    from nisqa_amd.engine import BatchPlan
    plan = BatchPlan.from_n_wins(n_wins)
    plan.tok_off = np.asarray(tok_off, np.int32)
    plan.total_tok = int(plan.tok_off[-1])
    assert len(plan.tok_off) == plan.n_clips + 1 and (np.diff(plan.tok_off) >= plan.n_wins).all()
    if frame_off is not None:
        plan.frame_off = np.asarray(frame_off, np.int32)
        plan.total_frames = int(plan.frame_off[-1])
    return plan


def eval_frame_to_arrays(prefix, df):
    """A results frame of eval_results as plain arrays (no pickles) under ``prefix``."""
    out = {prefix + 'columns': np.array(list(df.columns)), prefix + 'index': df.index.to_numpy()}
    for i, c in enumerate(df.columns):
        col = df[c]
        out['%scol%d' % (prefix, i)] = col.to_numpy().astype(str) if col.dtype == object else col.to_numpy()
    return out


def eval_frame_from_arrays(prefix, g):
    import pandas as pd
    cols = [str(c) for c in g[prefix + 'columns']]
    data = {}
    for i, c in enumerate(cols):
        a = g['%scol%d' % (prefix, i)]
        data[c] = a.astype(object) if a.dtype.kind == 'U' else a
    return pd.DataFrame(data, index=g[prefix + 'index'], columns=cols)
