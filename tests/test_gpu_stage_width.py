"""Every inference stage against float64, one stage at a time, at ragged token edges (run with -m gpu on an MI355X).

Stage width.  The GPU kernel and the CPU oracle (oracle/net.py, tests/de_oracle.py) get the SAME fp32 input; both are measured
against a float64 evaluation of that one stage, so errors of upstream stages never compound.  fp32 arithmetic's own distance from
float64 is measured twice, by two summation orders: CPU torch float32 (``cpu``) and the exact-fp32 MFMA kernels ('f32').  As in
tests/test_gpu_parity.py::test_rounding_error_of_the_precision_modes_against_float64, ``floor`` is the larger of the two over the
whole batch, and the three-term and f16 modes ('bf16x6', 'f16x4', 'f16x3') must stay, clip by clip, within FACTOR x floor plus
one fp32 ulp of that clip's largest output.  The exact-fp32 kernels themselves are held to F32_FACTOR x cpu (see there).  Where
'bf16x3' (16 operand bits) runs kernels of its own, it is the negative control: its error must be more than CONTROL times that of
'bf16x6', or the bound could not tell the two operand widths apart.  Stages that run the same kernel in several modes (the
BiLSTM in all five; self-attention and pooling in 'f16x4' / 'f16x3', which dispatch to the 'bf16x6' kernels) must give the same
bits in all of them.

Layout contract (include/nisqa_hip.h).  The exact-fp32 and two-term entries on 32-padded token layouts, with and without slack
rows, every entry on 64-padded layouts with slack, and every clip run alone must give the bits of the 64-padded batch; NaN or
+-3e38 in the padding rows of an input must not change a valid output bit; the CNN entries must leave the padding rows of
``feat`` as they found them; forward_pcm must not read its workspace before writing it.

Token counts sit on every 16 / 32-row tile, 64-token workgroup and 32-key block boundary of the kernels, three of the ring of
key blocks of csrc/td16_bf16x6.hip wrap around (> 96 keys), and 1 300 is the reference's ms_max_segments.  The second batch has
more 64-token workgroups than the device has CUs.
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import de_oracle as DO
from nisqa_amd import synth
from oracle import net as onet

pytestmark = pytest.mark.gpu

RAGGED = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1299, 1300]
CREDITABLE = ('f32', 'bf16x6', 'f16x4', 'f16x3')
ALL_MODES = CREDITABLE + ('bf16x3',)
FACTOR = 1.5            # tests/test_gpu_parity.py::test_rounding_error_of_the_precision_modes_against_float64
# The exact-fp32 kernels sum long dot products in one sequential FMA chain per output (P V over up to 1 300 keys, the BiLSTM's
# 148-term gates) where CPU torch sums in blocks, and the max over a batch of such errors moves with the order.  Measured on an
# MI355X against cpu alone: up to 2.75 x on the 1 300-token self-attention, 1.84 x on the BiLSTM sequence, 1.6 x on both CNNs;
# 'bf16x3' sits 14 - 83 x above cpu on the CNNs and 22 - 28 x on the self-attention.
F32_FACTOR = 3.0
CONTROL = 2.0           # 'bf16x3' must be more than this much further from float64 than 'bf16x6'
HEAD = 64               # rows of NaN behind every input buffer: a read past total_tok_padded shows up in the outputs
SENTINEL = 0x5EADBEEF   # bit pattern pre-filled into the CNN outputs (a finite float, 6.2e18)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check(rc, what):
    assert rc == 0, (what, rc)


def _sd(sd, dtype):
    return {k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(dtype)
            for k, v in sd.items() if k.split('.')[-1] != 'num_batches_tracked'}


# -- weights and engines -------------------------------------------------------------------------------------------------------
def _sets(kind):
    """(tag, args, state_dict): seeded random weights, and the published checkpoint of the architecture where one is staged."""
    if kind == 'cnn':
        cands = [('dim_rand', helpers.DIM_ARGS, ('NISQA_DIM', 7), 'nisqa.tar')]
    elif kind == 'sa':
        cands = [('dim_rand', helpers.DIM_ARGS, ('NISQA_DIM', 7), 'nisqa.tar'),
                 ('mos_rand', helpers.MOS_ARGS, ('NISQA', 8), 'nisqa_mos_only.tar')]
    else:
        cands = [('tts_rand', helpers.TTS_ARGS, ('NISQA_TTS', 9), 'nisqa_tts.tar')]
    out = []
    for tag, args, (model, seed), ckpt in cands:
        out.append((tag, dict(args), helpers.random_state_dict(seed, model)))
        path = helpers.find_weights(ckpt)
        if path is not None:
            a, sd = helpers.load_checkpoint(path)
            out.append((tag.replace('rand', 'real'), a, sd))
    return out


_ENG = {}


def _engine(tag, args, sd, precision):
    from nisqa_amd.engine import HipNisqa
    if (tag, precision) not in _ENG:
        _ENG[(tag, precision)] = HipNisqa(args, sd, 'cuda:0', precision=precision)
    return _ENG[(tag, precision)]


def _plan(n_wins):
    from nisqa_amd.engine import BatchPlan
    return BatchPlan.from_n_wins(np.asarray(n_wins, np.int64))


def _wide_counts():
    """Ragged clips of 1 .. 400 tokens with more 64-token workgroups in all than the device has CUs."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(11)
    n = [1, 64, 65, 97, 129]
    while sum(-(-k // 64) for k in n) <= int(1.25 * n_cu):
        n.append(int(rng.integers(1, 401)))
    return n


# -- direct calls of the C ABI: (engine, input laid out by plan) -> output rows in that layout -----------------------------
def _upload_rows(rows, plan, fill=0.0, width=None):
    """rows: the valid rows of each clip (list of [n_b, w] arrays) -> device [NP + HEAD, width] float32 in plan's layout;
    padding rows hold ``fill`` (0, nan, or 'big': +-3e38 alternating), the HEAD rows behind NP hold NaN."""
    w = width or rows[0].shape[1]
    a = np.empty((plan.total_tok + HEAD, w), np.float32)
    if fill == 'big':
        a[...] = np.where((np.arange(a.size).reshape(a.shape) % 2) == 0, 3e38, -3e38)
    else:
        a[...] = fill
    a[plan.total_tok:] = np.nan
    for b, r in enumerate(rows):
        t0 = int(plan.tok_off[b])
        a[t0:t0 + len(r)] = 0.0
        a[t0:t0 + len(r), :r.shape[1]] = r
    return torch.from_numpy(a).to('cuda:0')


def _valid(t, plan):
    """device rows in plan's layout -> list of the clips' valid rows (host)."""
    h = t.cpu().numpy()
    return [h[int(plan.tok_off[b]):int(plan.tok_off[b]) + int(plan.n_wins[b])] for b in range(plan.n_clips)]


def _padding_rows(plan):
    return np.concatenate([np.arange(int(plan.tok_off[b]) + int(plan.n_wins[b]), int(plan.tok_off[b + 1]))
                           for b in range(plan.n_clips)]).astype(np.int64)


def run_td(eng, feat, plan):
    d = plan.to(eng.device)
    np_ = plan.total_tok
    ws = torch.full((np_ * 64 * 9 + HEAD,), float('nan'), device=eng.device)
    x = torch.zeros((np_ + HEAD, 64), device=eng.device)
    a = (_p(feat), _p(d['tok_off']), _p(d['n_wins']), plan.n_clips, np_, eng.n_layers, _p(eng.td_w))
    if eng.td_precision == 'f32':
        _check(eng.lib.nisqa_td_selfatt(*a, _p(ws), _p(x), eng._stream()), 'nisqa_td_selfatt')
    else:
        fn = eng.lib.nisqa_td_selfatt_bf16 if eng.td_precision == 'bf16x3' else eng.lib.nisqa_td_selfatt_bf16x6
        _check(fn(*a, _p(eng.td_wb), _p(ws), _p(x), eng._stream()), 'nisqa_td_selfatt_' + eng.td_precision)
    return x


def run_pool(eng, x, plan, want_scores=False):
    """-> out [B, n_heads] (and with want_scores the per-token scores [NP, 8] the first pass leaves in ws)"""
    d = plan.to(eng.device)
    np_ = plan.total_tok
    ws = torch.full((np_ * 16 + plan.n_clips + HEAD,), float('nan'), device=eng.device)
    out = torch.empty((plan.n_clips, eng.n_heads), device=eng.device)
    a = (_p(x), _p(d['tok_off']), _p(d['n_wins']), plan.n_clips, np_, eng.n_heads, _p(eng.pool_w))
    if eng.td_precision == 'f32':
        _check(eng.lib.nisqa_pool_att(*a, _p(ws), _p(out), eng._stream()), 'nisqa_pool_att')
    else:
        fn = eng.lib.nisqa_pool_att_bf16 if eng.td_precision == 'bf16x3' else eng.lib.nisqa_pool_att_bf16x6
        _check(fn(*a, _p(eng.pool_wb), _p(ws), _p(out), eng._stream()), 'nisqa_pool_att_' + eng.td_precision)
    return (out, ws[:np_ * 8].view(np_, 8)) if want_scores else out


def run_td_pool(eng, feat, plan):
    assert eng.td_precision == 'bf16x6'
    d = plan.to(eng.device)
    np_ = plan.total_tok
    ws = torch.full((np_ * 64 * 9 + HEAD,), float('nan'), device=eng.device)
    wsp = torch.full((np_ * 16 + plan.n_clips + HEAD,), float('nan'), device=eng.device)
    x = torch.zeros((np_ + HEAD, 64), device=eng.device)
    out = torch.empty((plan.n_clips, eng.n_heads), device=eng.device)
    _check(eng.lib.nisqa_td_pool_bf16x6(_p(feat), _p(d['tok_off']), _p(d['n_wins']), plan.n_clips, np_, eng.n_layers, _p(eng.td_w),
                                        _p(eng.td_wb), eng.n_heads, _p(eng.pool_wb), _p(ws), _p(x), _p(wsp), _p(out), eng._stream()),
           'nisqa_td_pool_bf16x6')
    return out


def run_lstm(eng, feat20, plan):
    d = plan.to(eng.device)
    hfin = torch.full((plan.n_clips, 256), float('nan'), device=eng.device)
    seq = torch.zeros((plan.total_tok + HEAD, 256), device=eng.device)
    out = torch.empty((plan.n_clips, 1), device=eng.device)
    _check(eng.lib.nisqa_lstm_laststep(_p(feat20), _p(d['tok_off']), _p(d['n_wins']), plan.n_clips, _p(eng.td_w), _p(hfin), _p(seq),
                                       _p(out), eng._stream()), 'nisqa_lstm_laststep')
    return out, seq


def _sentinel_feat(plan, width, dev):
    return torch.full((plan.total_tok + HEAD, width), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def run_cnn_mel(eng, mel, floor, plan):
    """the AdaptCNN (arch 0) or StandardCNN + fc_out (arch 1) entry of eng's precision on mel_tm laid out by plan.frame_off"""
    d = plan.to(eng.device)
    np_ = plan.total_tok
    feat = _sentinel_feat(plan, 20 if eng.arch == 1 else 384, eng.device)
    a = (_p(mel), _p(d['frame_off']), _p(d['tok_off']), _p(d['n_wins']), _p(floor), plan.n_clips, np_, eng.seg_hop, _p(eng.cnn_w))
    st, L = eng._stream(), eng.lib
    std = eng.arch == 1
    if eng.precision == 'f32':
        p3 = torch.full((np_ + HEAD, 12 if std else 18, 64), float('nan'), device=eng.device)
        fn, name = (L.nisqa_cnn_standard, 'nisqa_cnn_standard') if std else (L.nisqa_cnn_adapt, 'nisqa_cnn_adapt')
        _check(fn(*a, _p(p3), _p(feat), st), name)
    elif eng.precision == 'bf16x3':
        if std:
            _check(L.nisqa_cnn_standard_bf16(*a, _p(eng.cnn_wb), _p(feat), st), 'nisqa_cnn_standard_bf16')
        else:
            _check(L.nisqa_cnn_adapt_bf16(*a, _p(eng.cnn_wb), None, _p(feat), st), 'nisqa_cnn_adapt_bf16')
    elif eng.precision == 'bf16x6':
        fn = L.nisqa_cnn_standard_bf16x6 if std else L.nisqa_cnn_adapt_bf16x6
        _check(fn(*a, _p(eng.cnn_wb), _p(feat), st), 'cnn_bf16x6')
    else:
        fn = L.nisqa_cnn_standard_f16 if std else L.nisqa_cnn_adapt_f16
        _check(fn(*a, _p(eng.cnn_wb), int(eng.precision[-1]), _p(feat), st), 'cnn_f16')
    return feat


def run_cnn_seg(eng, x, plan):
    """the AdaptCNN segment-tensor entry of eng's precision: x [B, L, 1, 48, 15] (device)"""
    d = plan.to(eng.device)
    np_ = plan.total_tok
    feat = _sentinel_feat(plan, 384, eng.device)
    a = (_p(x), x.shape[1], _p(d['tok_off']), _p(d['n_wins']), plan.n_clips, np_, _p(eng.cnn_w))
    st, L = eng._stream(), eng.lib
    if eng.precision == 'f32':
        p3 = torch.full((np_ + HEAD, 18, 64), float('nan'), device=eng.device)
        _check(L.nisqa_cnn_adapt_segments(*a, _p(p3), _p(feat), st), 'nisqa_cnn_adapt_segments')
    elif eng.precision in ('bf16x3', 'bf16x6'):
        fn = L.nisqa_cnn_adapt_segments_bf16 if eng.precision == 'bf16x3' else L.nisqa_cnn_adapt_segments_bf16x6
        _check(fn(*a, _p(eng.cnn_wb), _p(feat), st), 'nisqa_cnn_adapt_segments_' + eng.precision)
    else:
        _check(L.nisqa_cnn_adapt_segments_f16(*a, _p(eng.cnn_wb), int(eng.precision[-1]), _p(feat), st), 'nisqa_cnn_adapt_segments_f16')
    return feat


# -- inputs ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _mel_batch(arch):
    """GPU mel (clamped; the kernel is the same in every mode) of synthetic clips with exactly RAGGED segments each ->
    (mel_tm device, clip_floor device, frame_off, the clips' [48, T] host spectrograms).  The CNN entries apply the floor
    again on load: a no-op on a clamped spectrogram, so the oracle sees the same input."""
    def make():
        tag, args, sd = _sets('tts' if arch == 1 else 'cnn')[0]
        eng = _engine(tag, args, sd, 'f32')
        hop = eng.seg_hop
        T = [14 + 1 + hop * (n - 1) for n in RAGGED]
        pcm = [synth.synth_pcm16(500 + i, (t - 1) * 480 / 48000.0 + 0.1)[:(t - 1) * 480] for i, t in enumerate(T)]
        plan = eng.plan([len(p) for p in pcm], 48000)
        assert list(plan.n_wins) == RAGGED and list(np.diff(plan.frame_off)) == T
        mel, floor = eng.mel(torch.from_numpy(np.concatenate(pcm)).to(eng.device), plan, 48000, clamp=True)
        h = mel.cpu().numpy()
        specs = [h[plan.frame_off[b]:plan.frame_off[b + 1]].T for b in range(plan.n_clips)]
        return mel, floor, plan.frame_off.copy(), specs
    return _cached(('mel', arch), make)


def _segments(arch):
    """host segment stacks of the RAGGED clips, [n_b, 1, 48, 15] each"""
    def make():
        hop = 1 if arch == 1 else 4
        return [onet.segment_specs(s, 15, hop)[0].numpy() for s in _mel_batch(arch)[3]]
    return _cached(('seg', arch), make)


def _cnn_rows(tag, args, sd, arch):
    """rows of real CNN features: the exact-fp32 CNN of this weight set on three synthetic clips"""
    def make():
        eng = _engine(tag, args, sd, 'f32')
        pcm = [synth.synth_pcm16(900 + i, 4.0 + 2 * i) for i in range(3)]
        plan = eng.plan([len(p) for p in pcm], 48000)
        mel, floor = eng.mel(torch.from_numpy(np.concatenate(pcm)).to(eng.device), plan, 48000, clamp=False)
        feat = eng.cnn_std(mel, floor, plan) if arch == 1 else eng.cnn(mel, floor, plan)[0]
        return feat.cpu().numpy()[plan.token_index()]
    return _cached(('rows', tag), make)


def _sample(rows, counts, seed):
    rng = np.random.default_rng(seed)
    return [rows[rng.integers(0, len(rows), n)] for n in counts]


# -- the float64 yardstick ------------------------------------------------------------------------------------------------------
def _oracle_cnn(sd, segs, arch, dtype):
    s = _sd(sd, dtype)
    x = torch.from_numpy(np.concatenate(segs)).to(dtype)
    with torch.no_grad():
        f = [onet.standard_cnn(s, c) if arch == 1 else onet.adapt_cnn(s, c) for c in torch.split(x, 1024)]
    f = torch.cat(f).numpy()
    cut = np.cumsum([0] + [len(g) for g in segs])
    return [f[cut[b]:cut[b + 1]] for b in range(len(segs))]


def _oracle_sa(sd, feats, n_layers, dtype, heads=None, pfx='time_dependency.model.'):
    """per clip: the self-attention output [n, 64], and, with ``heads``, the pooled outputs [len(heads)]"""
    s = _sd(sd, dtype)
    td, out = [], []
    with torch.no_grad():
        for f in feats:
            x = onet.self_attention(s, torch.from_numpy(f).to(dtype), n_layers, pfx=pfx)
            td.append(x.numpy())
            if heads is not None:
                out.append(torch.cat([onet.pool_att_ff(s, x, h) for h in heads]).numpy())
    return td, out


def _oracle_pool(sd, xs, heads, dtype):
    s = _sd(sd, dtype)
    with torch.no_grad():
        return [torch.cat([onet.pool_att_ff(s, torch.from_numpy(x).to(dtype), h) for h in heads]).numpy() for x in xs]


def _oracle_scores(sd, xs, heads, dtype):
    """PoolAttFF's attention logits linear2(relu(linear1 x)) (NL:1176-1177), per clip [n, heads]"""
    s = _sd(sd, dtype)
    with torch.no_grad():
        out = []
        for x in xs:
            x = torch.from_numpy(x).to(dtype)
            out.append(torch.cat([torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(
                x, s[h + 'linear1.weight'], s[h + 'linear1.bias'])), s[h + 'linear2.weight'], s[h + 'linear2.bias'])
                for h in heads], 1).numpy())
        return out


def _oracle_lstm(sd, feats, dtype):
    s = _sd(sd, dtype)
    seq, out = [], []
    with torch.no_grad():
        for f in feats:
            y = onet.bilstm(s, torch.from_numpy(f).to(dtype))
            seq.append(y.numpy())
            out.append(onet.pool_last_step_bi(s, y).numpy())
    return seq, out


def _heads(args):
    return ['pool_layers.%d.model.' % h for h in range(5)] if args['model'] == 'NISQA_DIM' else ['pool.model.']


# -- the bound ------------------------------------------------------------------------------------------------------------------
def _per_clip(got, ref):
    return np.array([float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(got, ref)])


def judge(stage, counts, got, ref64, ref32):
    """got: mode -> per-clip outputs; ref64 / ref32: per-clip float64 / CPU-float32 outputs.  Prints one line, then asserts the
    per-clip bound for the creditable modes and, where 'bf16x3' was run, the negative control."""
    cpu = float(_per_clip(ref32, ref64).max())
    ulp = np.array([float(np.spacing(np.float32(np.abs(r).max()))) for r in ref64])
    err = {m: _per_clip(g, ref64) for m, g in got.items()}
    floor = max(cpu, float(err['f32'].max())) if 'f32' in err else cpu
    cells = []
    for m, e in err.items():
        w = int(np.argmax(e))
        cells.append('%s %.3g (x%.2f, worst n=%d)' % (m, e.max(), e.max() / floor, counts[w]))
    print('%-48s cpu %.3g floor %.3g | %s' % (stage, cpu, floor, ' | '.join(cells)))
    for m, e in err.items():
        if m in CREDITABLE:
            bound = (F32_FACTOR * cpu if m == 'f32' else FACTOR * floor) + ulp
            bad = np.nonzero(e > bound)[0]
            assert len(bad) == 0, (stage, m, 'clips with n =', [counts[b] for b in bad], e[bad], 'cpu', cpu, 'floor', floor)
    if 'bf16x3' in err and 'bf16x6' in err:
        assert err['bf16x3'].max() > CONTROL * err['bf16x6'].max(), (stage, err['bf16x3'].max(), err['bf16x6'].max())
    return err


def _same_bits(stage, a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (stage, 'clip', k)


# =============================================================================================================================
# 1. stage width
# =============================================================================================================================
def test_adapt_cnn_from_mel_and_from_segment_tensors_against_float64():
    mel, floor, frame_off, _ = _mel_batch(0)
    segs = _segments(0)
    plan = helpers.plan_with_layout(RAGGED, helpers.tok_offsets(RAGGED), frame_off)
    L = max(RAGGED)
    x = np.zeros((len(RAGGED), L, 1, 48, 15), np.float32)
    for b, s in enumerate(segs):
        x[b, :len(s)] = s
    xd = torch.from_numpy(x).to('cuda:0')
    for tag, args, sd in _sets('cnn'):
        ref64, ref32 = _oracle_cnn(sd, segs, 0, torch.float64), _oracle_cnn(sd, segs, 0, torch.float32)
        got_mel, got_seg = {}, {}
        for m in ALL_MODES:
            eng = _engine(tag, args, sd, m)
            got_mel[m] = _valid(run_cnn_mel(eng, mel, floor, plan), plan)
            got_seg[m] = _valid(run_cnn_seg(eng, xd, plan), plan)
        judge('AdaptCNN from mel [%s]' % tag, RAGGED, got_mel, ref64, ref32)
        judge('AdaptCNN from segment tensors [%s]' % tag, RAGGED, got_seg, ref64, ref32)


def test_standard_cnn_with_fc_out_against_float64():
    mel, floor, frame_off, _ = _mel_batch(1)
    segs = _segments(1)
    plan = helpers.plan_with_layout(RAGGED, helpers.tok_offsets(RAGGED), frame_off)
    for tag, args, sd in _sets('tts'):
        ref64, ref32 = _oracle_cnn(sd, segs, 1, torch.float64), _oracle_cnn(sd, segs, 1, torch.float32)
        got = {m: _valid(run_cnn_mel(_engine(tag, args, sd, m), mel, floor, plan), plan) for m in ALL_MODES}
        judge('StandardCNN + fc_out [%s]' % tag, RAGGED, got, ref64, ref32)


def _sa_inputs(tag, args, sd, counts, which):
    """(feat rows per clip, pool-input rows per clip, float64 and float32 oracle results) of one weight set and batch"""
    def make():
        feats = _sample(_cnn_rows(tag, args, sd, 0), counts, 1 if which == 'ragged' else 2)
        heads = _heads(args)
        n_layers = int(args['td_sa_num_layers'])
        td64, chain64 = _oracle_sa(sd, feats, n_layers, torch.float64, heads)
        td32, chain32 = _oracle_sa(sd, feats, n_layers, torch.float32, heads)
        xs = [t.astype(np.float32) for t in td64]          # pooling input: realistic LayerNorm'd rows, fp32
        return {'feat': feats, 'td64': td64, 'td32': td32, 'chain64': chain64, 'chain32': chain32, 'x': xs,
                'pool64': _oracle_pool(sd, xs, heads, torch.float64), 'pool32': _oracle_pool(sd, xs, heads, torch.float32),
                'sc64': _oracle_scores(sd, xs, heads, torch.float64), 'sc32': _oracle_scores(sd, xs, heads, torch.float32)}
    return _cached(('sa', tag, which), make)


@pytest.mark.parametrize('which', ['ragged', 'wide'])
def test_self_attention_and_pooling_against_float64(which):
    counts = RAGGED if which == 'ragged' else _wide_counts()
    plan = _plan(counts)
    for tag, args, sd in _sets('sa'):
        inp = _sa_inputs(tag, args, sd, counts, which)
        feat, x = _upload_rows(inp['feat'], plan), _upload_rows(inp['x'], plan)
        td, pool, score, chain = {}, {}, {}, {}
        nh = len(_heads(args))
        for m in ALL_MODES:
            eng = _engine(tag, args, sd, m)
            td[m] = _valid(run_td(eng, feat, plan), plan)
            o, sc = run_pool(eng, x, plan, want_scores=True)
            pool[m], score[m] = list(o.cpu().numpy()), [r[:, :nh] for r in _valid(sc, plan)]
            if eng.td_precision == 'bf16x6':
                chain[m] = list(run_td_pool(eng, feat, plan).cpu().numpy())
        chain['f32'] = list(run_pool(_engine(tag, args, sd, 'f32'), run_td(_engine(tag, args, sd, 'f32'), feat, plan), plan).cpu().numpy())
        for m in ('f16x4', 'f16x3'):                       # the same three-term kernels as 'bf16x6'
            _same_bits('td ' + m, td[m], td['bf16x6'])
            _same_bits('pool ' + m, pool[m], pool['bf16x6'])
            _same_bits('td_pool ' + m, chain[m], chain['bf16x6'])
        three = ('f32', 'bf16x6', 'bf16x3')
        judge('self-attention x%d [%s, %s]' % (args['td_sa_num_layers'], tag, which), counts,
              {m: td[m] for m in three}, inp['td64'], inp['td32'])
        # the outputs of the pooling are softmax-weighted means: the operand width of its two GEMMs shows in the attention logits
        # (measured: 'bf16x3' as close to float64 as 'bf16x6' there), so the control is asserted on those
        judge('pooling logits, %d head(s) [%s, %s]' % (nh, tag, which), counts, {m: score[m] for m in three}, inp['sc64'], inp['sc32'])
        judge('pooling, two-call, %d head(s) [%s, %s]' % (nh, tag, which), counts,
              {m: pool[m] for m in ('f32', 'bf16x6')}, inp['pool64'], inp['pool32'])
        judge('self-attention + pooling, fused [%s, %s]' % (tag, which), counts, {m: chain[m] for m in ('f32', 'bf16x6')},
              inp['chain64'], inp['chain32'])


def _lstm_inputs(tag, args, sd):
    def make():
        feats = _sample(_cnn_rows(tag, args, sd, 1), RAGGED, 3)
        s64, o64 = _oracle_lstm(sd, feats, torch.float64)
        s32, o32 = _oracle_lstm(sd, feats, torch.float32)
        return feats, s64, o64, s32, o32
    return _cached(('lstm', tag), make)


def test_bilstm_and_last_step_pooling_against_float64():
    plan = _plan(RAGGED)
    for tag, args, sd in _sets('tts'):
        feats, s64, o64, s32, o32 = _lstm_inputs(tag, args, sd)
        f = _upload_rows(feats, plan)
        seq, out = {}, {}
        for m in ALL_MODES:
            o, s = run_lstm(_engine(tag, args, sd, m), f, plan)
            seq[m], out[m] = _valid(s, plan), list(o.cpu().numpy())
        for m in ALL_MODES:                                 # fp32 VALU in every mode: one kernel
            _same_bits('BiLSTM ' + m, seq[m], seq['f32'])
            _same_bits('last-step pooling ' + m, out[m], out['f32'])
        judge('BiLSTM sequence [%s]' % tag, RAGGED, {'f32': seq['f32']}, s64, s32)
        judge('BiLSTM + last-step pooling [%s]' % tag, RAGGED, {'f32': out['f32']}, o64, o32)


def _de_engine(fuse, precision):
    from nisqa_amd.engine import HipNisqaDE
    key = ('de', fuse, precision)
    if key not in _ENG:
        _ENG[key] = HipNisqaDE(DO.de_args(fuse=fuse), DO.random_de_state_dict(2, fuse), 'cuda:0', precision=precision)
    return _ENG[key]


def _de_inputs(fuse, counts, which):
    """fused rows [x, y, x - y] / [x, y] of sampled pooling-input rows (first self-attention outputs) of the NISQA weights"""
    def make():
        tag, args, sd = [w for w in _sets('sa') if w[0] == 'mos_rand'][0]
        rows = np.concatenate(_sa_inputs(tag, args, sd, RAGGED, 'ragged')['x'])
        xs, ys = _sample(rows, counts, 4), _sample(rows, counts, 5)
        fused = [DO.fuse_rows(a, b, fuse).astype(np.float32) for a, b in zip(xs, ys)]
        sd2 = DO.random_de_state_dict(2, fuse)
        pf = 'time_dependency_2.model.'
        _, o64 = _oracle_sa(sd2, fused, 2, torch.float64, ['pool.model.'], pfx=pf)
        _, o32 = _oracle_sa(sd2, fused, 2, torch.float32, ['pool.model.'], pfx=pf)
        return fused, o64, o32
    return _cached(('de', fuse, which), make)


@pytest.mark.parametrize('fuse', ['x/y/-', 'x/y'])
@pytest.mark.parametrize('which', ['ragged', 'wide'])
def test_de_second_self_attention_and_pooling_against_float64(fuse, which):
    from nisqa_amd.engine import DE_FEAT_LD
    counts = RAGGED if which == 'ragged' else _wide_counts()
    plan = _plan(counts)
    fused, o64, o32 = _de_inputs(fuse, counts, which)
    f = _upload_rows(fused, plan, width=DE_FEAT_LD)
    got = {m: list(_de_engine(fuse, m).td2_pool(f, plan).cpu().numpy()) for m in ('f32', 'bf16x6', 'f16x4')}
    _same_bits('DE td2_pool f16x4', got.pop('f16x4'), got['bf16x6'])
    judge('DE self-attention 2 + pooling, %d wide [%s]' % (DO.FUSE_WIDTH[fuse], which), counts, got, o64, o32)


# =============================================================================================================================
# 2. layout and padding contract
# =============================================================================================================================
def _layouts(gran):
    """(name, tok_off) of the RAGGED batch: the token layouts an entry of granularity ``gran`` must accept"""
    out = [('pad64+slack', helpers.tok_offsets(RAGGED, 64, 64))]
    if gran == 32:
        out += [('pad32', helpers.tok_offsets(RAGGED, 32)), ('pad32+slack', helpers.tok_offsets(RAGGED, 32, 32))]
    return out


FILLS = (0.0, float('nan'), 'big')


def _check_layouts(stage, gran, run, rows):
    """run(plan, fill) -> list of per-clip outputs (valid rows, or pooled rows).  The 64-padded, zero-padded batch is the
    reference; every other layout, every padding fill and every clip alone must reproduce its bits."""
    ref = run(helpers.plan_with_layout(RAGGED, helpers.tok_offsets(RAGGED)), 0.0)
    variants = [(name, tok, fill) for name, tok in _layouts(gran) for fill in (FILLS if rows else (0.0,))]
    variants += [('pad64', helpers.tok_offsets(RAGGED), fill) for fill in (FILLS[1:] if rows else ())]
    for name, tok, fill in variants:
        got = run(helpers.plan_with_layout(RAGGED, tok), fill)
        _same_bits('%s, %s, padding %s' % (stage, name, fill), got, ref)
    for b, n in enumerate(RAGGED):                          # every kernel is clip-local: alone = in the batch
        got = run(helpers.plan_with_layout([n], helpers.tok_offsets([n])), 'big' if rows else 0.0, clip=b)
        _same_bits('%s, clip %d (n=%d) alone' % (stage, b, n), got, ref[b:b + 1])


def _rows_runner(fn, eng, rows, pooled=False, width=None):
    def run(plan, fill, clip=None):
        r = rows if clip is None else rows[clip:clip + 1]
        out = fn(eng, _upload_rows(r, plan, fill, width), plan)
        return list(out.cpu().numpy()) if pooled else _valid(out, plan)
    return run


@pytest.mark.parametrize('precision', ['f32', 'bf16x3', 'bf16x6'])
def test_self_attention_and_pooling_entries_honour_the_layout_contract(precision):
    gran = 64 if precision == 'bf16x6' else 32               # the three-term kernels document whole 64-token workgroups
    for tag, args, sd in [w for w in _sets('sa') if w[0].endswith('rand')]:      # five heads and one
        eng = _engine(tag, args, sd, precision)
        inp = _sa_inputs(tag, args, sd, RAGGED, 'ragged')
        _check_layouts('td %s %s' % (precision, tag), gran, _rows_runner(run_td, eng, inp['feat']), True)
        _check_layouts('pool %s %s' % (precision, tag), gran, _rows_runner(run_pool, eng, inp['x'], True), True)
        if precision == 'bf16x6':
            _check_layouts('td_pool %s' % tag, 64, _rows_runner(run_td_pool, eng, inp['feat'], True), True)


def test_lstm_entry_honours_the_layout_contract():
    tag, args, sd = _sets('tts')[0]
    feats = _lstm_inputs(tag, args, sd)[0]
    eng = _engine(tag, args, sd, 'f32')

    def run(plan, fill, clip=None):
        r = feats if clip is None else feats[clip:clip + 1]
        out, seq = run_lstm(eng, _upload_rows(r, plan, fill), plan)
        return [np.concatenate([s.reshape(-1), o]) for s, o in zip(_valid(seq, plan), out.cpu().numpy())]
    _check_layouts('BiLSTM', 32, run, True)


@pytest.mark.parametrize('precision', ['f32', 'bf16x6'])
def test_de_second_self_attention_entry_honours_the_layout_contract(precision):
    from nisqa_amd.engine import DE_FEAT_LD
    fused = _de_inputs('x/y/-', RAGGED, 'ragged')[0]
    eng = _de_engine('x/y/-', precision)
    _check_layouts('DE td2_pool %s' % precision, 64, _rows_runner(lambda e, f, p: e.td2_pool(f, p), eng, fused, True, DE_FEAT_LD), True)


@pytest.mark.parametrize('arch', [0, 1])
@pytest.mark.parametrize('precision', ALL_MODES)
def test_cnn_entries_honour_the_layout_contract_and_leave_padding_rows_untouched(arch, precision):
    """From mel (both architectures) and, for the AdaptCNN, from segment tensors whose padding segments hold NaN / +-3e38."""
    mel, floor, frame_off, _ = _mel_batch(arch)
    tag, args, sd = _sets('tts' if arch == 1 else 'cnn')[0]
    eng = _engine(tag, args, sd, precision)
    gran = 64 if precision in ('bf16x6', 'f16x4', 'f16x3') else 32
    width = 20 if arch == 1 else 384
    fo = np.asarray(frame_off)

    def checked(feat, plan):
        pad = _padding_rows(plan)
        if len(pad):
            bits = feat.view(torch.int32)[torch.from_numpy(pad).to(feat.device)]
            assert bool((bits == SENTINEL).all()), ('padding rows of feat written', precision, arch)
        return _valid(feat[:plan.total_tok], plan)

    def run_mel(plan, fill, clip=None):
        if clip is None:
            p = helpers.plan_with_layout(plan.n_wins, plan.tok_off, fo)
            return checked(run_cnn_mel(eng, mel, floor, p), p)
        p = helpers.plan_with_layout(plan.n_wins, plan.tok_off, [0, fo[clip + 1] - fo[clip]])
        return checked(run_cnn_mel(eng, mel[fo[clip]:fo[clip + 1]].contiguous(), floor[clip:clip + 1].contiguous(), p), p)
    _check_layouts('CNN from mel %s arch %d' % (precision, arch), gran, run_mel, False)
    if arch == 1:
        return
    segs = _segments(0)
    L = max(RAGGED)

    def run_seg(plan, fill, clip=None):
        ids = range(len(RAGGED)) if clip is None else [clip]
        x = np.empty((len(ids), L, 1, 48, 15), np.float32)
        x[...] = 3e38 if fill == 'big' else fill
        if fill == 'big':
            x[..., 1::2] = -3e38
        for k, b in enumerate(ids):
            x[k, :len(segs[b])] = segs[b]
        return checked(run_cnn_seg(eng, torch.from_numpy(x).to('cuda:0'), plan), plan)
    _check_layouts('CNN from segment tensors %s' % precision, gran, run_seg, True)


def _poison_allocator(byte):
    """Hand the caching allocator a large block full of ``byte``: the next torch.empty of the large pool is carved from it."""
    torch.cuda.synchronize()
    junk = torch.empty(1 << 30, dtype=torch.uint8, device='cuda:0')
    junk.fill_(byte)
    del junk


@pytest.mark.parametrize('arch', ['NISQA_DIM', 'NISQA_TTS'])
def test_forward_pcm_does_not_read_its_workspace_before_writing_it(arch):
    args = dict(helpers.DIM_ARGS) if arch == 'NISQA_DIM' else dict(helpers.TTS_ARGS)
    sd = helpers.random_state_dict(7 if arch == 'NISQA_DIM' else 9, arch)
    pcm = [synth.synth_pcm16(950 + i, s) for i, s in enumerate((0.16, 0.8, 3.3, 0.31, 13.0, 1.28))]
    for m in ALL_MODES:
        eng = _engine(arch, args, sd, m)
        plan = eng.plan([len(p) for p in pcm], 48000)
        dev = torch.from_numpy(np.concatenate(pcm)).to(eng.device)
        eng.forward_pcm(dev, plan, 48000)
        ws = eng._ws[torch.cuda.current_stream(eng.device).cuda_stream]
        ws.zero_()
        clean = eng.forward_pcm(dev, plan, 48000).cpu().numpy()
        ws.fill_(0xFF)                                      # every float of the workspace NaN
        dirty = eng.forward_pcm(dev, plan, 48000).cpu().numpy()
        assert np.isfinite(clean).all()
        _same_bits('forward_pcm %s %s, workspace 0xFF' % (arch, m), list(dirty), list(clean))


def test_de_forward_pcm_and_forward_segments_ignore_stale_device_memory():
    """HipNisqaDE.forward_pcm and forward_segments take their scratch from torch.empty: outputs must not depend on what the
    allocator hands out.  forward_segments also gets NaN / +-3e38 in the padding segments of its input."""
    eng = _de_engine('x/y/-', 'bf16x6')
    pcm = [synth.synth_pcm16(960 + i, s) for i, s in enumerate((2.0, 0.5, 3.1, 1.7))]
    plan = eng.plan([len(pcm[0]), len(pcm[1])], [len(pcm[2]), len(pcm[3])], 48000)
    dev = torch.from_numpy(np.concatenate(pcm)).to(eng.device)
    outs = []
    for byte in (0x00, 0xFF):
        _poison_allocator(byte)
        outs.append(eng.forward_pcm(dev, plan, 48000).cpu().numpy())
    assert np.isfinite(outs[0]).all()
    _same_bits('DE forward_pcm, stale memory', list(outs[1]), list(outs[0]))
    segs = _segments(0)
    ids = [0, 8, 9, 13, 23]                                          # 1, 63, 64, 96, 1299 segments
    L = 1300
    for m in ('f32', 'bf16x3', 'bf16x6', 'f16x4'):
        e = _engine('dim_rand', dict(helpers.DIM_ARGS), helpers.random_state_dict(7, 'NISQA_DIM'), m)
        res = []
        for fill, byte in ((0.0, 0x00), (float('nan'), 0xFF), ('big', 0xFF)):
            x = np.empty((len(ids), L, 1, 48, 15), np.float32)
            x[...] = 3e38 if fill == 'big' else fill
            for k, b in enumerate(ids):
                x[k, :len(segs[b])] = segs[b]
            _poison_allocator(byte)
            res.append(e.forward_segments(torch.from_numpy(x), [RAGGED[b] for b in ids]).cpu().numpy())
        assert np.isfinite(res[0]).all()
        for r in res[1:]:
            _same_bits('forward_segments %s' % m, list(r), list(res[0]))
