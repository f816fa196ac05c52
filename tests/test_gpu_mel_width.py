"""mel_frame_kernel and its finalisers (csrc/mel.hip): batch-independent bits, and fp32 width against float64.

1. Exact (uint32 views, no tolerance).  A clip's unclamped rows and its floor carry the same bits alone and in every batch:
   any order, behind leading clips of 15..18 frames (a probe's first frame on every residue of 4), at every frames-per-wave
   value the launcher picks (4, 5, 21, 32 and a two-round batch; a wave then walks across clip boundaries, republishes the
   clip maximum and resets its running one), from int16 or float32 samples, with the specialised or the generic filter bank.
   floor = max - 80 and the in-place clamp are restated in numpy; zeros give -80 / -160; a launch through the C ABI leaves
   the rows behind total_frames alone; nisqa_pcm16_to_f32 is exact past its grid's first stride.
2. Width.  mel_width_oracle.py: the error of a band is measured in mel AMPLITUDE relative to the frame's energy, against a
   float64 pipeline, in units of what a float32 CPU pipeline (numpy's complex64 FFT) leaves: e_gpu.max() <= FACTOR * floor
   per probe.  Measured on an MI355X (gpu / floor, worst probe), one line per front end:
       48 kHz fmax 20 kHz   floor 4.53   gpu x0.42        16 kHz    floor 3.59   gpu x0.53
       48 kHz fmax  8 kHz   floor 2.55   gpu x0.77        96 kHz    floor 2.97   gpu x0.92
                                                         192 kHz    floor 1.59   gpu x1.42   (the worst: FACTOR = 1.42 x 1.5 -> 3)
   tests/test_mel_width_host.py shows that four wrong pipelines miss this bound by far more than 2 x.
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import mel_width_oracle as mw

pytestmark = pytest.mark.gpu

# name -> (sr, fmax, reduced probe set); the first carries the full set and every launch shape
FRONT_ENDS = {'48k_fmax20k': (48000, 20000, False), '48k_fmax8k': (48000, 8000, True), '16k': (16000, 20000, True),
              '96k': (96000, 20000, True), '192k': (192000, 20000, True)}
# (front end, batch): total frames aimed at, and the (rounds, frames per wave) the launcher must pick for it
SPREAD = {('48k_fmax20k', 'fpw4'): (12000, (1, 4)), ('48k_fmax20k', 'fpw5'): (14000, (1, 5)),
          ('48k_fmax20k', 'fpw21'): (64064, (1, 21)), ('48k_fmax20k', 'fpw32'): (98300, (1, 32)),
          ('48k_fmax20k', 'two_rounds'): (98320, (2, 17)),
          ('48k_fmax8k', 'fpw5'): (14000, (1, 5)), ('16k', 'fpw5'): (14000, (1, 5)), ('96k', 'fpw5'): (9500, (1, 5)),
          ('192k', 'fpw5'): (4800, (1, 5))}
N_SHORT = 300                                                      # copies of the shortest clip in a spread batch, at least
SENTINEL = 0x7FC5A5A5


class FrontEnd(object):
    """Engine, probes and every clip's alone run (device uint32-as-int32 rows, floor) of one front end, built once."""
    _cache, _engines = {}, {}

    @classmethod
    def get(cls, name):
        if name not in cls._cache:
            cls._cache[name] = cls(name)
        return cls._cache[name]

    def __init__(self, name):
        from nisqa_amd.engine import HipNisqa
        self.name = name
        self.sr, self.fmax, reduced = FRONT_ENDS[name]
        self.hop, self.win = mw.geometry(self.sr)
        if self.fmax not in self._engines:
            self._engines[self.fmax] = HipNisqa(dict(helpers.DIM_ARGS, ms_fmax=self.fmax), helpers.random_state_dict(7, 'NISQA_DIM'))
        self.eng = self._engines[self.fmax]
        self.groups = mw.probes(self.sr, reduced)
        self.clips = dict(mw.flat(self.groups))
        if not reduced:                                            # fillers: full-scale 10 s noise, tiled
            rng = np.random.default_rng(5)
            for i in range(3):
                self.clips['filler10_%d' % i] = np.tile(rng.integers(-32767, 32768, 100 * self.hop).astype(np.int16), 10)
        for n in (15, 16, 17, 18):                                 # leading clips of n frames
            self.clips['lead%d' % n] = np.random.default_rng(n).integers(-32767, 32768, (n - 1) * self.hop + 3).astype(np.int16)
        self.alone = {}
        for n, x in self.clips.items():
            mel, floor, _ = self.run([n])
            self.alone[n] = (mel.view(torch.int32), floor.view(torch.int32))
        torch.cuda.synchronize()

    def frames(self, name):
        return 1 + len(self.clips[name]) // self.hop

    def run(self, names, clamp=False, as_f32=False):
        x = torch.from_numpy(np.concatenate([self.clips[n] for n in names])).to(self.eng.device)
        if as_f32:
            x = self.eng.pcm16_to_f32(x)
        plan = self.eng.plan([len(self.clips[n]) for n in names], self.sr)
        mel, floor = self.eng.mel(x, plan, self.sr, clamp=clamp)
        return mel, floor, plan

    def same_bits_as_alone(self, label, names, mel, floor, plan):
        """Every clip of the batch against its alone run, on the device (all copies of a clip in one gather)."""
        assert bool(torch.isfinite(mel).all()) and bool(torch.isfinite(floor).all()), label
        mel_i, floor_i = mel.view(torch.int32), floor.view(torch.int32)
        where = {}
        for k, n in enumerate(names):
            where.setdefault(n, []).append(k)
        bad = []
        for n, ks in where.items():
            rows, fl = self.alone[n]
            T = rows.shape[0]
            assert all(plan.frame_off[k + 1] - plan.frame_off[k] == T for k in ks)
            start = torch.from_numpy(plan.frame_off[ks].astype(np.int64)).to(mel.device)
            got = mel_i[start[:, None] + torch.arange(T, device=mel.device)[None, :]]          # [copies, T, 48]
            ok_rows = (got == rows[None]).all(2).all(1)
            ok_floor = floor_i[torch.tensor(ks, device=mel.device)] == fl
            for j in torch.nonzero(~(ok_rows & ok_floor)).reshape(-1).tolist()[:4]:
                bad.append((n, 'clip', ks[j], 'rows' if not bool(ok_rows[j]) else 'floor'))
        assert not bad, (label, bad)

    def spread(self, aim):
        """The probe groups spread through fillers (copies of the shortest clip, and 10 s noise where the front end has it)
        so that the batch has about ``aim`` frames."""
        base = sum(self.frames(n) for n, _ in mw.flat(self.groups))
        n10 = max(0, (aim - base - N_SHORT * 15) // 1001) if 'filler10_0' in self.clips else 0
        n_short = (aim - base - n10 * 1001) // 15
        assert n_short >= N_SHORT, (aim, n_short)
        fill = ['filler10_%d' % (i % 3) for i in range(n10)] + ['shortest'] * n_short
        fill = [fill[i] for i in np.random.default_rng(aim).permutation(len(fill))]
        out, step = [], len(fill) // (len(self.groups) + 1)
        for g, grp in enumerate(self.groups):
            out += fill[g * step:(g + 1) * step] + [n for n, _ in grp]
        return out + fill[len(self.groups) * step:]


def _np(t):
    return t.detach().cpu().numpy()


def _clamp_is_maximum_of_rows_and_floor(fe, label, names, mel_u, floor_u, plan):
    mel_c, floor_c, _ = fe.run(names, clamp=True)
    assert torch.equal(floor_c.view(torch.int32), floor_u.view(torch.int32)), label
    T = torch.from_numpy(np.diff(plan.frame_off).astype(np.int64)).to(mel_u.device)
    want = torch.maximum(mel_u, torch.repeat_interleave(floor_u, T)[:, None])
    assert torch.equal(mel_c.view(torch.int32), want.view(torch.int32)), label
    return mel_c


@pytest.fixture(scope='module', params=list(FRONT_ENDS))
def fe(request):
    return FrontEnd.get(request.param)


def test_alone_floor_is_max_minus_80_zeros_give_minus_80_and_clamp_is_np_maximum(fe):
    for n in fe.clips:
        rows = _np(fe.alone[n][0]).view(np.float32)
        floor = _np(fe.alone[n][1]).view(np.float32)
        assert rows.shape == (fe.frames(n), 48) and np.isfinite(rows).all(), n
        want = np.float32(rows.max()) - np.float32(80)
        assert floor.view(np.uint32)[0] == np.array([want], np.float32).view(np.uint32)[0], (n, floor, want)
        mel_c, floor_c, _ = fe.run([n], clamp=True)
        assert np.array_equal(_np(floor_c).view(np.uint32), floor.view(np.uint32)), n
        assert np.array_equal(_np(mel_c).view(np.uint32), np.maximum(rows, floor[0]).view(np.uint32)), n
        if n == 'zeros':
            assert (rows == np.float32(-80.0)).all() and floor[0] == np.float32(-160.0)
        if n == 'fall':                                            # the floor does cut this one
            assert (rows < floor[0]).any()


def test_probe_bits_do_not_move_with_order_leading_clip_input_type_or_filter_bank_form(fe, monkeypatch):
    order = [n for n, _ in mw.flat(fe.groups)]
    reverse = [n for g in reversed(fe.groups) for n, _ in reversed(g)]
    batches = [('in order', order), ('reversed', reverse)] + [('behind %d frames' % k, ['lead%d' % k] + order) for k in (15, 16, 17, 18)]
    assert [fe.frames('lead%d' % k) for k in (15, 16, 17, 18)] == [15, 16, 17, 18]
    assert any(int(np.cumsum([0] + [len(fe.clips[n]) for n in order])[k]) % 2 for k in range(len(order)))   # a clip at an odd int16 offset
    for label, names in batches:
        mel, floor, plan = fe.run(names)
        assert mw.launch_shape(plan.total_frames, fe.win)[:2] == (1, 4)
        fe.same_bits_as_alone(label, names, mel, floor, plan)
    mel, floor, plan = fe.run(order)
    mel_c = _clamp_is_maximum_of_rows_and_floor(fe, 'in order, clamp', order, mel, floor, plan)
    rows, fl = _np(mel), _np(floor)
    want = np.concatenate([np.maximum(rows[plan.frame_off[k]:plan.frame_off[k + 1]], fl[k]) for k in range(plan.n_clips)])
    assert np.array_equal(_np(mel_c).view(np.uint32), want.view(np.uint32))
    fe.same_bits_as_alone('in order, float32 input', order, *fe.run(order, as_f32=True))
    monkeypatch.setenv('NISQA_MEL_FB_GENERIC', '1')
    fe.same_bits_as_alone('in order, generic filter bank', order, *fe.run(order))
    fe.same_bits_as_alone('reversed, generic filter bank, float32 input', reverse, *fe.run(reverse, as_f32=True))


def test_spread_batches_cover_every_launch_shape():
    """The first front end is run at frames per wave 4, 5, 21, 32 and over two rounds; every other one above 4 once."""
    assert {v[1] for k, v in SPREAD.items() if k[0] == '48k_fmax20k'} == {(1, 4), (1, 5), (1, 21), (1, 32), (2, 17)}
    for name in FRONT_ENDS:
        assert any(k[0] == name and v[1][1] > 4 for k, v in SPREAD.items()), name
    assert 98304 == 3072 * 32 and mw.launch_shape(98304, 960)[:2] == (1, 32) and mw.launch_shape(98305, 960)[:2] == (2, 17)
    assert mw.launch_shape(64064, 960)[:2] == (1, 21) and mw.launch_shape(12288, 960)[:2] == (1, 4)


@pytest.mark.parametrize('case', sorted(SPREAD), ids=lambda c: '%s-%s' % c)
def test_probe_bits_do_not_move_with_frames_per_wave(case):
    fe = FrontEnd.get(case[0])
    aim, shape = SPREAD[case]
    names = fe.spread(aim)
    mel, floor, plan = fe.run(names)
    rounds, fpw, waves = mw.launch_shape(plan.total_frames, fe.win)
    print(case, 'clips', plan.n_clips, 'frames', plan.total_frames, 'rounds', rounds, 'frames per wave', fpw)
    assert (rounds, fpw) == shape and aim - 15 < plan.total_frames <= aim
    assert plan.n_clips > max(64, N_SHORT)                          # mel_floor_kernel runs more than one block
    fe.same_bits_as_alone(str(case), names, mel, floor, plan)
    _clamp_is_maximum_of_rows_and_floor(fe, str(case) + ', clamp', names, mel, floor, plan)
    fe.same_bits_as_alone(str(case) + ', float32 input', names, *fe.run(names, as_f32=True))


def test_c_abi_launch_leaves_the_rows_behind_total_frames_alone(fe):
    from nisqa_amd import lib as L_
    eng = fe.eng
    names = [n for n, _ in mw.flat(fe.groups)]
    x = torch.from_numpy(np.concatenate([fe.clips[n] for n in names])).to(eng.device)
    plan = eng.plan([len(fe.clips[n]) for n in names], fe.sr)
    _, fpw, waves = mw.launch_shape(plan.total_frames, fe.win)
    assert plan.total_frames % (waves * fpw) != 0                  # the last workgroup is partial
    mt, d = eng.mel_tables(fe.sr), plan.to(eng.device)
    out = torch.full((plan.total_frames + 64, 48), SENTINEL, dtype=torch.int32, device=eng.device)
    cmax = torch.full((plan.n_clips + 8,), SENTINEL, dtype=torch.int32, device=eng.device)
    cmax[:plan.n_clips] = 0
    floor = torch.full((plan.n_clips + 8,), SENTINEL, dtype=torch.int32, device=eng.device)
    p_ = lambda a: ctypes.c_void_p(a.data_ptr())
    L_.check(eng.lib.nisqa_mel_db_pcm16(p_(x), p_(d['clip_off']), p_(d['frame_off']), plan.n_clips, plan.total_frames,
                                        ctypes.byref(mt['cfg']), p_(mt['window']), p_(mt['twiddle']), p_(mt['band_start']),
                                        p_(mt['band_len']), p_(mt['band_woff']), p_(mt['band_w']), p_(out), p_(cmax), eng._stream()),
             'nisqa_mel_db_pcm16')
    L_.check(eng.lib.nisqa_mel_finalize(p_(out), p_(d['frame_off']), plan.n_clips, plan.total_frames, p_(cmax), 80.0, p_(floor), 0,
                                        eng._stream()), 'nisqa_mel_finalize')
    torch.cuda.synchronize()
    assert bool((out[plan.total_frames:] == SENTINEL).all())
    assert bool((cmax[plan.n_clips:] == SENTINEL).all()) and bool((floor[plan.n_clips:] == SENTINEL).all())
    fe.same_bits_as_alone('C ABI', names, out[:plan.total_frames].view(torch.float32), floor[:plan.n_clips].view(torch.float32), plan)


def test_pcm16_to_f32_is_exact_past_the_first_grid_stride():
    eng = FrontEnd.get('48k_fmax20k').eng
    x = np.random.default_rng(1).integers(-32768, 32768, 2 * 4096 * 256 + 3).astype(np.int16)
    got = _np(eng.pcm16_to_f32(torch.from_numpy(x).to(eng.device)))
    assert np.array_equal(got.view(np.uint32), (x.astype(np.float32) / np.float32(32768.0)).view(np.uint32))


def test_alone_rows_are_as_wide_as_fp32_against_float64(fe):
    clips = mw.flat(fe.groups)
    y = mw.Yardstick(clips, fe.sr, fe.fmax)
    rows = {n: _np(fe.alone[n][0]).view(np.float32).T for n, _ in clips}
    y.judge('mel %s' % fe.name, rows, mw.FACTOR)
