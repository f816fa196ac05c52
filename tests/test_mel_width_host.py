"""CPU checks of the mel width yardstick (tests/mel_width_oracle.py): the float64 pipeline is the oracle's, the launcher's rule
is restated right, and the bound FACTOR * floor that tests/test_gpu_mel_width.py holds the kernel to tells a wrong mel front
end from a right one -- four deliberately wrong CPU pipelines, everything else in float64, miss it by more than 2 x."""
import numpy as np
import pytest

import mel_width_oracle as mw
from oracle import mel as omel

SR, FMAX = 48000, 20000


@pytest.fixture(scope='module')
def yard():
    clips = mw.flat(mw.probes(SR))
    return clips, mw.Yardstick(clips, SR, FMAX)


def test_float64_pipeline_is_the_oracles(yard):
    clips, y = yard
    for n, x in clips:
        ref = omel.melspec_db_from_audio(x.astype(np.float32) / np.float32(32768.0), SR, fmax=FMAX, return_unclamped=True)
        loud = y.M64[n] > 1e-3
        assert ref.shape == y.M64[n].shape
        if loud.any():
            assert np.abs(mw.encode_db(y.M64[n]) - ref)[loud].max() <= 1e-4, n
    assert y.M64['zeros'].max() == 0.0 and y.norms['zeros'].max() == 0.0


def test_float32_pipeline_runs_a_complex64_fft_and_sets_a_floor_of_a_few_eps(yard):
    clips, y = yard
    assert np.fft.rfft(np.ones(8, np.float32)).dtype == np.complex64
    assert 1.0 < y.floor < 16.0, y.floor                            # between one eps32 of the frame's energy and one per radix-2 stage and more
    assert y.e32['zeros'] == 0.0
    y.judge('float32 CPU pipeline', {n: mw.encode_db(mw.mel_amplitudes(x, SR, FMAX, np.float32)[0]) for n, x in clips}, 1.0)


def test_probe_lengths_and_launch_rule():
    hop, win = mw.geometry(SR)
    assert (hop, win) == (480, 960)
    frames = {n: 1 + len(x) // hop for n, x in mw.flat(mw.probes(SR))}
    assert frames['shortest'] == 15 and frames['hop_minus_1'] == 15 and frames['hop'] == 16 and frames['odd'] == 15
    assert len(dict(mw.flat(mw.probes(SR)))['odd']) % 2 == 1
    for sr in (16000, 96000, 192000):
        names = [n for n, _ in mw.flat(mw.probes(sr, reduced=True))]
        assert names.index('loud_a') + 1 == names.index('quiet') == names.index('loud_b') - 1
    # mel_db_launch: whole rounds of the resident waves, then 4..32 frames per wave
    assert mw.launch_shape(12288, 960) == (1, 4, 12) and mw.launch_shape(12289, 960) == (1, 5, 12)
    assert mw.launch_shape(64064, 960) == (1, 21, 12) and mw.launch_shape(98304, 960) == (1, 32, 12)
    assert mw.launch_shape(98305, 960) == (2, 17, 12)
    assert mw.launch_shape(8193, 1920) == (1, 5, 4) and mw.launch_shape(4097, 3840) == (1, 5, 4)


@pytest.mark.parametrize('label,wrong', [('symmetric padding', dict(pad_mode='symmetric')),
                                         ('window shifted by one sample', dict(window_shift=1)),
                                         ('bank shifted by one bin', dict(bank_shift=1)),
                                         ('frames rounded to float16', dict(frame_dtype=np.float16))])
def test_a_wrong_front_end_misses_the_bound_by_more_than_2x(yard, label, wrong):
    clips, y = yard
    rows = {n: mw.encode_db(mw.mel_amplitudes(x, SR, FMAX, np.float64, **wrong)[0]) for n, x in clips}
    ratio = y.judge(label, rows)
    assert max(ratio.values()) > 2.0 * mw.FACTOR, (label, ratio)
    with pytest.raises(AssertionError):
        y.judge(label, rows, mw.FACTOR)
