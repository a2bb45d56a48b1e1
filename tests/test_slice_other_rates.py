"""The resident slice at 44.1, 88.2 and 22.05 kHz, the rates the other slice tests do not run (they use 48 and 96 kHz).
At these rates the 30 ms alignment segment is 1323, 2646 or 661 samples (not a multiple of 4: the lag search's LDS layout
rounds a's planes per pair), and head, fades, knee windows and the FIR length all take other values.

  * resident against the staged run_slice, BIT FOR BIT: a two-file layout (FL,FR + FC) with the alignments on, then with
    the decay stage as well; a 7.1 layout with both;
  * resident against the oracle composition (fp64): one measurement per rate, the bounds of the 48 kHz tests.

The FIRs are passed in (synthetic, of the length the reference designs at each rate)."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

RATES = [44100, 88200, 22050]
SEVEN_ONE = ["FL", "FR", "FC", "BL", "BR", "SL", "SR"]


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _setup(fs, spk_files, M, seed):
    from test_resident_slice import synth_firs, synth_frames
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.resident_slice import Layout, ResidentSlice
    e = ImpulseResponseEstimator(min_duration=1.0, fs=fs)
    meas = [[synth_frames(e, spk, seed + 1000 * m + 17 * k, rt60=0.2 + 0.04 * m) for k, spk in enumerate(spk_files)] for m in range(M)]
    layout = Layout(e, [(fr.shape[0], 2, spk) for fr, spk in zip(meas[0], spk_files)])
    rs = ResidentSlice(e, layout, max_measurements=M)
    firs = synth_firs(layout.tasks, rs.taps, seed)
    rs.set_firs(firs)
    return e, meas, layout, rs, firs


@pytest.mark.parametrize("fs", RATES)
def test_small_layout_alignment_and_decay_bitwise_and_oracle(fs):
    from test_resident_slice import TIME_TOL, assert_same_as_staged, oracle_measurement, rel, staged_measurement
    from oracle import estimator as oest
    from impulse_hip.resident_slice import _fir_taps
    files_spk = [["FL", "FR"], ["FC"]]
    e, meas, layout, rs, firs = _setup(fs, files_spk, 2, 3100 + fs // 50)
    assert rs.taps == _fir_taps(fs)
    try:
        rs.set_alignment(True)
        got = _quiet(rs.run, meas)
        rows, res = rs.slice.results()
        assert rs.stats["staged"] == 0, res["flags"]
        assert np.any(rows["shift_ipsilateral"] != 0) or np.any(rows["shift_onset"] != 0)     # the alignment moves rows
        for m in range(2):
            assert_same_as_staged(got[m], staged_measurement(e, list(zip(meas[m], files_spk)), firs, align=True))
        # the oracle composition of the same stages, one measurement
        files = list(zip(meas[0], files_spk))
        tail_ind, g, o_irs = oracle_measurement(oest.Estimator(min_duration=1.0, fs=fs), files, firs, fs, align=True)
        assert int(res["keep"][0]) == tail_ind
        assert got[0][1] == pytest.approx(g, abs=1e-5)
        for sp in o_irs:
            for sd in o_irs[sp]:
                y = got[0][0].irs[sp][sd].peek()
                assert y.shape == o_irs[sp][sd].shape, (sp, sd)
                assert rel(y, o_irs[sp][sd]) <= 2 * TIME_TOL, (sp, sd)
        # the decay stage as well: FL to a target faster than its decay, FR slower, FC none (the rooms' RT60 reads lower
        # at 22.05 kHz than at 48 kHz, below 0.5 s: FL's target is 0.1 s)
        decay = {"FL": 0.1, "FR": 5.0}
        rs.set_decay(decay)
        got = _quiet(rs.run, meas)
        rows, res = rs.slice.results()
        assert rs.stats["staged"] == 0, (res["flags"], rows["decay_flags"])
        R = rs.slice.rows
        for m in range(2):
            assert list(rows["decay_state"][m * R:(m + 1) * R]) == [1, 1, 2, 2, 0, 0]
            assert_same_as_staged(got[m], staged_measurement(e, list(zip(meas[m], files_spk)), firs, decay=decay, align=True))
    finally:
        rs.close()


@pytest.mark.parametrize("fs", RATES)
def test_seven_one_layout_alignment_and_decay_bitwise(fs):
    from test_resident_slice import assert_same_as_staged, staged_measurement
    e, meas, layout, rs, firs = _setup(fs, [SEVEN_ONE], 2, 5200 + fs // 50)
    decay = {"FL": 0.5, "SL": 0.4, "BR": 5.0}
    try:
        rs.set_alignment(True)
        rs.set_decay(decay)
        got = _quiet(rs.run, meas)
        rows, res = rs.slice.results()
        assert rs.stats["staged"] == 0, (res["flags"], rows["decay_flags"])
        assert np.any(rows["shift_ipsilateral"] != 0)
        for m in range(2):
            assert_same_as_staged(got[m], staged_measurement(e, [(meas[m][0], SEVEN_ONE)], firs, decay=decay, align=True))
    finally:
        rs.close()
