"""Microphone-deviation correction without a GPU: the NumPy model against the reference's fixtures, the host integers of
K14 against the reference's rules, run_slice's refusals and the new C ABI names."""
import os
import re

import numpy as np
import pytest

import micdev_inputs as mi
import micdev_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(mi.CASES))
def test_model_reproduces_the_reference_fixtures(golden, case):
    z = golden("mic_deviation")
    fs, irs, anchor, strength = mi.hrir_case(case)
    rows, used, mis, (avg, mx), skipped, firs = mm.stage(irs, fs, strength, anchor)
    p = case + "/"
    assert used == str(z[p + "anchor"])
    assert np.max(np.abs(mis - z[p + "mismatch_db"])) <= 1e-9
    assert abs(avg - float(z[p + "avg_error_db"])) <= 1e-9 and abs(mx - float(z[p + "max_error_db"])) <= 1e-9
    assert skipped == bool(z[p + "skipped"])
    # the oracle's firwin2 / homomorphic restatement agrees with SciPy's to ~1e-7 of the peak (the device K6: 5e-8, GPU tests)
    for got, key in zip(mm.firs(mis, fs, strength), ("left_fir", "right_fir")):
        want = z[p + key]
        assert got.shape == want.shape
        assert np.max(np.abs(got - want)) <= 2e-7 * np.max(np.abs(want))
    step = int(z["decim_step"])
    flat = np.stack([rows[sp][sd] for sp in irs for sd in ("left", "right")])
    assert flat.shape[1] == int(z[p + "out_len"])
    err = np.max(np.abs(flat[:, ::step] - z[p + "decim"]), axis=1) / z[p + "row_peak"]
    assert np.max(err) <= 2e-6


def test_host_integers_follow_the_reference_rules():
    from scipy.fft import next_fast_len
    from impulse_hip import microphone_deviation_correction as mdc
    for fs in (44100, 48000, 88200, 96000, 176400, 192000):
        for window_ms, pre_ms in ((5.0, 0.5), (2.5, 0.0), (0.1, 0.05), (100.0, 3.0)):
            win, pre = mdc.analysis_lengths(fs, window_ms, pre_ms)
            assert win == max(int(round(window_ms * fs / 1000.0)), 32)
            assert pre == max(int(round(pre_ms * fs / 1000.0)), 0)
    assert mdc.analysis_lengths(44100) == (220, 22)          # 220.5 rounds half to even
    for n in list(range(1, 2100)) + [8191, 8192, 8193, 8232, 8233, 9600, 65537, 100003]:
        assert mdc.next_fast_len_11(n) == next_fast_len(n) == mm.fast_len_11(n)
    # a window long enough for nfft != 8192: L = 8193 -> 8232
    win, pre = mdc.analysis_lengths(48000, window_ms=8193 / 48.0 - 0.5, pre_ms=0.5)
    start, end, nfft = mdc.segment_bounds(20000, 5000, win, pre)
    assert end - start == win + pre and nfft == next_fast_len(max(end - start, 8192))
    s, e, nf = mdc.segment_bounds(30000, 100, 8193 - 10, 10)
    assert (e - s, nf) == (8193, 8232)
    # the peak is clipped into the row; pre counts from the peak, not from what the row holds before it
    assert mdc.segment_bounds(100, 500, 240, 24)[:2] == (75, 100)
    assert mdc.segment_bounds(100, -3, 240, 24)[:2] == (0, 100)


@pytest.mark.parametrize("bad, why", [
    ({"strength": 0.7}, "unknown options"),
    ({"correction_strength": "0.7"}, "finite number"),
    ({"correction_strength": True}, "finite number"),
    ({"correction_strength": float("nan")}, "finite number"),
    ({"anchor": 3}, "anchor must be a string"),
    ([("correction_strength", 0.7)], "must be None or a dict"),
])
def test_run_slice_refuses_bad_mic_deviation_before_device_work(bad, why):
    from impulse_hip.pipeline_slice import run_slice

    class Untouchable:                                    # any use of the estimator would be device work
        def __getattr__(self, name):
            raise AssertionError(f"estimator touched: {name}")

    with pytest.raises(ValueError, match=why):
        run_slice(Untouchable(), [], mic_deviation=bad)


def test_new_abi_names_are_declared_bound_and_exported():
    from impulse_hip import _native
    header = open(os.path.join(ROOT, "include", "impulse_hip.h")).read()
    for name in ("imp_mic_mismatch_device", "imp_mic_mismatch"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _native.SIGNATURES
    lib = os.path.join(ROOT, "impulcifer-pip313_amd", "csrc", "libimpulse_hip.so")
    if os.path.exists(lib):
        import ctypes
        so = ctypes.CDLL(lib)
        assert hasattr(so, "imp_mic_mismatch_device") and hasattr(so, "imp_mic_mismatch")


def test_model_anchor_rule():
    assert mm.anchors(["FL", "FR", "FC"], "auto") == (["FC"], "frontal")
    assert mm.anchors(["FL", "FR", "TFC", "BC"], "frontal") == (["TFC", "BC"], "frontal")
    assert mm.anchors(["FL", "FR", "FC"], "diffuse") == (["FL", "FR", "FC"], "diffuse")
    assert mm.anchors(["FL", "FR"], "auto") == (["FL", "FR"], "diffuse")
    assert mm.anchors(["FL", "FC"], "something") == (["FL", "FC"], "diffuse")
    from impulse_hip.microphone_deviation_correction import anchor_flags
    assert anchor_flags(["FL", "FR", "FC"], "auto") == ([False, False, True], "frontal")
    assert anchor_flags(["FL", "FR"], "frontal") == ([True, True], "diffuse")
    assert anchor_flags(["FL", "FC"], None) == ([True, True], "diffuse")
