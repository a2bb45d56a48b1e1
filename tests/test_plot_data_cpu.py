"""Plot data without a GPU: spectrogram_geometry against the reference-run fixture (plot_data.npz) and branch by branch,
the axes against SciPy, the NumPy model of K16 against the fixture (which measures e_ref), the waterfall's host finishing
against the fixture, and the new C ABI names."""
import os
import re

import numpy as np
import pytest

import plot_data_inputs as pdi
import plot_data_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The reference's own rounding error: the largest difference between the fixture and the model in np.longdouble over all
# cases (spectrogram in dB, STFT magnitudes relative to the row's largest, finished waterfall in dB).
E_REF_SPEC_DB = 6.55e-13
E_REF_MAGNITUDE = 2.70e-16
E_REF_WATERFALL_DB = 4.37e-12


def _spec_rows():
    for name in pdi.SPEC_CASES:
        fs, f_res, n_segments, rows = pdi.spec_case(name)
        for k, x in enumerate(rows):
            yield name, k, fs, f_res, n_segments, x


def test_geometry_equals_the_reference_for_every_case(golden):
    from impulse_hip.plot_data import spectrogram_axes, spectrogram_geometry
    z = golden("plot_data")
    hops = {}
    for name, k, fs, f_res, n_segments, x in _spec_rows():
        p = f"spec/{name}/{k}/"
        geo = spectrogram_geometry(len(x), fs, f_res, n_segments)
        assert geo == tuple(int(v) for v in z[p + "geometry"]), (name, k, geo)
        nfft, noverlap = geo
        S = (len(x) - noverlap) // (nfft - noverlap)
        assert (nfft // 2, S) == tuple(int(v) for v in z[p + "shape"]), (name, k)
        f, t = spectrogram_axes(len(x), fs, nfft, noverlap)
        assert np.array_equal(f, z[p + "f"]) and np.array_equal(t, z[p + "t"]), (name, k)
        hops.setdefault(name, []).append((nfft, nfft - noverlap, S))
    # what the cases are there for
    assert hops["fs8000"] == [(800, 21, 201), (800, 21, 200), (800, 21, 196)]          # one call, odd and even S
    assert hops["fs22050"] == [(2205, 49, 201), (2205, 49, 200)]
    assert hops["fs48000"] == [(4800, 76, 201), (4800, 76, 200)]
    assert hops["short"] == [(250, 2, 126)] and hops["clip3"] == [(600, 3, 201)]
    assert hops["step_le_1"] == [(150, 75, 3)] and hops["nseg0"] == [(800, 400, 11)]
    assert hops["f_res20"][0][:2] != hops["f_res20"][1][:2]                            # two geometries in one request
    fs, n, nfft = pdi.UNSUPPORTED
    assert spectrogram_geometry(n, fs) == tuple(int(v) for v in z["unsupported/geometry"]) and spectrogram_geometry(n, fs)[0] == nfft


def test_geometry_branches():
    from impulse_hip.plot_data import spectrogram_geometry as g
    assert g(0, 48000) is None                                         # empty recording
    assert g(100, 4, f_res=10) is None                                 # round(fs / f_res) = 0
    assert g(391270, 48000) == (4800, 2867)                            # C2: step 1932.35, 200 segments
    assert (391270 - 2867) // (4800 - 2867) == 200
    assert g(1, 48000) == (1, 0) and g(3, 48000) == (1, 0)             # 2 n // 4 = 0 -> len; then nfft = 1
    assert g(4, 48000) == (2, 1)                                       # step 0.01 -> 50 %
    assert g(6000, 48000) == (3000, 2985)                              # clipped to 2 n // 4; step 15
    assert g(800, 8000) == (400, 398)                                  # step 2
    assert g(5000, 8000, n_segments=-3) == (800, 400)
    assert g(5000, 8000, n_segments=100000) == (800, 400)              # step 0.042
    assert g(5000, 8000, f_res=4000) == (2, 0)                         # int(2 - 24.99) < 0 -> 0
    for fs, nfft in ((22050, 2205), (44100, 4410), (48000, 4800), (88200, 8820), (96000, 9600), (176400, 17640), (192000, 19200)):
        assert g(10 * fs, fs)[0] == nfft


def test_axes_equal_scipy():
    from scipy import signal
    from impulse_hip.plot_data import spectrogram_axes, spectrogram_geometry
    for name in ("fs8000", "fs22050", "short", "step_le_1", "nseg0"):
        fs, f_res, n_segments, rows = pdi.spec_case(name)
        x = rows[0]
        nfft, noverlap = spectrogram_geometry(len(x), fs, f_res, n_segments)
        f, t, s = signal.spectrogram(x, fs=fs, window=signal.get_window("hann", nfft), nperseg=nfft, noverlap=noverlap, mode="psd")
        got_f, got_t = spectrogram_axes(len(x), fs, nfft, noverlap)
        assert np.array_equal(got_f, f[1:]) and np.array_equal(got_t, t) and s.shape == (len(f), len(t))


def test_model_within_e_ref_of_the_fixture(golden):
    z = golden("plot_data")
    worst = dict(spec=0.0, mag=0.0, wf=0.0)
    for name, k, fs, f_res, n_segments, x in _spec_rows():
        p = f"spec/{name}/{k}/"
        nfft, noverlap = (int(v) for v in z[p + "geometry"])
        m = pm.spectrogram_db(x, fs, nfft, noverlap)
        assert m.shape == tuple(z[p + "shape"])
        worst["spec"] = max(worst["spec"], float(np.max(np.abs(m[:, z[p + "cols"]] - z[p + "z"]))))
    for name in pdi.WF_CASES:
        fs, x = pdi.wf_case(name)
        mag, zz = pm.waterfall(x, fs)
        worst["mag"] = max(worst["mag"], float(np.max(np.abs(mag - z[f"wf/{name}/magnitude"])) / np.max(mag)))
        worst["wf"] = max(worst["wf"], float(np.max(np.abs(zz - z[f"wf/{name}/z"]))))
    print("e_ref", worst)
    assert worst["spec"] <= E_REF_SPEC_DB and worst["mag"] <= E_REF_MAGNITUDE and worst["wf"] <= E_REF_WATERFALL_DB
    # the constants are the measurement, not a bound with slack
    assert worst["spec"] > 0.9 * E_REF_SPEC_DB and worst["mag"] > 0.9 * E_REF_MAGNITUDE and worst["wf"] > 0.9 * E_REF_WATERFALL_DB


def test_silent_row_and_detrend_in_the_fixture(golden):
    z = golden("plot_data")
    assert np.all(z["spec/fs8000/2/z"] == 10 * np.log10(1e-9))         # the silent row
    # the drifting row: without the mean removed its lowest bins would carry the offset (about -30 dB); with it they do not
    fs, f_res, n_segments, rows = pdi.spec_case("fs8000")
    nfft, noverlap = (int(v) for v in z["spec/fs8000/1/geometry"])
    x = rows[1]
    seg = x[:nfft] * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(nfft) / nfft))
    raw = 10 * np.log10(2 * np.abs(np.fft.rfft(seg)[1]) ** 2 / (fs * 0.375 * nfft) + 1e-9)
    assert raw - z["spec/fs8000/1/z"][0, 0] > 3.0, (raw, z["spec/fs8000/1/z"][0, 0])


def test_waterfall_finishing_equals_the_reference(golden):
    from impulse_hip.plot_data import WATERFALL_SAMPLES, waterfall_finish
    z = golden("plot_data")
    assert WATERFALL_SAMPLES == 1792
    sizes = {}
    for name in pdi.WF_CASES:
        fs = pdi.WF_CASES[name][0]
        t_ms, log10_f, z_db = waterfall_finish(z[f"wf/{name}/magnitude"], fs)
        assert np.array_equal(t_ms, z[f"wf/{name}/t_ms"]) and np.array_equal(log10_f, z[f"wf/{name}/log10_f"])
        assert np.array_equal(z_db, z[f"wf/{name}/z"])
        sizes[name] = z_db.shape
    assert sizes["long48k"] == sizes["short48k"] == (261, 12) and sizes["fs96000"][0] > 261


def test_abi_names():
    from impulse_hip import _native
    text = open(os.path.join(ROOT, "include", "impulse_hip.h")).read()
    for name in ("imp_stft_db_device", "imp_stft_db"):
        assert name in _native.SIGNATURES
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert (_native.STFT_PSD_DB, _native.STFT_MAGNITUDE) == (0, 1)
    assert re.search(r"#define\s+IMP_STFT_PSD_DB\s+0", text) and re.search(r"#define\s+IMP_STFT_MAGNITUDE\s+1", text)
