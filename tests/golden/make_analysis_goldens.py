"""Generate tests/golden/analysis.npz by RUNNING the reference's binaural analysis functions (core/plotting/analysis.py,
loaded by file path: the package's __init__ imports the plot mixins) on the seeded inputs of tests/golden/analysis_inputs.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_analysis_goldens.py /path/to/reference

Data only, per case and pair: the band list, the three band sums, ILD, IPD, lags_ms, iacf, IACC, tau and both decay curves
(decimated, with their first and last samples); octave_bands at the five rates and for custom centres.  The conditions the
tests rely on are asserted here, so a fixture that violates them cannot be written.
"""
import importlib.util
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

import analysis_inputs as ai  # noqa: E402

RATES = (22050, 44100, 48000, 96000, 192000)
CUSTOM_CENTERS = (63, 500, 4000, 20000, 40000)


def load_reference(root):
    spec = importlib.util.spec_from_file_location("reference_analysis", os.path.join(root, "core", "plotting", "analysis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IMPULCIFER_REFERENCE", "."))
    out = {}
    for fs in RATES:
        out[f"octave_bands/{fs}"] = np.array(ref.octave_bands(fs), dtype=np.float64).reshape(-1, 2)
        out[f"octave_bands_custom/{fs}"] = np.array(ref.octave_bands(fs, CUSTOM_CENTERS), dtype=np.float64).reshape(-1, 2)
    n_bands = n_low = 0
    for name in ai.CASES:
        fs, pairs, bands, max_delay_ms = ai.case(name)
        bands = ref.octave_bands(fs) if bands is None else bands
        for k, (left, right) in enumerate(pairs):
            p = f"{name}/{k}/"
            sums = ref._band_cross_spectra(left, right, fs, bands)
            out[p + "bands"] = np.array(bands, dtype=np.float64).reshape(-1, 2)
            out[p + "power_l"] = np.array([s[0] for s in sums], dtype=np.float64)
            out[p + "power_r"] = np.array([s[1] for s in sums], dtype=np.float64)
            out[p + "cross"] = np.array([s[2] for s in sums], dtype=np.complex128)
            out[p + "ild_db"] = np.array(ref.band_interaural_level_difference(left, right, fs, bands), dtype=np.float64)
            out[p + "ipd_deg"] = np.array(ref.band_interaural_phase_difference(left, right, fs, bands), dtype=np.float64)
            lags_ms, iacf, iacc, tau = ref.interaural_cross_correlation(left, right, fs, max_delay_ms)
            out[p + "lags_ms"], out[p + "iacf"] = np.asarray(lags_ms, dtype=np.float64), np.asarray(iacf, dtype=np.float64)
            out[p + "iacc"], out[p + "tau_ms"] = np.float64(iacc), np.float64(tau)
            for side, x in (("left", left), ("right", right)):
                curve = ref.energy_decay_curve_db(x)
                out[p + f"edc_{side}_decim"] = curve[::ai.EDC_DECIM]
                out[p + f"edc_{side}_head"] = curve[:ai.EDC_EDGE]
                out[p + f"edc_{side}_tail"] = curve[-ai.EDC_EDGE:]
                out[p + f"edc_{side}_len"] = np.int64(len(curve))
            # ---- the conditions
            mags = np.sort(np.abs(iacf))
            if len(mags) >= 2:
                assert mags[-1] - mags[-2] > ai.GAP_MIN, (name, k, mags[-1] - mags[-2])
            live = ~np.isnan(out[p + "power_l"])
            coh = np.abs(out[p + "cross"][live]) / np.sqrt(out[p + "power_l"][live] * out[p + "power_r"][live])
            low = int(np.sum(~(coh >= ai.COHERENCE_MIN)))
            if name == "hrir71_48k":
                assert low == 0, (name, k, coh)
            n_bands += int(np.sum(live))
            n_low += low
            print(name, k, len(left), len(right), "iacc %.6f tau %.4f" % (iacc, tau), "min coherence", coh.min() if len(coh) else None)
    assert n_low * 8 <= n_bands, (n_low, n_bands)
    path = os.path.join(OUT, "analysis.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", n_low, "of", n_bands, "bands under the coherence threshold")


if __name__ == "__main__":
    main()
