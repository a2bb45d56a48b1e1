"""Generate tests/golden/curves_edges.npz by RUNNING the reference's own FrequencyResponse (autoeq/frequency_response.py:
_smoothen_fractional_octave, smoothen_heavy_light, equalize) on the grids and curves of tests/golden/curves_inputs.py:

    PYTHONPATH=/path/to/reference PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_curves_goldens.py

Recorded results only, float64.  Per grid G: the window sizes, the smoothing of the plain walk for every window pair, and
per curve C
    G/C/eq_raw, G/C/keep_raw        equalize() on the curve as it is (error_smoothed empty), and which samples it kept
    G/C/es, G/C/eq_sm, G/C/keep_sm  smoothen_heavy_light() then equalize() (the curves curves_inputs.smoothed_names lists)
    G/C/raises                      1 where equalize() raised because fewer than 3 samples survived (nothing else recorded)
The kept samples are read off the abscissae the reference hands to InterpolatedUnivariateSpline (its name in the reference's
module is wrapped by a recorder for the run).  The conditions the tests rely on are asserted here, so a fixture that
violates them cannot be written.  The archive is written with fixed member timestamps: it regenerates byte for byte.
"""
import io
import os
import sys
import zipfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

import curves_inputs as ci  # noqa: E402
import make_goldens  # noqa: E402


def save_npz(path, arrays):
    """np.savez_compressed with a fixed timestamp per member (NumPy stamps the time of writing)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    if make_goldens.REF not in sys.path:
        sys.path.insert(0, make_goldens.REF)
    make_goldens._install_stubs()
    import autoeq.frequency_response as ref
    FrequencyResponse = ref.FrequencyResponse

    seen = []
    spline = ref.InterpolatedUnivariateSpline

    def recording_spline(x, y, **kw):
        seen.append(np.array(x, dtype=np.float64))
        return spline(x, y, **kw)

    ref.InterpolatedUnivariateSpline = recording_spline

    def equalize(fr, freq):
        """(equalization, keep mask) or (None, None) where the reference raises for want of points"""
        seen.clear()
        try:
            fr.equalize(**ci.EQ_ARGS)
        except Exception as exc:                                   # noqa: BLE001 - dfitpack.error: m > k must hold
            assert "m>k" in str(exc).replace(" ", ""), exc
            return None, None
        assert len(seen) == 1
        keep = np.isin(np.log10(freq), seen[0])
        assert int(keep.sum()) == len(seen[0])
        return np.asarray(fr.equalization, dtype=np.float64), keep

    out = {}
    for g, (_, n_want, windows_want) in ci.GRIDS.items():
        freq = ci.grid(g)
        n, kh = len(freq), ci.kink_half(g)
        probe = FrequencyResponse(name="g", frequency=freq.copy(), raw=0)
        windows = tuple(probe._window_size(o) for o in ci.OCTAVES)
        assert n_want is None or n == n_want, (g, n)
        assert windows_want is None or windows == windows_want, (g, windows)
        assert windows == tuple(ci.window_size(freq, o) for o in ci.OCTAVES) and kh == (windows[0] - 1) // 2
        assert 8 <= n <= 2048
        out[f"{g}/windows"] = np.array(windows, dtype=np.int64)
        walk = ci.walk(g)
        for k, (wn, wt, fl, fu) in enumerate(ci.smoothing_pairs(g)):
            out[f"{g}/smooth{k}"] = np.asarray(probe._smoothen_fractional_octave(
                walk.copy(), window_size=wn, iterations=1, treble_window_size=wt, treble_iterations=1, treble_f_lower=fl,
                treble_f_upper=fu), dtype=np.float64)
        for c in ci.CURVES:
            err = ci.curve(g, c)
            p = f"{g}/{c}/"
            fr = FrequencyResponse(name=c, frequency=freq.copy(), raw=0, error=err.copy())
            eq, keep = equalize(fr, freq)                          # every curve is run and checked; raw_names are recorded
            keep_raw = keep
            # ---- the conditions, on the unsmoothed path
            if ci.too_few(g, c):
                assert eq is None, (g, c)
                if c in ci.raw_names(g):
                    out[p + "raises"] = np.int64(1)
            else:
                assert eq is not None and keep.sum() >= 3, (g, c)
                assert bool(keep[0]) != ci.drops_first(g, c), (g, c, keep[:12])
                assert keep[-2:].all()
                t = ci.first_transition(g, c)
                left = int(np.argmax(keep))                        # points before the first kept one: extrapolated
                if left:
                    # a left run exists only for a transition t <= kh and ends kh points past it
                    assert t is not None and t <= kh and left == t + kh + 1 <= 2 * kh + 1, (g, c, left, t, kh)
                if c in ci.raw_names(g):
                    out[p + "eq_raw"], out[p + "keep_raw"] = eq, keep.astype(np.uint8)
            if c in ci.smoothed_names(g):
                fr = FrequencyResponse(name=c, frequency=freq.copy(), raw=0, error=err.copy())
                fr.smoothen_heavy_light()
                es = np.asarray(fr.error_smoothed, dtype=np.float64).copy()
                eq, keep = equalize(fr, freq)
                assert eq is not None and keep.sum() >= 3 and keep[-2:].all(), (g, c)
                out[p + "es"], out[p + "eq_sm"], out[p + "keep_sm"] = es, eq, keep.astype(np.uint8)
            print(g, c, "kh", kh, "kept raw", None if keep_raw is None else int(keep_raw.sum()),
                  "kept smoothed", int(out[p + "keep_sm"].sum()) if p + "keep_sm" in out else None)
        # the pairs: a transition at exactly kink_half drops the first point, one sample later keeps it
        if kh >= 1:
            assert ci.drops_first(g, "first1") and ci.drops_first(g, "trans_at_kh") and not ci.drops_first(g, "trans_at_kh1")
            assert ci.drops_first(g, "comb")
        else:
            assert not any(ci.drops_first(g, c) for c in ci.CURVES)
    ref.InterpolatedUnivariateSpline = spline
    path = os.path.join(OUT, "curves_edges.npz")
    save_npz(path + ".tmp", out)
    size = os.path.getsize(path + ".tmp")
    assert size <= 1 << 20, size
    os.replace(path + ".tmp", path)
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
