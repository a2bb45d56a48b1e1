"""K12 (csrc/curves.hip) away from the product's grid: seven grids from 160 to 2048 points, curves whose clipping reaches
the first and the last samples, the limits of the grid size and of the windows, batches, the handle cache and the curve
that leaves too few points for a spline.  The referee is SciPy itself, written out below as the reference calls it
(scipy.signal.savgol_filter blended by scipy.special.expit; InterpolatedUnivariateSpline(k=2)), and the reference-run
fixture curves_edges.npz (tests/golden/make_curves_goldens.py) wherever it has a record.

Tolerances.  The project's numbers hold where the operation is the same: CURVE_TOL = 1e-12 dB for smoothing, clipping
and the gain grid, SPLINE_TOL = 1e-10 dB for the spline, applied as |got - want| <= tol * max(1, max |want|) (points
extrapolated beyond the first kept sample can be large).  SciPy's own fp64 rounding grows with the window (its edge fit
is np.polyfit over 0 .. w-1, uncentred), so it was measured: SciPy fp64 against the same operators in np.longdouble
(tests/model/curves_model.py) over every grid and curve of curves_inputs.py, as the same relative figure.  E_REF below
holds the measured values; test_scipy_rounding_stays_within_e_ref re-measures them on the CPU.  Where a measured value
exceeds the project's number the tolerance is 10 x the measured value (the margin DESIGN.md section 12 uses for K15):
that is the case for one entry, smoothen_heavy_light on the 2048-point grid (w = 237).  Nothing here comes from the
kernel's output.

    grid              n     windows          smooth     heavy-light  spline
    step1.05          160   1 3 5 19         2.15e-15   4.01e-15     1.14e-14
    step1.02          394   3 7 13 47        1.68e-14   2.13e-14     1.17e-14
    step1.01          783   7 13 23 91       1.03e-13   1.08e-13     2.20e-14
    step1.005         1561  13 23 47 181     7.75e-13   8.67e-13     3.91e-14
    geom2048          2048  15 31 61 237     7.93e-13   1.26e-12     3.00e-14
    step1.01_20_20k   695   7 13 23 91       1.03e-13   1.07e-13     6.26e-14
    jitter1.01        784   7 13 23 91       4.93e-14   1.14e-13     1.70e-14
"""
import numpy as np
import pytest

import curves_inputs as ci
import curves_model as cm

CURVE_TOL = 1e-12          # dB: smoothing, clipping, gain grid (the project's number, tests/test_hip_parity.py)
SPLINE_TOL = 1e-10         # dB: the kink-bridging spline (the project's number)
# measured: SciPy fp64 against np.longdouble, max |d| / max(1, max |want|), rounded up in the third digit
E_REF = {
    "step1.05": dict(smooth=2.2e-15, es=4.1e-15, spline=1.2e-14),
    "step1.02": dict(smooth=1.7e-14, es=2.2e-14, spline=1.2e-14),
    "step1.01": dict(smooth=1.1e-13, es=1.1e-13, spline=2.3e-14),
    "step1.005": dict(smooth=7.8e-13, es=8.7e-13, spline=4.0e-14),
    "geom2048": dict(smooth=8.0e-13, es=1.26e-12, spline=3.1e-14),
    "step1.01_20_20k": dict(smooth=1.1e-13, es=1.1e-13, spline=6.3e-14),
    "jitter1.01": dict(smooth=5.0e-14, es=1.2e-13, spline=1.8e-14),
}
# w = 3 is the identity: interior taps are exactly (0, 1, 0); an edge row is (1, 0, 0) to a few ulp per entry (three
# products of O(1) quotients), and the blend x (1 - k) + x k adds two roundings: 16 ulp of the largest sample covers it
IDENTITY_TOL = 16 * np.finfo(np.float64).eps
GRID_NAMES = tuple(ci.GRIDS)


def tol(grid_name, quantity):
    project = SPLINE_TOL if quantity == "spline" else CURVE_TOL
    e = E_REF[grid_name][quantity]
    return 10 * e if e > project else project


# ------------------------------------------------------------------ the reference's steps, with SciPy itself
def sigmoid(f, f_lower, f_upper, a_normal=0.0, a_treble=1.0):
    from scipy.special import expit
    f_center = np.sqrt(f_upper / f_lower) * f_lower
    half_range = np.log10(f_upper) - np.log10(f_center)
    a = expit((np.log10(f) - np.log10(f_center)) / (half_range / 4))
    return a * -(a_normal - a_treble) + a_normal


def smooth(f, x, wn, wt, f_lower, f_upper):
    """autoeq _smoothen_fractional_octave with the windows in grid points"""
    from scipy.signal import savgol_filter
    k = sigmoid(f, f_lower, f_upper)
    return savgol_filter(x, wn, 2) * (k * -1 + 1) + savgol_filter(x, wt, 2) * k


def heavy_light(f, x, w6, w3, w130):
    light = smooth(f, x, w6, w3, 100, 10000)
    heavy = smooth(f, x, w3, w130, 1000, 6000)
    return smooth(f, np.max(np.vstack([light, heavy]), axis=0), w3, w3, 100, 10000)


def equalize(f, es, kh, max_gain, treble_f_lower, treble_f_upper, treble_max_gain, treble_gain_k):
    """autoeq equalize: (equalization, keep mask)"""
    from scipy.interpolate import InterpolatedUnivariateSpline
    limit = sigmoid(f, treble_f_lower, treble_f_upper, max_gain, treble_max_gain)
    gain = -es * sigmoid(f, treble_f_lower, treble_f_upper, 1.0, treble_gain_k)
    clipped = gain > limit
    eq = np.where(clipped, limit, gain)
    n = len(f)
    keep = np.ones(n, dtype=bool)
    for i in np.flatnonzero(clipped[1:] != clipped[:-1]) + 1:
        keep[i - min(i, kh):i + 1 + min(n - i - 1, kh)] = False
    keep[n - 2:] = True
    x = np.log10(f)
    return InterpolatedUnivariateSpline(x[keep], eq[keep], k=2)(x), keep


def windows_of(grid_name):
    f = ci.grid(grid_name)
    return [ci.window_size(f, o) for o in ci.OCTAVES]


def smoothing_inputs(grid_name):
    return np.stack([ci.walk(grid_name), ci.curve(grid_name, "comb")])


def live_curves(grid_name):
    return [c for c in ci.CURVES if not ci.too_few(grid_name, c)]


_scipy_cache = {}


def scipy_chain(grid_name, smoothen_first):
    """{curve: (es, eq, keep)} with SciPy, computed once per grid and path and left unchanged"""
    key = (grid_name, smoothen_first)
    if key not in _scipy_cache:
        f, w, kh = ci.grid(grid_name), windows_of(grid_name), ci.kink_half(grid_name)
        out = {}
        for c in live_curves(grid_name):
            es = ci.curve(grid_name, c)
            if smoothen_first:
                es = heavy_light(f, es, *w[1:])
            eq, keep = equalize(f, es, kh, **ci.EQ_ARGS)
            for a in (es, eq, keep):
                a.setflags(write=False)
            out[c] = (es, eq, keep)
        _scipy_cache[key] = out
    return _scipy_cache[key]


# ------------------------------------------------------------------ CPU: what the tolerances assume
@pytest.mark.parametrize("grid_name", GRID_NAMES)
def test_scipy_rounding_stays_within_e_ref(grid_name):
    """SciPy fp64 against the long-double operators over every input the GPU tests use: no figure above E_REF, and E_REF
    is not padded (the largest figure of a grid is at least half its entry)."""
    f, w, kh = ci.grid(grid_name), windows_of(grid_name), ci.kink_half(grid_name)
    fig = dict(smooth=0.0, es=0.0, spline=0.0)
    for x in smoothing_inputs(grid_name):
        for on, ot, fl, fu in ci.smoothing_pairs(grid_name):
            wn, wt = ci.window_size(f, on), ci.window_size(f, ot)
            fig["smooth"] = max(fig["smooth"], cm.rel_err(smooth(f, x, wn, wt, fl, fu), cm.smooth(f, x, wn, wt, fl, fu)))
    for smoothen_first in (True, False):
        for c, (es, eq, keep) in scipy_chain(grid_name, smoothen_first).items():
            if smoothen_first:
                fig["es"] = max(fig["es"], cm.rel_err(es, cm.heavy_light(f, ci.curve(grid_name, c), *w[1:])))
            fig["spline"] = max(fig["spline"], cm.rel_err(eq, cm.equalize(f, es, keep, **ci.EQ_ARGS)))
    print(grid_name, {k: f"{v:.2e}" for k, v in fig.items()})
    for k, v in fig.items():
        assert 0.5 * E_REF[grid_name][k] <= v <= E_REF[grid_name][k], (k, v)


def test_fixture_agrees_with_the_steps_written_here(golden):
    """The reference run and the SciPy steps above are the same computation: identical kept samples, curves equal to
    SciPy's rounding (they call the same routines; only the order of a few blends could differ)."""
    z = golden("curves_edges")
    for g in GRID_NAMES:
        assert tuple(z[f"{g}/windows"]) == tuple(windows_of(g))
        for smoothen_first, eq_key, keep_key in ((False, "eq_raw", "keep_raw"), (True, "eq_sm", "keep_sm")):
            for c, (es, eq, keep) in scipy_chain(g, smoothen_first).items():
                p = f"{g}/{c}/"
                if p + eq_key in z:
                    assert np.array_equal(z[p + keep_key].astype(bool), keep), (g, c)
                    assert cm.rel_err(eq, z[p + eq_key]) <= tol(g, "spline"), (g, c)
                    if smoothen_first:
                        assert cm.rel_err(es, z[p + "es"]) <= tol(g, "es"), (g, c)
        for c in ci.CURVES:
            assert (f"{g}/{c}/raises" in z) == (ci.too_few(g, c) and c in ci.raw_names(g))


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("grid_name", GRID_NAMES)
def test_smoothing_matches_scipy_for_every_window(gpu_ctx, golden, grid_name):
    from impulse_hip.frequency_response import curves_for, smooth_curves
    z = golden("curves_edges")
    f, x = ci.grid(grid_name), smoothing_inputs(grid_name)
    h = curves_for(f)
    octaves = [o for o in ci.OCTAVES if ci.window_size(f, o) >= 3]
    assert [h.window_size(o) for o in ci.OCTAVES] == windows_of(grid_name)
    worst, used = 0.0, set()
    for k, (on, ot, fl, fu) in enumerate(ci.smoothing_pairs(grid_name)):
        wn, wt = ci.window_size(f, on), ci.window_size(f, ot)
        used |= {wn, wt}
        got = smooth_curves(f, x, on, ot, fl, fu)
        for b in range(len(x)):
            worst = max(worst, cm.rel_err(got[b], smooth(f, x[b], wn, wt, fl, fu)))
        worst = max(worst, cm.rel_err(got[0], z[f"{grid_name}/smooth{k}"]))
    assert used == {ci.window_size(f, o) for o in octaves}
    print(f"{grid_name}: smoothing vs SciPy and the fixture {worst:.2e} (tolerance {tol(grid_name, 'smooth'):.2e})")
    assert worst <= tol(grid_name, "smooth")
    for o in octaves:
        if ci.window_size(f, o) == 3:                               # the identity operator
            got = smooth_curves(f, x, o, o, 100, 10000)
            assert np.max(np.abs(got - x)) <= IDENTITY_TOL * np.max(np.abs(x))


@pytest.mark.gpu
@pytest.mark.parametrize("smoothen_first", (False, True))
@pytest.mark.parametrize("grid_name", GRID_NAMES)
def test_equalization_matches_scipy_and_the_reference_run(gpu_ctx, golden, grid_name, smoothen_first):
    """Every curve of the grid in one launch.  On step1.05 the smoothed path works because its 1/6-octave window is 3."""
    from impulse_hip.frequency_response import curves_for
    z = golden("curves_edges")
    f = ci.grid(grid_name)
    want = scipy_chain(grid_name, smoothen_first)
    names = list(want)
    errors = np.stack([ci.curve(grid_name, c) for c in names])
    assert len(names) <= 32
    es, eq, used = curves_for(f).equalization(errors, smoothen_first, **ci.EQ_ARGS)
    fig = dict(es=0.0, spline=0.0, es_fixture=0.0, spline_fixture=0.0)
    for b, c in enumerate(names):
        w_es, w_eq, keep = want[c]
        assert int(used[b]) == int(not keep.all()), (c, used[b])
        if smoothen_first:
            fig["es"] = max(fig["es"], cm.rel_err(es[b], w_es))
        else:
            assert np.array_equal(es[b], errors[b])
        fig["spline"] = max(fig["spline"], cm.rel_err(eq[b], w_eq))
        p = f"{grid_name}/{c}/"
        if p + ("eq_sm" if smoothen_first else "eq_raw") in z:
            assert int(used[b]) == int(not z[p + ("keep_sm" if smoothen_first else "keep_raw")].all())
            fig["spline_fixture"] = max(fig["spline_fixture"], cm.rel_err(eq[b], z[p + ("eq_sm" if smoothen_first else "eq_raw")]))
            if smoothen_first:
                fig["es_fixture"] = max(fig["es_fixture"], cm.rel_err(es[b], z[p + "es"]))
    print(grid_name, smoothen_first, {k: f"{v:.2e}" for k, v in fig.items()})
    assert max(fig["es"], fig["es_fixture"]) <= tol(grid_name, "es")
    assert max(fig["spline"], fig["spline_fixture"]) <= tol(grid_name, "spline")


@pytest.mark.gpu
@pytest.mark.parametrize("normalize", (False, True))                 # several tiles per curve / one
@pytest.mark.parametrize("f_res", (5, 50))                           # 50: f_min = 25 Hz > frequency[0]
@pytest.mark.parametrize("fs", (44100, 48000))
@pytest.mark.parametrize("grid_name", ("step1.05", "step1.01_20_20k", "jitter1.01"))
def test_gain_grid_matches_log_interp(gpu_ctx, golden, grid_name, fs, f_res, normalize):
    from impulse_hip.frequency_response import curves_for, fir_design_gain
    from oracle.impulse_response import interpolate_log
    from oracle.scipy_restated import next_fast_len_real
    f = ci.grid(grid_name)
    curves = np.stack([ci.walk(grid_name), golden("curves_edges")[f"{grid_name}/comb/eq_raw"]])
    got = fir_design_gain(f, curves, fs, f_res, normalize)
    ntaps = next_fast_len_real(round(fs // 2 / (f_res / 2)))
    assert got.shape == (2, ntaps) and curves_for(f).fir_taps(fs, f_res) == ntaps
    fq = np.linspace(0.0, fs // 2, ntaps)
    f_min = max(f[0], f_res / 2)
    assert (f_min > f[0]) == (f_res == 50)
    if grid_name == "step1.01_20_20k":                              # the design grid leaves the curve's grid at both ends
        assert fq[0] < f[0] and fq[-1] > f[-1]
    for b in range(2):
        with np.errstate(divide="ignore", invalid="ignore"):
            raw = interpolate_log(f, curves[b], fq)
        raw[fq <= f_min] = interpolate_log(f, curves[b], np.array([f_min]))[0]
        if normalize:
            raw -= np.max(raw)
            raw -= 0.5
        want = 10 ** (raw * 2 / 20)
        want[-1] = 0.0
        assert np.max(np.abs(got[b] - want) / np.maximum(want, 1e-300)) <= CURVE_TOL


@pytest.mark.gpu
def test_limits_of_the_grid_and_of_the_windows(gpu_ctx):
    from impulse_hip import _native
    from impulse_hip.frequency_response import curves_for, equalization_curves, smooth_curves
    ctx = _native.default_context()
    assert curves_for(ci.grid("geom2048")).n == 2048
    for n in (2049, 7):
        with pytest.raises(Exception, match=r"8 \.\. 2048 supported"):
            _native.Curves(ctx, np.geomspace(10, 24000, n))
    f12 = 10 * 1.05 ** np.arange(12)                               # 1.3 octaves are 19 points here
    with pytest.raises(Exception, match="does not fit a grid of 12 points"):
        smooth_curves(f12, np.zeros(12), 1 / 3, 1.3)
    f11 = 10 * 1.1 ** np.arange(82)                                # step 1.1: the 1/6-octave window is 1 point
    assert ci.window_size(f11, 1 / 6) == 1 and ci.window_size(f11, 1 / 12) == 1
    err = 3 * np.sin(np.arange(82) / 5.0)
    err[30:34] -= 70.0
    with pytest.raises(Exception, match="smoothing window of 1 points"):
        equalization_curves(f11, err, smoothen_first=True, **ci.EQ_ARGS)
    # equalize() alone needs no smoothing window: kink_half = 0 on this grid
    _, eq = equalization_curves(f11, err, smoothen_first=False, **ci.EQ_ARGS)
    want, keep = equalize(f11, err, 0, **ci.EQ_ARGS)
    assert keep.sum() == 80 and cm.rel_err(eq, want) <= SPLINE_TOL


@pytest.mark.gpu
def test_batches_regrow_and_reuse_the_work_buffers(gpu_ctx):
    """B = 1, then 27, then 3 on one fresh handle: every row bit-identical to its own B = 1 call."""
    from impulse_hip import _native
    g = "step1.01"
    f, names = ci.grid(g), live_curves(g)
    rows = np.stack([ci.curve(g, names[i % len(names)]) + 0.125 * (i // len(names)) for i in range(27)])
    h = _native.Curves(_native.default_context(), f)
    try:
        got = {}
        for sel in (slice(5, 6), slice(0, 27), slice(11, 14)):
            got[sel.start] = (sel, h.smooth(rows[sel], 1 / 6, 1.3, 1000, 6000),
                              h.equalization(rows[sel], True, **ci.EQ_ARGS), h.equalization(rows[sel], False, **ci.EQ_ARGS))
        for sel, sm, eq_s, eq_r in got.values():
            for k, b in enumerate(range(sel.start, sel.stop)):
                assert np.array_equal(sm[k], h.smooth(rows[b], 1 / 6, 1.3, 1000, 6000))
                for batch, first in ((eq_s, True), (eq_r, False)):
                    es1, eq1, used1 = h.equalization(rows[b], first, **ci.EQ_ARGS)
                    assert np.array_equal(batch[0][k], es1) and np.array_equal(batch[1][k], eq1) and batch[2][k] == used1[0]
    finally:
        h.close()


@pytest.mark.gpu
def test_cache_evicts_the_oldest_grid_and_a_held_handle_says_so(gpu_ctx):
    from impulse_hip.frequency_response import curves_for
    grids = [np.geomspace(10, 24000, 300 + 7 * i) for i in range(10)]
    x = np.cumsum(np.random.default_rng(3).standard_normal(300)) * 0.4
    x[:2] -= 70.0
    h0 = curves_for(grids[0])
    first = (h0.smooth(x, 1 / 6, 1 / 3, 100, 10000), h0.equalization(x, True, **ci.EQ_ARGS))
    assert curves_for(grids[0]) is h0
    for f in grids[1:]:
        y = np.zeros(len(f))
        assert np.array_equal(curves_for(f).smooth(y, 1 / 3, 1 / 3, 100, 10000), y * 0.0)
    # nine newer grids: the cache of 8 has let the first one go, and its handle refuses instead of touching freed memory
    for call in (lambda: h0.smooth(x, 1 / 6, 1 / 3, 100, 10000), lambda: h0.equalization(x, True, **ci.EQ_ARGS),
                 lambda: h0.window_size(1 / 3), lambda: h0.fir_taps(48000, 5), lambda: h0.fir(x, 48000, 50, True)):
        with pytest.raises(RuntimeError, match="handle is closed"):
            call()
    h1 = curves_for(grids[0])
    assert h1 is not h0
    again = (h1.smooth(x, 1 / 6, 1 / 3, 100, 10000), h1.equalization(x, True, **ci.EQ_ARGS))
    assert np.array_equal(first[0], again[0])
    assert all(np.array_equal(a, b) for a, b in zip(first[1], again[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("grid_name", [g for g in GRID_NAMES if ci.too_few(g, "alternating")])
def test_too_few_survivors_are_refused(gpu_ctx, grid_name):
    """Only the last two samples survive the kink rule: the reference raises (FITPACK needs m > k); the device flags the
    curve and the call that downloads the flags refuses, alone or inside a batch."""
    from impulse_hip.frequency_response import curves_for
    f, h = ci.grid(grid_name), curves_for(ci.grid(grid_name))
    bad, good = ci.curve(grid_name, "alternating"), ci.curve(grid_name, "single")
    with pytest.raises(Exception, match="fewer than 3 points"):
        h.equalization(bad, False, **ci.EQ_ARGS)
    with pytest.raises(Exception, match="curve 1 keeps fewer than 3 points"):
        h.equalization(np.stack([good, bad, good]), False, **ci.EQ_ARGS)
    # the handle goes on working, and without the kink bridge the curve is only clipped
    _, eq, used = h.equalization(good, False, **ci.EQ_ARGS)
    assert used[0] == 1 and cm.rel_err(eq, scipy_chain(grid_name, False)["single"][1]) <= tol(grid_name, "spline")
    _, eq, used = h.equalization(bad, False, smoothen_kinks=False, **ci.EQ_ARGS)
    limit = sigmoid(f, 10000, ci.FS / 2, 40, 6.0)
    assert used[0] == 0 and cm.rel_err(eq, np.minimum(-bad, limit)) <= CURVE_TOL
