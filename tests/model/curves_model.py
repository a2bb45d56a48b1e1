"""The K12 curve operators evaluated in np.longdouble on the CPU: the yardstick that says how far SciPy's own fp64
results are from the exact operator (tests/test_curves_edges.py measures it over the fixture inputs on the CPU; its
tolerances come from those figures, never from the kernel's output).  Inputs are the fp64 values the
reference sees (the grid, log10 of it, the curve); everything from there on is carried in extended precision.

    savgol(x, w)                 scipy.signal.savgol_filter(x, w, 2), mode='interp'
    smooth(f, x, wn, wt, fl, fu) autoeq _smoothen_fractional_octave (one iteration per window)
    heavy_light(f, x, windows)   autoeq smoothen_heavy_light's error_smoothed
    spline2(xk, yk, xq)          InterpolatedUnivariateSpline(xk, yk, k=2)(xq), ext = 0
    equalize(f, es, keep, ...)   autoeq equalize with the kept samples given (the clip decisions are the caller's)
"""
import numpy as np

LD = np.longdouble


def savgol(x, w):
    x = np.asarray(x, dtype=LD)
    n, m = len(x), w // 2
    k = np.arange(-m, m + 1, dtype=LD)
    dm = LD(m)
    coeff = (3 * (3 * dm * dm + 3 * dm - 1) - 15 * k * k) / ((2 * dm - 1) * (2 * dm + 1) * (2 * dm + 3))
    y = np.empty(n, dtype=LD)
    for i in range(m, n - m):
        y[i] = np.dot(coeff, x[i - m:i + m + 1])
    # edges: the least-squares parabola through the first / last w samples, by projection on the discrete orthogonal
    # polynomials 1, t, t^2 - (w^2 - 1) / 12 over t = j - (w - 1) / 2
    dw = LD(w)
    t = np.arange(w, dtype=LD) - (dw - 1) / 2
    mu2 = (dw * dw - 1) / 12
    p = np.stack([np.ones(w, dtype=LD), t, t * t - mu2])
    norm = np.array([dw, dw * (dw * dw - 1) / 12, dw * (dw * dw - 1) * (dw * dw - 4) / 180], dtype=LD)
    for head in (True, False):
        seg = x[:w] if head else x[n - w:]
        c = (p @ seg) / norm
        fit = c @ p
        if head:
            y[:m] = fit[:m]
        else:
            y[n - m:] = fit[w - m:]
    return y


def sigmoid(f, f_lower, f_upper, a_normal=0.0, a_treble=1.0):
    f = np.asarray(f, dtype=LD)
    f_center = np.sqrt(LD(f_upper) / LD(f_lower)) * LD(f_lower)
    half_range = np.log10(LD(f_upper)) - np.log10(f_center)
    a = 1 / (1 + np.exp(-((np.log10(f) - np.log10(f_center)) / (half_range / 4))))
    return a * -(LD(a_normal) - LD(a_treble)) + LD(a_normal)


def smooth(f, x, wn, wt, f_lower, f_upper):
    k = sigmoid(f, f_lower, f_upper)
    return savgol(x, wn) * (k * -1 + 1) + savgol(x, wt) * k


def heavy_light(f, x, w6, w3, w130):
    light = smooth(f, x, w6, w3, 100, 10000)
    heavy = smooth(f, x, w3, w130, 1000, 6000)
    return smooth(f, np.maximum(light, heavy), w3, w3, 100, 10000)


def spline2(xk, yk, xq):
    """FITPACK's interpolating quadratic spline (fpcurf, s = 0, k = 2): knots x0 x0 x0, the midpoints of (x1, x2) ..
    (x_{m-3}, x_{m-2}), x_{m-1} three times; tridiagonal collocation; beyond the ends the end pieces continue."""
    xk, yk, xq = (np.asarray(a, dtype=LD) for a in (xk, yk, xq))
    m = len(xk)
    assert m >= 3
    t = np.concatenate([[xk[0]] * 3, (xk[1:m - 2] + xk[2:m - 1]) / 2, [xk[-1]] * 3])

    def basis(s, x):
        # the three degree-2 B-splines s-2 .. s on span [t_s, t_{s+1}) (and its continuation)
        tm1, t0, t1, t2 = t[s - 1], t[s], t[s + 1], t[s + 2]
        a1, b1 = (t1 - x) / (t1 - t0), (x - t0) / (t1 - t0)
        return np.array([(t1 - x) / (t1 - tm1) * a1, (x - tm1) / (t1 - tm1) * a1 + (t2 - x) / (t2 - t0) * b1,
                         (x - t0) / (t2 - t0) * b1], dtype=LD)

    def span(x):
        s = int(np.searchsorted(t, x, side="right")) - 1
        return min(max(s, 2), m - 1)

    A = np.zeros((m, m), dtype=LD)
    for i in range(m):
        s = span(xk[i])
        A[i, s - 2:s + 1] = basis(s, xk[i])
    # A is tridiagonal (row i: columns i-1 .. i+1) and totally positive: plain elimination
    sub, dia, sup = np.zeros(m, dtype=LD), np.diag(A).copy(), np.zeros(m, dtype=LD)
    sub[1:], sup[:-1] = np.diag(A, -1), np.diag(A, 1)
    assert np.count_nonzero(A) <= 3 * m and np.all(np.triu(A, 2) == 0) and np.all(np.tril(A, -2) == 0)
    rhs = yk.copy()
    for i in range(1, m):
        fct = sub[i] / dia[i - 1]
        dia[i] -= fct * sup[i - 1]
        rhs[i] -= fct * rhs[i - 1]
    c = np.empty(m, dtype=LD)
    c[m - 1] = rhs[m - 1] / dia[m - 1]
    for i in range(m - 2, -1, -1):
        c[i] = (rhs[i] - sup[i] * c[i + 1]) / dia[i]
    out = np.empty(len(xq), dtype=LD)
    for j, x in enumerate(xq):
        s = span(x)
        out[j] = np.dot(c[s - 2:s + 1], basis(s, x))
    return out


def equalize(f, es, keep, max_gain, treble_f_lower, treble_f_upper, treble_max_gain=6.0, treble_gain_k=1.0):
    limit = sigmoid(f, treble_f_lower, treble_f_upper, max_gain, treble_max_gain)
    gain = -np.asarray(es, dtype=LD) * sigmoid(f, treble_f_lower, treble_f_upper, 1.0, treble_gain_k)
    eq = np.where(gain > limit, limit, gain)
    x = np.log10(np.asarray(f, dtype=np.float64)).astype(LD)            # the fp64 abscissae SciPy is given
    return spline2(x[keep], eq[keep], x)


def rel_err(got, want):
    """max |got - want| / max(1, max |want|): the form every K12 edge comparison uses (extrapolated points can be large)"""
    want = np.asarray(want)
    return float(np.max(np.abs(np.asarray(got) - want)) / max(1.0, float(np.max(np.abs(want)))))
