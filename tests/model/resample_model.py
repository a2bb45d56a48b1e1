"""NumPy model of K17 and the cases its tests share.

resample_poly(x, up, down, taps) is the closed form that scipy.signal.resample_poly(x, up, down, window=taps) collapses to
(its pre-pad, post-pad and trim included): with up / down reduced by their gcd, L = len(taps), half = (L - 1) // 2 and
n_out = ceil(n_in up / down),

    y[m] = up * sum_k taps[m down + half - k up] x[k]        0 <= m < n_out, 0 <= k < n_in, tap index in [0, L)

and a copy of the row when up == down.  The dtype of the arithmetic is selectable, np.longdouble by default.
"""
from math import gcd

import numpy as np

# ---- the model ----------------------------------------------------------------------------------------------------


def out_len(n_in, up, down):
    g = gcd(up, down)
    return -((-n_in * (up // g)) // (down // g))


def resample_poly(x, up, down, taps, dtype=np.longdouble):
    g = gcd(up, down)
    up, down = up // g, down // g
    x = np.asarray(x, dtype=dtype).ravel()
    if up == down:
        return x.copy()
    h = np.asarray(taps, dtype=dtype).ravel()
    L, n_in = len(h), len(x)
    half = (L - 1) // 2
    n_out = -((-n_in * up) // down)
    y = np.zeros(n_out, dtype=dtype)
    if n_out == 0:
        return y
    nph = -(-L // up)                                            # terms per output
    m = np.arange(n_out, dtype=np.int64)
    t = m * down + half
    k0, p = t // up, t % up
    # x[k0 - nph + 1 .. k0] is row k0 of the windows of the padded row
    xpad = np.concatenate([np.zeros(nph - 1, dtype=dtype), x, np.zeros(max(int(k0[-1]) + 1 - n_in, 0), dtype=dtype)])
    win = np.lib.stride_tricks.sliding_window_view(xpad, nph)
    for phase in range(min(up, L)):
        sel = m[p == phase]                                      # outputs of this phase: every up-th, k0 down apart
        if len(sel) == 0:
            continue
        run = np.zeros(nph, dtype=dtype)                         # taps[phase], taps[phase + up], ..., reversed
        own = h[phase::up]
        run[nph - len(own):] = own[::-1]
        rows = win[int(k0[sel[0]])::down][:len(sel)]
        for a in range(0, len(sel), 2048):
            y[sel[a:a + 2048]] = rows[a:a + 2048] @ run
    return y * dtype(up)


# ---- the cases ----------------------------------------------------------------------------------------------------
RATIOS = [(147, 160), (160, 147), (2, 1), (1, 2), (640, 147), (147, 320), (3, 2), (48000, 48000)]
# ragged in one call; the long row spans several tiles of 256 outputs and several staged input spans at every ratio
ROW_LENGTHS = [0, 1, 5, 257, 700, 20000]
SHORT_TAPS = [100, 7, 1]                                         # firwin filters tried on 147/160 and 2/1 besides L = 16001
SHORT_TAP_RATIOS = [(147, 160), (2, 1)]


def case_ids():
    ids = [f"{u}_{d}_L16001" for u, d in RATIOS]
    ids += [f"{u}_{d}_L{L}" for u, d in SHORT_TAP_RATIOS for L in SHORT_TAPS]
    return ids


def case_taps(up, down, L):
    from scipy.signal import firwin
    if L == 16001:
        if up == down:
            return np.ones(1)                                    # never read: the rows are copied
        from impulse_hip.resampling import kaiser_null_filter
        return kaiser_null_filter(up, down)
    if L == 1:
        return np.ones(1)
    return firwin(L, 1 / max(up, down), window=("kaiser", 5.0))


def case_rows(up, down, L):
    """decaying noise, seeded per case, float32-valued so that device rows hold the same numbers"""
    rng = np.random.default_rng([up, down, L])
    rows = []
    for n in ROW_LENGTHS:
        x = rng.standard_normal(n) * np.exp(-np.arange(n) / max(n / 6.0, 1.0))
        rows.append(x.astype(np.float32).astype(np.float64))
    return rows


def case(name):
    """(up, down, taps, rows) of a case id"""
    u, d, L = name.split("_")
    up, down, L = int(u), int(d), int(L[1:])
    return up, down, case_taps(up, down, L), case_rows(up, down, L)


_REFERENCE = {}


def reference(name):
    """(model in longdouble, scipy in float64) per row of a case, computed once"""
    if name not in _REFERENCE:
        from scipy.signal import resample_poly as scipy_resample_poly
        up, down, taps, rows = case(name)
        _REFERENCE[name] = ([resample_poly(x, up, down, taps) for x in rows],
                            [scipy_resample_poly(x, up, down, window=taps) for x in rows])
    return _REFERENCE[name]
