"""K15's formulation of the binaural analysis metrics in NumPy fp64: the two ears as one complex signal through one
transform and the Hermitian split, a host table of bin ranges, direct lag sums per tile of 1 024 samples added in tile
order, a reverse running sum for the decay curve.  ext=True carries every sum in np.longdouble (the transform stays
fp64): against the reference's fixture that measures the reference's own rounding error."""
import numpy as np

TILE = 1024


def fast_len_11(n):
    m = max(int(n), 1)
    while True:
        r = m
        for p in (2, 3, 5, 7, 11):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 1


def bin_table(nfft, fs, bands):
    """(k0, k1) per band: first and one past the last bin of the mask on the bin frequencies k fs / nfft, k <= (nfft - 1) / 2"""
    freqs = np.fft.fftfreq(nfft, d=1 / fs)
    out = np.zeros((len(bands), 2), dtype=np.int64)
    for b, (lo, hi) in enumerate(bands):
        hi = min(hi, fs / 2)
        if lo >= hi:
            continue
        idx = np.nonzero((freqs >= lo) & (freqs < hi))[0]
        if len(idx):
            assert idx[-1] - idx[0] + 1 == len(idx) and idx[-1] <= (nfft - 1) // 2
            out[b] = (idx[0], idx[-1] + 1)
    return out


def band_sums(left, right, fs, bands, ext=False):
    """[bands, 4]: sum |L|^2, sum |R|^2, re and im of sum L conj R; NaN rows for empty bands"""
    acc = np.longdouble if ext else np.float64
    nfft = fast_len_11(max(len(left), len(right)))
    z = np.zeros(nfft, dtype=np.complex128)
    z[:len(left)] += left
    z[:len(right)] += 1j * np.asarray(right)
    Z = np.fft.fft(z)
    out = np.full((len(bands), 4), np.nan)
    for b, (k0, k1) in enumerate(bin_table(nfft, fs, bands)):
        if k0 >= k1:
            continue
        k = np.arange(k0, k1)
        a, c = Z[k], np.conj(Z[(nfft - k) % nfft])
        ar, ai, cr, ci = (v.astype(acc) for v in (a.real, a.imag, c.real, c.imag))
        lx, ly = (ar + cr) / 2, (ai + ci) / 2                    # L = (Z[k] + conj Z[-k]) / 2
        rx, ry = (ai - ci) / 2, (cr - ar) / 2                    # R = (Z[k] - conj Z[-k]) / (2i)
        out[b] = (np.sum(lx * lx + ly * ly), np.sum(rx * rx + ry * ry), np.sum(lx * rx + ly * ry), np.sum(ly * rx - lx * ry))
    return out


def iacf(left, right, D, ext=False):
    """(lags, iacf over the lags 'full' mode has within +-D, first argmax |iacf|, E_l, E_r); lags empty without energy"""
    acc = np.longdouble if ext else np.float64
    left, right = np.asarray(left, dtype=acc), np.asarray(right, dtype=acc)
    nl, nr = len(left), len(right)
    nmax, nlag = max(nl, nr), 2 * D + 1
    sums = np.zeros(nlag, dtype=acc)
    el = er = acc(0)
    for t0 in range(0, nmax, TILE):
        sl = np.zeros(TILE + 2 * D, dtype=acc)
        sr = np.zeros(TILE, dtype=acc)
        a, b = max(t0 - D, 0), min(t0 + TILE + D, nl)
        if b > a:
            sl[a - (t0 - D):b - (t0 - D)] = left[a:b]
        if t0 < nr:
            sr[:min(TILE, nr - t0)] = right[t0:t0 + TILE]
        sums += np.lib.stride_tricks.sliding_window_view(sl, TILE)[:nlag] @ sr
        el += np.sum(sl[D:D + TILE] ** 2)
        er += np.sum(sr ** 2)
    lo, hi = max(-D, -(nr - 1)), min(D, nl - 1)
    if not el * er > 0 or lo > hi:
        return np.array([], dtype=int), np.array([]), -1, float(el), float(er)
    vals = (sums / np.sqrt(el * er))[lo + D:hi + D + 1]
    return np.arange(lo, hi + 1), vals.astype(np.float64), int(np.argmax(np.abs(vals))), float(el), float(er)


def edc_db(x, floor_db=-80.0, ext=False):
    acc = np.longdouble if ext else np.float64
    x = np.asarray(x, dtype=acc)
    e = np.cumsum((x * x)[::-1])[::-1]
    if not len(e) or e[0] <= 1e-12:
        return np.full(len(e), floor_db)
    return (10 * np.log10(e / (e[0] + acc(1e-12)) + acc(1e-12))).astype(np.float64)
