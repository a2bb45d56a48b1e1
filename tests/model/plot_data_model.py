"""NumPy model of K16's arithmetic in np.longdouble: scipy.signal.spectrogram with a periodic Hann window and
detrend="constant" as the reference's plot_spectrogram and plot_waterfall call it (core/plotting/impulse_response_plotter.py
:214-256, :506-575), bin 0 dropped.  scipy.fft transforms long doubles natively.  The fixtures' distance from this model is
the reference's own rounding error (e_ref), which sets the device tolerance."""
import numpy as np
import scipy.fft

LD = np.longdouble
PI = LD(4) * np.arctan(LD(1))


def _segments(x, nfft, noverlap):
    x = np.asarray(x, dtype=LD)
    hop = nfft - noverlap
    S = (len(x) - noverlap) // hop if len(x) >= nfft else 0
    seg = x[np.arange(S)[:, None] * hop + np.arange(nfft)[None, :]]
    seg = seg - seg.mean(axis=1, keepdims=True)
    w = LD(0.5) - LD(0.5) * np.cos(2 * PI * np.arange(nfft, dtype=LD) / nfft)
    return scipy.fft.rfft(seg * w, axis=1), np.sum(w * w)


def spectrogram_db(x, fs, nfft, noverlap):
    """[nfft // 2, S] long double: 10 log10(|psd| + 1e-9)"""
    X, w2 = _segments(x, nfft, noverlap)
    p = (X.real ** 2 + X.imag ** 2) / (LD(fs) * w2)
    last = p.shape[1] - 1 if nfft % 2 == 0 else p.shape[1]
    p[:, 1:last] *= 2
    return (10 * np.log10(np.abs(p) + LD(1e-9)))[:, 1:].T


def stft_magnitude(x, fs, nfft, noverlap):
    """[nfft // 2, S] long double: |X| sqrt(1 / (fs sum w^2))"""
    X, w2 = _segments(x, nfft, noverlap)
    return (np.abs(X) * np.sqrt(1 / (LD(fs) * w2)))[:, 1:].T


def waterfall(x, fs):
    """(magnitudes [128, 13], z_db) long double: the reference's fixed set-up (first 1792 samples, zero padded, nfft 256, 50 %
    overlap) and its finishing: linear interpolation (and extrapolation) in log10 f onto 10 * 1.03^k, normalised, clipped to
    -100 dB, 3 x 3 mean with zeros outside, outer frame dropped as the reference drops it."""
    s = np.zeros(5 * 256 + 512, dtype=LD)
    m = min(len(x), len(s))
    s[:m] = np.asarray(x, dtype=LD)[:m]
    mag = stft_magnitude(s, fs, 256, 128)
    freqs = np.arange(1, 129, dtype=LD) * LD(fs) / 256
    n_freqs = int(np.log(fs / 2 / 10) / np.log(1.03))
    f = 10 * 1.03 ** np.arange(n_freqs)                            # the reference's fp64 grid, then exact
    lx, lq = np.log10(freqs), np.log10(f.astype(LD))
    i = np.clip(np.searchsorted(lx, lq, side="right") - 1, 0, len(lx) - 2)
    frac = ((lq - lx[i]) / (lx[i + 1] - lx[i]))[:, None]
    z = mag[i] + frac * (mag[i + 1] - mag[i])
    z = z / np.max(z)
    z = 20 * np.log10(np.clip(z, LD(10 ** (-100 / 20)), np.max(z)))
    pad = np.zeros((z.shape[0] + 2, z.shape[1] + 2), dtype=LD)
    pad[1:-1, 1:-1] = z
    sm = sum(pad[a:a + z.shape[0], b:b + z.shape[1]] for a in range(3) for b in range(3)) / 9
    return mag, sm[1:-1, :-1]
