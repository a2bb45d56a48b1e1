"""Seeded inputs of the plot-data fixtures (plot_data.npz), shared by the golden generator and the tests.
Inputs only, NumPy only: every row is rounded to float32 before either side sees it."""
import numpy as np

# spectrogram cases: name -> (fs, f_res, n_segments, [(kind, samples, seed)])
#   kind "sweep": a logarithmic sweep with noise; "drift": the same on a constant plus a slow ramp (a missing detrend
#   shows); "zeros": silence
SPEC_CASES = {
    # nfft 800, one pass; the three rows share (nfft, hop) = (800, 21): S = 201 (odd), 200 (even), 196
    "fs8000": (8000, 10, 200, [("sweep", 5000, 1), ("drift", 4979, 2), ("zeros", 4900, 3)]),
    # nfft 2205 = 3^2 5 7^2: odd, radix 7, no Nyquist bin; hop 49: S = 201 and 200
    "fs22050": (22050, 10, 200, [("sweep", 12005, 4), ("drift", 11990, 5)]),
    # nfft 4800 = 75 x 64: two passes; hop 76: S = 201 and 200
    "fs48000": (48000, 10, 200, [("sweep", 20000, 6), ("sweep", 19950, 7)]),
    # shorter than fs / 10: nfft clipped to 2 n / 4 = 250, hop 2
    "short": (8000, 10, 200, [("sweep", 500, 8)]),
    # the 3-segment clip on a longer row: nfft 600, hop 3
    "clip3": (8000, 10, 200, [("drift", 1200, 9)]),
    # step_size <= 1: nfft 150, 50 % overlap, S = 3
    "step_le_1": (8000, 10, 200, [("sweep", 300, 10)]),
    # n_segments = 0: 50 % overlap, S = 11
    "nseg0": (8000, 10, 0, [("sweep", 5000, 11)]),
    # another resolution: nfft 400, two rows of different geometry in one request
    "f_res20": (8000, 20, 200, [("sweep", 3000, 12), ("drift", 2100, 13)]),
}
UNSUPPORTED = (48000, 4036, 2018)       # (fs, samples, clipped nfft = 2 x 1009)
SPEC_DECIM = 32                         # the fixture keeps every 32nd column plus the first and the last

# waterfall cases: name -> (fs, samples, seed)
WF_CASES = {
    "long48k": (48000, 3000, 21),       # longer than the 1792 samples the reference keeps
    "short48k": (48000, 1000, 22),      # zero padded
    "fs96000": (96000, 4000, 23),       # the log grid has more points
}


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def row(kind, n, seed, fs):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n)
    t = np.arange(n) / fs
    T = n / fs
    f0, f1 = 20.0, 0.45 * fs
    phase = 2 * np.pi * f0 * T / np.log(f1 / f0) * (np.exp(t / T * np.log(f1 / f0)) - 1)
    x = 0.5 * np.sin(phase) + 0.01 * rng.standard_normal(n)
    if kind == "drift":
        x = x + 0.3 + 0.4 * t / T
    return _f32(x)


def spec_case(name):
    """(fs, f_res, n_segments, [float32-rounded fp64 rows])"""
    fs, f_res, n_segments, rows = SPEC_CASES[name]
    return fs, f_res, n_segments, [row(kind, n, seed, fs) for kind, n, seed in rows]


def kept_columns(S):
    """the columns of a [bins, S] spectrogram the fixture stores"""
    return np.unique(np.concatenate([np.arange(0, S, SPEC_DECIM), [0, S - 1]])).astype(np.int64)


def wf_case(name):
    """(fs, float32-rounded fp64 response): decaying noise after a short pre-delay"""
    fs, n, seed = WF_CASES[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * np.exp(-np.arange(n) / (0.006 * fs))
    x[:40] *= 0.01
    return fs, _f32(x)
