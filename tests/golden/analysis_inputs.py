"""Seeded inputs of the binaural-analysis fixtures (analysis.npz), shared by the golden generator and the tests.
Inputs only, NumPy only: every row is rounded to float32 before either side sees it."""
import numpy as np

from micdev_inputs import LAYOUT_71, _response

C2_ROW = 42000          # samples of a finished row of the 7.1 measurement at 48 kHz

# name -> (fs, kind, (left length, right length), pairs, bands (None: octave_bands(fs)), max_delay_ms, seed)
CASES = {
    "hrir71_48k": (48000, "room", (C2_ROW, C2_ROW), len(LAYOUT_71), None, 1.0, 11),
    "fs44100": (44100, "room", (3000, 3000), 2, None, 1.0, 12),
    "fs96000": (96000, "room", (6000, 6000), 2, None, 1.0, 13),
    "fs192000_5ms": (192000, "room", (12000, 12000), 1, None, 5.0, 14),
    "fs22050": (22050, "room", (2000, 2000), 2, None, 1.0, 15),
    "unequal": (48000, "room", (2500, 3100), 2, None, 1.0, 16),
    "unequal_left_longer": (48000, "room", (3300, 2048), 1, None, 5.0, 17),
    "len3430": (48000, "room", (3430, 3430), 1, None, 1.0, 18),
    "one_sample": (48000, "one", (1, 1), 1, None, 1.0, 19),
    "zero_ear": (48000, "zero", (3000, 3000), 1, None, 1.0, 20),
    "delayed_copy": (48000, "delay", (3000, 3000), 1, None, 1.0, 21),
    "custom_bands": (48000, "room", (3000, 3000), 1,
                     ((100.0, 200.0), (1001.0, 1007.0), (5000.0, 30000.0), (30000.0, 40000.0), (0.0, 50.0)), 5.0, 22),
}
DELAY = 7               # samples the right ear of "delayed_copy" lags the left by
ATTENUATION = 0.5


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def case(name):
    """(fs, [(left, right)] float32-rounded fp64 arrays, bands or None, max_delay_ms)"""
    fs, kind, (nl, nr), count, bands, max_delay_ms, seed = CASES[name]
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(count):
        if kind == "one":
            left, right = np.array([0.5]), np.array([-0.25])
        else:
            n = max(nl, nr)
            common = _response(rng, n + 16, fs, 20 + 3 * k)
            own_l, own_r = _response(rng, n, fs, 24 + k), _response(rng, n, fs, 29 + k)
            left = (common[:n] + 0.25 * own_l)[:nl]
            right = (0.8 * common[3 + (k % 4):3 + (k % 4) + n] + 0.25 * own_r)[:nr]
            if kind == "zero":
                right = np.zeros(nr)
            if kind == "delay":
                right = np.zeros(nr)
                right[DELAY:] = ATTENUATION * left[:nr - DELAY]
        pairs.append((_f32(left), _f32(right)))
    return fs, pairs, (None if bands is None else [tuple(b) for b in bands]), max_delay_ms


# What the tests rely on; make_analysis_goldens.py asserts them on the reference's outputs before it writes the fixture.
GAP_MIN = 1e-9                  # the reference's two largest |iacf| of every case differ by more than this
COHERENCE_MIN = 0.05            # IPD is compared in degrees on bands whose reference coherence is at least this
EDC_DECIM = 32                  # every 32nd sample of a decay curve, plus its first and last EDC_EDGE samples
EDC_EDGE = 64
