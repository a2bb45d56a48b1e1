"""Seeded inputs of the microphone-deviation fixtures (mic_deviation.npz), shared by the golden generator and the tests.
Inputs only, NumPy only: every response is rounded to float32 before either side sees it."""
import numpy as np

LAYOUT_71 = ("FL", "FR", "FC", "SL", "SR", "BL", "BR")

# name -> (fs, speakers, n samples, anchor, correction_strength, mismatch kind, seed)
CASES = {
    "fc71_48k_auto": (48000, LAYOUT_71, 3000, "auto", 0.7, "tilt", 1),
    "fc71_48k_diffuse": (48000, LAYOUT_71, 3000, "diffuse", 0.7, "tilt", 1),
    "nofc_44k": (44100, ("FL", "FR", "SL", "SR"), 2800, "auto", 0.7, "tilt", 2),
    "fc_96k": (96000, ("FL", "FR", "FC"), 5000, "auto", 0.7, "tilt", 3),
    "large_strength1": (48000, ("FL", "FR", "FC"), 3000, "auto", 1.0, "large", 4),
    "matched": (48000, ("FL", "FR"), 3000, "auto", 0.7, "none", 5),
    "strength0": (48000, ("FL", "FR", "FC"), 3000, "auto", 0.0, "tilt", 6),
}


def _response(rng, n, fs, delay):
    """a direct impulse, a few early reflections and a decaying noise tail"""
    x = np.zeros(n)
    x[delay] = 1.0
    x[delay + 1] = -0.35
    for _ in range(4):
        x[delay + rng.integers(int(0.002 * fs), int(0.012 * fs))] += rng.uniform(-0.4, 0.4)
    t = np.arange(n - delay)
    x[delay:] += 0.05 * rng.standard_normal(n - delay) * np.exp(-t / (0.05 * fs))
    return x


def _mic(kind, rng):
    """the left microphone's deviation as a short FIR (right: none)"""
    if kind == "none":
        return np.array([1.0])
    if kind == "large":
        return np.array([4.0, -3.6, 0.9])             # ~16 dB of tilt: reaches the clamps
    return np.array([1.0, 0.12 * rng.uniform(0.5, 1.5), -0.05])


def hrir_case(name):
    """(fs, {speaker: {"left": float32-rounded fp64 array, "right": ...}}, anchor, correction_strength)"""
    fs, speakers, n, anchor, strength, kind, seed = CASES[name]
    rng = np.random.default_rng(seed)
    mic = _mic(kind, rng)
    irs = {}
    for k, sp in enumerate(speakers):
        delay = 20 + 3 * k
        right = _response(rng, n, fs, delay + (k % 3))
        left = right.copy() if kind == "none" else np.convolve(np.roll(right, -(k % 3)), mic)[:n]
        irs[sp] = {"left": left.astype(np.float32).astype(np.float64), "right": right.astype(np.float32).astype(np.float64)}
    return fs, irs, anchor, strength
