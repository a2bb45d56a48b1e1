"""Grids and named error curves of the K12 edge fixtures (curves_edges.npz), shared by the golden generator and the tests.
Inputs only, NumPy only.  A curve is a seeded random walk held within +-WALK_DB (so that nothing clips by accident: the
smallest gain limit is 6 dB) plus one edit that pushes chosen samples far past the 40 dB limit."""
import math

import numpy as np

WALK_DB = 4.0
# equalize() as the product's worker calls it (core/parallel_workers.py): 40 dB, 6 dB from 10 kHz up to fs / 2
FS = 48000
EQ_ARGS = dict(max_gain=40, treble_f_lower=10000, treble_f_upper=FS / 2, treble_max_gain=6.0, treble_gain_k=1.0)
OCTAVES = (1 / 12, 1 / 6, 1 / 3, 1.3)


def _stepped(f_min, f_max, step):
    out, f = [], f_min
    while f <= f_max:                       # repeated multiplication, as generate_frequencies does
        out.append(f)
        f *= step
    return np.array(out, dtype=np.float64)


def _jittered(f_min, f_max, step, rel, seed):
    rng = np.random.default_rng(seed)
    out, f = [], f_min
    while f <= f_max:
        out.append(f)
        f *= step * (1.0 + rel * rng.uniform(-1.0, 1.0))
    return np.array(out, dtype=np.float64)


# name -> (builder, expected number of points, expected windows for OCTAVES or None)
GRIDS = {
    "step1.05": (lambda: _stepped(10, 24000, 1.05), 160, (1, 3, 5, 19)),
    "step1.02": (lambda: _stepped(10, 24000, 1.02), 394, (3, 7, 13, 47)),
    "step1.01": (lambda: _stepped(10, 24000, 1.01), 783, (7, 13, 23, 91)),
    "step1.005": (lambda: _stepped(10, 24000, 1.005), 1561, (13, 23, 47, 181)),
    "geom2048": (lambda: np.geomspace(10, 24000, 2048), 2048, None),
    "step1.01_20_20k": (lambda: _stepped(20, 20000, 1.01), None, None),
    "jitter1.01": (lambda: _jittered(10, 24000, 1.01, 0.003, 7), None, None),
}
# The fixture records every curve on both paths for the three smaller grids; the two large grids and the two variations
# of the product's grid record the subsets below (a committed file has a size limit).  The tests run EVERY curve on every
# grid against SciPy itself and compare with the fixture wherever it has a record.
FULL_GRIDS = ("step1.05", "step1.02", "step1.01")
RAW_SUBSET = ("first1", "trans_at_kh", "trans_at_kh1", "last3", "comb", "toggle", "alternating")
SMOOTHED_SUBSET = ("trans_at_kh", "comb")

_grid_cache = {}


def grid(name):
    if name not in _grid_cache:
        f = GRIDS[name][0]()
        f.setflags(write=False)
        _grid_cache[name] = f
    return _grid_cache[name]


def window_size(frequency, octaves):
    """autoeq _window_size: odd window (grid points) that covers `octaves`."""
    steps = [frequency[i] / frequency[i - 1] for i in range(1, len(frequency))]
    step = sum(steps) / len(steps)
    w = round(math.log(2 ** octaves) / math.log(step))
    return w + 1 if not w % 2 else w


def kink_half(name):
    return (window_size(grid(name), 1 / 12) - 1) // 2


def walk(name):
    """The grid's random walk, scaled into +-WALK_DB."""
    seed = 100 + list(GRIDS).index(name)
    w = np.cumsum(np.random.default_rng(seed).standard_normal(len(grid(name))))
    return w * (WALK_DB / np.max(np.abs(w)))


# name -> edit(e, n, kh, w12).  t = max(kh, 1): index 0 is never a transition, so with kh = 0 the pair below degenerates
# to a transition at 1 and at 2 (the first point is kept in both: with kh = 0 only the transition sample itself is dropped).
def _edit(select, db=70.0):
    def apply(e, n, kh, w12):
        e[select(n, kh, w12)] -= db
    return apply


def _toggle(n, kh, w12):
    i = np.arange(n // 3, 2 * n // 3)
    return i[((i - i[0]) // 3) % 2 == 0]


CURVES = {
    "first1": _edit(lambda n, kh, w12: slice(0, 1)),
    "first2": _edit(lambda n, kh, w12: slice(0, 2)),
    "trans_at_kh": _edit(lambda n, kh, w12: slice(0, max(kh, 1))),             # first point dropped (kh >= 1)
    "trans_at_kh1": _edit(lambda n, kh, w12: slice(0, max(kh, 1) + 1)),        # ... and kept
    "last3": _edit(lambda n, kh, w12: slice(n - 3, n)),
    "last1": _edit(lambda n, kh, w12: slice(n - 1, n)),
    "single": _edit(lambda n, kh, w12: n // 2),
    "comb": _edit(lambda n, kh, w12: slice(None, None, w12 + 2), 90.0),        # doomed windows merge into long gaps
    "toggle": _edit(_toggle),                                                  # three in, three out, mid-grid only
    "none": _edit(lambda n, kh, w12: slice(0, 0)),
    "all": _edit(lambda n, kh, w12: slice(None)),                              # no transition, nothing dropped
    # every sample from 1 on is a transition: only the last two survive (and the first, when kh = 0)
    "alternating": _edit(lambda n, kh, w12: slice(None, None, 2)),
}


def curve(grid_name, curve_name):
    f = grid(grid_name)
    e = walk(grid_name).copy()
    CURVES[curve_name](e, len(f), kink_half(grid_name), window_size(f, 1 / 12))
    return e


def raw_names(grid_name):
    """The curves whose equalize() results on the curve as it is are recorded for the grid."""
    return tuple(CURVES) if grid_name in FULL_GRIDS else RAW_SUBSET


def smoothed_names(grid_name):
    """The curves whose smoothen_heavy_light + equalize results are recorded for the grid."""
    return tuple(CURVES) if grid_name in FULL_GRIDS else SMOOTHED_SUBSET


def first_transition(grid_name, curve_name):
    """Index of the first clip on/off transition of the UNSMOOTHED curve (None: no transition).  Edits reach -70 dB
    or below and the walk stays within WALK_DB, so a sample is clipped exactly where the edit touched it."""
    clipped = curve(grid_name, curve_name) < -35.0
    t = np.flatnonzero(clipped[1:] != clipped[:-1])
    return int(t[0]) + 1 if len(t) else None


def drops_first(grid_name, curve_name):
    """What the kink rule says about index 0 on the unsmoothed path: dropped iff a transition lies within kink_half of it."""
    t, kh = first_transition(grid_name, curve_name), kink_half(grid_name)
    return t is not None and t <= kh


def too_few(grid_name, curve_name):
    return curve_name == "alternating" and kink_half(grid_name) >= 1


def smoothing_pairs(grid_name):
    """(window, treble window, treble_f_lower, treble_f_upper): pairs in octaves that between them use every window the
    grid admits (w >= 3), with the two blends the product uses."""
    f = grid(grid_name)
    ok = [o for o in OCTAVES if 3 <= window_size(f, o) <= len(f)]
    blends = ((100, 10000), (1000, 6000))
    return tuple((ok[i], ok[(i + 1) % len(ok)]) + blends[(i // 2) % 2] for i in range(0, len(ok), 2))
