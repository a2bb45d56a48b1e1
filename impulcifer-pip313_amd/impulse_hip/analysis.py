"""Binaural analysis metrics (surface of reference core/plotting/analysis.py: the numerical core of its ILD / IPD / IACC /
ETC plots, which HRIRPlotter.generate_*_bokeh_layout call on the finished rows of every speaker pair).

The arithmetic runs on the device, K15 (imp_binaural_metrics*, imp_energy_decay_db*):
  - per octave band sum |L|^2, sum |R|^2 and sum L conj R of the nfft = next_fast_len(max(len)) point spectra; which bins
    belong to a band is decided here, with the reference's own expression on np.fft.fftfreq, and reaches the device as a
    table of bin ranges;
  - the normalised interaural cross-correlation at the lags within round(max_delay_ms fs / 1000) samples, its largest
    magnitude and where it lies;
  - the Schroeder energy decay curve in dB.
The dozen scalars per pair that follow (10 log10 of the power ratio, the angle of the cross sum) are taken on the host.
Rows that live on the device (device_rows.py) are read where they are; host arrays are uploaded as float64.
`binaural_metrics` is the batched form: any number of pairs of one sample rate in one call.  The single-pair functions
have the reference's arguments, defaults, return types and NaN / empty conventions.  One deviation: a band whose lower
edge is negative would select negative-frequency bins in the reference; here it raises ValueError.  Plots are not provided.
"""
import numpy as np

from . import _native
from .microphone_deviation_correction import next_fast_len_11

DEFAULT_OCTAVE_CENTERS = (125, 250, 500, 1000, 2000, 4000, 8000, 16000)
MAX_LAG_SAMPLES = 2048          # K15's limit on round(max_delay_ms fs / 1000): 10 ms at 192 kHz is 1920


def octave_bands(fs, centers=DEFAULT_OCTAVE_CENTERS):
    """(lower, upper) edges of the octave bands around `centers`; the upper edge is clamped to Nyquist and the list ends
    with the band that reaches it (reference :14-28)."""
    bands = []
    for center in centers:
        lower = center / (2 ** (1 / 2))
        upper = min(center * (2 ** (1 / 2)), fs / 2)
        if lower < upper:
            bands.append((lower, upper))
        if upper >= fs / 2:
            break
    return bands


def band_bin_ranges(nfft, fs, bands):
    """[len(bands), 2] int64 (k0, k1): the bins k0 <= k < k1 of an nfft-point spectrum that the reference's
    (fftfreq >= f_low) & (fftfreq < min(f_high, fs / 2)) selects (:42-52); k0 == k1 where it selects none."""
    nfft = int(nfft)
    pos = np.fft.fftfreq(nfft, d=1 / fs)[:(nfft - 1) // 2 + 1]           # the non-negative frequencies, ascending
    out = np.zeros((len(bands), 2), dtype=np.int64)
    for b, (f_low, f_high) in enumerate(bands):
        f_high = min(f_high, fs / 2)
        if f_low >= f_high:
            continue
        if f_low < 0:
            raise ValueError(f"band ({f_low}, {f_high}): a negative lower edge is not supported")
        k0 = int(np.searchsorted(pos, f_low, side="left"))
        k1 = int(np.searchsorted(pos, f_high, side="left"))
        if k1 > k0:
            out[b] = (k0, k1)
    return out


def _rows_of(irs):
    """(device rows or None, host rows) of ImpulseResponse objects or arrays"""
    rows = [getattr(ir, "_row", None) if getattr(ir, "_data", 0) is None else None for ir in irs]
    ctx = _native.default_context()
    if rows and all(r is not None and r.block.ctx is ctx for r in rows):
        return rows, None
    return None, [np.asarray(ir.data if hasattr(ir, "peak_index") else ir, dtype=np.float64).ravel() for ir in irs]


def binaural_metrics(pairs, fs, bands=None, max_delay_ms=1.0, edc=False, floor_db=-80.0):
    """The metrics of every (left, right) pair of `pairs` (arrays, or ImpulseResponse objects whose device rows are read in
    place) at sample rate fs, in one device call (two with edc).  bands: (lower, upper) edges, default octave_bands(fs).
    Returns one dict per pair: "bands", "band_sums" [bands, 4] (power left, power right, re and im of the cross sum),
    "ild_db", "ipd_deg" (lists, NaN for an empty band), "lags_ms", "iacf", "iacc", "tau_ms" (the reference's
    interaural_cross_correlation tuple) and with edc "edc_db": (left curve, right curve)."""
    ctx = _native.default_context()
    pairs = list(pairs)
    bands = octave_bands(fs) if bands is None else [tuple(b) for b in bands]
    if not pairs:
        return []
    D = round(max_delay_ms * fs / 1000)
    if D > MAX_LAG_SAMPLES:
        raise ValueError(f"max_delay_ms = {max_delay_ms} at {fs} Hz is {D} samples: above the limit of {MAX_LAG_SAMPLES}")
    irs = [ir for pair in pairs for ir in pair]
    dev, host = _rows_of(irs)
    if dev is not None:
        from .device_rows import span
        base, offs, lens = span(dev)
        rows = (offs, lens)
    else:
        base, rows, lens = None, host, np.array([len(r) for r in host], dtype=np.int64)
    P = len(pairs)
    nfft = np.array([next_fast_len_11(max(int(lens[2 * p]), int(lens[2 * p + 1]))) for p in range(P)], dtype=np.int64)
    tables = {}
    bins = np.zeros((P, len(bands), 2), dtype=np.int64)
    for p in range(P):
        n = int(nfft[p])
        if n not in tables:
            tables[n] = band_bin_ranges(n, fs, bands)
        bins[p] = tables[n]
    try:
        sums, iacf, peak, energy = ctx.binaural_metrics(rows, nfft, bins, max(D, 0), dptr=base)
        curves = ctx.energy_decay_db(rows, floor_db, dptr=base) if edc else None
    except _native.NativeError as exc:
        if exc.code == _native.IMP_ERR_UNSUPPORTED:
            raise ValueError(str(exc)) from exc
        raise
    out = []
    for p in range(P):
        pl, pr, cross = sums[p, :, 0], sums[p, :, 1], sums[p, :, 2] + 1j * sums[p, :, 3]
        ild = [np.nan if np.isnan(a) else 10 * np.log10((a + 1e-12) / (b + 1e-12)) for a, b in zip(pl, pr)]
        ipd = [np.nan if np.isnan(c.real) else float(np.degrees(np.angle(c))) for c in cross]
        res = {"bands": list(bands), "band_sums": sums[p].copy(), "ild_db": ild, "ipd_deg": ipd}
        n_l, n_r = int(lens[2 * p]), int(lens[2 * p + 1])
        lo, hi = max(-D, -(n_r - 1)), min(D, n_l - 1)
        if energy[p, 0] * energy[p, 1] <= 0 or lo > hi:
            res.update(lags_ms=np.array([]), iacf=np.array([]), iacc=np.nan, tau_ms=np.nan)
        else:
            lags_ms = np.arange(lo, hi + 1) * 1000 / fs
            row = iacf[p, lo + D:hi + D + 1].copy()
            k = int(peak[p]) - (lo + D)
            res.update(lags_ms=lags_ms, iacf=row, iacc=float(np.abs(row[k])), tau_ms=float(lags_ms[k]))
        if edc:
            res["edc_db"] = (curves[2 * p], curves[2 * p + 1])
        out.append(res)
    return out


def band_interaural_level_difference(left, right, fs, bands):
    """ILD per band in dB, left over right power (reference :61-69)."""
    return binaural_metrics([(np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64))], fs, bands,
                            max_delay_ms=0.0)[0]["ild_db"]


def band_interaural_phase_difference(left, right, fs, bands):
    """IPD per band in degrees, left minus right: the angle of the band's cross-spectrum sum (reference :72-87)."""
    return binaural_metrics([(np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64))], fs, bands,
                            max_delay_ms=0.0)[0]["ipd_deg"]


def energy_decay_curve_db(data, floor_db=-80.0):
    """Schroeder energy decay curve in dB re the total energy; floor_db for a signal without energy (reference :90-100)."""
    ctx = _native.default_context()
    data = np.asarray(data, dtype=np.float64)
    if not len(data):
        return np.full(0, floor_db)
    return ctx.energy_decay_db([data], floor_db)[0]


def interaural_cross_correlation(left, right, fs, max_delay_ms=1.0):
    """(lags_ms, iacf, iacc, tau_ms) of ISO 3382-1's normalised interaural cross-correlation within +-max_delay_ms
    (reference :103-138); (array([]), array([]), nan, nan) when an ear has no energy."""
    res = binaural_metrics([(np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64))], fs, [],
                           max_delay_ms=max_delay_ms)[0]
    return res["lags_ms"], res["iacf"], res["iacc"], res["tau_ms"]
