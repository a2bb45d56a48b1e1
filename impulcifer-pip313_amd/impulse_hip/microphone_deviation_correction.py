"""Interaural microphone-deviation correction (surface of reference core/microphone_deviation_correction.py:42-417).

The direction-independent left/right magnitude difference of the microphones is estimated from the direct sound of every
speaker and corrected with two minimum-phase FIRs (left -delta/2, right +delta/2).  The arithmetic runs on the device:
  - direct-sound power on the log grid and the interaural dB ratio of the anchor speakers: K14 (imp_mic_mismatch*), every
    row of every HRIR of a call in one launch sequence, on device rows where they are;
  - fractional-octave smoothing of the ratio: K12 (smooth_curves), all HRIRs in one call;
  - the two FIRs per HRIR: K6 (minimum_phase_impulse_responses, f_res = 10, not normalised), all HRIRs in one call;
  - the full convolution of every speaker with its ear's FIR: K5 (HRIR.equalize_channels), one call per HRIR.
Band weight, clamps and the summary scalars are a few hundred numbers per HRIR and follow the reference's NumPy on the host.

The skip test (max_error_db < 0.05) is a decision on a float: when max_error_db lies within DECISION_GUARD_DB of the
threshold the HRIR's analysis is recomputed on the host with np.fft / np.interp (the reference's arithmetic) and the
decision is taken from that.  Plots are not provided: plot_analysis=True warns and goes on.
"""
import warnings

import numpy as np

from . import _native
from .frequency_response import generate_frequencies, minimum_phase_impulse_responses, smooth_curves

_CENTER_SPEAKERS = ("FC", "TFC", "BC")
_SINGLE_SPEAKER = "SINGLE"
_EPS = 1e-20
_BANDS = (250, 500, 1000, 2000, 4000, 8000)
SKIP_BELOW_DB = 0.05            # the reference's threshold on max_error_db
DECISION_GUARD_DB = 1e-9        # |max_error_db - SKIP_BELOW_DB| below this: decided from the host analysis
MIN_SEGMENT = 8                 # shorter direct-sound segments have zero power


def next_fast_len_11(n):
    """scipy.fft.next_fast_len(n) as the reference calls it (real=False): the smallest 2^a 3^b 5^c 7^d 11^e >= n."""
    m = max(int(n), 1)
    while True:
        r = m
        for p in (2, 3, 5, 7, 11):
            while r % p == 0:
                r //= p
        if r == 1:
            return m
        m += 1


def analysis_lengths(fs, window_ms=5.0, pre_ms=0.5):
    """(win, pre) in samples as the reference's constructor forms them (round() is Python's half-to-even)."""
    win = max(int(round(float(window_ms) * int(fs) / 1000.0)), 32)
    pre = max(int(round(float(pre_ms) * int(fs) / 1000.0)), 0)
    return win, pre


def segment_bounds(n, peak, win, pre):
    """(start, end, nfft) of a row's analysis segment (reference :114-129)"""
    peak = int(np.clip(peak, 0, max(n - 1, 0)))
    start, end = max(peak - pre, 0), min(peak + win, n)
    return start, end, next_fast_len_11(max(end - start, 8192))


def anchor_flags(speakers, anchor):
    """(per-speaker anchor flags, anchor used): the speakers of _CENTER_SPEAKERS that are present for 'auto' / 'frontal',
    every speaker otherwise or when none is present (reference :207-218)"""
    center = [s for s in speakers if s in _CENTER_SPEAKERS]
    if (anchor == "frontal" and center) or (anchor == "auto" and center):
        return [s in _CENTER_SPEAKERS for s in speakers], "frontal"
    return [True] * len(speakers), "diffuse"


def _host_windowed_power(ir, peak, fs, win, pre, frequency):
    """The reference's _windowed_power (:106-140) in NumPy: the host side of the guarded decision."""
    ir = np.asarray(ir, dtype=float)
    n = len(ir)
    if n == 0:
        return np.zeros_like(frequency)
    start, end, nfft = segment_bounds(n, peak, win, pre)
    seg = ir[start:end]
    if len(seg) < MIN_SEGMENT:
        return np.zeros_like(frequency)
    w = np.ones(len(seg))
    fade_in = min(pre, len(seg) // 4)
    if fade_in > 1:
        w[:fade_in] = np.hanning(2 * fade_in)[:fade_in]
    fade_out = max(len(seg) // 4, 1)
    if fade_out > 1:
        w[-fade_out:] = np.hanning(2 * fade_out)[fade_out:]
    mag = np.abs(np.fft.rfft(seg * w, n=nfft))
    return np.interp(frequency, np.fft.rfftfreq(nfft, 1.0 / fs), mag, left=mag[0], right=mag[-1]) ** 2


def _rows_of(pairs):
    """(device rows or None, host rows) of [(speaker, left_ir, right_ir)] in row order left, right, left, ..."""
    irs = [ir for _, l, r in pairs for ir in (l, r)]
    rows = [getattr(ir, "_row", None) if getattr(ir, "_data", 0) is None else None for ir in irs]
    ctx = _native.default_context()
    if rows and all(r is not None and r.block.ctx is ctx for r in rows):
        return rows, None
    return None, [np.asarray(ir.data, dtype=np.float64) for ir in irs]


def interaural_mismatch_raw(groups, fs, win, pre, frequency, anchor="auto", want_power=False):
    """K14 for G groups (one per HRIR) of [(speaker, left ImpulseResponse, right ImpulseResponse)] at one rate: the peaks
    (K3) and then one launch sequence for every row.  Returns (raw [G, M], power [2 S, M] or None, anchors used, peaks)."""
    pairs = [p for g in groups for p in g]
    group = np.repeat(np.arange(len(groups)), [2 * len(g) for g in groups])
    side = np.tile([0, 1], len(pairs))
    flags, used = [], []
    for g in groups:
        f, u = anchor_flags([sp for sp, _, _ in g], anchor)
        flags.extend(v for v in f for _ in (0, 1))
        used.append(u)
    ctx = _native.default_context()
    dev, host = _rows_of(pairs)
    if dev is not None:
        from .device_rows import span
        base, offs, lens = span(dev)
        peaks, _ = ctx.peak_index_device(base, offs, lens)
        raw, power = ctx.mic_mismatch((offs, lens), peaks, group, side, flags, len(groups), win, pre, fs, frequency,
                                      want_power=want_power, dptr=base)
    else:
        peaks = np.zeros(len(host), dtype=np.int64)
        live = [k for k, r in enumerate(host) if len(r)]
        if live:
            peaks[live] = ctx.peak_index([host[k] for k in live])[0]
        raw, power = ctx.mic_mismatch(host, peaks, group, side, flags, len(groups), win, pre, fs, frequency,
                                      want_power=want_power)
    return raw, power, used, peaks


class MicrophoneMatchingCorrector:
    """Direction-independent interaural microphone mismatch correction (reference :50-321)."""

    def __init__(self, sample_rate, correction_strength=0.7, max_correction_db=6.0, smoothing_octave=1.0 / 6.0, f_min=200.0,
                 f_max=16000.0, window_ms=5.0, pre_ms=0.5, anchor="auto"):
        self.fs = int(sample_rate)
        self.correction_strength = float(np.clip(correction_strength, 0.0, 1.0))
        self.max_correction_db = float(max_correction_db)
        self.smoothing_octave = float(smoothing_octave)
        nyq = self.fs / 2.0
        self.f_min = float(np.clip(f_min, 1.0, nyq * 0.5))
        self.f_max = float(np.clip(f_max, self.f_min * 2.0, nyq * 0.98))
        self.window_ms = float(window_ms)
        self.pre_ms = float(pre_ms)
        self.anchor = anchor
        self.win_samples, self.pre_samples = analysis_lengths(self.fs, self.window_ms, self.pre_ms)
        self.frequency = generate_frequencies(f_step=1.01, f_min=20.0, f_max=nyq)
        self.speaker_power = {}
        self.mismatch_db = None
        self.anchor_used = None
        self._rows = {}                 # speaker -> (left, right, left peak, right peak): what estimate runs K14 on

    # ---- analysis --------------------------------------------------------------------------------
    def _powers(self, rows, peaks):
        """K14 power of host rows (every row its own ear of group 0)"""
        rows = [np.asarray(r, dtype=float) for r in rows]
        peaks = [int(np.argmax(np.abs(r))) if (p is None and len(r)) else (0 if p is None else int(p))
                 for r, p in zip(rows, peaks)]
        _, power = _native.default_context().mic_mismatch(rows, peaks, [0] * len(rows), [0, 1] * (len(rows) // 2),
                                                          [1] * len(rows), 1, self.win_samples, self.pre_samples, self.fs,
                                                          self.frequency, want_power=True)
        return power

    def _windowed_power(self, ir, peak_index):
        return self._powers([ir, ir], [peak_index, peak_index])[0]

    def collect_speaker(self, speaker_name, left_ir, right_ir, left_peak_index=None, right_peak_index=None):
        left_ir, right_ir = np.asarray(left_ir, dtype=float), np.asarray(right_ir, dtype=float)
        power = self._powers([left_ir, right_ir], [left_peak_index, right_peak_index])
        self._rows[speaker_name] = (left_ir, right_ir, left_peak_index, right_peak_index)
        self.speaker_power[speaker_name] = {"left": power[0], "right": power[1]}
        return self.speaker_power[speaker_name]

    def collect_speaker_deviation(self, speaker_name, left_ir, right_ir, left_peak_index=None, right_peak_index=None):
        self.collect_speaker(speaker_name, left_ir, right_ir, left_peak_index, right_peak_index)
        p = self.speaker_power[speaker_name]
        delta = 10.0 * np.log10((p["left"] + _EPS) / (p["right"] + _EPS))
        return {b: float(np.interp(b, self.frequency, delta)) for b in _BANDS if b < self.fs / 2}

    def _band_weight(self):
        """1 inside [f_min, f_max], log-axis raised-cosine tapers to 0 outside (reference :166-191)."""
        f = self.frequency
        w = np.ones_like(f)
        logf = np.log10(f)
        lo2, lo1 = np.log10(self.f_min), np.log10(max(self.f_min / 2.0, 1.0))
        hi1 = np.log10(self.f_max)
        hi2 = np.log10(min(self.f_max * 2.0, self.fs / 2.0 * 0.999))
        low_band = (logf >= lo1) & (logf < lo2)
        w[logf < lo1] = 0.0
        if np.any(low_band):
            x = (logf[low_band] - lo1) / max(lo2 - lo1, 1e-9)
            w[low_band] = 0.5 - 0.5 * np.cos(np.pi * x)
        high_band = (logf > hi1) & (logf <= hi2)
        w[logf > hi2] = 0.0
        if np.any(high_band):
            x = (logf[high_band] - hi1) / max(hi2 - hi1, 1e-9)
            w[high_band] = 0.5 + 0.5 * np.cos(np.pi * x)
        return w

    def _finish(self, raws):
        """smoothing (K12, every row of raws [G, M] at once), band weight, +-2 max clip (reference :220-235)"""
        raws = np.atleast_2d(np.asarray(raws, dtype=np.float64))
        smoothed = smooth_curves(self.frequency, raws, self.smoothing_octave, self.smoothing_octave, 100.0, 10000.0)
        smoothed = np.atleast_2d(smoothed) * self._band_weight()
        return np.clip(smoothed, -2.0 * self.max_correction_db, 2.0 * self.max_correction_db)

    def estimate_interaural_mismatch(self):
        if not self.speaker_power:
            warnings.warn("no speaker data collected; call collect_speaker first")
            self.mismatch_db = np.zeros_like(self.frequency)
            self.anchor_used = "none"
            return self.mismatch_db
        names = list(self._rows)
        flags, self.anchor_used = anchor_flags(names, self.anchor)
        rows = [r for sp in names for r in self._rows[sp][:2]]
        peaks = [p for sp in names for p in self._powers_peaks(sp)]
        raw, _ = _native.default_context().mic_mismatch(rows, peaks, [0] * len(rows), [0, 1] * len(names),
                                                        [f for f in flags for _ in (0, 1)], 1, self.win_samples,
                                                        self.pre_samples, self.fs, self.frequency)
        self.mismatch_db = self._finish(raw)[0]
        return self.mismatch_db

    def _powers_peaks(self, speaker):
        left, right, lp, rp = self._rows[speaker]
        return [int(np.argmax(np.abs(r))) if (p is None and len(r)) else (0 if p is None else int(p))
                for r, p in ((left, lp), (right, rp))]

    def separate_microphone_error(self):
        delta = self.estimate_interaural_mismatch()
        return {b: float(np.interp(b, self.frequency, delta)) for b in _BANDS if b < self.fs / 2}

    # ---- correction ------------------------------------------------------------------------------
    def _half(self, mismatch=None):
        mismatch = self.mismatch_db if mismatch is None else mismatch
        return np.clip((mismatch * self.correction_strength) / 2.0, -self.max_correction_db, self.max_correction_db)

    def design_correction_filters(self):
        """(left FIR, right FIR): -delta/2 and +delta/2 through K6 in one batch (reference :244-276)."""
        if self.mismatch_db is None:
            self.estimate_interaural_mismatch()
        return tuple(design_filters(self, [self.mismatch_db])[0])

    def get_analysis_summary(self):
        if self.mismatch_db is None:
            return {"error": "분석 미완료"}
        return _summary(self, self.mismatch_db, self.anchor_used, list(self.speaker_power.keys()))


def design_filters(corrector, mismatches):
    """[(left FIR, right FIR)] of every mismatch curve, all 2 G curves in one K6 call (f_res = 10, normalize=False)."""
    if not len(mismatches):
        return []
    curves = []
    for m in mismatches:
        delta = np.asarray(m) * corrector.correction_strength
        half = np.clip(delta / 2.0, -corrector.max_correction_db, corrector.max_correction_db)
        curves.extend((-half, half))
    firs = minimum_phase_impulse_responses(corrector.frequency, np.stack(curves), corrector.fs, f_res=10, normalize=False)
    max_len = min(2048, corrector.fs // 10)
    firs = [np.asarray(f)[:max_len] for f in firs]
    return [(firs[2 * i], firs[2 * i + 1]) for i in range(len(mismatches))]


def _summary(corrector, mismatch, anchor_used, speakers):
    applied = corrector._half(mismatch)
    nz = np.abs(applied[corrector._band_weight() > 0])
    return {
        "method": "interaural_v4",
        "anchor": anchor_used,
        "avg_error_db": float(np.mean(nz)) if len(nz) else 0.0,
        "max_error_db": float(np.max(nz)) if len(nz) else 0.0,
        "speakers_analyzed": list(speakers),
        "correction_strength": corrector.correction_strength,
    }


def _host_analysis(corrector, pairs, peaks):
    """(mismatch, anchor used) of one group from the reference's NumPy arithmetic (the guarded decision)"""
    names = [sp for sp, _, _ in pairs]
    flags, used = anchor_flags(names, corrector.anchor)
    power = [_host_windowed_power(ir.peek(), pk, corrector.fs, corrector.win_samples, corrector.pre_samples,
                                  corrector.frequency) for (_, l, r), pl, pr in zip(pairs, peaks[0::2], peaks[1::2])
             for ir, pk in ((l, pl), (r, pr))]
    sel = [k for k, f in enumerate(flags) if f]
    left = np.mean([power[2 * k] for k in sel], axis=0)
    right = np.mean([power[2 * k + 1] for k in sel], axis=0)
    raw = 10.0 * np.log10((left + _EPS) / (right + _EPS))
    return corrector._finish(raw)[0], used


def _near_threshold(value):
    return abs(value - SKIP_BELOW_DB) <= DECISION_GUARD_DB


def apply_microphone_deviation_correction_to_hrirs(hrirs, correction_strength=0.7, anchor="auto", plot_analysis=False,
                                                   plot_dir=None):
    """apply_microphone_deviation_correction_to_hrir for many HRIRs: one K14 sequence, one K12 and one K6 call per sampling
    rate for all of them, then one K5 batch per HRIR (its rows live in a device block of their own).  Returns the
    summaries in the order of `hrirs`; each HRIR ends exactly as the single form leaves it."""
    hrirs = list(hrirs)
    out = [None] * len(hrirs)
    if plot_analysis and plot_dir:
        warnings.warn("microphone-deviation plots are not provided; the correction goes on without them")
    by_fs = {}
    for i, h in enumerate(hrirs):
        pairs = [(sp, pair["left"], pair["right"]) for sp, pair in h.irs.items()]
        if not pairs:
            out[i] = {"error": "스피커 데이터 없음"}
            continue
        by_fs.setdefault(int(h.fs), []).append((i, pairs))
    for fs, items in by_fs.items():
        corr = MicrophoneMatchingCorrector(sample_rate=fs, correction_strength=correction_strength, anchor=anchor)
        raw, power, used, peaks = interaural_mismatch_raw([p for _, p in items], fs, corr.win_samples, corr.pre_samples,
                                                          corr.frequency, anchor=anchor)
        mismatch = corr._finish(raw)
        todo, r0 = [], 0
        for (i, pairs), m, u in zip(items, mismatch, used):
            names = [sp for sp, _, _ in pairs]
            summary = _summary(corr, m, u, names)
            if _near_threshold(summary["max_error_db"]):
                m, u = _host_analysis(corr, pairs, peaks[r0:r0 + 2 * len(pairs)])
                summary = _summary(corr, m, u, names)
            r0 += 2 * len(pairs)
            out[i] = summary
            if summary["max_error_db"] < SKIP_BELOW_DB:
                summary["speakers_processed"] = []
            else:
                todo.append((i, names, m))
        firs = design_filters(corr, [m for _, _, m in todo])
        for (i, names, _), (lf, rf) in zip(todo, firs):
            hrirs[i].equalize_channels({(sp, sd): (lf if sd == "left" else rf) for sp in names for sd in ("left", "right")})
            out[i]["speakers_processed"] = list(names)
    return out


def apply_microphone_deviation_correction_to_hrir(hrir, correction_strength=0.7, anchor="auto", plot_analysis=False,
                                                  plot_dir=None):
    """The reference's entry point (:324-382): analyse every speaker's direct sound, correct both ears of every speaker
    with +-delta/2 minimum-phase FIRs (ITD kept).  Returns the analysis summary."""
    return apply_microphone_deviation_correction_to_hrirs([hrir], correction_strength, anchor, plot_analysis, plot_dir)[0]


class MicrophoneDeviationCorrector(MicrophoneMatchingCorrector):
    """Compatibility wrapper (reference :254-321); unused v2/v3 keywords are ignored."""

    def __init__(self, sample_rate, correction_strength=0.7, max_correction_db=6.0, smoothing_octave=1.0 / 6.0, f_min=200.0,
                 f_max=16000.0, window_ms=5.0, anchor="auto", **legacy_kwargs):
        super().__init__(sample_rate=sample_rate, correction_strength=correction_strength, max_correction_db=max_correction_db,
                         smoothing_octave=smoothing_octave, f_min=f_min, f_max=f_max, window_ms=window_ms, anchor=anchor)
        if legacy_kwargs.get("enable_phase_correction"):
            warnings.warn("enable_phase_correction was removed: v4.0 corrects magnitude only (minimum phase) and keeps the ITD",
                          DeprecationWarning)

    def correct_microphone_deviation(self, left_ir, right_ir, left_peak_index=None, right_peak_index=None,
                                     plot_analysis=False, plot_dir=None):
        """One speaker pair (diagnostics / compatibility); the lengths are kept (signal.convolve(mode="same"))."""
        from .impulse_response import ImpulseResponse, fir_convolve_full_batch
        left_ir = np.asarray(left_ir, dtype=float)
        right_ir = np.asarray(right_ir, dtype=float)
        if len(left_ir) != len(right_ir):
            n = min(len(left_ir), len(right_ir))
            left_ir, right_ir = left_ir[:n], right_ir[:n]
        self.speaker_power.clear()
        self._rows.clear()
        self.collect_speaker(_SINGLE_SPEAKER, left_ir, right_ir, left_peak_index, right_peak_index)
        self.anchor = "diffuse"
        self.estimate_interaural_mismatch()
        applied = self._half()
        significant = float(np.max(np.abs(applied))) if len(applied) else 0.0
        if _near_threshold(significant):
            pairs = [(_SINGLE_SPEAKER, ImpulseResponse(left_ir, self.fs), ImpulseResponse(right_ir, self.fs))]
            self.mismatch_db, self.anchor_used = _host_analysis(self, pairs, self._powers_peaks(_SINGLE_SPEAKER))
            applied = self._half()
            significant = float(np.max(np.abs(applied))) if len(applied) else 0.0
        analysis = {"method": "interaural_v4", "anchor": self.anchor_used, "mismatch_db": self.mismatch_db,
                    "frequency": self.frequency}
        if significant < SKIP_BELOW_DB:
            analysis["correction_applied"] = False
            return left_ir.copy(), right_ir.copy(), analysis
        left_fir, right_fir = self.design_correction_filters()
        n = len(left_ir)
        full = fir_convolve_full_batch([left_ir, right_ir], [left_fir, right_fir])
        corrected = [y[(len(h) - 1) // 2:(len(h) - 1) // 2 + n] if len(y) else np.zeros(n)
                     for y, h in zip(full, (left_fir, right_fir))]
        summary = self.get_analysis_summary()
        analysis.update({"correction_applied": True, "correction_filters": {"left_fir": left_fir, "right_fir": right_fir},
                         "avg_error_db": summary["avg_error_db"], "max_error_db": summary["max_error_db"]})
        if plot_analysis and plot_dir:
            warnings.warn("microphone-deviation plots are not provided; the correction goes on without them")
        return corrected[0], corrected[1], analysis
