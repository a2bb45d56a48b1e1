"""NumPy model of the microphone-deviation stage (core/microphone_deviation_correction.py), for the tests.

Written from the reference's description of the stage: direct-sound window around the first peak, zero-padded spectrum
re-gridded as power, anchor mean per ear, interaural dB ratio, fractional-octave smoothing, band weight, clamps, two
minimum-phase FIRs and the full convolution of every row.  Smoothing and FIR design come from the oracle (pure NumPy).
"""
import numpy as np

CENTER = ("FC", "TFC", "BC")


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


def lengths(fs, window_ms=5.0, pre_ms=0.5):
    return max(int(round(window_ms * fs / 1000.0)), 32), max(int(round(pre_ms * fs / 1000.0)), 0)


def grid(fs):
    out, f = [], 20.0
    while f <= fs / 2.0:
        out.append(f)
        f *= 1.01
    return np.array(out)


def half_hann(m):
    """np.hanning(m) written out: 0.5 + 0.5 cos(pi k / (m - 1)), k = 1 - m, 3 - m, ..., m - 1"""
    k = np.arange(1 - m, m, 2)
    return 0.5 + 0.5 * np.cos(np.pi * k / (m - 1))


def power(row, peak, fs, win, pre, freq=None):
    freq = grid(fs) if freq is None else freq
    row = np.asarray(row, dtype=np.float64)
    n = len(row)
    if n == 0:
        return np.zeros_like(freq)
    peak = min(max(int(peak), 0), n - 1)
    seg = row[max(peak - pre, 0):min(peak + win, n)].copy()
    L = len(seg)
    if L < 8:
        return np.zeros_like(freq)
    fi, fo = min(pre, L // 4), max(L // 4, 1)
    if fi > 1:
        seg[:fi] *= half_hann(2 * fi)[:fi]
    if fo > 1:
        seg[L - fo:] *= half_hann(2 * fo)[fo:]
    nfft = fast_len_11(max(L, 8192))
    mag = np.abs(np.fft.rfft(seg, nfft))
    bins = np.arange(nfft // 2 + 1) * (1.0 / (nfft * (1.0 / fs)))
    return np.interp(freq, bins, mag, left=mag[0], right=mag[-1]) ** 2


def anchors(speakers, anchor):
    center = [s for s in speakers if s in CENTER]
    if anchor in ("auto", "frontal") and center:
        return center, "frontal"
    return list(speakers), "diffuse"


def raw_mismatch(irs, fs, anchor="auto", peaks=None):
    """irs {speaker: {"left", "right"}} -> (raw dB curve, anchor used, powers {speaker: (left, right)})"""
    from oracle.impulse_response import peak_index
    win, pre = lengths(fs)
    freq = grid(fs)
    pw = {}
    for sp, pair in irs.items():
        pl = peak_index(pair["left"]) if peaks is None else peaks[sp][0]
        pr = peak_index(pair["right"]) if peaks is None else peaks[sp][1]
        pw[sp] = (power(pair["left"], pl, fs, win, pre, freq), power(pair["right"], pr, fs, win, pre, freq))
    use, used = anchors(list(irs), anchor)
    left = np.mean([pw[s][0] for s in use], axis=0)
    right = np.mean([pw[s][1] for s in use], axis=0)
    return 10.0 * np.log10((left + 1e-20) / (right + 1e-20)), used, pw


def band_weight(fs, f_min=200.0, f_max=16000.0):
    nyq = fs / 2.0
    f_min = float(np.clip(f_min, 1.0, nyq * 0.5))
    f_max = float(np.clip(f_max, f_min * 2.0, nyq * 0.98))
    lf = np.log10(grid(fs))
    lo1, lo2 = np.log10(max(f_min / 2.0, 1.0)), np.log10(f_min)
    hi1, hi2 = np.log10(f_max), np.log10(min(f_max * 2.0, fs / 2.0 * 0.999))
    w = np.ones_like(lf)
    w[lf < lo1] = 0.0
    m = (lf >= lo1) & (lf < lo2)
    w[m] = 0.5 - 0.5 * np.cos(np.pi * (lf[m] - lo1) / max(lo2 - lo1, 1e-9))
    w[lf > hi2] = 0.0
    m = (lf > hi1) & (lf <= hi2)
    w[m] = 0.5 + 0.5 * np.cos(np.pi * (lf[m] - hi1) / max(hi2 - hi1, 1e-9))
    return w


def mismatch(raw, fs, max_db=6.0):
    from oracle.frequency_response import smoothen
    sm = smoothen(grid(fs), raw, 1 / 6, 1 / 6, 100.0, 10000.0)
    return np.clip(sm * band_weight(fs), -2 * max_db, 2 * max_db)


def summary(mis, fs, strength, max_db=6.0):
    strength = float(np.clip(strength, 0.0, 1.0))
    applied = np.clip(mis * strength / 2.0, -max_db, max_db)
    nz = np.abs(applied[band_weight(fs) > 0])
    return float(np.mean(nz)), float(np.max(nz))


def firs(mis, fs, strength, max_db=6.0):
    from oracle.minphase import minimum_phase_impulse_response
    half = np.clip(mis * float(np.clip(strength, 0.0, 1.0)) / 2.0, -max_db, max_db)
    keep = min(2048, fs // 10)
    return [minimum_phase_impulse_response(grid(fs), c, fs, f_res=10, normalize=False)[:keep] for c in (-half, half)]


def stage(irs, fs, strength=0.7, anchor="auto"):
    """the whole stage: (rows {speaker: {side: array}}, anchor used, mismatch, (avg, max), skipped, (left FIR, right FIR))"""
    raw, used, _ = raw_mismatch(irs, fs, anchor)
    mis = mismatch(raw, fs)
    avg, mx = summary(mis, fs, strength)
    if mx < 0.05:
        return {sp: dict(pair) for sp, pair in irs.items()}, used, mis, (avg, mx), True, None
    lf, rf = firs(mis, fs, strength)
    rows = {sp: {"left": np.convolve(pair["left"], lf), "right": np.convolve(pair["right"], rf)} for sp, pair in irs.items()}
    return rows, used, mis, (avg, mx), False, (lf, rf)
