#!/usr/bin/env python3
"""Wall time of the binaural analysis metrics (K15) for a C2 measurement's finished rows (48 kHz, 8 speaker pairs of n
samples, device resident): one HRIR and G HRIRs batched, with and without the decay curves, and the reference's formulation
(scipy.fft.fft, scipy.signal.correlate, np.cumsum) on the host for the same rows.  Every timing ends in a device
synchronise; every shape is warmed first.  Prints one JSON line.
python tools/binaural_analysis_rate.py [n=42000] [G=8] [reps=20]      (per-kernel device times: run under rocprofv3 --stats)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "impulcifer-pip313_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

FS = 48000
PAIRS = 8


def responses(seed, n):
    rng = np.random.default_rng(seed)
    pairs = []
    for k in range(PAIRS):
        d = 40 + 5 * k
        x = np.zeros(n + 8)
        x[d] = 1.0
        x[d:] += 0.05 * rng.standard_normal(n + 8 - d) * np.exp(-np.arange(n + 8 - d) / (0.05 * FS))
        left = x[:n] + 0.01 * rng.standard_normal(n)
        right = 0.8 * x[3:3 + n] + 0.01 * rng.standard_normal(n)
        pairs.append((left.astype(np.float32), right.astype(np.float32)))
    return pairs


def host_formulation(pairs, bands, max_delay_ms=1.0):
    """the reference's arithmetic (core/plotting/analysis.py) restated with the same library calls"""
    from scipy import signal
    from scipy.fft import fft, next_fast_len
    out = []
    for left, right in pairs:
        left, right = np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64)
        nfft = next_fast_len(max(len(left), len(right)))
        fl, fr = fft(left, n=nfft), fft(right, n=nfft)
        freqs = np.fft.fftfreq(nfft, d=1 / FS)
        cross = fl * np.conj(fr)
        sums = []
        for lo, hi in bands:
            idx = np.where((freqs >= lo) & (freqs < min(hi, FS / 2)))[0]
            sums.append((np.sum(np.abs(fl[idx]) ** 2), np.sum(np.abs(fr[idx]) ** 2), np.sum(cross[idx])))
        energy = np.sum(left ** 2) * np.sum(right ** 2)
        corr = signal.correlate(left, right, mode="full") / np.sqrt(energy)
        lags = signal.correlation_lags(len(left), len(right), mode="full")
        iacf = corr[np.abs(lags) <= round(max_delay_ms * FS / 1000)]
        edc = [np.cumsum((x ** 2)[::-1])[::-1] for x in (left, right)]
        out.append((sums, iacf, [10 * np.log10(e / (np.max(e) + 1e-12) + 1e-12) for e in edc]))
    return out


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return round(float(np.median(out)) * 1e3, 3), round(float(np.min(out)) * 1e3, 3)


def main():
    from impulse_hip import _native, analysis
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.impulse_response import ImpulseResponse
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 42000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    ctx = _native.default_context()
    sets = [responses(s, n) for s in range(G)]
    pitch = (n + 63) // 64 * 64
    block = DeviceBlock(ctx, pitch * 2 * PAIRS * G)
    flat = np.zeros(pitch * 2 * PAIRS * G, dtype=np.float32)
    irs = []
    for i, x in enumerate(x for s in sets for pair in s for x in pair):
        flat[i * pitch:i * pitch + n] = x
        irs.append(ImpulseResponse.on_device(Row(block, i * pitch, n), FS))
    ctx.h2d(block.ptr, flat)
    pairs = list(zip(irs[0::2], irs[1::2]))
    bands = analysis.octave_bands(FS)

    def run(count, edc):
        analysis.binaural_metrics(pairs[:count], FS, edc=edc)
        ctx.synchronize()

    res = {"what": "binaural_analysis_rate", "fs": FS, "pairs_per_hrir": PAIRS, "n": n, "G": G, "reps": reps}
    for label, count in (("one_hrir_ms", PAIRS), ("batched_ms", PAIRS * G)):
        for edc in (False, True):
            run(count, edc)                                          # warm: roots, pool blocks, staging ring
            med, low = timed(lambda: run(count, edc), reps)
            hrirs = count // PAIRS
            res[label + ("_with_edc" if edc else "")] = {"median": med, "min": low, "per_hrir": round(med / hrirs, 3)}
    host_formulation(sets[0], bands)
    res["host_reference_formulation_one_hrir_ms"] = dict(zip(("median", "min"), timed(lambda: host_formulation(sets[0], bands), 5)))
    assert all(ir._data is None for ir in irs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
