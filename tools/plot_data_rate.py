#!/usr/bin/env python3
"""Wall time of the spectrogram data (K16) for a C2 measurement's recordings (48 kHz, 16 channels of n samples, device
resident: nfft 4800, 200 segments): one HRIR and G HRIRs batched, float64 and float32 output, the waterfall data of the 16
responses, and scipy.signal.spectrogram on the host for the same recordings.  Every timing ends with the results on the host;
every shape is warmed first.  Prints one JSON line.
python tools/plot_data_rate.py [n=391270] [G=8] [reps=5]      (per-kernel device times: run under rocprofv3 --stats)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "impulcifer-pip313_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

FS = 48000
CHANNELS = 16


def host_spectrograms(rows, nfft, noverlap):
    """the reference's arithmetic (plot_spectrogram) with the same library calls"""
    from scipy import signal
    out = []
    for x in rows:
        f, t, s = signal.spectrogram(np.asarray(x, dtype=np.float64), fs=FS, window=signal.get_window("hann", nfft), nperseg=nfft,
                                     noverlap=noverlap, mode="psd")
        out.append(10 * np.log10(np.abs(s[1:, :]) + 1e-9))
    return out


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return round(float(np.median(out)) * 1e3, 3), round(float(np.min(out)) * 1e3, 3)


def main():
    from impulse_hip import _native, plot_data
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.impulse_response import ImpulseResponse
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 391270
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    ctx = _native.default_context()
    rng = np.random.default_rng(0)
    t = np.arange(n) / FS
    T = n / FS
    sweep = np.sin(2 * np.pi * 20.0 * T / np.log(1000.0) * (np.exp(t / T * np.log(1000.0)) - 1))
    pitch = (n + 63) // 64 * 64
    count = CHANNELS * G
    block = DeviceBlock(ctx, pitch * count)
    flat = np.zeros(pitch * count, dtype=np.float32)
    recs = []
    for i in range(count):
        flat[i * pitch:i * pitch + n] = (0.3 + 0.05 * (i % 7)) * sweep + 0.01 * rng.standard_normal(n)
        recs.append(ImpulseResponse.on_device(Row(block, i * pitch, n), FS))
    ctx.h2d(block.ptr, flat)
    nfft, noverlap = plot_data.spectrogram_geometry(n, FS)
    segments = (n - noverlap) // (nfft - noverlap)
    res = {"what": "plot_data_rate", "fs": FS, "channels_per_hrir": CHANNELS, "n": n, "nfft": nfft, "noverlap": noverlap,
           "segments": segments, "G": G, "reps": reps}
    for label, rows in (("one_hrir_ms", recs[:CHANNELS]), ("batched_ms", recs)):
        for dtype in (np.float64, np.float32):
            plot_data.spectrograms(rows, FS, dtype=dtype)             # warm: roots, pool blocks, staging ring
            med, low = timed(lambda: plot_data.spectrograms(rows, FS, dtype=dtype), reps)
            res[label + ("_f32" if dtype is np.float32 else "")] = {"median": med, "min": low, "per_hrir": round(med / (len(rows) // CHANNELS), 3)}
    irs = recs[:CHANNELS]                                             # any 16 device rows of more than 1792 samples
    plot_data.waterfalls(irs, FS)
    res["waterfalls_one_hrir_ms"] = dict(zip(("median", "min"), timed(lambda: plot_data.waterfalls(irs, FS), reps)))
    plot_data.waterfall_magnitudes(irs, FS)
    res["waterfall_magnitudes_one_hrir_ms"] = dict(zip(("median", "min"), timed(lambda: plot_data.waterfall_magnitudes(irs, FS), reps)))
    host_rows = [flat[i * pitch:i * pitch + n] for i in range(CHANNELS)]
    got = plot_data.spectrograms(irs, FS)
    want = host_spectrograms(host_rows, nfft, noverlap)
    res["max_abs_difference_from_scipy_db"] = float(max(np.max(np.abs(a[2] - b)) for a, b in zip(got, want)))
    res["host_scipy_one_hrir_ms"] = dict(zip(("median", "min"), timed(lambda: host_spectrograms(host_rows, nfft, noverlap), 3)))
    assert all(ir._data is None for ir in recs)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
