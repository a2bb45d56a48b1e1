#!/usr/bin/env python3
"""Wall time of resampling a C2 HRIR (16 device-resident responses of n samples, 16 001-tap filter) at 48 k -> 44.1 k
(147/160, about 109 taps per output sample) and 48 k -> 96 k (2/1, 8 001 taps per output sample): the device path (K17,
resample_rows on device rows, the results left on the device, timed to the end of the stream's work) and
scipy.signal.resample_poly with the same filter on this machine's host, row after row, in the same run.  The filter design
is warmed first and is not in either figure.  Also the largest difference between the two, relative to each row's largest
sample.  Prints one JSON line and exits 1 if the device path does not beat the host at both ratios.
python tools/resample_rate.py [n=60000] [reps=5] [host_reps=1]      (per-kernel device times: run under rocprofv3 --stats)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "impulcifer-pip313_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

CHANNELS = 16
RATES = [(44100, 48000), (96000, 48000)]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return round(float(np.median(out)) * 1e3, 3), round(float(np.min(out)) * 1e3, 3)


def main():
    from scipy.signal import resample_poly
    from impulse_hip import _native, resampling
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.impulse_response import ImpulseResponse
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    host_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 1
    ctx = _native.default_context()
    rng = np.random.default_rng(0)
    pitch = (n + 63) // 64 * 64
    flat = np.zeros(pitch * CHANNELS, dtype=np.float32)
    for i in range(CHANNELS):
        flat[i * pitch:i * pitch + n] = rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 8.0))
    block = DeviceBlock(ctx, pitch * CHANNELS)
    ctx.h2d(block.ptr, flat)
    host_rows = [flat[i * pitch:i * pitch + n].astype(np.float64) for i in range(CHANNELS)]
    res = {"what": "resample_rate", "channels_per_hrir": CHANNELS, "n": n, "taps": 16001, "reps": reps, "host_reps": host_reps}
    ok = True
    for fs_new, fs_old in RATES:
        irs = [ImpulseResponse.on_device(Row(block, i * pitch, n), fs_old) for i in range(CHANNELS)]
        taps = resampling.kaiser_null_filter(fs_new, fs_old)

        def device():
            out = resampling.resample_rows(irs, fs_new, fs_old)
            ctx.synchronize()
            return out

        got = device()                                               # warm: the pool's blocks, the staging ring
        dev = dict(zip(("median", "min"), timed(device, reps)))
        want = [resample_poly(x, fs_new, fs_old, window=taps) for x in host_rows[:2]]
        host = dict(zip(("median", "min"), timed(lambda: [resample_poly(x, fs_new, fs_old, window=taps) for x in host_rows], host_reps)))
        # fp32 rows: one rounding of the result on top of the arithmetic
        diff = max(float(np.max(np.abs(g.peek() - w)) / np.max(np.abs(w))) for g, w in zip(got, want))
        key = f"{fs_old}_to_{fs_new}"
        res[key] = {"device_ms_per_hrir": dev, "host_scipy_ms_per_hrir": host, "speedup": round(host["median"] / dev["median"], 1),
                    "max_difference_from_scipy_rel": diff}
        ok = ok and dev["median"] < host["median"] and diff < 1e-6
        assert all(ir._data is None for ir in irs) and all(g._data is None for g in got)
    res["device_beats_host_at_both_ratios"] = ok
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
