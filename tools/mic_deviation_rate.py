#!/usr/bin/env python3
"""Wall time of the microphone-deviation stage at C2 (48 kHz, 8 speakers, device rows of n samples): one HRIR
(apply_microphone_deviation_correction_to_hrir) and G HRIRs batched (apply_microphone_deviation_correction_to_hrirs), and
the NumPy model of the same stage on the host as the CPU baseline.  Prints one JSON line.
python tools/mic_deviation_rate.py [n=24000] [G=8] [reps=20]      (per-kernel device times: run under rocprofv3 --stats)"""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "impulcifer-pip313_amd"), os.path.join(ROOT, "tests", "model")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

SPEAKERS = ("FL", "FR", "FC", "BL", "BR", "SL", "SR", "WL")
FS = 48000


def responses(seed, n):
    rng = np.random.default_rng(seed)
    mic = np.array([1.0, 0.1, -0.05])
    irs = {}
    for k, sp in enumerate(SPEAKERS):
        d = 40 + 5 * k
        x = np.zeros(n)
        x[d] = 1.0
        x[d:] += 0.05 * rng.standard_normal(n - d) * np.exp(-np.arange(n - d) / (0.05 * FS))
        right = x.astype(np.float32).astype(np.float64)
        left = np.convolve(right, mic)[:n].astype(np.float32).astype(np.float64)
        irs[sp] = {"left": left, "right": right}
    return irs


def device_hrir(irs):
    from impulse_hip import _native
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse

    class Est:
        fs = FS

    rows = [irs[sp][sd] for sp in irs for sd in ("left", "right")]
    n = len(rows[0])
    pitch = (n + 63) // 64 * 64
    ctx = _native.default_context()
    block = DeviceBlock(ctx, pitch * len(rows))
    flat = np.zeros(pitch * len(rows), dtype=np.float32)
    for i, r in enumerate(rows):
        flat[i * pitch:i * pitch + n] = r
    ctx.h2d(block.ptr, flat)
    h = HRIR(Est())
    for i, (sp, sd) in enumerate((sp, sd) for sp in irs for sd in ("left", "right")):
        h.irs.setdefault(sp, {})[sd] = ImpulseResponse.on_device(Row(block, i * pitch, n), FS)
    return h


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)) * 1e3, float(np.min(out)) * 1e3


def main():
    from impulse_hip import _native
    from impulse_hip.microphone_deviation_correction import (apply_microphone_deviation_correction_to_hrir,
                                                             apply_microphone_deviation_correction_to_hrirs)
    import micdev_model as mm
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24000
    G = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    sets = [responses(s, n) for s in range(G)]
    ctx = _native.default_context()
    warnings.simplefilter("ignore")

    def one():
        h = device_hrir(sets[0])
        apply_microphone_deviation_correction_to_hrir(h)
        h.irs["FL"]["left"]._row.block.ctx.synchronize()

    def batch():
        hs = [device_hrir(s) for s in sets]
        apply_microphone_deviation_correction_to_hrirs(hs)
        ctx.synchronize()

    def upload_only():
        device_hrir(sets[0])
        ctx.synchronize()

    one(), batch()                                                    # warm: plans, grids, tables
    up_ms, _ = timed(upload_only, reps)
    one_ms, one_min = timed(one, reps)
    batch_ms, batch_min = timed(batch, max(reps // 2, 3))
    model_ms, _ = timed(lambda: mm.stage(sets[0], FS), 3)
    print(json.dumps({"what": "mic_deviation_rate", "fs": FS, "speakers": len(SPEAKERS), "n": n, "G": G,
                      "upload_one_ms": round(up_ms, 3),
                      "one_hrir_ms": {"median": round(one_ms, 3), "min": round(one_min, 3)},
                      "batched_ms": {"median": round(batch_ms, 3), "min": round(batch_min, 3),
                                     "per_hrir": round(batch_ms / G, 3)},
                      "numpy_model_one_hrir_ms": round(model_ms, 3),
                      "note": "stage times include the upload of the rows (upload_one_ms per HRIR)"}))


if __name__ == "__main__":
    main()
