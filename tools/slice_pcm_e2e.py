#!/usr/bin/env python3
"""End-to-end SlicePipeline job (host PCM frames -> host results, C2 7.1 layout, alignments on) with output="hrir" (float64
responses) and output="pcm" (PCM_32 words quantised and interleaved on the device), alternately in one process: ms per
measurement, IR/s, the bytes each measurement brings down the link, the stage times of SlicePipeline.times(), and the host
cost of writing hrir.wav + hesuvi.wav per measurement (file I/O: BrirFrames.write_brirs against HRIR.write_wav of the float64
result):  python tools/slice_pcm_e2e.py [measurements=24] [rounds=3]"""
import os
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "impulcifer-pip313_amd"))
import bench  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
est = bench.make_estimator("c2")
rec, L, pitch, _ = bench.synth_recordings(est, 16, seed0=0xC2)
from impulse_hip.constants import HESUVI_TRACK_ORDER  # noqa: E402
from impulse_hip.resident_slice import Layout, SlicePipeline, _fir_taps  # noqa: E402

speakers = bench.SLICE_SPEAKERS["c2"][:rec.shape[0] // 2]
frames = bench.measurement_frames(est, rec, L, speakers)
layout = Layout(est, [(frames.shape[0], 2, speakers)])
rng = np.random.default_rng(5)
taps = _fir_taps(est.fs)
firs = {t: np.r_[1.0, np.zeros(taps - 1)] + rng.standard_normal(taps) * np.exp(-np.arange(taps) / 300.0) * 0.05 for t in layout.tasks}
runner = SlicePipeline(est, layout)
modes = ("hrir", "pcm")
rates = {k: [] for k in modes}
stage = {k: {} for k in modes}
down = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for mode in modes:
        runner.run([[frames]] * reps, firs, align=True, output=mode)         # warm-up: plans, rings, pinned blocks
    staged0 = runner.rs.stats["staged"]
    runner.times()
    for _ in range(rounds):
        for mode in modes:
            t0 = time.perf_counter()
            out = runner.run([[frames]] * reps, firs, align=True, output=mode)
            dt = (time.perf_counter() - t0) / reps
            for k, v in runner.times().items():
                stage[mode][k] = stage[mode].get(k, 0.0) + v
            rates[mode].append(dt)
            r0 = out[0][0]
            down[mode] = r0.frames.nbytes if mode == "pcm" else sum(ir.data.nbytes for p in r0.irs.values() for ir in p.values())
            print(f"output={mode:4s}: {dt * 1e3:.3f} ms per measurement = {len(layout.tasks) / dt / 1e3:.1f} k IR/s")
            if mode == "pcm":
                pcm_out = out
            else:
                hrir_out = out
            del out, r0
    staged_n = runner.rs.stats["staged"] - staged0
    runner.close()
tmp = tempfile.mkdtemp(prefix="slice_pcm_e2e_")
try:
    t0 = time.perf_counter()
    for fr, _ in pcm_out:
        fr.write_brirs(tmp)
    t_pcm = (time.perf_counter() - t0) / len(pcm_out)
    t0 = time.perf_counter()
    for h, _ in hrir_out:
        h.write_wav(os.path.join(tmp, "hrir.wav"))
        h.write_wav(os.path.join(tmp, "hesuvi.wav"), track_order=HESUVI_TRACK_ORDER)
    t_f64 = (time.perf_counter() - t0) / len(hrir_out)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
med = {k: float(np.median(v)) for k, v in rates.items()}
print(f"median: hrir {med['hrir'] * 1e3:.3f} ms ({len(layout.tasks) / med['hrir'] / 1e3:.1f} k IR/s), pcm {med['pcm'] * 1e3:.3f} ms "
      f"({len(layout.tasks) / med['pcm'] / 1e3:.1f} k IR/s) per measurement; pcm / hrir rate {med['hrir'] / med['pcm'] * 100:.1f} %")
print(f"download per measurement: hrir {down['hrir']} B, pcm {down['pcm']} B (ratio {down['pcm'] / down['hrir']:.3f})")
for mode in modes:
    n = stage[mode].get("measurements", 1.0)
    print(f"times() per measurement, output={mode}: " + ", ".join(f"{k} {v / n * 1e3:.3f} ms" for k, v in sorted(stage[mode].items())
                                                                  if k != "measurements"))
print(f"host cost of hrir.wav + hesuvi.wav per measurement: BrirFrames.write_brirs {t_pcm * 1e3:.2f} ms, HRIR.write_wav of the "
      f"float64 result {t_f64 * 1e3:.2f} ms; measurements left to the staged path: {staged_n}")
