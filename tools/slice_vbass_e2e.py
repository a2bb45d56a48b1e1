#!/usr/bin/env python3
"""End-to-end SlicePipeline job (host PCM frames -> host float64 responses, C2 7.1 layout, alignments on) with the virtual-bass
stage off and on, alternately in one process, against the staged run_slice(vbass=...) per measurement:
python tools/slice_vbass_e2e.py [measurements=24] [rounds=3]"""
import os
import sys
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
from impulse_hip.pipeline_slice import run_slice  # noqa: E402
from impulse_hip.resident_slice import Layout, SlicePipeline, _fir_taps  # noqa: E402

speakers = bench.SLICE_SPEAKERS["c2"][:rec.shape[0] // 2]
frames = bench.measurement_frames(est, rec, L, speakers)
layout = Layout(est, [(frames.shape[0], 2, speakers)])
rng = np.random.default_rng(5)
taps = _fir_taps(est.fs)
firs = {t: np.r_[1.0, np.zeros(taps - 1)] + rng.standard_normal(taps) * np.exp(-np.arange(taps) / 300.0) * 0.05 for t in layout.tasks}
runner = SlicePipeline(est, layout)
rates = {False: [], True: []}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for on in (False, True):
        runner.run([[frames]] * reps, firs, align=True, vbass={} if on else None)         # warm-up: plans, designs, allocator
    staged0 = runner.rs.stats["staged"]
    for _ in range(rounds):
        for on in (False, True):
            t0 = time.perf_counter()
            runner.run([[frames]] * reps, firs, align=True, vbass={} if on else None)
            dt = (time.perf_counter() - t0) / reps
            rates[on].append(dt)
            print(f"virtual bass {'on ' if on else 'off'}: {dt * 1e3:.3f} ms per measurement = {len(layout.tasks) / dt / 1e3:.1f} k IR/s")
    staged_n = runner.rs.stats["staged"] - staged0
    runner.close()
    t_st = []
    for _ in range(4):
        t0 = time.perf_counter()
        run_slice(est, [((est.fs, frames), speakers)], firs=firs, align=True, vbass={})
        t_st.append(time.perf_counter() - t0)
off, on = np.median(rates[False]), np.median(rates[True])
print(f"median: off {off * 1e3:.3f} ms, on {on * 1e3:.3f} ms per measurement ({len(layout.tasks) / on / 1e3:.1f} k IR/s; on / off rate "
      f"{off / on * 100:.1f} %); measurements left to the staged path: {staged_n}; staged run_slice(vbass=...) "
      f"{np.median(t_st[1:]) * 1e3:.2f} ms per measurement")
