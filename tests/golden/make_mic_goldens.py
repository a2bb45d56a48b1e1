"""Generate tests/golden/mic_deviation.npz by RUNNING the reference's microphone-deviation stage
(core/microphone_deviation_correction.py) on the seeded inputs of tests/golden/micdev_inputs.py:

    PYTHONPATH=/root/reference PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_mic_goldens.py

Data only: the anchor used, the mismatch curve, both FIRs, the summary scalars, the skip decision, the output lengths and
every 8th sample of the corrected rows.
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

import make_goldens  # noqa: E402
import micdev_inputs as mi  # noqa: E402

DECIM = 8


def main():
    if make_goldens.REF not in sys.path:
        sys.path.insert(0, make_goldens.REF)
    make_goldens._install_stubs()
    from core.hrir import HRIR
    from core.impulse_response import ImpulseResponse
    from core.microphone_deviation_correction import (MicrophoneMatchingCorrector,
                                                      apply_microphone_deviation_correction_to_hrir)

    out = {}
    for name in mi.CASES:
        fs, irs, anchor, strength = mi.hrir_case(name)

        class _Est:
            pass

        est = _Est()
        est.fs = fs
        h = HRIR(est)
        h.irs = {sp: {sd: ImpulseResponse(x.copy(), fs) for sd, x in pair.items()} for sp, pair in irs.items()}
        # the FIRs and the curve as the stage forms them (a second corrector over the same inputs)
        corr = MicrophoneMatchingCorrector(sample_rate=fs, correction_strength=strength, anchor=anchor)
        for sp, pair in h.irs.items():
            corr.collect_speaker(sp, pair["left"].data, pair["right"].data, pair["left"].peak_index(),
                                 pair["right"].peak_index())
        corr.estimate_interaural_mismatch()
        lf, rf = corr.design_correction_filters()
        summary = apply_microphone_deviation_correction_to_hrir(h, correction_strength=strength, anchor=anchor)
        rows = np.stack([h.irs[sp][sd].data for sp in irs for sd in ("left", "right")])
        p = name + "/"
        out[p + "anchor"] = np.array(summary["anchor"])
        out[p + "mismatch_db"] = corr.mismatch_db
        out[p + "left_fir"] = lf
        out[p + "right_fir"] = rf
        out[p + "avg_error_db"] = np.float64(summary["avg_error_db"])
        out[p + "max_error_db"] = np.float64(summary["max_error_db"])
        out[p + "skipped"] = np.array(summary["speakers_processed"] == [])
        out[p + "out_len"] = np.int64(rows.shape[1])
        out[p + "decim"] = rows[:, ::DECIM]
        out[p + "row_peak"] = np.max(np.abs(rows), axis=1)
        print(name, summary["anchor"], round(summary["max_error_db"], 4), rows.shape)
    np.savez_compressed(os.path.join(OUT, "mic_deviation.npz"), decim_step=np.int64(DECIM), **out)


if __name__ == "__main__":
    main()
