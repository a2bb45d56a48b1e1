"""Microphone-deviation correction on the MI355X: K14 against the NumPy model, the whole stage against the reference's
fixtures, device rows against host arrays, the batched form against one HRIR at a time, the skip branches, the guarded
decision and run_slice's stage."""
import warnings

import numpy as np
import pytest

import micdev_inputs as mi
import micdev_model as mm

ROW_TOL = 2e-6
FIR_TOL = 5e-7


class _Est:
    def __init__(self, fs):
        self.fs = fs


def host_hrir(fs, irs):
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse
    h = HRIR(_Est(fs))
    h.irs = {sp: {sd: ImpulseResponse(np.array(x, dtype=np.float64), fs) for sd, x in pair.items()} for sp, pair in irs.items()}
    return h


def device_hrir(fs, irs):
    """the same responses as fp32 rows of one device block (equal pitch, in order: the layout the slice leaves)"""
    from impulse_hip import _native
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse
    rows = [np.asarray(pair[sd], dtype=np.float32) for pair in irs.values() for sd in ("left", "right")]
    n = len(rows[0])
    pitch = (n + 63) // 64 * 64
    ctx = _native.default_context()
    block = DeviceBlock(ctx, pitch * len(rows))
    flat = np.zeros(pitch * len(rows), dtype=np.float32)
    for i, r in enumerate(rows):
        flat[i * pitch:i * pitch + n] = r
    ctx.h2d(block.ptr, flat)
    h = HRIR(_Est(fs))
    i = 0
    for sp in irs:
        h.irs[sp] = {}
        for sd in ("left", "right"):
            h.irs[sp][sd] = ImpulseResponse.on_device(Row(block, i * pitch, n), fs)
            i += 1
    return h


def rows_of(h):
    return np.stack([h.irs[sp][sd].peek() for sp in h.irs for sd in ("left", "right")])


def apply(h, **kw):
    from impulse_hip.microphone_deviation_correction import apply_microphone_deviation_correction_to_hrir
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return apply_microphone_deviation_correction_to_hrir(h, **kw)


# ---- K14 against the model -------------------------------------------------------------------------------------------------

def _k14_case(fs, seed, n=2000, window_ms=5.0):
    rng = np.random.default_rng(seed)
    win, pre = mm.lengths(fs, window_ms)
    rows, peaks = [], []
    specials = [0, max(pre - 3, 0), n - 1, None, "zero", "short"]
    for k in range(12):
        kind = specials[k] if k < len(specials) else None
        if kind == "short":
            rows.append(rng.standard_normal(5))
            peaks.append(2)
            continue
        r = rng.standard_normal(n) * np.exp(-np.arange(n) / (0.004 * fs))
        if kind == "zero":
            r[:] = 0.0
        rows.append(r.astype(np.float32).astype(np.float64))
        peaks.append(int(rng.integers(0, n)) if kind in (None, "zero") else kind)
    return rows, np.array(peaks), win, pre


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [44100, 48000, 96000, 192000])
@pytest.mark.parametrize("window_ms", [5.0, 200.0], ids=["nfft8192", "long_window"])
def test_k14_power_and_ratio_against_the_model(fs, window_ms):
    from impulse_hip import _native
    from impulse_hip.device_rows import DeviceBlock
    n = 2000 if window_ms == 5.0 else int(0.25 * fs)
    rows, peaks, win, pre = _k14_case(fs, fs + int(window_ms), n=n, window_ms=window_ms)
    if window_ms != 5.0:
        assert mm.fast_len_11(max(min(win + pre, n), 8192)) != 8192
    freq = mm.grid(fs)
    B = len(rows)
    group = np.repeat([0, 1, 2], [4, 4, 4])
    side = np.tile([0, 1], B // 2)
    anchor = np.array([1, 1, 0, 0, 1, 1, 1, 1, 0, 0, 1, 1])
    want_p = np.stack([mm.power(r, p, fs, win, pre, freq) for r, p in zip(rows, peaks)])
    want_raw = []
    for g in range(3):
        sel = [b for b in range(B) if group[b] == g and anchor[b]]
        left = np.mean([want_p[b] for b in sel if side[b] == 0], axis=0)
        right = np.mean([want_p[b] for b in sel if side[b] == 1], axis=0)
        want_raw.append(10 * np.log10((left + 1e-20) / (right + 1e-20)))
    want_raw = np.stack(want_raw)
    ctx = _native.default_context()
    raw_h, p_h = ctx.mic_mismatch(rows, peaks, group, side, anchor, 3, win, pre, fs, freq, want_power=True)
    # fp32 device rows, deliberately at uneven offsets
    offs = np.cumsum([0] + [len(r) + 7 for r in rows[:-1]]).astype(np.int64)
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    flat = np.zeros(int(offs[-1] + lens[-1]), dtype=np.float32)
    for o, r in zip(offs, rows):
        flat[o:o + len(r)] = r
    block = DeviceBlock(ctx, len(flat))
    ctx.h2d(block.ptr, flat)
    raw_d, p_d = ctx.mic_mismatch((offs, lens), peaks, group, side, anchor, 3, win, pre, fs, freq, want_power=True,
                                  dptr=block.ptr)
    for got in (p_h, p_d):
        for b in range(B):
            scale = max(float(np.max(want_p[b])), 1e-300)
            assert np.max(np.abs(got[b] - want_p[b])) <= 1e-10 * scale, (fs, b)
    assert np.all(p_h[4] == 0) and np.all(p_h[5] == 0)                  # the all-zero row and the 5-sample row
    for got in (raw_h, raw_d):
        assert np.max(np.abs(got - want_raw)) <= 1e-9
    assert np.array_equal(raw_h, raw_d) and np.array_equal(p_h, p_d)    # same fp32 values, same arithmetic


@pytest.mark.gpu
def test_k14_refuses_bad_arguments():
    from impulse_hip import _native
    ctx = _native.default_context()
    rows = [np.ones(100), np.ones(100)]
    freq = mm.grid(48000)
    with pytest.raises(_native.NativeError, match="no anchor row"):
        ctx.mic_mismatch(rows, [0, 0], [0, 0], [0, 1], [1, 0], 1, 240, 24, 48000, freq)
    with pytest.raises(_native.NativeError, match="side"):
        ctx.mic_mismatch(rows, [0, 0], [0, 0], [0, 2], [1, 1], 1, 240, 24, 48000, freq)
    with pytest.raises(_native.NativeError, match="group"):
        ctx.mic_mismatch(rows, [0, 0], [0, 1], [0, 1], [1, 1], 1, 240, 24, 48000, freq)
    with pytest.raises(_native.NativeError, match="increasing"):
        ctx.mic_mismatch(rows, [0, 0], [0, 0], [0, 1], [1, 1], 1, 240, 24, 48000, freq[::-1])


# ---- the whole stage against the reference's fixtures ------------------------------------------------------------------------

def check_against_fixture(z, case, h, summary, irs):
    p = case + "/"
    assert summary["anchor"] == str(z[p + "anchor"])
    assert abs(summary["avg_error_db"] - float(z[p + "avg_error_db"])) <= 1e-9
    assert abs(summary["max_error_db"] - float(z[p + "max_error_db"])) <= 1e-9
    assert (summary["speakers_processed"] == []) == bool(z[p + "skipped"])
    if not bool(z[p + "skipped"]):
        assert summary["speakers_processed"] == list(irs)
    rows = rows_of(h)
    assert rows.shape[1] == int(z[p + "out_len"])
    step = int(z["decim_step"])
    err = np.max(np.abs(rows[:, ::step] - z[p + "decim"]), axis=1) / z[p + "row_peak"]
    assert np.max(err) <= ROW_TOL, (case, float(np.max(err)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(mi.CASES))
def test_stage_against_reference_fixtures(golden, case):
    from impulse_hip.microphone_deviation_correction import MicrophoneMatchingCorrector
    z = golden("mic_deviation")
    fs, irs, anchor, strength = mi.hrir_case(case)
    # the corrector's own surface: mismatch and FIRs
    corr = MicrophoneMatchingCorrector(fs, correction_strength=strength, anchor=anchor)
    from oracle.impulse_response import peak_index
    for sp, pair in irs.items():
        corr.collect_speaker(sp, pair["left"], pair["right"], peak_index(pair["left"]), peak_index(pair["right"]))
    mis = corr.estimate_interaural_mismatch()
    assert corr.anchor_used == str(z[case + "/anchor"])
    assert np.max(np.abs(mis - z[case + "/mismatch_db"])) <= 1e-9
    for got, key in zip(corr.design_correction_filters(), ("left_fir", "right_fir")):
        want = z[case + "/" + key]
        assert got.shape == want.shape
        # K6 at the stage's f_res = 10, normalize=False: measured 2.9e-7 of the peak at worst (1.4e-7 for a flat curve)
        assert np.max(np.abs(got - want)) <= FIR_TOL * np.max(np.abs(want)), (case, key)
    s = corr.get_analysis_summary()
    assert abs(s["max_error_db"] - float(z[case + "/max_error_db"])) <= 1e-9
    # the HRIR entry point on host arrays and on device rows
    for make in (host_hrir, device_hrir):
        h = make(fs, irs)
        summary = apply(h, correction_strength=strength, anchor=anchor)
        check_against_fixture(z, case, h, summary, irs)


@pytest.mark.gpu
def test_device_rows_against_host_arrays():
    fs, irs, anchor, strength = mi.hrir_case("fc71_48k_auto")
    hh, hd = host_hrir(fs, irs), device_hrir(fs, irs)
    sh, sd = apply(hh), apply(hd)
    assert sh["anchor"] == sd["anchor"]
    assert abs(sh["max_error_db"] - sd["max_error_db"]) <= 1e-9 and abs(sh["avg_error_db"] - sd["avg_error_db"]) <= 1e-9
    assert all(ir._data is None for pair in hd.irs.values() for ir in pair.values())     # still on the device
    a, b = rows_of(hd), rows_of(hh)
    assert a.shape == b.shape
    assert np.max(np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)) <= ROW_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("make", ["host", "device"])
def test_batched_is_bit_identical_to_one_hrir_at_a_time(make):
    from impulse_hip.microphone_deviation_correction import apply_microphone_deviation_correction_to_hrirs
    mk = host_hrir if make == "host" else device_hrir
    cases = ["fc71_48k_auto", "large_strength1", "matched", "strength0", "nofc_44k", "fc71_48k_diffuse"]
    inputs = [mi.hrir_case(c) for c in cases]
    batch = [mk(fs, irs) for fs, irs, _, _ in inputs]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sums = apply_microphone_deviation_correction_to_hrirs(batch, correction_strength=0.7, anchor="auto")
    for (fs, irs, _, _), hb, sb in zip(inputs, batch, sums):
        hs = mk(fs, irs)
        ss = apply(hs, correction_strength=0.7, anchor="auto")
        assert ss == sb
        assert np.array_equal(rows_of(hs), rows_of(hb))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["matched", "strength0"])
def test_skip_branches_leave_rows_untouched(case):
    fs, irs, anchor, strength = mi.hrir_case(case)
    for make in (host_hrir, device_hrir):
        h = make(fs, irs)
        before = rows_of(h)
        s = apply(h, correction_strength=strength, anchor=anchor)
        assert s["speakers_processed"] == []
        assert np.array_equal(rows_of(h), before)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fc71_48k_auto", "matched"])
def test_widened_guard_band_takes_the_host_path(golden, monkeypatch, case):
    from impulse_hip import microphone_deviation_correction as mdc
    z = golden("mic_deviation")
    calls = []
    real = mdc._host_analysis

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(mdc, "DECISION_GUARD_DB", 100.0)
    monkeypatch.setattr(mdc, "_host_analysis", spy)
    fs, irs, anchor, strength = mi.hrir_case(case)
    h = host_hrir(fs, irs)
    s = apply(h, correction_strength=strength, anchor=anchor)
    assert calls
    check_against_fixture(z, case, h, s, irs)


# ---- run_slice(mic_deviation=...) ---------------------------------------------------------------------------------------------

def _slice_inputs():
    from test_resident_slice import synth_frames, synth_firs
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.resident_slice import _fir_taps
    e = ImpulseResponseEstimator(min_duration=1.0, fs=48000)
    spk = ["FL", "FR", "FC"]
    frames = synth_frames(e, spk, 11)
    tasks = [(sp, sd) for sp in spk for sd in ("left", "right")]
    return e, [((e.fs, frames), spk)], synth_firs(tasks, _fir_taps(e.fs), 12)


@pytest.mark.gpu
@pytest.mark.parametrize("vbass", [None, {}], ids=["plain", "vbass"])
def test_run_slice_stage_matches_the_module(vbass):
    from impulse_hip.pipeline_slice import run_slice
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse
    e, recs, firs = _slice_inputs()
    opts = dict(correction_strength=1.0, anchor="auto")
    stages = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, gain = run_slice(e, recs, firs=firs, stages=stages, vbass=vbass, mic_deviation=opts)
    before = stages["vbass" if vbass is not None else "crop_tails"]
    h = HRIR(e)
    for (sp, sd), x in before.items():
        h.irs.setdefault(sp, {})[sd] = ImpulseResponse(np.array(x), e.fs)
    s = apply(h, **opts)
    assert s["speakers_processed"]                                        # the stage did correct
    for (sp, sd), x in stages["mic_deviation"].items():
        y = h.irs[sp][sd].peek()
        assert x.shape == y.shape
        assert np.max(np.abs(x - y)) <= ROW_TOL * np.max(np.abs(y)), (sp, sd)
    h.equalize_channels(firs)
    want_gain = h.normalize(peak_target=-0.1)
    assert abs(gain - want_gain) <= 1e-5
    for sp in h.irs:
        for sd in ("left", "right"):
            a, b = got.irs[sp][sd].peek(), h.irs[sp][sd].peek()
            assert a.shape == b.shape
            assert np.max(np.abs(a - b)) <= ROW_TOL * np.max(np.abs(b)), (sp, sd)


@pytest.mark.gpu
def test_run_slice_skips_the_stage_under_headphone_compensation():
    from impulse_hip.pipeline_slice import run_slice
    e, recs, firs = _slice_inputs()
    stages = {}
    with pytest.warns(UserWarning, match="microphone-deviation correction skipped"):
        run_slice(e, recs, firs=firs, stages=stages, hp_left=object(), mic_deviation=dict(correction_strength=0.7))
    assert "mic_deviation" not in stages
    plain = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run_slice(e, recs, firs=firs, stages=plain)
    for k in stages["normalize"]:
        assert np.array_equal(stages["normalize"][k], plain["normalize"][k])
