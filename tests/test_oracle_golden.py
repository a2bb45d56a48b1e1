"""Pins the CPU oracle (oracle/) to fixtures produced by running the reference
(tests/golden/make_goldens.py) and to the golden artefact the reference ships
(data/demo/room-responses.wav).  CPU only."""
import numpy as np
import pytest

from oracle import decay as odecay
from oracle import estimator as oest
from oracle import hrir as ohrir
from oracle import impulse_response as oir
from oracle import minphase as omin
from oracle import scipy_restated as sr


# ------------------------------------------------------------------ SciPy restatements vs SciPy itself
def test_next_fast_len_matches_scipy():
    import scipy.fft
    import scipy.fftpack
    for n in list(range(1, 300)) + [686539, 691200, 1463929, 32890, 43199, 2 ** 21 - 1]:
        assert sr.next_fast_len_real(n) == scipy.fft.next_fast_len(n, real=True)
        assert sr.next_fast_len_real(n) == scipy.fftpack.next_fast_len(n)


def test_restated_signal_routines_match_scipy():
    import scipy.signal as ss
    from scipy.interpolate import InterpolatedUnivariateSpline
    from scipy.stats import linregress
    rng = np.random.default_rng(5)
    x, h = rng.standard_normal(5000), rng.standard_normal(1234)
    for mode in ("full", "same"):
        np.testing.assert_allclose(sr.fft_convolve(x, h, mode), ss.fftconvolve(x, h, mode), rtol=0, atol=1e-11)
    for M in (0, 1, 2, 7, 96, 97):
        np.testing.assert_allclose(sr.hann(M), ss.windows.hann(M), atol=1e-15)
        np.testing.assert_allclose(sr.hamming(M), ss.windows.hamming(M), atol=1e-15)
    y = np.round(rng.standard_normal(3000) * 3) / 3          # many plateaus
    for sig in (y, -y):
        np.testing.assert_array_equal(sr.find_peaks_height(sig, 0.3), ss.find_peaks(sig, height=0.3)[0])
    s, i = sr.linregress(x[:50], h[:50])
    ref = linregress(x[:50], h[:50])
    assert s == pytest.approx(ref.slope, rel=1e-13) and i == pytest.approx(ref.intercept, rel=1e-13)
    f = np.linspace(0, 24000, 9600)
    g = 10 ** (np.sin(f / 3000.0) / 2)
    g[-1] = 0
    fir = sr.firwin2_hamming(19200, f, g, 48000)
    np.testing.assert_allclose(fir, ss.firwin2(19200, f, g, fs=48000), atol=1e-15)
    np.testing.assert_allclose(sr.minimum_phase_homomorphic(fir, 19200), ss.minimum_phase(fir, n_fft=19200), atol=1e-14)
    xk = np.sort(rng.uniform(1, 4, 40))
    yk = rng.standard_normal(40)
    xq = np.linspace(0.5, 4.5, 101)
    np.testing.assert_allclose(sr.spline1_eval(xk, yk, xq), InterpolatedUnivariateSpline(xk, yk, k=1)(xq), atol=1e-12)


# ------------------------------------------------------------------ estimator known answers
@pytest.mark.parametrize("fs,dur", [(48000, 1.0), (48000, 5.0), (96000, 5.0), (44100, 5.0)])
def test_estimator_known_answers(golden, fs, dur):
    g = golden("estimator")
    k = f"e{fs}_{int(dur)}"
    e = oest.Estimator(min_duration=dur, fs=fs)
    assert len(e) == int(g[k + "_N"])
    assert e.n_octaves == float(g[k + "_P"])
    assert e.low == float(g[k + "_low"])
    assert e.duration == float(g[k + "_duration"])
    for nm, arr in (("ts", e.test_signal), ("inv", e.inverse_filter)):
        scale = np.max(np.abs(arr))
        np.testing.assert_allclose(arr[:64], g[f"{k}_{nm}_head"], rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(arr[-64:], g[f"{k}_{nm}_tail"], rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(arr[::1024], g[f"{k}_{nm}_dec"], rtol=0, atol=1e-12 * scale)
    base = e.estimate(e.test_signal)
    pk = int(np.argmax(np.abs(base)))
    assert pk == int(g[k + "_baseline_peak"]) == len(e) // 2
    assert base[pk] == pytest.approx(float(g[k + "_baseline_val"]), abs=1e-11)


@pytest.fixture(scope="module")
def est1():
    return oest.Estimator(min_duration=1.0, fs=48000)


def test_estimate_cases(golden, est1):
    g = golden("estimate")
    e = est1
    assert len(e) == int(g["N"])
    for delay in (0, 1, 127, 1000):
        sysir = np.zeros(delay + 1)
        sysir[delay] = 1.0
        rec = sr.fft_convolve(e.test_signal, sysir, "full").astype(np.float32).astype(np.float64)
        y = e.estimate(rec)
        assert len(y) == int(g[f"delay{delay}_len"])
        assert int(np.argmax(np.abs(y))) == int(g[f"delay{delay}_argmax"]) == int(g["baseline_peak"]) + delay
        assert y[np.argmax(np.abs(y))] == pytest.approx(float(g[f"delay{delay}_peakval"]), abs=1e-9)
    rec = sr.fft_convolve(e.test_signal, g["decay_ir"], "full").astype(np.float32).astype(np.float64)
    y = e.estimate(rec)
    bp = int(g["baseline_peak"])
    np.testing.assert_allclose(y[bp - 64: bp + 4096], g["decay_win"], atol=1e-10)
    np.testing.assert_allclose(y[::61], g["decay_dec"], atol=1e-10)
    assert oir.peak_index(y) == int(g["decay_peak_index"])
    A = np.abs(np.fft.rfft(y))
    np.testing.assert_allclose(A[g["decay_bins"]], g["decay_amp"], atol=1e-9 * float(g["decay_amax"]))
    x = np.random.default_rng(0).standard_normal(int(g["noise_L"])).astype(np.float32).astype(np.float64)
    y = e.estimate(x)
    np.testing.assert_allclose(y[100000:100000 + 4096], g["noise_win"], atol=1e-9)
    np.testing.assert_allclose(y[::61], g["noise_dec"], atol=1e-9)
    assert oir.peak_index(y) == int(g["noise_peak_index"])


def test_peak_index_cases(golden):
    g = golden("peak_index")
    names = sorted(k[:-2] for k in g.files if k.endswith("_x"))
    assert len(names) >= 20
    for nm in names:
        x = g[nm + "_x"].astype(np.float64)
        start, end = (int(v) for v in g[nm + "_kw"])
        got = oir.peak_index(x, start=start, end=None if end < 0 else end)
        assert got == int(g[nm + "_idx"]), nm


def _decaying_sine(fs, duration_s, rt60, freq=1000.0, floor_db=-90.0, seed=0):
    r = np.random.default_rng(seed)
    n = int(duration_s * fs)
    t = np.arange(n) / fs
    env = 10 ** ((-60.0 / rt60) * t / 20.0)
    return np.cos(2 * np.pi * freq * t) * env + r.standard_normal(n) * 10 ** (floor_db / 20.0)


@pytest.mark.parametrize("rt60", [0.3, 0.6, 1.0, 1.5])
@pytest.mark.parametrize("seed", [0, 11, 22])
def test_decay_analysis(golden, rt60, seed):
    g = golden("decay")
    k = f"rt{int(rt60 * 10)}_s{seed}"
    data = _decaying_sine(48000, 3.0, rt60, seed=seed).astype(np.float32).astype(np.float64)
    p = odecay.decay_params(data, 48000)
    exp = g[k + "_params"]
    assert (int(p[0]), int(p[1]), int(p[3])) == (int(exp[0]), int(exp[1]), int(exp[3]))
    assert p[2] == pytest.approx(exp[2], abs=1e-9)
    times = odecay.decay_times(data, 48000)
    for got, want in zip(times, g[k + "_times"]):
        if np.isnan(want):
            assert got is None
        else:
            assert got == pytest.approx(want, rel=1e-9)
    for target in (0.2, 0.5):
        kk = f"{k}_t{int(target * 10)}"
        want = g[kk + "_adj"]
        if np.all(np.isinf(want)):
            with pytest.raises(TypeError):
                odecay.decay_adjustment_params(data, 48000, target)
            continue
        adj = odecay.decay_adjustment_params(data, 48000, target)
        if np.all(np.isnan(want)):
            assert adj is None
            continue
        assert tuple(int(v) for v in adj[:3]) == tuple(int(v) for v in want[:3])
        assert adj[3] == pytest.approx(want[3], rel=1e-9)
        out = odecay.apply_decay_window(data.copy(), adj)
        np.testing.assert_allclose(out[::37], g[kk + "_out_dec"], atol=1e-12)
        assert np.sum(out ** 2) == pytest.approx(float(g[kk + "_out_energy"]), rel=1e-10)


def test_decay_degenerate(golden):
    g = golden("decay")
    assert tuple(float(v) for v in odecay.decay_params(np.array([1.0, 0.5, 0.25, 0.1]), 48000)) == tuple(g["short4_params"])
    assert tuple(float(v) for v in odecay.decay_params(np.array([]), 48000)) == tuple(g["empty_params"])


def test_hrir_ops(golden):
    g = golden("hrir_ops")
    for name in ("left_first", "right_first", "tie", "near_start"):
        irs = {"FC": {"left": g[f"ch_{name}_in_l"].astype(np.float64), "right": g[f"ch_{name}_in_r"].astype(np.float64)}}
        out = ohrir.crop_heads(irs, 48000, head_ms=1)
        np.testing.assert_allclose(out["FC"]["left"], g[f"ch_{name}_out_l"], atol=1e-15)
        np.testing.assert_allclose(out["FC"]["right"], g[f"ch_{name}_out_r"], atol=1e-15)
    irs = {sp: {sd: g[f"ct_in_{sp}_{sd}"].astype(np.float64) for sd in ("left", "right")} for sp in ("FL", "FR")}
    for sp in irs:
        for sd in irs[sp]:
            p = odecay.decay_params(irs[sp][sd], 48000)
            exp = g[f"ct_params_{sp}_{sd}"]
            assert (int(p[0]), int(p[1]), int(p[3])) == (int(exp[0]), int(exp[1]), int(exp[3]))
    tail_ind, out = ohrir.crop_tails(irs, 48000, 48000 * 6, 10)
    assert tail_ind == int(g["ct_tail_ind"])
    for sp in irs:
        for sd in irs[sp]:
            np.testing.assert_allclose(out[sp][sd], g[f"ct_out_{sp}_{sd}"], atol=1e-15)
    for name, seed, scales, kw in (("peak", 1, (0.3, 0.1, 0.05, 0.2), dict(peak_target=-0.1)),
                                   ("avg", 2, (0.4, 0.25, 0.15, 0.3), dict(peak_target=None, avg_target=-12.0))):
        rr = np.random.default_rng(seed)
        a = [(rr.standard_normal(4096) * s).astype(np.float32).astype(np.float64) for s in scales]
        irs = {"FL": {"left": a[0], "right": a[1]}, "FR": {"left": a[2], "right": a[3]}}
        gain = ohrir.normalization_gain_db(irs, 48000, **kw)
        assert gain == pytest.approx(float(g[f"nm_{name}_gain_db"]), abs=1e-10)
        np.testing.assert_allclose(a[0] * 10 ** (gain / 20), g[f"nm_{name}_out_FL_left"], rtol=1e-12)


def test_magnitude_response_bit_exact(golden):
    """The reference pins this path bit-exactly (tests/test_magnitude_response_parity.py)."""
    g = golden("magnitude")
    for seed, sizes in ((0xA110, (8, 1024, 48000)), (0xA111, (9, 1025, 48001))):
        rr = np.random.default_rng(seed)
        for n in sizes:
            x = rr.standard_normal(n).astype(np.float32).astype(np.float64)
            f, m = oir.magnitude_response(x, 48000)
            assert np.array_equal(f, g[f"n{n}_f"])
            assert np.array_equal(m, g[f"n{n}_db"])


def test_real_demo_column_reproduces_shipped_room_response(golden):
    """data/demo/room-FC-left.wav column -> estimate -> crop_head(1 ms) -> crop/fade -> PCM_32 must
    equal the FC-left track of the room-responses.wav the reference ships, to 0 LSB."""
    g = golden("demo_fc")
    sweep_len, P = int(g["N"]), float(g["P"])
    # the sweep itself is regenerated: the bundled 6.15 s sweep is the (48 kHz, 5.0 s) grid point
    e = oest.Estimator(min_duration=(sweep_len - 1) / 48000, fs=48000)
    assert len(e) == sweep_len and e.n_octaves == P
    col = g["column_i32"].astype(np.float64) / 2 ** 31
    y = e.estimate(col)
    pk = oir.peak_index(y)
    assert pk == int(g["peak_index"])
    assert int(np.argmax(np.abs(y))) == int(g["argmax"])
    # from_wav keeps the GENERATED sweep (the WAV differs from it by < 1e-4, impulse_response_estimator.py:256-260)
    np.testing.assert_allclose(y[pk - 64: pk + 8192], g["win"], rtol=0, atol=1e-15)
    ir = oir.crop_head(y, 48000, 1)
    n_out = int(g["responses_len"])
    fo = 2 * int(48000 * (sweep_len / 48000 / P) * (1 / 24))
    w = sr.hann(fo)[fo // 2:]
    d = ir[:n_out].copy()
    d *= np.concatenate([np.ones(n_out - len(w)), w])
    pcm = np.rint(d * 2 ** 31).astype(np.int64)
    want = g["responses_fc_left_i32"].astype(np.int64)
    assert np.max(np.abs(pcm - want)) == 0       # 0 LSB against the file the reference ships
    dp = odecay.decay_params(ir, 48000)
    exp = g["decay_params"]
    assert (int(dp[0]), int(dp[3])) == (int(exp[0]), int(exp[3]))


@pytest.mark.parametrize("fs", [48000, 96000])
def test_minimum_phase_fir(golden, fs):
    g = golden("minphase")
    freq = g[f"fs{fs}_freq"]
    np.testing.assert_array_equal(oir.generate_frequencies(10, fs / 2, 1.01), freq)
    for name in ("flat", "wavy", "tilt"):
        fir = omin.minimum_phase_impulse_response(freq, g[f"fs{fs}_{name}_eq"], fs, f_res=5, normalize=False)
        want = g[f"fs{fs}_{name}_fir"]
        assert fir.shape == want.shape == ((9600,) if fs == 48000 else (19200,))
        # The homomorphic log at the forced Nyquist zero (|H| ~ 1e-12 of rounding noise) amplifies
        # 1-ulp input differences to ~5e-9 of the FIR peak: SciPy's own minimum_phase lands 5e-9 away
        # from the fixture on a curve that differs by 1 ulp.  5e-8 is that reproducibility floor.
        np.testing.assert_allclose(fir, want, rtol=0, atol=5e-8 * np.max(np.abs(want)))


# ------------------------------------------------------------------ curve logic: smoothing, equalize, room correction
def test_equalization_worker_curves(golden):
    from oracle import frequency_response as ofr
    g = golden("minphase")
    for fs in (48000, 96000):
        freq = g[f"fs{fs}_freq"]
        for nm in ("flat", "wavy", "tilt"):                   # 'tilt' clips in the treble -> spline bridge
            eq = ofr.equalization_worker_curve(freq, g[f"fs{fs}_{nm}_error"], 0.0, fs)
            np.testing.assert_allclose(eq, g[f"fs{fs}_{nm}_eq"], rtol=0, atol=1e-11)


def test_room_correction_and_worker_on_real_ir(golden):
    """FC-left room IR of data/demo: frequency_response -> mic calibration -> level -> compensate ->
    400 Hz limit -> EQ worker curve -> minimum-phase FIR -> equalize, against the reference's outputs."""
    from oracle import frequency_response as ofr
    from oracle.scipy_restated import fft_convolve
    g, d = golden("room_fc"), golden("demo_fc")
    N, P, n_out = int(d["N"]), float(d["P"]), int(d["responses_len"])
    fo = 2 * int(48000 * (N / 48000 / P) * (1 / 24))
    ir = d["cropped_head"].copy()
    ir[n_out - fo // 2:] *= sr.hann(fo)[fo // 2:]
    freq, raw0 = oir.frequency_response(ir, 48000)
    np.testing.assert_array_equal(freq, g["frequency"])
    np.testing.assert_allclose(raw0, g["fr_raw_initial"], rtol=0, atol=1e-10)
    freq, raw, error, _ = ofr.specific_room_correction(ir, 48000, g["target_raw"], g["mic_raw"], limit=400)
    np.testing.assert_allclose(raw, g["fr_raw"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(error, g["fr_error"], rtol=0, atol=1e-10)
    eq = ofr.equalization_worker_curve(freq, error, 0.0, 48000)
    fir = omin.minimum_phase_impulse_response(freq, eq, 48000, f_res=5, normalize=False)
    # This curve asks for up to 72 dB of (doubled) gain; the homomorphic design then amplifies a 1e-12
    # perturbation of the input curve into 1e-6 of the FIR peak (measured).  The curve recomputed here
    # differs from the reference's by 8e-13 (Savitzky-Golay restatement), so the chained FIR is held to
    # 5e-6; the design itself is pinned at 5e-8 on bit-identical inputs in test_minimum_phase_fir.
    np.testing.assert_allclose(fir, g["worker_fir"], rtol=0, atol=5e-6 * np.max(np.abs(g["worker_fir"])))
    y = fft_convolve(ir, g["worker_fir"], "full")
    assert len(y) == int(g["equalized_len"])
    np.testing.assert_allclose(y[::5], g["equalized_dec"], rtol=0, atol=1e-12 * np.max(np.abs(y)))


def test_pipeline_slice(golden):
    """a18: synthetic FL,FR folder through ingest -> crop_heads -> crop_tails -> EQ FIR -> equalize ->
    normalize, stage by stage against the reference's own objects."""
    from oracle import frequency_response as ofr
    from oracle.scipy_restated import fft_convolve
    g = golden("pipeline_slice")
    e = oest.Estimator(min_duration=1.0, fs=48000)
    N, fs = len(e), 48000
    assert N == int(g["N"])
    import slice_input                                   # tests/golden/slice_input.py (inputs only)
    pcm = slice_input.to_pcm32(slice_input.make_tracks(e.test_signal, fs)).astype(np.float64) / 2 ** 31
    order = [("FL", "left"), ("FL", "right"), ("FR", "left"), ("FR", "right")]
    jobs = ohrir.split_recording(pcm, ["FL", "FR"], N, fs)
    assert [(sp, sd) for sp, sd, _ in jobs] == order
    irs = {}
    for sp, sd, col in jobs:
        irs.setdefault(sp, {})[sd] = e.estimate(col)
    assert [oir.peak_index(irs[sp][sd]) for sp, sd in order] == list(g["ingest_peaks"])
    assert len(irs["FL"]["left"]) == int(g["ingest_len"])
    irs = ohrir.crop_heads(irs, fs, head_ms=1)
    assert [len(irs[sp][sd]) for sp, sd in order] == list(g["heads_len"])
    for sp, sd in order:
        np.testing.assert_allclose(irs[sp][sd][:512], g[f"heads_{sp}_{sd}"], rtol=0, atol=1e-9)
    tail_ind, irs = ohrir.crop_tails(irs, fs, N, e.n_octaves)
    assert tail_ind == int(g["tail_ind"])
    common = oir.generate_frequencies(10, fs / 2, 1.01)
    for sp, sd in order:
        np.testing.assert_allclose(irs[sp][sd][::3], g[f"tails_{sp}_{sd}"], rtol=0, atol=1e-9)
        eq = ofr.equalization_worker_curve(common, g[f"room_error_{sp}_{sd}"], 0.0, fs)
        fir = omin.minimum_phase_impulse_response(common, eq, fs, f_res=5, normalize=False)
        want = g[f"fir_{sp}_{sd}"]
        np.testing.assert_allclose(fir, want, rtol=0, atol=5e-6 * np.max(np.abs(want)))   # chained, see above
        irs[sp][sd] = fft_convolve(irs[sp][sd], want, "full")
    assert len(irs["FL"]["left"]) == int(g["eq_len"])
    gain = ohrir.normalization_gain_db(irs, fs, peak_target=-0.1)
    assert gain == pytest.approx(float(g["norm_gain_db"]), abs=1e-7)
    for sp, sd in order:
        np.testing.assert_allclose(irs[sp][sd] * 10 ** (gain / 20), g[f"final_{sp}_{sd}"], rtol=0, atol=1e-8)


def test_ipsilateral_alignment(golden):
    """Oracle restatement of HRIR.align_ipsilateral_all against the reference run (fixture section 11),
    plus the reference's own assertion (tests/test_dsp_stages.py:105-121: a 7-sample offset is found)."""
    from make_goldens import alignment_inputs
    from impulse_hip.constants import IPSILATERAL_PAIRS
    g = golden("alignment")
    irs = alignment_inputs()
    for name, pairs in (("ipsi", IPSILATERAL_PAIRS), ("chain", [("FL", "FR"), ("FR", "SL"), ("SL", "FL")])):
        out = ohrir.align_ipsilateral_all(irs, 48000, pairs)
        for sp in irs:
            for sd in ("left", "right"):
                d = out[sp][sd]
                assert int(np.argmax(np.abs(d))) == int(g[f"{name}_{sp}_{sd}_peak"])
                np.testing.assert_array_equal(d[:96], g[f"{name}_{sp}_{sd}_head"])
                np.testing.assert_array_equal(d[-96:], g[f"{name}_{sp}_{sd}_tail"])
                assert float(np.sum(d)) == float(g[f"{name}_{sp}_{sd}_sum"])
    a = np.zeros(2048)
    b = np.zeros(2048)
    a[60] = 1.0
    b[67] = 1.0
    assert abs(ohrir.ipsilateral_lag(a, b, 1440)) == 7
    # align_onset_groups_peak_leftref (core/hrir.py:960-1001) against the same reference run
    out = ohrir.align_onset_groups_peak_leftref(irs)
    for sp in irs:
        for sd in ("left", "right"):
            d = out[sp][sd]
            assert int(np.argmax(np.abs(d))) == int(g[f"onset_{sp}_{sd}_peak"])
            np.testing.assert_array_equal(d[:96], g[f"onset_{sp}_{sd}_head"])
            np.testing.assert_array_equal(d[-96:], g[f"onset_{sp}_{sd}_tail"])
            assert float(np.sum(d)) == float(g[f"onset_{sp}_{sd}_sum"])


@pytest.mark.parametrize("fs", [44100, 88200])
def test_ipsilateral_and_onset_alignment_at_other_rates(golden, fs):
    """The oracle's align_ipsilateral_all and align_onset_groups_peak_leftref against the reference run at 44.1 and
    88.2 kHz (fixture section 11 at those rates): 30 ms segments of 1323 and 2646 samples, lengths that are not a
    multiple of 4 (odd at 44.1 kHz)."""
    from make_goldens import alignment_inputs
    from impulse_hip.constants import IPSILATERAL_PAIRS
    g = golden(f"alignment_fs{fs}")
    irs = alignment_inputs(fs=fs)
    for name, run in (("ipsi", lambda x: ohrir.align_ipsilateral_all(x, fs, IPSILATERAL_PAIRS)),
                      ("chain", lambda x: ohrir.align_ipsilateral_all(x, fs, [("FL", "FR"), ("FR", "SL"), ("SL", "FL")])),
                      ("onset", ohrir.align_onset_groups_peak_leftref)):
        out = run(irs)
        for sp in irs:
            for sd in ("left", "right"):
                d = out[sp][sd]
                assert int(np.argmax(np.abs(d))) == int(g[f"{name}_{sp}_{sd}_peak"]), (name, sp, sd)
                np.testing.assert_array_equal(d[:96], g[f"{name}_{sp}_{sd}_head"])
                np.testing.assert_array_equal(d[-96:], g[f"{name}_{sp}_{sd}_tail"])
                assert float(np.sum(d)) == float(g[f"{name}_{sp}_{sd}_sum"])
    # the alignment really moves responses at these rates
    ins = {k: int(np.argmax(np.abs(irs[k[0]][k[1]]))) for k in ((sp, sd) for sp in irs for sd in ("left", "right"))}
    assert any(int(g[f"ipsi_{sp}_{sd}_peak"]) != p for (sp, sd), p in ins.items())


def test_sosfilt_restatement(golden):
    """oracle.virtual_bass.sosfilt against scipy.signal.sosfilt outputs captured in the reference run
    (fixture section 12): the same separately rounded operations, so the same bits."""
    from oracle import virtual_bass as ovb
    g = golden("virtual_bass")
    x = g["sosfilt_in"]
    np.testing.assert_array_equal(ovb.sosfilt(g["sos_hp8_250"], x), g["sosfilt_hp8"])
    np.testing.assert_array_equal(ovb.sosfilt(g["sos_lp8_250"], ovb.sosfilt(g["sos_hp4_15"], x)), g["sosfilt_lp8_of_hp4"])


# ------------------------------------------------------------------ round 2: from_wav, class-level convolve / adjust_decay,
# HRIR.equalize / write_wav, room_correction() with generic measurements (round2.npz, reference run)
def _r2():
    import round2_inputs as r2
    return r2


def test_from_wav_branches(golden):
    g, r2 = golden("round2"), _r2()
    e1 = oest.Estimator(1.0, 48000)
    cases = {"offgrid": r2.off_grid_sweep(), "perturbed": r2.perturbed(e1.test_signal, 3e-4), "ongrid": e1.test_signal}
    for name, sig in cases.items():
        samples = r2.to_pcm32(sig).astype(np.float64) / 2 ** 31          # what the WAV reader returns
        e = oest.from_wav_samples(samples, 48000)
        assert len(e) == int(g[f"fw_{name}_N"]) and e.duration == float(g[f"fw_{name}_duration"])
        assert e.n_octaves == float(g[f"fw_{name}_P"])
        assert bool(np.array_equal(e.test_signal, samples)) == bool(g[f"fw_{name}_sig_is_file"])
        for got, key in ((e.inverse_filter[:64], "inv_head"), (e.inverse_filter[-64:], "inv_tail"),
                         (e.inverse_filter[::509], "inv_dec")):
            np.testing.assert_allclose(got, g[f"fw_{name}_{key}"], rtol=1e-13, atol=0)
        imp = np.zeros(len(e) + 2 * 48000)
        imp[100: 100 + len(e)] = e.test_signal
        y = e.estimate(imp)
        assert int(np.argmax(np.abs(y))) == int(g[f"fw_{name}_selfpeak"]) == 100 + len(e) // 2
        assert y[int(np.argmax(np.abs(y)))] == pytest.approx(float(g[f"fw_{name}_selfpeak_value"]), abs=1e-12)


def test_class_level_convolve_and_adjust_decay(golden):
    g, r2 = golden("round2"), _r2()
    d = r2.decaying_ir(0x1111)
    x = np.random.default_rng(0x2222).standard_normal(1500).astype(np.float32).astype(np.float64)
    np.testing.assert_allclose(sr.fft_convolve(x, d, "full"), g["conv_y"], rtol=0, atol=1e-12)
    for tgt in (0.2, 0.12):
        out = d.copy()
        odecay.apply_decay_window(out, odecay.decay_adjustment_params(d, 48000, tgt))
        np.testing.assert_allclose(out, g[f"adj_{tgt}"], rtol=0, atol=1e-15)
    assert odecay.decay_adjustment_params(d, 48000, 5.0) is None and bool(g["adj_noop_equal"])


def test_hrir_equalize_and_write_wav_frames(golden):
    g, r2 = golden("round2"), _r2()
    base, firs = r2.hrir_set(), r2.fir_pair()
    for name, arg in (("two_rows", firs), ("one_row", firs[:1]), ("flat", firs[1]), ("ir_list", firs), ("array_list", firs)):
        out = ohrir.equalize_all(base, arg)
        for sp in ("FL", "SR"):
            for sd in ("left", "right"):
                np.testing.assert_allclose(out[sp][sd], g[f"heq_{name}_{sp}_{sd}"], rtol=0, atol=1e-12)
    for name, order, subtype in (("hesuvi", ohrir.HESUVI_TRACK_ORDER, "PCM_32"), ("hexa", None, "PCM_24"),
                                 ("hexa16", ohrir.HEXADECAGONAL_TRACK_ORDER, "PCM_16")):
        frames = ohrir.write_wav_frames(base, order)
        assert tuple(frames.shape) == tuple(g[f"ww_{name}_shape"]) and str(g[f"ww_{name}_subtype"]) == subtype
        assert np.array_equal(frames[:64], g[f"ww_{name}_head"]) and np.array_equal(frames.sum(axis=0), g[f"ww_{name}_colsum"])
    # PCM_32: scale 2^31, saturating (pinned below against the reference's own files); 16 / 24 bit keep the top bits of that
    # 32-bit value (libsndfile's published clip path; no narrower file ships: unpinned, see oracle/hrir.py)
    q = ohrir.pcm_quantise(np.array([0.0, 0.5, -0.5, 1.0, -1.0, 0.9999999, 1.5, -1.5, 2.0 ** -16, -2.0 ** -17]), 16)
    assert q.tolist() == [0, 16384, -16384, 32767, -32768, 32767, 32767, -32768, 0, -1]
    assert ohrir.pcm_quantise(np.array([1.0, -1.0, 1.0 - 2.0 ** -33, 3.0, -3.0]), 32).tolist() == \
        [2147483647, -2147483648, 2147483647, 2147483647, -2147483648]
    assert ohrir.pcm_quantise(np.array([0.5, -1.0, 1.0]), 24).tolist() == [1 << 22, -(1 << 23), (1 << 23) - 1]


def _check_against_shipped(q, g, key, layout_tracks=None):
    """q: int64 [frames, tracks] produced here; g[key + ...]: every 37th frame, the full-scale samples and the bounds of the
    non-silent stretches of the file the reference ships.  >= 99.9 % of the samples identical, the rest within 1 LSB (libm
    differences in sin/exp between the machine that wrote the file and this one), full-scale samples saturated, not wrapped."""
    assert tuple(q.shape) == tuple(g[key + "_shape"])
    want = g[key + "_dec"].astype(np.int64)
    got = q[::int(g["stride"])]
    tracks = range(q.shape[1]) if layout_tracks is None else layout_tracks
    for t in tracks:
        d = np.abs(got[:, t] - want[:, t])
        assert d.max() <= 1 and np.mean(d == 0) >= 0.999, (key, t, d.max(), np.mean(d == 0))
        nz = np.flatnonzero(q[:, t])
        assert [int(nz[0]), int(nz[-1])] == g[key + "_nonzero_bounds"][t].tolist() if len(nz) else \
            g[key + "_nonzero_bounds"][t].tolist() == [-1, -1]
    for (i, t), v in zip(g[key + "_fullscale_idx"], g[key + "_fullscale_val"].astype(np.int64)):
        if layout_tracks is None or t in layout_tracks:
            assert abs(int(q[i, t]) - int(v)) <= 1 and (abs(int(v)) < 2 ** 31 - 1 or int(q[i, t]) == int(v))


def test_pcm32_conversion_against_shipped_sweep_wavs(golden):
    """The four sweep WAVs under the reference's data/ were written by core/impulse_response_estimator.py:306-322 through
    core/audio_io.py:82-97 (soundfile, PCM_32): the oracle's sweep + sweep_sequence layout + pcm_quantise must reproduce
    them.  The sweep reaches 0.99999999996, so the files hold both a saturated +2147483647 and two -2147483648: this is what
    tells clip(lrint(x 2^31)) from lrint(x (2^31 - 1)) with wrap-around (38 % identical) - see VERDICT round 2."""
    g = golden("sweep_wavs")
    e = oest.Estimator(min_duration=5.0, fs=48000)
    N = len(e)
    assert N == int(g["sweep_shape"][0]) == 295270
    q = ohrir.pcm_quantise(e.test_signal, 32)
    _check_against_shipped(q[:, None], g, "sweep")
    assert np.max(np.abs(q[:256] - g["sweep_head"])) <= 1 and np.max(np.abs(q[-256:] - g["sweep_tail"])) <= 1
    assert q.max() == 2147483647 and q.min() == -2147483648                      # saturated, not wrapped
    wrong = np.rint(e.test_signal * (2.0 ** 31 - 1)).astype(np.int64)[::37]
    assert np.mean(wrong == g["sweep_dec"][:, 0]) < 0.5                          # the round-2 rule does NOT reproduce the file
    total, starts = oest.sweep_sequence_layout(1, N, 48000)
    assert total == int(g["seg_fl_mono_shape"][0]) and starts == [96000]
    seq = np.zeros((total, 2))
    seq[starts[0]:starts[0] + N, 0] = e.test_signal
    _check_against_shipped(ohrir.pcm_quantise(seq[:, :1], 32), g, "seg_fl_mono")
    _check_against_shipped(ohrir.pcm_quantise(seq, 32), g, "seg_fl_stereo")
    # the shipped FR file predates the positional "stereo" mapping of :196-206 (its sweep sits on track 1; today's code
    # puts a lone FR on track 0): it pins the conversion, not today's layout
    _check_against_shipped(ohrir.pcm_quantise(seq[:, ::-1], 32), g, "seg_fr_stereo")


def _room_curves_on_grid(path_target, path_cal, fs):
    """_open_room_target / _open_mic_calibration (core/room_correction.py:431-461): CSV -> log grid 10..fs/2 -> centred"""
    from oracle import frequency_response as ofr
    grid = oir.generate_frequencies(10, fs / 2, 1.01)
    out = []
    for p in (path_target, path_cal):
        tab = np.loadtxt(p, delimiter=",", skiprows=1)
        raw = oir.interpolate_log(tab[:, 0], tab[:, 1], grid)
        out.append(raw - ofr.center_shift(grid, raw, 1000))
    return grid, out[0], out[1]


@pytest.mark.parametrize("name,method,slimit,glimit,with_generic", [("avg", "average", 400, 300, True),
                                                                     ("cons", "conservative", 600, 500, True),
                                                                     ("specific_only", "average", 400, 300, False)])
def test_room_correction_top_level(golden, tmp_path, name, method, slimit, glimit, with_generic):
    from scipy.io import wavfile
    from oracle import frequency_response as ofr
    g, r2 = golden("round2"), _r2()
    fs = 48000
    e = oest.Estimator(1.0, fs)
    N = len(e)
    r2.room_folder(str(tmp_path), e.test_signal, with_generic=with_generic)
    grid, target, cal = _room_curves_on_grid(tmp_path / "room-target.csv", tmp_path / "room-mic-calibration.csv", fs)
    np.testing.assert_array_equal(grid, g[f"rc_{name}_freq"])
    col = 2 * fs + N
    irs = {"FL": {}, "FR": {}}
    for side in ("left", "right"):
        track = wavfile.read(tmp_path / f"room-FL,FR-{side}.wav")[1].astype(np.float64) / 2 ** 31
        for i, sp in enumerate(("FL", "FR")):
            irs[sp][side] = oir.crop_head(e.estimate(track[2 * fs + i * col: 2 * fs + (i + 1) * col]), fs, 1)
    tail, cropped = ohrir.crop_tails(irs, fs, N, e.n_octaves)
    assert tail == int(g[f"rc_{name}_rir_len"])
    frames = ohrir.write_wav_frames(cropped)
    assert tuple(frames.shape) == tuple(g[f"rc_{name}_responses_shape"])
    np.testing.assert_allclose(frames.sum(axis=0), g[f"rc_{name}_responses_colsum"], rtol=0, atol=1e-12)
    ref_gain = None
    # the reference walks rir.irs in insertion order = os.listdir order of the room-*.wav files, and levels every
    # channel to the FIRST one (core/room_correction.py:189-199): the order the golden run saw is part of the fixture
    for key in g[f"rc_{name}_order"]:
        sp, sd = str(key).split("-")
        f, raw, err, ref_gain = ofr.specific_room_correction(cropped[sp][sd], fs, target, cal, slimit, ref_gain)
        np.testing.assert_allclose(raw, g[f"rc_{name}_{sp}_{sd}_raw"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(err, g[f"rc_{name}_{sp}_{sd}_error"], rtol=0, atol=1e-9)
    speakers = sorted(str(s) for s in g[f"rc_{name}_speakers"])
    if not with_generic:
        assert speakers == ["FL", "FR"]
        return
    assert "FC" in speakers and "LFE" not in speakers and len(speakers) == 15
    track = wavfile.read(tmp_path / "room.wav")[1].astype(np.float64) / 2 ** 31
    n_cols = int(round((len(track) / fs - 2) / (len(e) / fs + 2)))
    assert n_cols == 3
    datas = [oir.crop_head(e.estimate(track[2 * fs + i * col: min(2 * fs + (i + 1) * col, len(track))]), fs, 1)
             for i in range(n_cols)]
    f, raw, err, err_s = ofr.generic_room_correction(datas, fs, target, cal, method, glimit)
    for sp in ("FC", "BL"):
        for sd in ("left", "right"):                                # every missing speaker gets a copy of the curve
            np.testing.assert_allclose(raw, g[f"rc_{name}_{sp}_{sd}_raw"], rtol=0, atol=1e-9)
            np.testing.assert_allclose(err, g[f"rc_{name}_{sp}_{sd}_error"], rtol=0, atol=1e-9)
            np.testing.assert_allclose(err_s, g[f"rc_{name}_{sp}_{sd}_error_smoothed"], rtol=0, atol=1e-9)


def test_headphone_compensation_curves(golden, tmp_path):
    from scipy.io import wavfile
    from oracle import frequency_response as ofr
    g, r2 = golden("round2"), _r2()
    fs = 48000
    e = oest.Estimator(1.0, fs)
    path = tmp_path / "headphones.wav"
    r2.headphone_file(str(path), e.test_signal)
    pcm = wavfile.read(path)[1].astype(np.float64).T / 2 ** 31            # [2 tracks, n]
    col = 2 * fs + len(e)
    fl_left = e.estimate(pcm[0, 2 * fs: 2 * fs + col])                    # column 0 = FL, track 0 = left
    fr_right = e.estimate(pcm[1, 2 * fs + col: 2 * fs + 2 * col])         # column 1 = FR, track 1 = right
    f, left, right = ofr.headphone_curves(fl_left, fr_right, fs)
    np.testing.assert_array_equal(f, g["hp_freq"])
    for nm, raw in (("left", left), ("right", right)):
        np.testing.assert_allclose(raw, g[f"hp_{nm}_raw"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(raw, g[f"hp_{nm}_error"], rtol=0, atol=1e-9)
        assert not np.any(g[f"hp_{nm}_target"])
    assert tuple(g["hp_responses_shape"]) == (col, 32) and bool(g["hp_missing"][0])


def test_reflection_levels_match_the_reference_run(golden):
    """HRIR.calculate_reflection_levels (core/hrir.py:1003-1090), default and wide windows, on responses whose windows are
    cut by the end of the data, a silent channel and a response with a pre-echo as first peak."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import round2_inputs as r2
    from oracle.hrir import reflection_levels
    g = golden("reflection")
    irs = r2.reflection_set()
    for tag, kw in (("default", {}), ("wide", dict(direct_sound_duration_ms=5, early_ref_start_ms=5, early_ref_end_ms=80,
                                                   late_ref_start_ms=80, late_ref_end_ms=400))):
        got = reflection_levels(irs, r2.FS, **kw)
        for sp, pair in got.items():
            for sd, v in pair.items():
                want = g[f"{tag}_{sp}_{sd}"]
                assert v["early_db"] == want[0] and v["late_db"] == want[1], (tag, sp, sd)


# ------------------------------------------------------------------ K12 edges: the oracle against the reference run
def _rel(got, want):
    return float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))


@pytest.mark.parametrize("grid_name", ["step1.05", "step1.02", "step1.01", "step1.005", "geom2048", "step1.01_20_20k",
                                       "jitter1.01"])
def test_oracle_curves_match_the_reference_run_on_other_grids(golden, grid_name):
    """oracle.frequency_response smoothing and equalize against curves_edges.npz (the reference's FrequencyResponse run on
    tests/golden/curves_inputs.py): curves whose first point the kink rule drops are extrapolated with the end piece of
    the spline, as InterpolatedUnivariateSpline does.  1e-12 dB for smoothing and 1e-10 dB for the spline, relative to
    max(1, max |want|): over the recorded curves SciPy's own rounding stays below both (tests/test_curves_edges.py)."""
    import curves_inputs as ci
    from oracle import frequency_response as ofr
    z = golden("curves_edges")
    f = ci.grid(grid_name)
    assert tuple(z[f"{grid_name}/windows"]) == tuple(ofr.window_size(f, o) for o in ci.OCTAVES)
    for k, (on, ot, fl, fu) in enumerate(ci.smoothing_pairs(grid_name)):
        got = ofr.smoothen_fractional_octave(f, ci.walk(grid_name), on, ot, fl, fu)
        assert _rel(got, z[f"{grid_name}/smooth{k}"]) <= 1e-12, (on, ot)
    seen = dropped_first = 0
    for c in ci.CURVES:
        p, err = f"{grid_name}/{c}/", ci.curve(grid_name, c)
        if p + "raises" in z:
            with pytest.raises(ValueError, match="m > k"):
                ofr.equalize(f, err, **ci.EQ_ARGS)
        if p + "eq_raw" in z:
            assert _rel(ofr.equalize(f, err, **ci.EQ_ARGS), z[p + "eq_raw"]) <= 1e-10, c
            seen += 1
            dropped_first += int(not z[p + "keep_raw"][0])
        if p + "es" in z:
            es = ofr.smoothen_heavy_light(f, err)
            assert _rel(es, z[p + "es"]) <= 1e-12, c
            assert _rel(ofr.equalize(f, es, **ci.EQ_ARGS), z[p + "eq_sm"]) <= 1e-10, c
    assert seen >= 6 and (dropped_first >= 3 or ci.kink_half(grid_name) == 0)
