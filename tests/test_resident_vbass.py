"""Virtual bass as a resident-slice stage between crop_tails and equalize (imp_slice_set_virtual_bass, K13), against

  * the staged class path run_slice(vbass=...) (apply_virtual_bass_to_hrir on the cropped responses, SciPy-order K11);
  * the oracle composition (oracle.hrir crops / alignments + oracle.virtual_bass + FIR + normalize, fp64).

The chunk-parallel scan reassociates the recurrence, so the contract is a tolerance, not bits (include/impulse_hip.h):
integers equal, the fp64 high-passed rows within 1e-12 of the row's peak of scipy.signal.sosfilt, the virtual-bass gain
within 1e-10 relative, gain_db within 1e-5 dB, final rows within 2e-6 of the row's peak."""
import os
import sys
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROW_TOL = 2e-6
HI_TOL = 1e-12
VB_OPTS = [dict(), dict(crossover_freq=300, invert_polarity=True, head_ms=1.5)]     # defaults; the vb_inverted_300 golden's


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def assert_within_contract(got, want, what=""):
    (h1, g1), (h2, g2) = got, want
    assert list(h1.irs) == list(h2.irs)
    assert abs(g1 - g2) <= 1e-5, (what, g1, g2)
    worst = 0.0
    for sp in h1.irs:
        for sd in ("left", "right"):
            a, b = np.asarray(h1.irs[sp][sd].peek(), dtype=np.float64), np.asarray(h2.irs[sp][sd].peek(), dtype=np.float64)
            assert a.shape == b.shape, (what, sp, sd, a.shape, b.shape)
            err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
            assert err <= ROW_TOL, (what, sp, sd, err)
            worst = max(worst, err)
    return worst


def staged(e, files, firs, vbass, decay=None, align=False, stages=None):
    from impulse_hip.pipeline_slice import run_slice
    return _quiet(run_slice, e, [((e.fs, fr), sp) for fr, sp in files], firs=firs, decay=decay, align=align, vbass=vbass,
                  stages=stages)


def oracle_vbass(irs, fs, crossover_freq=250, head_ms=1.0, hp_freq=15.0, invert_polarity=None):
    """core/virtual_bass.py:82-176 composed from oracle.virtual_bass (fp64, SciPy's serial recurrence restated)"""
    from scipy import signal
    from impulse_hip.constants import speaker_side
    from impulse_hip.virtual_bass import _rbj_high_shelf
    from oracle import virtual_bass as ovb
    from oracle.impulse_response import peak_index
    n = max(len(x) for pair in irs.values() for x in pair.values())
    imp = np.zeros(n)
    imp[0] = 1.0
    hp4 = signal.butter(4, hp_freq / (fs / 2), btype="high", output="sos")
    lp8 = np.vstack([signal.butter(4, crossover_freq / (fs / 2), btype="low", output="sos")] * 2)
    hp8 = np.vstack([signal.butter(4, crossover_freq / (fs / 2), btype="high", output="sos")] * 2)
    ild = np.vstack([_rbj_high_shelf(fc, fs, g, q) for fc, g, q in ((150.0, -1.5, 0.760), (400.0, -3.0, 0.660), (800.0, -3.5, 0.610))])
    mpbass = ovb.sosfilt(lp8, ovb.sosfilt(hp4, imp))[0]
    keys = [(sp, sd) for sp in irs for sd in ("left", "right")]
    highs = ovb.sosfilt(hp8, np.stack([irs[sp][sd] for sp, sd in keys]))
    g = float(np.mean([ovb.mag_at(h, fs, crossover_freq) for h in highs])) / (ovb.mag_at(mpbass, fs, crossover_freq) + 1e-20)
    head = int(round(head_ms * 1e-3 * fs))
    direct_u = mpbass * g * (-1.0 if invert_polarity else 1.0)
    cross_u = ovb.sosfilt(ild, direct_u)[0]
    out = {}
    for i, sp in enumerate(irs):
        on_left = speaker_side(sp) == "left"
        itd = peak_index(irs[sp]["right"]) - peak_index(irs[sp]["left"])
        direct = ovb.delay_signal(direct_u, head, n)
        cross = ovb.delay_signal(cross_u, head + (itd if on_left else -itd), n)
        out[sp] = {"left": highs[2 * i] + (direct if on_left else cross), "right": highs[2 * i + 1] + (cross if on_left else direct)}
    return out, g


def host_gain(cropped, tasks, fs, n, crossover_freq=250, hp_freq=15.0, **_):
    """g of core/virtual_bass.py:150-153 on the cropped rows: scipy.signal.sosfilt + np.fft (the reference's own arithmetic)"""
    from scipy import signal
    from impulse_hip.virtual_bass import _mag_at, slice_designs
    sos, mp, _ = slice_designs(fs, n, crossover_freq, hp_freq, sosfilt=lambda s_, rows: [signal.sosfilt(s_, r) for r in rows])
    mags = [_mag_at(signal.sosfilt(sos, np.asarray(cropped[t], dtype=np.float64)), fs, crossover_freq) for t in tasks]
    return float(np.mean(mags)) / (_mag_at(mp, fs, crossover_freq) + 1e-20)


def oracle_measurement(oe, files, firs, fs, vbass, align=False):
    from oracle import hrir as ohrir
    from oracle.scipy_restated import fft_convolve
    N = len(oe)
    irs = {}
    for fr, speakers in files:
        stored = fr.T.astype(np.float64) / 2.0 ** 31
        for sp, sd, col in ohrir.split_recording(stored, speakers, N, fs):
            irs.setdefault(sp, {})[sd] = oe.estimate(col)
    irs = ohrir.crop_heads(irs, fs, head_ms=1)
    if align:
        pairs = (("FL", "FR"), ("SL", "SR"), ("BL", "BR"), ("TFL", "TFR"), ("TSL", "TSR"), ("TBL", "TBR"), ("FC", "FC"), ("WL", "WR"))
        irs = ohrir.align_ipsilateral_all(irs, fs, pairs, segment_ms=30)
        irs = ohrir.align_onset_groups_peak_leftref(irs)
    keep, irs = ohrir.crop_tails(irs, fs, N, oe.n_octaves)
    irs, vg = oracle_vbass(irs, fs, **vbass)
    for sp in irs:
        for sd in irs[sp]:
            irs[sp][sd] = fft_convolve(irs[sp][sd], firs[(sp, sd)], "full")
    g = ohrir.normalization_gain_db(irs, fs, peak_target=-0.1)
    return keep, g, vg, {sp: {sd: irs[sp][sd] * 10 ** (g / 20) for sd in irs[sp]} for sp in irs}


def _setup(spk_files, fs=48000, seconds=1.0, M=2, seed=0, max_measurements=None):
    from test_resident_slice import synth_frames, synth_firs
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.resident_slice import Layout, ResidentSlice
    e = ImpulseResponseEstimator(min_duration=seconds, fs=fs)
    meas = [[synth_frames(e, spk, seed + 1000 * m + 17 * k, rt60=0.2 + 0.03 * m) for k, spk in enumerate(spk_files)] for m in range(M)]
    layout = Layout(e, [(fr.shape[0], 2, spk) for fr, spk in zip(meas[0], spk_files)])
    rs = ResidentSlice(e, layout, max_measurements=max_measurements or M)
    firs = synth_firs(layout.tasks, rs.taps, 5 + seed)
    rs.set_firs(firs)
    return e, meas, layout, rs, firs


# ---- 1. small layouts: staged path and oracle composition -----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("opts", VB_OPTS, ids=["default", "inverted_300"])
def test_small_layout_against_staged_and_oracle(opts):
    _small_layout_against_staged_and_oracle(opts, 48000)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", VB_OPTS, ids=["default", "inverted_300"])
def test_small_layout_against_staged_and_oracle_at_44k1(opts):
    """the same at 44.1 kHz: other head, crossover bin, FIR length and crop"""
    _small_layout_against_staged_and_oracle(opts, 44100)


def _small_layout_against_staged_and_oracle(opts, fs):
    from oracle import estimator as oest
    spk_files = [["FL", "FR"], ["FC"]]
    e, meas, layout, rs, firs = _setup(spk_files, fs=fs, M=2, seed=3)
    rs.set_virtual_bass(**opts)
    got = _quiet(rs.run, meas)
    rows, res = rs.slice.results()
    assert rs.stats["staged"] == 0, res["flags"]
    oe = oest.Estimator(min_duration=1.0, fs=e.fs)
    for m in range(2):
        files = list(zip(meas[m], spk_files))
        stages = {}
        want = staged(e, files, firs, opts, stages=stages)
        assert_within_contract(got[m], want, f"staged m={m}")
        # the integers: keep, the pairs' ITDs on the cropped rows
        keep = len(next(iter(stages["crop_tails"].values())))
        assert int(res["keep"][m]) == keep
        from impulse_hip.impulse_response import ImpulseResponse
        for q, sp in enumerate(layout.speakers):
            pl = ImpulseResponse(stages["crop_tails"][(sp, "left")], e.fs).peak_index()
            pr = ImpulseResponse(stages["crop_tails"][(sp, "right")], e.fs).peak_index()
            assert rows["vbass_itd"][m * rs.slice.rows + 2 * q] == pr - pl
        # the virtual-bass gain of the same cropped fp32 rows, SciPy / np.fft on the host: 1e-10 relative
        hg = host_gain(stages["crop_tails"], layout.tasks, e.fs, keep, **opts)
        assert abs(float(res["vbass_gain"][m]) - hg) <= 1e-10 * hg, (res["vbass_gain"][m], hg)
        tail, g, vg, o_irs = oracle_measurement(oe, files, firs, e.fs, opts)
        assert int(res["keep"][m]) == tail
        # the oracle deconvolves in fp64: its cropped rows differ from the fp32 device rows by ~1e-7, and so does its gain
        assert abs(float(res["vbass_gain"][m]) - vg) <= 1e-6 * abs(vg), (res["vbass_gain"][m], vg)
        assert got[m][1] == pytest.approx(g, abs=1e-5)
        for sp in o_irs:
            for sd in o_irs[sp]:
                y = got[m][0].irs[sp][sd].peek()
                assert y.shape == o_irs[sp][sd].shape
                err = float(np.max(np.abs(y - o_irs[sp][sd])) / np.max(np.abs(o_irs[sp][sd])))
                assert err <= ROW_TOL, (m, sp, sd, err)
    rs.close()


@pytest.mark.gpu
@pytest.mark.parametrize("opts", VB_OPTS, ids=["default", "inverted_300"])
def test_seven_one_layout_against_staged(opts):
    spk = ["FL", "FR", "FC", "BL", "BR", "SL", "SR", "WL"]
    e, meas, layout, rs, firs = _setup([spk], M=2, seed=9)
    rs.set_virtual_bass(**opts)
    got = _quiet(rs.run, meas)
    assert rs.stats["staged"] == 0
    for m in range(2):
        assert_within_contract(got[m], staged(e, [(meas[m][0], spk)], firs, opts), f"m={m}")
    rs.close()


# ---- 2. full size: C2 / C3 with the alignments, with and without the decay stage -------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("config", ["c2", "c3"])
def test_full_size_with_alignment_and_decay(config):
    from scipy import signal
    from test_resident_slice import synth_frames, synth_firs
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.resident_slice import Layout, ResidentSlice
    if config == "c2":
        fs, spk, M = 48000, ["FL", "FR", "FC", "BL", "BR", "SL", "SR", "WL"], 8
    else:
        from impulse_hip.constants import TRUEHD_13CH_ORDER
        fs, spk, M = 96000, list(TRUEHD_13CH_ORDER), 2
    e = ImpulseResponseEstimator(min_duration=5.0, fs=fs)
    base = synth_frames(e, spk, 0xC2 if config == "c2" else 0xC3, rt60=0.22)
    meas = [[base]]
    rng = np.random.default_rng(99)
    for m in range(1, M):
        noise = rng.standard_normal(base.shape) * (2.0 ** 31 * 10 ** (-80 / 20))
        meas.append([np.clip(np.rint(base * (1.0 - 0.07 * m) + noise), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)])
    layout = Layout(e, [(base.shape[0], 2, spk)])
    rs = ResidentSlice(e, layout, max_measurements=M)
    firs = synth_firs(layout.tasks, rs.taps, 21)
    rs.set_firs(firs)
    rs.set_alignment(True)
    rs.set_virtual_bass()
    _quiet(rs.run, meas[:1])                                          # (sizes the slice for these responses first)
    R = rs.slice.rows
    hi = rs.ctx.malloc(M * R * rs.keep_cap * 8)                      # the test hook: the fp64 high-passed rows
    cap = rs.keep_cap
    rs.slice.vbass_hi_device(hi, rs.keep_cap)
    got = _quiet(rs.run, meas)
    rows, res = rs.slice.results()
    rs.slice.vbass_hi_device(None)
    print(f"{config}: flags {list(res['flags'])}, staged {rs.stats['staged']} of {M + 1}")
    assert rs.stats["staged"] <= 1, res["flags"]
    assert rs.keep_cap == cap                                         # the hook's buffer was sized for this slice
    host_hi = np.empty(M * R * rs.keep_cap)
    rs.ctx.d2h(host_hi, hi)
    rs.ctx.free(hi)
    host_hi = host_hi.reshape(M * R, rs.keep_cap)
    sos = np.vstack([signal.butter(4, 250 / (fs / 2), btype="high", output="sos")] * 2)
    worst_hi = 0.0
    for m in range(M):
        stages = {}
        want = staged(e, [(meas[m][0], spk)], firs, {}, align=True, stages=stages if m == 0 else None)
        if res["flags"][m] == 0:
            assert_within_contract(got[m], want, f"{config} m={m}")
        if m == 0:
            assert res["flags"][0] == 0
            n = int(res["keep"][0])
            for r, t in enumerate(layout.tasks):
                x = np.asarray(stages["crop_tails"][t], dtype=np.float64)
                assert len(x) == n
                ref = signal.sosfilt(sos, x)
                worst_hi = max(worst_hi, float(np.max(np.abs(host_hi[r, :n] - ref)) / np.max(np.abs(ref))))
    print(f"{config}: fp64 high-passed rows against scipy.signal.sosfilt at length {int(res['keep'][0])}: {worst_hi:.2e}")
    assert worst_hi <= HI_TOL
    # with the decay stage as well
    rs.set_decay(0.3)
    got = _quiet(rs.run, meas[:2])
    _, res = rs.slice.results()
    print(f"{config} + decay: flags {list(res['flags'])}")
    for m in range(2):
        if res["flags"][m] == 0:
            assert_within_contract(got[m], staged(e, [(meas[m][0], spk)], firs, {}, decay=0.3, align=True), f"{config} decay m={m}")
    rs.close()


# ---- 3. the chunk-parallel IIR on its own ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_chunked_iir_against_scipy_and_golden(gpu_ctx, golden):
    from scipy import signal
    from impulse_hip import _native
    L = _native.IIR_CHUNK
    g = golden("virtual_bass")
    got = gpu_ctx.sosfilt(g["sos_hp8_250"], list(g["sosfilt_in"]), chunked=True)
    for y, want in zip(got, g["sosfilt_hp8"]):
        assert np.max(np.abs(y - want)) <= HI_TOL * np.max(np.abs(want))
    rng = np.random.default_rng(5)
    lengths = [1, L - 1, L, L + 1, 7 * L + 3, 55937]
    rows = [rng.standard_normal(n) * np.exp(-np.arange(n) / 3000.0) for n in lengths]
    rows.append(np.zeros(3 * L + 5))
    last = np.zeros(9 * L + 17)
    last[-5] = 1.0                                                    # one impulse in the last chunk
    rows.append(last)
    for sos in (g["sos_hp8_250"], signal.butter(4, 300 / 24000, btype="high", output="sos"),
                signal.butter(16, 0.01, btype="high", output="sos")):  # 4, 2 and 8 sections
        got = gpu_ctx.sosfilt(sos, rows, chunked=True)
        for x, y in zip(rows, got):
            want = signal.sosfilt(sos, x)
            assert y.shape == want.shape
            peak = np.max(np.abs(want))
            if peak == 0:
                assert np.all(y == 0)
            else:
                assert np.max(np.abs(y - want)) <= HI_TOL * peak, (len(x), float(np.max(np.abs(y - want)) / peak))
    with pytest.raises(Exception, match="sections"):
        gpu_ctx.sosfilt(signal.butter(18, 0.1, output="sos"), rows[:1], chunked=True)


# ---- 4. edge cases ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_negative_and_long_cross_delays_and_both_itd_signs():
    spk = ["FL", "FR", "FC"]
    e, meas, layout, rs, firs = _setup([spk], M=2, seed=41)
    meas[1] = [np.ascontiguousarray(meas[1][0][:, ::-1])]             # ears swapped: the ITDs change sign
    for opts in (dict(head_ms=-30.0), dict(head_ms=-5000.0), dict(head_ms=5000.0), dict(head_ms=0.2)):
        rs.set_virtual_bass(**opts)
        got = _quiet(rs.run, meas)
        rows, res = rs.slice.results()
        itd = rows["vbass_itd"]
        assert np.any(itd > 0) and np.any(itd < 0), itd
        for m in range(2):
            if res["flags"][m] == 0:
                assert_within_contract(got[m], staged(e, [(meas[m][0], spk)], firs, opts), (opts, m))
    rs.close()


@pytest.mark.gpu
def test_crossover_at_nyquist_leaves_the_rows_bit_identical():
    spk = ["FL", "FR"]
    e, meas, layout, rs, firs = _setup([spk], M=2, seed=51)
    off = _quiet(rs.run, meas)
    rs.set_virtual_bass(crossover_freq=e.fs / 2)
    on = _quiet(rs.run, meas)
    for (h1, g1), (h2, g2) in zip(on, off):
        assert g1 == g2
        for sp in h1.irs:
            for sd in ("left", "right"):
                assert np.array_equal(h1.irs[sp][sd].peek(), h2.irs[sp][sd].peek())
    # ... and the staged path agrees that nothing happens
    assert_within_contract(on[0], staged(e, [(meas[0][0], spk)], firs, dict(crossover_freq=e.fs / 2)))
    rs.close()


@pytest.mark.gpu
def test_guard_flag_takes_the_staged_path():
    from impulse_hip import _native
    from impulse_hip.constants import speaker_side
    from impulse_hip.virtual_bass import slice_designs
    spk = ["FL", "FR"]
    e, meas, layout, rs, firs = _setup([spk], M=2, seed=61)
    rs.set_virtual_bass()
    _quiet(rs.run, meas[:1])                                          # (sizes the slice for these responses)
    sos, mp, ild = slice_designs(e.fs, rs.keep_cap)
    # a synthesised reference whose DFT overflows: the gain's denominator is not finite and the device does not guess
    rs.slice.set_virtual_bass(sos, mp / np.max(np.abs(mp)) * 1e308, ild, 250, 48, False, [speaker_side(s) == "left" for s in spk])
    rs._vb_key = ("forced",)
    rs.grow_for = lambda rows: False                                  # (no re-made slice: keep the forced design)
    rs.stats.update(measurements=0, staged=0)
    got = _quiet(rs.run, meas)
    _, res = rs.slice.results()
    assert np.all(res["flags"] & _native.SLICE_VBASS_GUARD), res["flags"]
    assert rs.stats["staged"] == 2
    for m in range(2):
        assert_within_contract(got[m], staged(e, [(meas[m][0], spk)], firs, {}))
    rs.close()


# ---- 5. runners ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_runners_with_vbass(tmp_path):
    from test_resident_slice import synth_frames, synth_firs
    from impulse_hip.audio_io import write_wav_frames
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.pipeline_slice import run_measurement_dirs, run_slice
    from impulse_hip.resident_slice import Layout, SlicePipeline, _fir_taps, run_slice_jobs
    fs = 48000
    e = ImpulseResponseEstimator(min_duration=1.0, fs=fs)
    spk = ["FL", "FR", "FC"]
    meas = [[synth_frames(e, spk, 3100 + m, rt60=0.18 + 0.02 * m)] for m in range(4)]
    layout = Layout(e, [(meas[0][0].shape[0], 2, spk)])
    firs = synth_firs(layout.tasks, _fir_taps(fs), 31)
    opts = VB_OPTS[1]
    want = [staged(e, [(meas[m][0], spk)], firs, opts, align=True) for m in range(4)]
    runner = SlicePipeline(e, layout)
    try:
        got = _quiet(runner.run, meas, firs, align=True, vbass=opts)
        for m in range(4):
            assert_within_contract(got[m], want[m], f"pipeline m={m}")
        plain = _quiet(runner.run, meas[:1], firs, align=True)              # the next job without it: the stage is off again
        assert_within_contract(plain[0], staged(e, [(meas[0][0], spk)], firs, None, align=True))
        with pytest.raises(ValueError, match="unknown options"):
            runner.run(meas[:1], firs, vbass=dict(crossover=250))
    finally:
        runner.close()
    for workers in (None, 2):
        got = _quiet(run_slice_jobs, e, layout, meas, firs, workers=workers, align=True, vbass=opts)
        for m in range(4):
            assert_within_contract(got[m], want[m], f"run_slice_jobs workers={workers} m={m}")
    dirs = []
    for m in range(2):
        d = tmp_path / f"measurement{m}"
        d.mkdir()
        write_wav_frames(str(d / "FL,FR.wav"), fs, synth_frames(e, ["FL", "FR"], 3900 + m), 32)
        dirs.append(str(d))
    whole = _quiet(run_measurement_dirs, e, dirs, vbass=dict(crossover_freq=200))
    for m in range(2):
        ref = _quiet(run_slice, e, [(os.path.join(dirs[m], "FL,FR.wav"), ["FL", "FR"])], align=True, vbass=dict(crossover_freq=200))
        assert_within_contract(whole[m], ref, f"dirs m={m}")


# ---- 6. CPU ---------------------------------------------------------------------------------------------------------------------

def test_set_virtual_bass_refuses_bad_arguments_with_reasons():
    from impulse_hip.resident_slice import ResidentSlice, _check_vbass
    stub = types.SimpleNamespace(fs=48000)                             # refused before anything touches a device
    for kw, msg in ((dict(crossover_freq="250"), "crossover_freq must be a finite number"),
                    (dict(crossover_freq=float("nan")), "crossover_freq must be a finite number"),
                    (dict(crossover_freq=True), "crossover_freq must be a finite number"),
                    (dict(crossover_freq=-5), "crossover_freq must be positive"),
                    (dict(hp_freq=0.0), r"hp_freq must lie in \(0, fs / 2"),
                    (dict(hp_freq=30000.0), r"hp_freq must lie in \(0, fs / 2"),
                    (dict(head_ms=float("inf")), "head_ms must be a finite number"),
                    (dict(invert_polarity="yes"), "invert_polarity must be None, True or False")):
        with pytest.raises(ValueError, match=msg):
            ResidentSlice.set_virtual_bass(stub, **kw)
    with pytest.raises(ValueError, match="unknown options"):
        _check_vbass(48000, dict(xover=250))
    with pytest.raises(ValueError, match="dict"):
        _check_vbass(48000, 250)
    _check_vbass(48000, None)
    _check_vbass(48000, dict(crossover_freq=300, invert_polarity=True, head_ms=1.5))


def test_abi_table_has_the_virtual_bass_entries():
    from impulse_hip import _native
    for name in ("imp_slice_set_virtual_bass", "imp_slice_vbass_hi_device", "imp_sosfilt_chunked"):
        assert name in _native.SIGNATURES
    assert _native.SLICE_VBASS_GUARD & _native.SLICE_REDO
    text = open(os.path.join(ROOT, "include", "impulse_hip.h")).read()
    assert "#define IMP_SLICE_VBASS_GUARD 512" in text and f"#define IMP_IIR_CHUNK {_native.IIR_CHUNK}" in text
    # the new result fields are appended: the earlier layout is unchanged
    names = [f[0] for f in _native.SliceRowResult._fields_]
    assert names[-2:] == ["vbass_itd", "vbass_mag"] and names.index("shift_onset") == len(names) - 3
    assert [f[0] for f in _native.SliceResult._fields_][-3:] == ["flags", "vbass_gain", "vbass_bin"]


def test_host_designs_are_prefixes_of_the_reference_construction():
    """mpbass / ild_mpbass for the slice's capacity: their first n samples are what the reference builds at length n
    (core/virtual_bass.py:100-123 with scipy.signal.sosfilt), bit for bit"""
    from scipy import signal
    from impulse_hip.virtual_bass import _rbj_high_shelf, slice_designs

    def scipy_rows(sos, rows):
        return [signal.sosfilt(sos, r) for r in rows]

    fs = 48000
    for xo, hp in ((250, 15.0), (300, 20.0)):
        sos, mp, ild = slice_designs(fs, 6000, xo, hp, sosfilt=scipy_rows)
        assert sos.shape == (4, 6)
        for n in (1, 255, 2048, 5999, 6000):
            imp = np.zeros(n)
            imp[0] = 1.0
            hp4 = signal.butter(4, hp / (fs / 2), btype="high", output="sos")
            lp8 = np.vstack([signal.butter(4, xo / (fs / 2), btype="low", output="sos")] * 2)
            want = signal.sosfilt(lp8, signal.sosfilt(hp4, imp))
            assert np.array_equal(mp[:n], want)
            shelves = np.vstack([_rbj_high_shelf(fc, fs, g, q) for fc, g, q in ((150.0, -1.5, 0.760), (400.0, -3.0, 0.660),
                                                                                 (800.0, -3.5, 0.610))])
            assert np.array_equal(ild[:n], signal.sosfilt(shelves, want))
