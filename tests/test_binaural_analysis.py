"""Binaural analysis metrics on the MI355X (K15): every fixture case against the reference-run fixture (analysis.npz), device
rows against host arrays, batched against one pair at a time, the properties the reference's own tests
(tests/test_bokeh_analysis.py) pin, HRIR.binaural_analysis on the rows run_slice leaves, and the entries' refusals."""
import warnings

import numpy as np
import pytest

import analysis_inputs as ai

# e_ref: the reference's own rounding error per quantity, measured on the CPU (the NumPy model with np.longdouble sums
# against the fixture: tests/test_binaural_analysis_cpu.py); the device is held to 10 x e_ref.
E_REF_POWER, TOL_POWER = 6.94e-16, 6.94e-15            # band powers, relative to the sum itself
E_REF_CROSS, TOL_CROSS = 4.15e-16, 4.15e-15            # cross sum, relative to sqrt(pl pr)
E_REF_IACF, TOL_IACF = 5.56e-16, 5.56e-15              # iacf, absolute (normalised to [-1, 1])
E_REF_EDC_DB, TOL_EDC_DB = 5.33e-14, 5.33e-13          # decay curve, dB
# derived: ILD = 10 log10 of a ratio of two powers, each within TOL_POWER: 10 / ln 10 * 2 TOL_POWER
TOL_ILD_DB = 10 / np.log(10) * 2 * TOL_POWER
# IPD on bands whose reference coherence c >= ai.COHERENCE_MIN: the cross term's error over c, as an angle in degrees
TOL_IPD_DEG = np.degrees(TOL_CROSS)
# an ear of exact zeros: what the pair-packed transform's Hermitian split leaves of the other ear (see the CPU test file)
ZERO_EAR_LEAK = TOL_POWER ** 2


def _cases():
    return [(name, k) for name, spec in ai.CASES.items() for k in range(spec[3])]


def _check_pair(z, p, fs, res, edc=None):
    pl, pr, cross = z[p + "power_l"], z[p + "power_r"], z[p + "cross"]
    s = res["band_sums"]
    assert np.array_equal(np.isnan(pl), np.isnan(s[:, 0])) and np.array_equal(np.isnan(pl), np.isnan(s[:, 3]))
    fig = dict(power=0.0, cross=0.0, ild=0.0, ipd=0.0, iacf=0.0, edc=0.0)
    for b in np.nonzero(~np.isnan(pl))[0]:
        for got, want, other in ((s[b, 0], pl[b], pr[b]), (s[b, 1], pr[b], pl[b])):
            if want > 0:
                fig["power"] = max(fig["power"], abs(got - want) / want)
            else:
                assert 0.0 <= got <= ZERO_EAR_LEAK * other
        if pl[b] > 0 and pr[b] > 0:
            scale = np.sqrt(pl[b] * pr[b])
            fig["cross"] = max(fig["cross"], abs(s[b, 2] + 1j * s[b, 3] - cross[b]) / scale)
            coh = abs(cross[b]) / scale
            if coh >= ai.COHERENCE_MIN:
                d = (res["ipd_deg"][b] - z[p + "ipd_deg"][b] + 180.0) % 360.0 - 180.0
                fig["ipd"] = max(fig["ipd"], abs(d) * coh)
        fig["ild"] = max(fig["ild"], abs(res["ild_db"][b] - z[p + "ild_db"][b]))
    assert np.array_equal(np.isnan(res["ild_db"]), np.isnan(z[p + "ild_db"]))
    assert np.array_equal(np.isnan(res["ipd_deg"]), np.isnan(z[p + "ipd_deg"]))
    want = z[p + "iacf"]
    assert res["iacf"].shape == want.shape and res["lags_ms"].shape == want.shape
    if len(want):
        fig["iacf"] = float(np.max(np.abs(res["iacf"] - want)))
        assert np.array_equal(res["lags_ms"], z[p + "lags_ms"])
        assert res["tau_ms"] == float(z[p + "tau_ms"])                 # exact: the fixture's gap condition holds for every case
        assert abs(res["iacc"] - float(z[p + "iacc"])) <= TOL_IACF
    else:
        assert np.isnan(res["iacc"]) and np.isnan(res["tau_ms"]) and np.isnan(z[p + "iacc"])
    if edc is not None:
        for side, c in zip(("left", "right"), edc):
            assert len(c) == int(z[p + f"edc_{side}_len"])
            for got, key in ((c[::ai.EDC_DECIM], "decim"), (c[:ai.EDC_EDGE], "head"), (c[-ai.EDC_EDGE:], "tail")):
                fig["edc"] = max(fig["edc"], float(np.max(np.abs(got - z[p + f"edc_{side}_{key}"]))))
    print(p, {k: float(v) for k, v in fig.items()})
    assert fig["power"] <= TOL_POWER
    assert fig["cross"] <= TOL_CROSS
    assert fig["ild"] <= TOL_ILD_DB
    assert fig["ipd"] <= TOL_IPD_DEG
    assert fig["iacf"] <= TOL_IACF
    assert fig["edc"] <= TOL_EDC_DB


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ai.CASES))
def test_binaural_metrics_against_the_reference_fixture(golden, name):
    from impulse_hip import analysis
    z = golden("analysis")
    fs, pairs, bands, max_delay_ms = ai.case(name)
    res = analysis.binaural_metrics(pairs, fs, bands=bands, max_delay_ms=max_delay_ms, edc=True)
    assert len(res) == len(pairs)
    for k, r in enumerate(res):
        assert np.array_equal(np.array(r["bands"], dtype=np.float64).reshape(-1, 2), z[f"{name}/{k}/bands"])
        _check_pair(z, f"{name}/{k}/", fs, r, r["edc_db"])


@pytest.mark.gpu
@pytest.mark.parametrize("name, k", _cases())
def test_drop_in_functions_against_the_reference_fixture(golden, name, k):
    from impulse_hip import analysis
    z = golden("analysis")
    fs, pairs, bands, max_delay_ms = ai.case(name)
    left, right = pairs[k]
    bands = analysis.octave_bands(fs) if bands is None else bands
    ild = analysis.band_interaural_level_difference(left, right, fs, bands)
    ipd = analysis.band_interaural_phase_difference(left, right, fs, bands)
    lags_ms, iacf, iacc, tau = analysis.interaural_cross_correlation(left, right, fs, max_delay_ms)
    curves = [analysis.energy_decay_curve_db(left), analysis.energy_decay_curve_db(right)]
    assert isinstance(ild, list) and isinstance(ipd, list) and len(ild) == len(ipd) == len(bands)
    assert isinstance(lags_ms, np.ndarray) and isinstance(iacf, np.ndarray) and isinstance(iacc, float) and isinstance(tau, float)
    batched = analysis.binaural_metrics([(left, right)], fs, bands=bands, max_delay_ms=max_delay_ms)[0]
    assert np.array_equal(ild, batched["ild_db"], equal_nan=True) and np.array_equal(ipd, batched["ipd_deg"], equal_nan=True)
    assert np.array_equal(iacf, batched["iacf"])
    res = dict(batched, ild_db=ild, ipd_deg=ipd, lags_ms=lags_ms, iacf=iacf, iacc=iacc, tau_ms=tau)
    _check_pair(z, f"{name}/{k}/", fs, res, curves)


@pytest.mark.gpu
def test_empty_and_floor_conventions():
    from impulse_hip import analysis
    x = np.random.default_rng(1).standard_normal(500)
    for left, right in ((x, np.zeros(500)), (np.zeros(500), x), (np.zeros(3), np.zeros(3))):
        lags_ms, iacf, iacc, tau = analysis.interaural_cross_correlation(left, right, 48000)
        assert lags_ms.shape == (0,) and iacf.shape == (0,) and np.isnan(iacc) and np.isnan(tau)
    assert np.array_equal(analysis.energy_decay_curve_db(np.zeros(100)), np.full(100, -80.0))
    assert np.array_equal(analysis.energy_decay_curve_db(np.full(100, 1e-8), floor_db=-60.0), np.full(100, -60.0))   # energy 1e-14
    assert analysis.energy_decay_curve_db([]).shape == (0,)
    bands = [(1001.0, 1007.0), (30000.0, 40000.0), (500.0, 400.0)]
    assert np.all(np.isnan(analysis.band_interaural_level_difference(x, x, 48000, bands)))
    assert np.all(np.isnan(analysis.band_interaural_phase_difference(x, x, 48000, bands)))
    assert analysis.binaural_metrics([], 48000) == []
    with pytest.raises(ValueError, match="above the limit"):
        analysis.interaural_cross_correlation(x, x, 192000, max_delay_ms=11.0)


def _device_rows(rows):
    """the rows as fp32 in one device block: (block, [Row])"""
    from impulse_hip import _native
    from impulse_hip.device_rows import DeviceBlock, Row
    ctx = _native.default_context()
    pitch = [(len(r) + 63) // 64 * 64 for r in rows]
    offs = np.concatenate([[0], np.cumsum(pitch)[:-1]]).astype(np.int64)
    flat = np.zeros(int(sum(pitch)) + 64, dtype=np.float32)
    for r, o in zip(rows, offs):
        flat[o:o + len(r)] = r
    block = DeviceBlock(ctx, len(flat))
    ctx.h2d(block.ptr, flat)
    return block, [Row(block, int(o), len(r)) for r, o in zip(rows, offs)]


def _same(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for key in ("band_sums", "ild_db", "ipd_deg", "lags_ms", "iacf"):
            assert np.array_equal(np.asarray(ra[key]), np.asarray(rb[key]), equal_nan=True), key
        assert np.array_equal([ra["iacc"], ra["tau_ms"]], [rb["iacc"], rb["tau_ms"]], equal_nan=True)
        if "edc_db" in ra:
            assert all(np.array_equal(x, y) for x, y in zip(ra["edc_db"], rb["edc_db"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hrir71_48k", "unequal", "len3430", "zero_ear", "one_sample", "fs192000_5ms"])
def test_device_rows_equal_host_arrays_bit_for_bit(name):
    from impulse_hip import analysis
    from impulse_hip.impulse_response import ImpulseResponse
    fs, pairs, bands, max_delay_ms = ai.case(name)
    block, rows = _device_rows([x for pair in pairs for x in pair])
    irs = [ImpulseResponse.on_device(r, fs) for r in rows]
    dev = analysis.binaural_metrics(list(zip(irs[0::2], irs[1::2])), fs, bands=bands, max_delay_ms=max_delay_ms, edc=True)
    assert all(ir._data is None for ir in irs)                          # read where they are
    host = analysis.binaural_metrics(pairs, fs, bands=bands, max_delay_ms=max_delay_ms, edc=True)
    _same(dev, host)
    block.close()


@pytest.mark.gpu
def test_batch_of_eight_hrirs_equals_one_pair_at_a_time():
    from impulse_hip import analysis
    fs = 48000
    rng = np.random.default_rng(5)
    pairs = []
    for g in range(8):                                                  # 8 HRIRs of 3 pairs, lengths mixed across and inside them
        for k in range(3):
            nl, nr = int(rng.integers(1500, 5000)), int(rng.integers(1500, 5000))
            if k == 0:
                nr = nl = (3430, 3000, 4096, 2187, 4375, 3993, 2401, 4802)[g]
            x = rng.standard_normal(max(nl, nr) + 8) * np.exp(-np.arange(max(nl, nr) + 8) / 600.0)
            left = x[:nl] + 0.1 * rng.standard_normal(nl)
            right = 0.7 * x[5:5 + nr] + 0.1 * rng.standard_normal(nr)
            pairs.append((left.astype(np.float32).astype(np.float64), right.astype(np.float32).astype(np.float64)))
    batched = analysis.binaural_metrics(pairs, fs, max_delay_ms=2.0, edc=True)
    single = [analysis.binaural_metrics([p], fs, max_delay_ms=2.0, edc=True)[0] for p in pairs]
    _same(batched, single)


# ---- the reference's own properties (tests/test_bokeh_analysis.py) ----------------------------------------------------------

FS = 48000


def _noise(seed, n=4096):
    return np.random.default_rng(seed).standard_normal(n)


@pytest.mark.gpu
def test_identical_signals_give_one_at_zero_lag():
    """test_identical_signals_give_unity_at_zero_lag"""
    from impulse_hip import analysis
    x = _noise(1)
    _, iacf, iacc, tau = analysis.interaural_cross_correlation(x, x, FS)
    assert abs(iacc - 1.0) <= 1e-12 and tau == 0.0 and np.all(np.abs(iacf) <= 1.0 + 1e-12)


@pytest.mark.gpu
def test_delayed_attenuated_copy_keeps_full_correlation_at_the_delay():
    """test_delayed_attenuated_copy_keeps_full_correlation: the right ear = the left delayed by d peaks at lag -d"""
    from impulse_hip import analysis
    x = _noise(2)
    d = 12
    right = np.concatenate([np.zeros(d), 0.3 * x])
    left = np.concatenate([x, np.zeros(d)])
    _, _, iacc, tau = analysis.interaural_cross_correlation(left, right, FS)
    assert abs(iacc - 1.0) <= 1e-12 and tau == -d * 1000 / FS
    _, _, iacc, tau = analysis.interaural_cross_correlation(x, right, FS)        # unequal lengths, same convention
    assert abs(iacc - 1.0) <= 1e-12 and tau == -d * 1000 / FS


@pytest.mark.gpu
def test_uncorrelated_noise_is_low():
    """test_uncorrelated_noise_has_low_iacc"""
    from impulse_hip import analysis
    _, _, iacc, _ = analysis.interaural_cross_correlation(_noise(3, 48000), _noise(4, 48000), FS)
    assert iacc < 0.1


@pytest.mark.gpu
def test_pure_delay_gives_the_band_centre_phase_and_wraps():
    """test_pure_delay_gives_band_center_phase / test_ipd_wraps_to_plus_minus_180: a delay of dt seconds on the right ear is
    2 pi f dt of phase at every bin; the energy-weighted mean over a band of white noise sits at the band's middle"""
    from impulse_hip import analysis
    n, d = 48000, 5
    x = _noise(6, n)
    right = np.roll(x, d)                                               # circular: every bin's phase is exactly 2 pi k d / n
    bands = analysis.octave_bands(FS)
    ipd = analysis.band_interaural_phase_difference(x, right, FS, bands)
    assert all(-180.0 <= v <= 180.0 for v in ipd)
    for (lo, hi), v in zip(bands, ipd):
        if (hi - lo) * d / FS < 0.45:                                   # the band spans less than half a turn: the mean is defined
            mid = 360.0 * 0.5 * (lo + min(hi, FS / 2)) * d / FS
            assert abs((v - mid + 180.0) % 360.0 - 180.0) < 10.0, (lo, hi, v, mid)
    assert any(abs(360.0 * 0.5 * (lo + hi) * d / FS) > 180.0 for lo, hi in bands)        # some band did wrap


@pytest.mark.gpu
def test_level_scaled_copy_gives_a_uniform_ild():
    """test_level_scaled_copy_gives_uniform_ild"""
    from impulse_hip import analysis
    x = _noise(7)
    ild = analysis.band_interaural_level_difference(x, 0.5 * x, FS, analysis.octave_bands(FS))
    assert np.max(np.abs(np.array(ild) - 20 * np.log10(2.0))) <= 1e-9


@pytest.mark.gpu
def test_edc_is_the_schroeder_integral():
    """test_edc_is_schroeder_integral / starts at 0 dB / never rises"""
    from impulse_hip import analysis
    x = _noise(8, 20000) * np.exp(-np.arange(20000) / 3000.0)
    c = analysis.energy_decay_curve_db(x)
    e = np.cumsum((x ** 2)[::-1])[::-1]
    assert abs(c[0]) <= 1e-9 and np.all(np.diff(c) <= 0.0)
    assert np.max(np.abs(c - 10 * np.log10(e / (e[0] + 1e-12) + 1e-12))) <= TOL_EDC_DB


# ---- HRIR.binaural_analysis on the rows run_slice leaves ----------------------------------------------------------------

@pytest.mark.gpu
def test_hrir_binaural_analysis_on_device_rows_of_run_slice():
    from test_mic_deviation import _slice_inputs
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse
    from impulse_hip.pipeline_slice import run_slice
    e, recs, firs = _slice_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, _ = run_slice(e, recs, firs=firs)
    irs = [ir for pair in got.irs.values() for ir in pair.values()]
    assert all(ir._data is None for ir in irs)
    dev = got.binaural_analysis(max_delay_ms=1.0, edc=True)
    assert all(ir._data is None for ir in irs)                          # still on the device
    assert list(dev) == list(got.irs)
    h = HRIR(e)
    for sp, pair in got.irs.items():
        h.irs[sp] = {sd: ImpulseResponse(np.array(ir.data, dtype=np.float64), e.fs) for sd, ir in pair.items()}
    host = h.binaural_analysis(max_delay_ms=1.0, edc=True)
    for sp in dev:
        assert set(dev[sp]) == {"bands", "ild_db", "ipd_deg", "iacc", "tau_ms", "lags_ms", "iacf", "edc_db"}
        for key in ("ild_db", "ipd_deg", "lags_ms", "iacf"):
            assert np.array_equal(np.asarray(dev[sp][key]), np.asarray(host[sp][key]), equal_nan=True), (sp, key)
        assert dev[sp]["iacc"] == host[sp]["iacc"] and dev[sp]["tau_ms"] == host[sp]["tau_ms"]
        assert 0.0 < dev[sp]["iacc"] <= 1.0 + 1e-12
        for sd in ("left", "right"):
            assert np.array_equal(dev[sp]["edc_db"][sd], host[sp]["edc_db"][sd])


# ---- refusals: argument checks only ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_bad_arguments_are_refused():
    import ctypes as C
    from impulse_hip import _native
    ctx = _native.default_context()
    lib, h = ctx._lib, ctx._h
    x = np.random.default_rng(9).standard_normal(200)
    rows = [x[:100], x[100:]]
    good = dict(nfft=[100], bins=[[[1, 5]]], D=4)

    def code(call):
        with pytest.raises(_native.NativeError) as info:
            call()
        return info.value.code

    INVALID, UNSUPPORTED = -1, _native.IMP_ERR_UNSUPPORTED
    assert ctx.binaural_metrics(rows, **good)[0].shape == (1, 1, 4)
    assert code(lambda: ctx.binaural_metrics(rows, [100], [[[1, 5]]], 2049)) == UNSUPPORTED          # D above the cap
    assert code(lambda: ctx.binaural_metrics(rows, [100], [[[1, 5]]], -1)) == INVALID
    assert code(lambda: ctx.binaural_metrics(rows, [96], [[[1, 5]]], 4)) == INVALID                   # nfft shorter than a row
    assert code(lambda: ctx.binaural_metrics(rows, [202], [[[1, 5]]], 4)) == UNSUPPORTED              # 2 * 101: not 11-smooth
    assert code(lambda: ctx.binaural_metrics(rows, [100], [[[1, 52]]], 4)) == INVALID                 # beyond nfft / 2 + 1
    assert code(lambda: ctx.binaural_metrics(rows, [100], [[[5, 1]]], 4)) == INVALID
    assert code(lambda: ctx.binaural_metrics(rows, [100], [[[-1, 5]]], 4)) == INVALID
    i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    off, ln = np.array([0, 100], dtype=np.int64), np.array([100, 100], dtype=np.int64)
    neg = np.array([100, -1], dtype=np.int64)
    iacf, energy, peak = np.zeros(9), np.zeros(2), np.zeros(1, dtype=np.int64)
    out = (iacf.ctypes.data_as(f64), peak.ctypes.data_as(i64), energy.ctypes.data_as(f64))
    args = lambda xp, lp: (h, xp, off.ctypes.data_as(i64), lp.ctypes.data_as(i64), 1, None, None, 0, 4, None) + out   # noqa: E731
    assert lib.imp_binaural_metrics(*args(None, ln)) == INVALID                                       # null rows
    assert lib.imp_binaural_metrics_device(*args(None, ln)) == INVALID
    assert lib.imp_binaural_metrics(*args(x.ctypes.data_as(f64), neg)) == INVALID                     # negative length
    curve = np.zeros(200)
    edc = lambda xp, lp: (h, xp, off.ctypes.data_as(i64), lp.ctypes.data_as(i64), 2, -80.0, curve.ctypes.data_as(f64))   # noqa: E731
    assert lib.imp_energy_decay_db(*edc(None, ln)) == INVALID
    assert lib.imp_energy_decay_db_device(*edc(None, ln)) == INVALID
    assert lib.imp_energy_decay_db(*edc(x.ctypes.data_as(f64), neg)) == INVALID
    assert lib.imp_energy_decay_db(*edc(x.ctypes.data_as(f64), ln)) == 0
    assert np.all(np.diff(curve[:100]) <= 0) and abs(curve[0]) <= 1e-9          # 10 log10(e / (e + 1e-12) + 1e-12): not exactly 0
