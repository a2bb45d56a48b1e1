"""Polyphase resampling on the MI355X (K17): every case against the NumPy model in np.longdouble and against SciPy, device
rows against host arrays, batched against one row at a time, silence, reduced ratios, resample_hrir(s) through normalize and
write_wav, and the refusals.  The cases (ratios, ragged row lengths, filters) live in tests/model/resample_model.py; the
20 000-sample row gives 78 to 341 tiles of 256 outputs at the ratios here, and with 16 001 taps its outputs need several
staged input spans (4096 samples each) at 2/1, 1/2 and 3/2."""
import numpy as np
import pytest

import resample_model as rm

# e_ref: SciPy's own rounding error, the largest |scipy.signal.resample_poly in float64 - the model in np.longdouble| over
# the cases, relative to each row's largest output sample, measured on the CPU (tests/test_resample_cpu.py, which asserts
# that it still holds); the device is held to 10 x e_ref.  Worst case measured on the MI355X: see DESIGN.md section 14.
E_REF = 1.19e-14
TOL = 1.19e-13

CASES = rm.case_ids()


def _device_rows(rows, fs):
    """the rows as fp32 device rows of one block, as ImpulseResponse objects (as tests/test_plot_data.py builds them)"""
    from impulse_hip import _native
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.impulse_response import ImpulseResponse
    pitch = [(len(r) + 63) // 64 * 64 for r in rows]
    offs = np.concatenate([[0], np.cumsum(pitch)[:-1]]).astype(np.int64)
    ctx = _native.default_context()
    block = DeviceBlock(ctx, int(sum(pitch)))
    flat = np.zeros(int(sum(pitch)), dtype=np.float32)
    for o, r in zip(offs, rows):
        flat[o:o + len(r)] = r
    ctx.h2d(block.ptr, flat)
    return [ImpulseResponse.on_device(Row(block, int(o), len(r)), fs) for o, r in zip(offs, rows)]


def _peak(a):
    return float(np.max(np.abs(a))) if len(a) else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_host_entry_against_model_and_scipy(name, gpu_ctx):
    from impulse_hip.resampling import resample_poly_rows
    up, down, taps, rows = rm.case(name)
    model, scipy_rows = rm.reference(name)
    got = resample_poly_rows(rows, up, down, taps)
    worst_model = worst_scipy = 0.0
    for k, (y, a, b) in enumerate(zip(got, model, scipy_rows)):
        assert isinstance(y, np.ndarray) and y.dtype == np.float64 and len(y) == len(b) == len(a), (name, k)
        if len(y) and _peak(a) > 0:
            worst_model = max(worst_model, float(np.max(np.abs(y - a))) / _peak(a))
            worst_scipy = max(worst_scipy, float(np.max(np.abs(y - b))) / _peak(a))
    print(f"{name}: device - model {worst_model / E_REF:.3f} e_ref, device - scipy {worst_scipy / E_REF:.3f} e_ref")
    assert worst_model <= TOL and worst_scipy <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_rows_are_read_in_place_and_share_the_arithmetic(name, gpu_ctx):
    from impulse_hip.resampling import resample_poly_rows, resample_rows
    up, down, taps, rows = rm.case(name)                         # float32-valued
    model, _ = rm.reference(name)
    fs_new, fs_old = 300 * up, 300 * down                        # 147/160 is 44.1 k from 48 k
    irs = _device_rows(rows, fs_old)
    got = resample_rows(irs, fs_new, fs_old, taps=taps)          # nnresample's argument order
    assert all(ir._data is None and ir._row is not None and ir.fs == fs_old for ir in irs)   # the sources stayed as they were
    assert all(y._data is None and y._row is not None and y.fs == fs_new for y in got)
    assert len({id(y._row.block) for y in got}) == 1 and got[0]._row.block is not irs[0]._row.block
    host = resample_poly_rows(rows, up, down, taps)
    for k, (y, a, h) in enumerate(zip(got, model, host)):
        assert len(y) == len(a), (name, k)
        dev = y.peek().astype(np.float32)
        assert y._data is None                                   # peek leaves it on the device
        assert np.array_equal(dev, h.astype(np.float32)), (name, k)           # one arithmetic behind both entry points
        want = a.astype(np.float32)
        assert np.all(np.abs(dev.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["147_160_L16001", "2_1_L16001", "1_2_L16001", "3_2_L16001", "640_147_L16001", "2_1_L100", "147_160_L7"])
def test_batch_equals_single_rows_in_any_order(name, gpu_ctx):
    from impulse_hip.resampling import resample_poly_rows
    up, down, taps, rows = rm.case(name)
    batch = resample_poly_rows(rows, up, down, taps)
    for k, x in enumerate(rows):
        assert np.array_equal(resample_poly_rows([x], up, down, taps)[0], batch[k]), (name, k)
    order = [5, 0, 3, 1, 4, 2]
    for k, y in zip(order, resample_poly_rows([rows[k] for k in order], up, down, taps)):
        assert np.array_equal(y, batch[k]), (name, k)
    # device rows: alone, and in another order in another block
    irs = _device_rows(rows, 48000)
    dev = [r.to_host() for r in resample_poly_rows(irs, up, down, taps)]
    other = _device_rows([rows[k] for k in order], 48000)
    for k, r in zip(order, resample_poly_rows(other, up, down, taps)):
        assert np.array_equal(r.to_host(), dev[k]), (name, k)
    assert np.array_equal(resample_poly_rows([irs[5]], up, down, taps)[0].to_host(), dev[5])
    # a mix: device rows stay on the device, arrays come back as arrays, each as in its own batch
    mixed = resample_poly_rows([irs[5], rows[4], irs[3], rows[5]], up, down, taps)
    assert np.array_equal(mixed[0].to_host(), dev[5]) and np.array_equal(mixed[2].to_host(), dev[3])
    assert np.array_equal(mixed[1], batch[4]) and np.array_equal(mixed[3], batch[5])
    assert irs[5]._data is None and irs[3]._data is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["147_160_L16001", "2_1_L16001", "147_320_L16001", "2_1_L1"])
def test_silent_row_gives_exact_zeros(name, gpu_ctx):
    from impulse_hip.resampling import resample_poly_rows
    up, down, taps, rows = rm.case(name)
    got = resample_poly_rows([rows[4], np.zeros(1500), rows[3]], up, down, taps)
    assert len(got[1]) == rm.out_len(1500, up, down) and not got[1].any()
    dev = resample_poly_rows(_device_rows([rows[4], np.zeros(1500)], 48000), up, down, taps)
    assert dev[1].n == len(got[1]) and not dev[1].to_host().any()


@pytest.mark.gpu
@pytest.mark.parametrize("up,down", [(48000, 48000), (7, 7), (1, 1)])
def test_equal_rates_copy_the_rows(up, down, gpu_ctx):
    from impulse_hip.resampling import kaiser_null_filter, resample_poly_rows, resample_rows
    rows = rm.case_rows(up, down, 16001)
    for taps in (np.ones(1), kaiser_null_filter(2, 1)):          # the filter is not applied, whatever it is
        got = resample_poly_rows(rows, up, down, taps)
        for x, y in zip(rows, got):
            assert np.array_equal(x, y) and y is not x
    irs = _device_rows(rows, up)
    got = resample_rows(irs, up, down)
    for ir, y, x in zip(irs, got, rows):
        assert y is not ir and y._row is not ir._row and y._row.block is not ir._row.block
        assert np.array_equal(y.peek(), x) and y.fs == up


def _hrir(rows, fs, device):
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse

    class _Est:
        pass

    est = _Est()
    est.fs = fs
    h = HRIR(est)
    irs = _device_rows(rows, fs) if device else [ImpulseResponse(x.copy(), fs) for x in rows]
    for (sp, sd), ir in zip([("FL", "left"), ("FL", "right"), ("FR", "left"), ("FR", "right")], irs):
        h.irs.setdefault(sp, {})[sd] = ir
    return h


@pytest.mark.gpu
def test_resample_hrir(gpu_ctx, tmp_path):
    from scipy.signal import resample_poly
    from impulse_hip import _native
    from impulse_hip.audio_io import read_wav
    from impulse_hip.resampling import kaiser_null_filter, resample_hrir, resample_hrirs
    rng = np.random.default_rng(17)
    rows = [(rng.standard_normal(3000) * np.exp(-np.arange(3000) / 400.0)).astype(np.float32).astype(np.float64) for _ in range(4)]
    taps = kaiser_null_filter(44100, 48000)
    want = [resample_poly(x, 44100, 48000, window=taps) for x in rows]
    done = {}
    for device in (True, False):
        h = _hrir(rows, 48000, device)
        assert resample_hrir(h, 44100) is h and h.fs == 44100
        irs = [ir for _, _, ir in h._all_irs()]
        assert all(ir.fs == 44100 and len(ir) == 2757 for ir in irs)
        assert all((ir._data is None) == device for ir in irs)   # device rows stayed on the device, arrays on the host
        done[device] = [ir.peek() for ir in irs]
        for y, w in zip(done[device], want):
            tol = TOL * _peak(w) + (np.spacing(np.float32(_peak(w))) / 2 if device else 0.0)     # the fp32 row's one rounding
            assert np.max(np.abs(y - w)) <= tol
        # the stages that follow in the reference: normalize, then the WAV
        h.normalize(peak_target=-0.1)
        path = str(tmp_path / f"hrir_{int(device)}.wav")
        h.write_wav(path, track_order=["FL-left", "FL-right", "FR-left", "FR-right"])
        fs_file, frames = read_wav(path)
        assert fs_file == 44100 and frames.shape == (4, 2757)
    # many HRIRs in one call: the same bits as one at a time
    both = [_hrir(rows, 48000, True), _hrir(rows, 48000, False)]
    assert resample_hrirs(both, 44100) == both
    for h, device in zip(both, (True, False)):
        assert h.fs == 44100
        for (_, _, ir), y in zip(h._all_irs(), done[device]):
            assert ir.fs == 44100 and (ir._data is None) == device and np.array_equal(ir.peek(), y)
    # taps= is used as handed in
    h = _hrir(rows, 48000, False)
    resample_hrir(h, 44100, taps=np.ones(1))
    assert np.array_equal(h.irs["FL"]["left"].data, resample_poly(rows[0], 44100, 48000, window=np.ones(1)))
    # the rate it already has: nothing changes and nothing is launched
    h = _hrir(rows, 48000, True)
    before = [ir._row for _, _, ir in h._all_irs()]
    ctx = _native.default_context()
    real = ctx.resample_poly
    ctx.resample_poly = None                                     # any call would raise
    try:
        assert resample_hrir(h, 48000) is h
    finally:
        del ctx.resample_poly
    assert ctx.resample_poly == real
    assert h.fs == 48000 and all(ir._row is r and ir.fs == 48000 for (_, _, ir), r in zip(h._all_irs(), before))


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(gpu_ctx):
    from impulse_hip import _native
    from impulse_hip.resampling import resample_poly_rows
    x = [np.arange(50.0), np.ones(3)]
    ok = np.array([0.25, 0.5, 0.25])
    for up, down, taps in ((0, 1, ok), (2, 0, ok), (2, 1, np.ones(0)), (2, 1, np.ones((3, 3))), (2, 1, np.ones(65537))):
        with pytest.raises(ValueError):
            resample_poly_rows(x, up, down, taps)
        with pytest.raises(ValueError):
            resample_poly_rows(_device_rows(x, 48000), up, down, taps)
    with pytest.raises(_native.NativeError) as exc:
        gpu_ctx.resample_poly(x, 2, 1, np.ones(65537))
    assert exc.value.code == _native.IMP_ERR_UNSUPPORTED and "65537" in str(exc.value)
    with pytest.raises(_native.NativeError) as exc:
        gpu_ctx.resample_poly(x, 0, 1, ok)
    assert exc.value.code == _native.IMP_ERR_INVALID
    # the next valid call passes, the longest filter the entry takes included; an empty batch is fine
    from scipy.signal import resample_poly
    got = resample_poly_rows(x, 2, 1, ok)
    for y, row in zip(got, x):
        assert np.max(np.abs(y - resample_poly(row, 2, 1, window=ok))) <= TOL * _peak(y)
    long_taps = np.zeros(65536)
    long_taps[32767] = 1.0                                       # the centre tap of an even filter: half = 32767
    assert np.array_equal(resample_poly_rows(x, 1, 1, long_taps)[0], x[0])
    got = resample_poly_rows(x, 1, 3, long_taps)[0]
    assert np.array_equal(got, x[0][::3])
    assert resample_poly_rows([], 2, 1, ok) == [] and gpu_ctx.resample_poly([], 2, 1, ok) == []


@pytest.mark.gpu
@pytest.mark.parametrize("up,down", [(1, 9), (1, 20), (1, 5000), (4, 1), (500, 1), (1001, 1000)])
def test_tiles_of_other_ratios(up, down, gpu_ctx):
    """ratios whose plan differs from the listed ones: a tile cut down to 103 outputs (1/20) or to one (1/5000) because
    the inputs of 256 outputs would not fit the staged span, up = 4 (no phase shared by a wave), more phases than taps
    (500/1, 1001/1000 with 101 taps: the later phases are zero).  Fewer terms per output than in the cases E_REF comes
    from, so TOL holds with room."""
    from scipy.signal import firwin, resample_poly
    from impulse_hip.resampling import resample_poly_rows
    rng = np.random.default_rng([up, down])
    rows = [rng.standard_normal(n) for n in (12345, 0, 700, 3)]
    taps = firwin(101, 1 / max(up, down), window=("kaiser", 5.0))
    got = resample_poly_rows(rows, up, down, taps)
    for x, y in zip(rows, got):
        want = resample_poly(x, up, down, window=taps)
        assert len(y) == len(want) == rm.out_len(len(x), up, down)
        if len(y):
            assert np.max(np.abs(y - want)) <= TOL * _peak(want), (up, down, len(x))
