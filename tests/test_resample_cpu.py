"""K17 without a GPU: the result length from the library, the NumPy model of the polyphase arithmetic against SciPy on
every case the GPU test uses (and the reference's own error E_REF that the GPU tolerance is ten times of), the host-side
filter design kaiser_null_filter, and the refusals that stay."""
import numpy as np
import pytest

import resample_model as rm
from test_resample import E_REF, TOL

LENGTHS = [0, 1, 2, 159, 160, 161, 4099]


def _scipy_len(n, up, down):
    from scipy.signal import resample_poly
    return len(resample_poly(np.zeros(n), up, down))


@pytest.mark.parametrize("up,down", rm.RATIOS)
def test_length_entry_equals_scipy(up, down):
    from impulse_hip import _native
    for n in LENGTHS:
        assert _native.resample_poly_len(n, up, down) == _scipy_len(n, up, down) == rm.out_len(n, up, down), (n, up, down)


def test_length_entry_refuses():
    from impulse_hip import _native
    for n, up, down in ((10, 0, 1), (10, 1, 0), (10, -3, 2), (-1, 1, 2)):
        with pytest.raises(_native.NativeError) as exc:
            _native.resample_poly_len(n, up, down)
        assert exc.value.code == _native.IMP_ERR_INVALID
    with pytest.raises(_native.NativeError) as exc:
        _native.resample_poly_len(2 ** 40, 2 ** 30, 1)
    assert exc.value.code == _native.IMP_ERR_UNSUPPORTED
    assert _native.resample_poly_len(2 ** 40, 2 ** 20, 2 ** 21) == 2 ** 39


def test_model_against_scipy_and_e_ref():
    worst = 0.0
    for name in rm.case_ids():
        up, down, taps, rows = rm.case(name)
        model, scipy_rows = rm.reference(name)
        for x, a, b in zip(rows, model, scipy_rows):
            assert len(a) == len(b) == rm.out_len(len(x), up, down), (name, len(x))
            if len(a) and np.max(np.abs(a)) > 0:
                worst = max(worst, float(np.max(np.abs(b - a)) / np.max(np.abs(a))))
    print(f"e_ref {worst:.4e}")
    assert worst <= E_REF and TOL == pytest.approx(10 * E_REF, rel=1e-12)
    assert worst > 0.9 * E_REF                                   # the constant is the measurement, not a bound with slack


def test_model_in_float64_and_short_rows():
    from scipy.signal import firwin, resample_poly
    rng = np.random.default_rng(5)
    for up, down in ((147, 160), (2, 1), (3, 2), (147, 320)):
        for L in (100, 7):
            taps = firwin(L, 1 / max(up, down))
            for n in (1, 5, 50, 333):
                x = rng.standard_normal(n)
                want = resample_poly(x, up, down, window=taps)
                got = rm.resample_poly(x, up, down, taps, dtype=np.float64)
                assert got.dtype == np.float64 and len(got) == len(want)
                assert np.max(np.abs(got - want)) <= 1e-14 * np.max(np.abs(want))
    x = rng.standard_normal(9)
    assert np.array_equal(rm.resample_poly(x, 7, 7, np.ones(3), dtype=np.float64), x)


DESIGN_RATIOS = [(147, 160), (2, 1), (640, 147), (3, 2), (147, 320)]


@pytest.mark.parametrize("up,down", DESIGN_RATIOS)
def test_kaiser_null_filter(up, down):
    from scipy.signal import firwin
    from impulse_hip.resampling import kaiser_null_filter, null_filter_cutoff
    h = kaiser_null_filter(up, down)
    assert h.dtype == np.float64 and h.shape == (16001,)
    assert np.array_equal(h, h[::-1])
    assert abs(h.sum() - 1) <= 1e-12
    assert np.array_equal(h, firwin(16001, null_filter_cutoff(up, down), window=("kaiser", 5.0)))
    assert kaiser_null_filter(up, down) is h and kaiser_null_filter(up, down, beta=5.0, L=16001) is h
    assert kaiser_null_filter(300 * up, 300 * down) is h
    # the first null sits on the slower rate's Nyquist frequency: a direct DFT there
    max_rate = max(up, down)
    w = np.exp(-1j * np.pi * np.arange(len(h)) / max_rate)
    null = abs(np.sum(h * w))
    plain = abs(np.sum(firwin(16001, 1 / max_rate, window=("kaiser", 5.0)) * w))
    print(f"{up}/{down}: |H(1 / max_rate)| = {null:.2e} (unshifted design {plain:.3f})")
    assert null <= 1e-3 and plain > 0.4


def test_kaiser_null_filter_other_arguments():
    from impulse_hip.resampling import kaiser_null_filter
    assert kaiser_null_filter(44100, 48000) is kaiser_null_filter(147, 160)
    short = kaiser_null_filter(2, 1, beta=8.0, L=801)
    assert short.shape == (801,) and np.array_equal(short, short[::-1]) and short is not kaiser_null_filter(2, 1)
    for bad in ((0, 1), (1, -1), (1.5, 2)):
        with pytest.raises(ValueError):
            kaiser_null_filter(*bad)
    with pytest.raises(ValueError):
        kaiser_null_filter(48000, 48000)


@pytest.mark.parametrize("up,down", DESIGN_RATIOS)
def test_kaiser_null_filter_equals_nnresample(up, down):
    nn = pytest.importorskip("nnresample")
    from impulse_hip.resampling import kaiser_null_filter
    assert np.array_equal(kaiser_null_filter(up, down), nn.compute_filt(up, down, beta=5.0, L=16001))


def test_class_methods_still_refuse_and_the_module_is_there():
    from impulse_hip import resampling
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse

    class _Est:
        fs = 48000

    with pytest.raises(NotImplementedError, match="nnresample"):
        HRIR(_Est()).resample(44100)
    with pytest.raises(NotImplementedError, match="nnresample"):
        ImpulseResponse(np.zeros(8), 48000).resample(44100)
    for name in ("kaiser_null_filter", "resample_poly_rows", "resample_rows", "resample_hrir", "resample_hrirs"):
        assert callable(getattr(resampling, name))
    # refused before anything reaches a device
    for rows, up, down, taps in (([np.ones(4)], 0, 1, np.ones(3)), ([np.ones(4)], 1, 2, np.ones(0)), ([np.ones(4)], 1, 2, np.ones((2, 2)))):
        with pytest.raises(ValueError):
            resampling.resample_poly_rows(rows, up, down, taps)
