"""Resampling of responses to another sample rate: the --fs stage of the reference (core/pipeline.py:851-863 _stage_resample ->
core/hrir.py:890-919 HRIR.resample -> core/impulse_response.py:121-124), which is

    ir.data = nnresample.resample(ir.data, fs, ir.fs);  ir.fs = fs

nnresample.resample(s, up, down, beta=5.0, L=16001) is a one-off filter design on the host (compute_filt) followed by
scipy.signal.resample_poly(s, up, down, window=taps).  Here the polyphase arithmetic runs on the device, K17
(imp_resample_poly*): fp64 products and sums, rows that live on the device (device_rows.py) read where they are and written
as new device rows, host arrays uploaded as float64.  That arithmetic is pinned to SciPy by the tests.

The filter design stays on the host: kaiser_null_filter restates nnresample.compute_filt.  It is written from knowledge of
that package (0.2.4) and cannot be compared with it where nnresample is not importable, so the parity of the DEFAULT filter is
unpinned there.  Every function takes taps=: hand in nnresample.compute_filt(up, down, beta, L) itself and the result is
the reference's, with no caveat.

HRIR.resample and ImpulseResponse.resample keep refusing; resample_hrir(hrir, fs) is what a pipeline calls in their place.
"""
from math import gcd

import numpy as np

from . import _native

_FILTERS = {}


def _reduced(up, down):
    if int(up) != up or int(down) != down:
        raise ValueError(f"resampling needs whole-number rates (got {up}, {down})")
    up, down = int(up), int(down)
    if up <= 0 or down <= 0:
        raise ValueError(f"resampling needs positive rates (got {up}, {down})")
    g = gcd(up, down)
    return up // g, down // g


def null_filter_cutoff(up, down, beta=5.0, L=16001):
    """The cutoff (in units of Nyquist) of the second firwin call of nnresample.compute_filt: 2 / max_rate minus the first
    null of the plain Kaiser design, found on a 2^19-point grid."""
    from scipy.signal import firwin
    up, down = _reduced(up, down)
    max_rate = max(up, down)
    if max_rate == 1:
        raise ValueError("equal rates need no filter")
    L = int(L)
    first = firwin(L, 1 / max_rate, window=("kaiser", beta))
    N = 2 ** 19
    NBINS = N / 2 + 1
    padded = np.zeros(N)
    padded[:L] = first
    F = np.fft.rfft(padded)
    bot = int(np.floor(NBINS / max_rate))
    top = int(np.ceil(NBINS * (1 / max_rate + 2 * np.sqrt(1 + (beta / np.pi) ** 2) / L)))
    firstnull = (np.argmin(np.abs(F[bot:top])) + bot) / NBINS
    return 2 / max_rate - firstnull


def kaiser_null_filter(up, down, beta=5.0, L=16001):
    """nnresample.compute_filt(up, down, beta, L), restated: a Kaiser-windowed low-pass of L taps whose cutoff is moved so that
    the design's first null, not its -6 dB point, falls on the Nyquist frequency of the slower rate.  Host only
    (scipy.signal.firwin twice, one 2^19-point rfft); cached per reduced (up, down, beta, L), so equal arguments return the
    same read-only array.

    This recipe is written from knowledge of nnresample 0.2.4.  It cannot be compared with the package on a machine where
    the package is not importable; there the parity of this filter with the reference's is unpinned.  Where nnresample is
    available, pass taps=nnresample.compute_filt(...) to the functions below."""
    from scipy.signal import firwin
    up, down = _reduced(up, down)
    key = (up, down, float(beta), int(L))
    if key not in _FILTERS:
        taps = np.ascontiguousarray(firwin(int(L), null_filter_cutoff(up, down, beta, L), window=("kaiser", beta)), dtype=np.float64)
        taps.setflags(write=False)
        _FILTERS[key] = taps
    return _FILTERS[key]


def _is_response(r):
    return hasattr(r, "peak_index")


def _device_row(r, ctx):
    """the device row of a response that lives on ctx's device, else None"""
    row = getattr(r, "_row", None) if getattr(r, "_data", 0) is None else None
    return row if row is not None and row.block.ctx is ctx else None


def _host_row(r):
    if _is_response(r):
        return np.asarray(r.peek() if r._data is None else r._data, dtype=np.float64).ravel()
    return np.asarray(r, dtype=np.float64).ravel()


def _call(fn, *args, **kwargs):
    try:
        return fn(*args, **kwargs)
    except _native.NativeError as exc:
        if exc.code in (_native.IMP_ERR_UNSUPPORTED, _native.IMP_ERR_INVALID):
            raise ValueError(str(exc)) from exc
        raise


def resample_poly_rows(rows, up, down, taps):
    """scipy.signal.resample_poly(row, up, down, window=taps) of every row, on the device (K17).  rows: ndarrays,
    ImpulseResponse objects, or a mix.  A response that lives on the device is read in place and comes back as a
    device_rows.Row of one new DeviceBlock (fp32, one launch for all of them); anything else comes back as a float64 array (one
    more launch for all of those).  Refused arguments raise ValueError."""
    rows = list(rows)
    taps = np.asarray(taps, dtype=np.float64)
    if taps.ndim != 1 or taps.size == 0:
        raise ValueError(f"taps of shape {taps.shape}: need a one-dimensional filter of at least one tap")
    _reduced(up, down)
    up, down = int(up), int(down)
    if not rows:
        return []
    ctx = _native.default_context()
    dev = [_device_row(r, ctx) for r in rows]
    out = [None] * len(rows)
    on_dev = [k for k, r in enumerate(dev) if r is not None]
    on_host = [k for k, r in enumerate(dev) if r is None]
    if on_dev:
        from .device_rows import DeviceBlock, Row, span
        base, offs, lens = span([dev[k] for k in on_dev])
        n_out = [_call(_native.resample_poly_len, n, up, down) for n in lens]
        pitch = [(n + 63) // 64 * 64 for n in n_out]
        dst_off = np.concatenate([[0], np.cumsum(pitch)[:-1]]).astype(np.int64)
        block = DeviceBlock(ctx, int(sum(pitch)))
        _call(ctx.resample_poly, (offs, lens), up, down, taps, dptr=base, d_dst=block.ptr, dst_off=dst_off)
        for k, o, n in zip(on_dev, dst_off, n_out):
            out[k] = Row(block, int(o), int(n))
    if on_host:
        for k, y in zip(on_host, _call(ctx.resample_poly, [_host_row(rows[k]) for k in on_host], up, down, taps)):
            out[k] = y
    return out


def resample_rows(rows, fs_new, fs_old, beta=5.0, L=16001, taps=None):
    """nnresample.resample(row, fs_new, fs_old, beta=beta, L=L) of every row (argument order and defaults as there).
    taps: the filter to use instead of kaiser_null_filter(fs_new, fs_old, beta, L), e.g. nnresample.compute_filt(...) itself.
    A device-resident response comes back as a device-resident ImpulseResponse at fs_new, anything else as a float64 array."""
    up, down = _reduced(fs_new, fs_old)
    if taps is None:
        taps = np.ones(1) if up == down else kaiser_null_filter(up, down, beta, L)
    from .impulse_response import ImpulseResponse
    return [ImpulseResponse.on_device(y, fs_new) if not isinstance(y, np.ndarray) else y
            for y in resample_poly_rows(rows, up, down, taps)]


def resample_hrirs(hrirs, fs, taps=None):
    """HRIR.resample(fs) (core/hrir.py:890-919) of every HRIR of `hrirs`: the responses of all of them go through one call
    per residency (device rows stay on the device, host arrays stay on the host) and per rate they come from; every ir.fs
    and hrir.fs is set to fs.  An HRIR that already is at fs is left alone, as _stage_resample skips it.  Returns hrirs."""
    hrirs = list(hrirs)
    groups = {}
    for h in hrirs:
        if h.fs == fs:
            continue
        for pair in h.irs.values():
            for ir in pair.values():
                groups.setdefault(ir.fs, []).append(ir)
    for fs_old, irs in groups.items():
        for ir, y in zip(irs, resample_rows(irs, fs, fs_old, taps=taps)):
            if isinstance(y, np.ndarray):
                ir.data = y
            else:
                ir._data, ir._row = None, y._row
            ir.fs = fs
    for h in hrirs:
        h.fs = fs
    return hrirs


def resample_hrir(hrir, fs, taps=None):
    """HRIR.resample(fs) of the reference for one HRIR; see resample_hrirs."""
    resample_hrirs([hrir], fs, taps=taps)
    return hrir
