"""The numbers behind ImpulseResponse.plot() of the reference (core/plotting/impulse_response_plotter.py): the spectrogram of
every channel's recorded sweep (:114-293 plot_spectrogram) and the decay waterfall of every response (:459-609
plot_waterfall).  Nothing is drawn here; the functions return what the reference hands to pcolormesh and plot_surface.

The short-time transforms run on the device, K16 (imp_stft_db*): scipy.signal.spectrogram with a periodic Hann window, every
segment freed of its mean, bin 0 dropped, as 10 log10(|psd| + 1e-9) or as scaled magnitudes.  Rows of one geometry (nfft, hop)
share one device call; rows that live on the device (device_rows.py) are read where they are, host arrays are uploaded as
float64.  The waterfall's finishing - 233 x 13 values per row at 48 kHz - stays in NumPy and SciPy on the host, as in the
reference.  A segment length the fp64 tile transform does not hold raises ValueError: there is no host fallback.
"""
import numpy as np

from . import _native
from .analysis import _rows_of

WATERFALL_NFFT = 256
WATERFALL_SAMPLES = 5 * 256 + 512          # hop_length * 5 + window_length of the reference's padded copy


def spectrogram_geometry(n, fs, f_res=10, n_segments=200):
    """(nfft, noverlap) the reference chooses for a recording of n samples (:131-212), or None where it draws nothing
    (an empty recording, nfft = 0)."""
    n = int(n)
    if n == 0:
        return None
    min_time_segments = 3
    max_nfft = (2 * n) // (min_time_segments + 1)
    if max_nfft <= 0:
        max_nfft = n
    nfft = round(fs / f_res)
    if nfft > max_nfft and max_nfft > 0:                   # at least 3 segments
        nfft = max_nfft
    if nfft > n:
        nfft = n
    if nfft == 0:
        return None
    if n_segments > 0 and (n - nfft) > 0:
        step_size = (n - nfft) / n_segments
        noverlap = nfft // 2 if step_size <= 1 else int(nfft - step_size)
    else:                                                  # n_segments <= 0, or len <= nfft
        noverlap = nfft // 2
    if noverlap >= nfft:
        noverlap = max(0, nfft - 1)
    if noverlap < 0:
        noverlap = 0
    return int(nfft), int(noverlap)


def spectrogram_axes(n, fs, nfft, noverlap):
    """(f, t) of scipy.signal.spectrogram for n samples, bin 0 dropped from f."""
    f = np.fft.rfftfreq(nfft, 1 / fs)[1:]
    t = np.arange(nfft / 2, n - nfft / 2 + 1, nfft - noverlap) / float(fs)
    return f, t


def _stft(rows_dev, rows_host, nfft, hop, fs, mode, dtype):
    """one device call for rows of one geometry; ValueError for a length K16 does not hold"""
    ctx = _native.default_context()
    try:
        if rows_dev is not None:
            from .device_rows import span
            base, offs, lens = span(rows_dev)
            return ctx.stft_db((offs, lens), nfft, hop, fs, mode, dtype, dptr=base)
        return ctx.stft_db(rows_host, nfft, hop, fs, mode, dtype)
    except _native.NativeError as exc:
        if exc.code == _native.IMP_ERR_UNSUPPORTED:
            raise ValueError(f"segment length {nfft}: {exc}") from exc
        raise


def spectrograms(recordings, fs, f_res=10, n_segments=200, dtype=np.float64):
    """(f, t, z_db) per recording as plot_spectrogram hands them to pcolormesh: f = freqs[1:], t as SciPy returns them,
    z_db [len(f), len(t)] = 10 log10(|psd| + 1e-9); None for a recording the reference draws nothing for (None, empty, or a
    spectrum of one bin).  recordings: arrays, or ImpulseResponse objects whose device rows are read in place.  One device
    call per distinct (nfft, hop); dtype float64 or float32."""
    recordings = list(recordings)
    out = [None] * len(recordings)
    live = [i for i, r in enumerate(recordings) if r is not None]
    if not live:
        return out
    dev, host = _rows_of([recordings[i] for i in live])
    lens = [r.n for r in dev] if dev is not None else [len(r) for r in host]
    groups = {}
    for k, n in enumerate(lens):
        geo = spectrogram_geometry(n, fs, f_res, n_segments)
        if geo is None or geo[0] < 2:                      # nfft = 1: spectrum.shape[0] <= 1
            continue
        groups.setdefault(geo, []).append(k)
    for (nfft, noverlap), members in groups.items():
        z = _stft(None if dev is None else [dev[k] for k in members], None if dev is not None else [host[k] for k in members],
                  nfft, nfft - noverlap, fs, _native.STFT_PSD_DB, dtype)
        for k, zk in zip(members, z):
            f, t = spectrogram_axes(lens[k], fs, nfft, noverlap)
            out[live[k]] = (f, t, zk)
    return out


def waterfall_finish(magnitudes, fs):
    """(t_ms, log10_f, z_db) as plot_waterfall hands them to plot_surface, from the [128, 13] magnitudes of the first
    WATERFALL_SAMPLES samples (:548-575): linear interpolation in log10 f onto 10 * 1.03^k, normalised, clipped to -100 dB,
    smoothed 3 x 3, outer frame dropped."""
    from scipy import interpolate, ndimage
    spectrum = np.asarray(magnitudes, dtype=np.float64)
    freqs, t = spectrogram_axes(WATERFALL_SAMPLES, fs, WATERFALL_NFFT, WATERFALL_NFFT // 2)
    f_max, f_min, step = fs / 2, 10, 1.03
    n_freqs = int(np.log(f_max / f_min) / np.log(step))
    f = f_min * step ** np.arange(n_freqs)
    z = np.ones((len(f), spectrum.shape[1]))
    for i in range(spectrum.shape[1]):
        z[:, i] = interpolate.InterpolatedUnivariateSpline(np.log10(freqs), spectrum[:, i], k=1)(np.log10(f))
    f = np.log10(f)
    z /= np.max(z)
    z = np.clip(z, 10 ** (-100 / 20), np.max(z))
    z = 20 * np.log10(z)
    z = ndimage.uniform_filter(z, size=3, mode="constant")
    t, f = np.meshgrid(t, f)
    return t[1:-1, :-1] * 1000, f[1:-1, :-1], z[1:-1, :-1]


def waterfall_magnitudes(irs, fs):
    """[128, 13] scaled STFT magnitudes of every response's first WATERFALL_SAMPLES samples, zero padded: nfft 256, 50 %
    overlap, mode "magnitude" (:466-530).  One device call; device rows of at least that length are read in place."""
    irs = list(irs)
    if not irs:
        return []
    dev, host = _rows_of(irs)
    if dev is not None and all(r.n >= WATERFALL_SAMPLES for r in dev):
        from .device_rows import Row
        dev = [Row(r.block, r.off, WATERFALL_SAMPLES) for r in dev]
    else:                                                  # a shorter row is zero padded: on the host, the rows stay put
        if host is None:
            host = [ir.peek() if hasattr(ir, "peek") else r.to_host() for ir, r in zip(irs, dev)]
        dev = None
        padded = []
        for x in host:
            s = np.zeros(WATERFALL_SAMPLES)
            m = min(len(x), WATERFALL_SAMPLES)
            s[:m] = x[:m]
            padded.append(s)
        host = padded
    return _stft(dev, host, WATERFALL_NFFT, WATERFALL_NFFT // 2, fs, _native.STFT_MAGNITUDE, np.float64)


def waterfalls(irs, fs):
    """(t_ms, log10_f, z_db) per response as plot_waterfall hands them to plot_surface."""
    return [waterfall_finish(m, fs) for m in waterfall_magnitudes(irs, fs)]
