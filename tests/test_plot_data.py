"""Plot data on the MI355X (K16): every fixture case against the reference-run fixture (plot_data.npz) and the NumPy model,
float32 output, device rows against host arrays, batched against one row at a time, HRIR.spectrograms, the plot-worker
convolutions as device rows, the waterfalls, and the entries' refusals."""
import numpy as np
import pytest

import plot_data_inputs as pdi
import plot_data_model as pm

# e_ref: the reference's own rounding error per quantity, measured on the CPU (the model in np.longdouble against the
# fixture: tests/test_plot_data_cpu.py); the device is held to 10 x e_ref.
# Worst case measured on the MI355X: see DESIGN.md section 13.
E_REF_SPEC_DB, TOL_SPEC_DB = 6.55e-13, 6.55e-12              # spectrogram, dB
E_REF_MAGNITUDE, TOL_MAGNITUDE = 2.70e-16, 2.70e-15          # STFT magnitudes, relative to the row's largest
E_REF_WATERFALL_DB, TOL_WATERFALL_DB = 4.37e-12, 4.37e-11    # finished waterfall, dB

_MODEL = {}


def _model(name):
    """the model's spectrograms of a case at full resolution, computed once"""
    if name not in _MODEL:
        from impulse_hip.plot_data import spectrogram_geometry
        fs, f_res, n_segments, rows = pdi.spec_case(name)
        _MODEL[name] = [np.asarray(pm.spectrogram_db(x, fs, *spectrogram_geometry(len(x), fs, f_res, n_segments)), dtype=np.float64)
                        for x in rows]
    return _MODEL[name]


def _device_rows(rows, fs):
    """the rows as fp32 device rows of one block, as ImpulseResponse objects"""
    from impulse_hip import _native
    from impulse_hip.device_rows import DeviceBlock, Row
    from impulse_hip.impulse_response import ImpulseResponse
    pitch = [(len(r) + 63) // 64 * 64 for r in rows]
    offs = np.concatenate([[0], np.cumsum(pitch)[:-1]]).astype(np.int64)
    ctx = _native.default_context()                              # device rows belong to the context the classes use
    block = DeviceBlock(ctx, int(sum(pitch)))
    flat = np.zeros(int(sum(pitch)), dtype=np.float32)
    for o, r in zip(offs, rows):
        flat[o:o + len(r)] = r
    ctx.h2d(block.ptr, flat)
    return [ImpulseResponse.on_device(Row(block, int(o), len(r)), fs) for o, r in zip(offs, rows)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pdi.SPEC_CASES))
def test_spectrograms_against_fixture_and_model(name, golden, gpu_ctx):
    from impulse_hip.plot_data import spectrograms
    z = golden("plot_data")
    fs, f_res, n_segments, rows = pdi.spec_case(name)
    got = spectrograms(rows, fs, f_res=f_res, n_segments=n_segments)
    model = _model(name)
    worst_model = worst_fixture = 0.0
    for k, (f, t, zk) in enumerate(got):
        p = f"spec/{name}/{k}/"
        assert zk.dtype == np.float64 and zk.shape == tuple(z[p + "shape"]) == model[k].shape
        assert np.array_equal(f, z[p + "f"]) and np.array_equal(t, z[p + "t"])
        worst_model = max(worst_model, float(np.max(np.abs(zk - model[k]))))
        worst_fixture = max(worst_fixture, float(np.max(np.abs(zk[:, z[p + "cols"]] - z[p + "z"]))))
    print(f"{name}: device - model {worst_model:.3e} dB, device - fixture {worst_fixture:.3e} dB")
    assert worst_model <= TOL_SPEC_DB and worst_fixture <= TOL_SPEC_DB


@pytest.mark.gpu
def test_silent_row_is_exactly_the_floor(gpu_ctx):
    from impulse_hip.plot_data import spectrograms
    fs, f_res, n_segments, rows = pdi.spec_case("fs8000")
    assert not rows[2].any()
    got = spectrograms(rows, fs, f_res=f_res, n_segments=n_segments)
    assert np.all(got[2][2] == 10 * np.log10(1e-9))
    assert np.all(spectrograms([rows[2]], fs)[0][2] == 10 * np.log10(1e-9))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fs8000", "fs22050", "fs48000"])
def test_float32_output_is_the_float64_output_rounded(name, gpu_ctx):
    from impulse_hip.plot_data import spectrograms
    fs, f_res, n_segments, rows = pdi.spec_case(name)
    a = spectrograms(rows, fs, f_res=f_res, n_segments=n_segments)
    b = spectrograms(rows, fs, f_res=f_res, n_segments=n_segments, dtype=np.float32)
    for (fa, ta, za), (fb, tb, zb) in zip(a, b):
        assert zb.dtype == np.float32 and np.array_equal(zb, za.astype(np.float32))
        assert np.array_equal(fa, fb) and np.array_equal(ta, tb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fs8000", "fs22050", "fs48000", "f_res20"])
def test_device_rows_equal_host_arrays_and_batch_equals_single(name, gpu_ctx):
    from impulse_hip.plot_data import spectrograms
    fs, f_res, n_segments, rows = pdi.spec_case(name)            # float32-representable
    host = spectrograms(rows, fs, f_res=f_res, n_segments=n_segments)
    irs = _device_rows(rows, fs)
    dev = spectrograms(irs, fs, f_res=f_res, n_segments=n_segments)
    assert all(ir._data is None for ir in irs)                   # still on the device
    for k, x in enumerate(rows):
        assert np.array_equal(dev[k][2], host[k][2]), (name, k)
        one = spectrograms([x], fs, f_res=f_res, n_segments=n_segments)[0]
        assert np.array_equal(one[2], host[k][2]), (name, k)
        one = spectrograms([irs[k]], fs, f_res=f_res, n_segments=n_segments)[0]
        assert np.array_equal(one[2], host[k][2]), (name, k)
    # another order, and None entries, change nothing
    mixed = spectrograms([rows[-1], None] + rows[:-1], fs, f_res=f_res, n_segments=n_segments)
    assert mixed[1] is None and np.array_equal(mixed[0][2], host[-1][2]) and np.array_equal(mixed[2][2], host[0][2])


@pytest.mark.gpu
def test_rows_the_reference_draws_nothing_for(gpu_ctx):
    from impulse_hip.plot_data import spectrograms
    fs, _, _, rows = pdi.spec_case("short")
    got = spectrograms([np.zeros(0), rows[0], np.ones(3)], fs)
    assert got[0] is None and got[2] is None and got[1][2].shape == (125, 126)


@pytest.mark.gpu
def test_unsupported_segment_length_raises_value_error(gpu_ctx):
    from impulse_hip.plot_data import spectrogram_geometry, spectrograms
    fs, n, nfft = pdi.UNSUPPORTED
    assert spectrogram_geometry(n, fs)[0] == nfft == 2 * 1009
    with pytest.raises(ValueError, match=str(nfft)):
        spectrograms([pdi.row("sweep", n, 99, fs)], fs)


@pytest.mark.gpu
def test_hrir_spectrograms_equal_the_per_row_calls(gpu_ctx):
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse
    from impulse_hip.plot_data import spectrograms

    class _Est:
        fs = 8000

    fs, f_res, n_segments, rows = pdi.spec_case("fs8000")
    rows = rows + pdi.spec_case("nseg0")[3]
    h = HRIR(_Est())
    keys = [("FL", "left"), ("FL", "right"), ("FR", "left"), ("FR", "right")]
    for (sp, sd), x in zip(keys, rows):
        h.irs.setdefault(sp, {})[sd] = ImpulseResponse(np.zeros(8), fs, recording=x)
    got = h.spectrograms()
    assert list(got) == ["FL", "FR"] and list(got["FL"]) == ["left", "right"]
    for (sp, sd), x in zip(keys, rows):
        f, t, zk = spectrograms([x], fs)[0]
        assert np.array_equal(got[sp][sd][0], f) and np.array_equal(got[sp][sd][1], t) and np.array_equal(got[sp][sd][2], zk)
        one = h.irs[sp][sd].spectrogram_data()
        assert np.array_equal(one[2], zk)
    # the reference's recordings[speaker][side] mapping; a channel without a recording gives None
    mapping = {"FL": {"left": rows[1]}, "FR": {"right": rows[0]}}
    got = h.spectrograms(recordings=mapping, dtype=np.float32)
    assert got["FL"]["right"] is None and got["FR"]["left"] is None
    assert np.array_equal(got["FL"]["left"][2], spectrograms([rows[1]], fs, dtype=np.float32)[0][2])
    assert np.array_equal(got["FR"]["right"][2], spectrograms([rows[0]], fs, dtype=np.float32)[0][2])
    assert ImpulseResponse(np.zeros(8), fs).spectrogram_data() is None


@pytest.mark.gpu
def test_plot_worker_convolutions_as_device_rows(gpu_ctx):
    from impulse_hip.parallel_workers import process_plot_batch, process_plot_worker
    from impulse_hip.plot_data import spectrograms
    fs = 8000
    rng = np.random.default_rng(31)
    sweep = pdi.row("sweep", 4000, 32, fs)
    irs = [rng.standard_normal(600) * np.exp(-np.arange(600) / 80.0) for _ in range(3)]
    tasks = [("FL", "left", irs[0], sweep, fs), ("FL", "right", irs[1], sweep, fs), ("FR", "left", irs[2], sweep, fs)]
    res = process_plot_batch(tasks)
    assert [(sp, sd) for sp, sd, _ in res] == [t[:2] for t in tasks]
    recs = [r for _, _, r in res]
    assert all(r._data is None and len(r) == 4599 for r in recs)
    dev = spectrograms(recs, fs)
    assert all(r._data is None for r in recs)                    # read in place
    host = spectrograms([r.peek() for r in recs], fs)
    for a, b in zip(dev, host):
        assert np.array_equal(a[2], b[2])
    # the same convolution as the per-channel worker's, to K5's fp32 precision
    _, _, want = process_plot_worker(tasks[1])
    assert np.max(np.abs(recs[1].peek() - want)) <= 1e-5 * np.max(np.abs(want))
    with pytest.raises(ValueError):
        process_plot_batch([tasks[0], ("FR", "right", irs[0][:100], sweep, fs)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(pdi.WF_CASES))
def test_waterfalls_against_fixture_and_model(name, golden, gpu_ctx):
    from impulse_hip.impulse_response import ImpulseResponse
    from impulse_hip.plot_data import waterfall_magnitudes, waterfalls
    z = golden("plot_data")
    fs, x = pdi.wf_case(name)
    mag = waterfall_magnitudes([x], fs)[0]
    m_mag, m_z = pm.waterfall(x, fs)
    assert mag.shape == (128, 13)
    e_mag = max(float(np.max(np.abs(mag - z[f"wf/{name}/magnitude"]))), float(np.max(np.abs(mag - m_mag)))) / float(np.max(m_mag))
    t_ms, log10_f, z_db = waterfalls([x], fs)[0]
    assert np.array_equal(t_ms, z[f"wf/{name}/t_ms"]) and np.array_equal(log10_f, z[f"wf/{name}/log10_f"])
    e_z = max(float(np.max(np.abs(z_db - z[f"wf/{name}/z"]))), float(np.max(np.abs(z_db - m_z))))
    print(f"{name}: magnitudes {e_mag:.3e} of the largest, waterfall {e_z:.3e} dB")
    assert e_mag <= TOL_MAGNITUDE and e_z <= TOL_WATERFALL_DB
    # device rows: read in place when long enough, brought over (and left on the device) when they need padding
    ir = _device_rows([x], fs)[0]
    assert np.array_equal(waterfall_magnitudes([ir], fs)[0], mag) and ir._data is None
    assert np.array_equal(ir.waterfall_data()[2], z_db) and ir._data is None
    assert np.array_equal(ImpulseResponse(x, fs).waterfall_data()[2], z_db)


@pytest.mark.gpu
def test_waterfalls_batch_equals_single(gpu_ctx):
    from impulse_hip.plot_data import waterfall_magnitudes
    xs = [pdi.wf_case(name)[1] for name in ("long48k", "short48k")]
    both = waterfall_magnitudes(xs, 48000)
    for x, m in zip(xs, both):
        assert np.array_equal(waterfall_magnitudes([x], 48000)[0], m)


@pytest.mark.gpu
def test_refusals(gpu_ctx):
    from impulse_hip import _native
    x = [np.ones(100)]
    for nfft, hop, fs, mode in ((1, 1, 8000.0, 0), (64, 0, 8000.0, 0), (64, 65, 8000.0, 0), (64, 32, 0.0, 0), (64, 32, 8000.0, 2)):
        with pytest.raises((_native.NativeError, ValueError)):
            gpu_ctx.stft_db(x, nfft, hop, fs, mode)
    with pytest.raises(_native.NativeError) as exc:
        gpu_ctx.stft_db([np.ones(5000)], 2018, 1009, 48000.0)
    assert exc.value.code == _native.IMP_ERR_UNSUPPORTED and "2018" in str(exc.value)
    with pytest.raises(ValueError):
        gpu_ctx.stft_db(x, 64, 32, 8000.0, dtype=np.float16)
    # a row shorter than nfft has no segments; the others are unaffected
    got = gpu_ctx.stft_db([np.ones(10), np.arange(200.0)], 64, 32, 8000.0)
    assert got[0].shape == (32, 0) and got[1].shape == (32, 5)
    assert np.array_equal(got[1], gpu_ctx.stft_db([np.arange(200.0)], 64, 32, 8000.0)[0])
