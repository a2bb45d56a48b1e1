"""Generate tests/golden/plot_data.npz by RUNNING the reference's ImpulseResponsePlotter.plot_spectrogram and
plot_waterfall (core/plotting/impulse_response_plotter.py) on the seeded inputs of tests/golden/plot_data_inputs.py:

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_plot_data_goldens.py /path/to/reference

The methods run on a bare object that carries data, fs and recording, with matplotlib's Agg backend, and the arrays are
read back from what was drawn: the QuadMesh pcolormesh made (its coordinates give t and f, its array z) and the arguments
of a wrapped plot_surface.  Modules the reference imports but that are not installed are replaced by inert stand-ins.
The (nperseg, noverlap) the reference hands to scipy.signal.spectrogram and the f and t it gets back are recorded by a
wrapper around that name in the plotter's module.
Data only: per spectrogram row its shape, (nfft, noverlap), f, t and every plot_data_inputs.SPEC_DECIM-th column of z plus
the first and the last; the waterfalls whole, with the short-time magnitudes they were made from.
"""
import os
import sys
import types

import matplotlib
matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)

import plot_data_inputs as pdi  # noqa: E402


CALLS = []          # (nperseg, noverlap, f, t, spectrum) of every scipy.signal.spectrogram call the reference made


def load_plotter(root):
    class _Any(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return lambda *a, **k: None

    for name in ("soundfile", "nnresample", "seaborn", "bokeh", "bokeh.plotting", "bokeh.models", "bokeh.palettes", "bokeh.layouts"):
        if name not in sys.modules:
            m = _Any(name)
            m.__path__ = []
            sys.modules[name] = m
    sys.path.insert(0, root)
    import core.plotting.impulse_response_plotter as mod
    inner = mod.spectrogram

    def recording_spectrogram(x, **kw):
        f, t, s = inner(x, **kw)
        CALLS.append((int(kw["nperseg"]), int(kw["noverlap"]), np.array(f), np.array(t), np.array(s)))
        return f, t, s

    mod.spectrogram = recording_spectrogram
    return mod.ImpulseResponsePlotter


def drawn_spectrogram(Plotter, x, fs, f_res, n_segments):
    """(f, t, z) read back from the QuadMesh, or None when nothing was drawn"""
    obj = Plotter.__new__(Plotter)
    obj.data, obj.fs, obj.recording = np.zeros(1), fs, x
    fig, ax = plt.subplots()
    obj.plot_spectrogram(fig=fig, ax=ax, f_res=f_res, n_segments=n_segments)
    meshes = [c for c in ax.collections if type(c).__name__ == "QuadMesh"]
    res = None
    if meshes:
        mesh = meshes[0]
        z = np.asarray(mesh.get_array(), dtype=np.float64)
        rows, cols = z.shape
        coords = np.asarray(mesh.get_coordinates(), dtype=np.float64)      # [rows + 1, cols + 1, 2] cell corners
        assert coords.shape == (rows + 1, cols + 1, 2), coords.shape
        res = (rows, cols, z)
    plt.close(fig)
    return res


def drawn_waterfall(Plotter, x, fs):
    obj = Plotter.__new__(Plotter)
    obj.data, obj.fs, obj.recording = x, fs, None
    fig = plt.figure()
    ax = fig.add_subplot(111, projection="3d")
    seen = []
    inner = ax.plot_surface
    ax.plot_surface = lambda t, f, z, **k: (seen.append((np.array(t), np.array(f), np.array(z))), inner(t, f, z, **k))[1]
    obj.plot_waterfall(fig=fig, ax=ax)
    plt.close(fig)
    assert len(seen) == 1
    return seen[0]


def main():
    Plotter = load_plotter(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IMPULCIFER_REFERENCE", "."))
    out = {}
    for name in pdi.SPEC_CASES:
        fs, f_res, n_segments, rows = pdi.spec_case(name)
        for k, x in enumerate(rows):
            res = drawn_spectrogram(Plotter, x, fs, f_res, n_segments)
            assert res is not None, (name, k)
            bins, S, z = res
            p = f"spec/{name}/{k}/"
            out[p + "shape"] = np.array([bins, S], dtype=np.int64)
            nfft, noverlap, f, t, _ = CALLS[-1]
            out[p + "geometry"] = np.array([nfft, noverlap], dtype=np.int64)
            out[p + "f"], out[p + "t"] = f[1:], t
            out[p + "cols"] = pdi.kept_columns(S)
            out[p + "z"] = z[:, out[p + "cols"]]
            print(name, k, len(x), "z", z.shape, "range %.3f .. %.3f" % (z.min(), z.max()))
    fs, n, _ = pdi.UNSUPPORTED
    res = drawn_spectrogram(Plotter, pdi.row("sweep", n, 99, fs), fs, 10, 200)
    out["unsupported/shape"] = np.array(res[:2], dtype=np.int64)       # the reference itself draws this one
    out["unsupported/geometry"] = np.array(CALLS[-1][:2], dtype=np.int64)
    for name in pdi.WF_CASES:
        fs, x = pdi.wf_case(name)
        t, f, z = drawn_waterfall(Plotter, x, fs)
        out[f"wf/{name}/t_ms"], out[f"wf/{name}/log10_f"], out[f"wf/{name}/z"] = t, f, z
        assert CALLS[-1][:2] == (256, 128)
        out[f"wf/{name}/magnitude"] = CALLS[-1][4][1:]                  # what scipy returned to the reference, bin 0 dropped
        print(name, len(x), "z", z.shape, "range %.3f .. %.3f" % (z.min(), z.max()))
    path = os.path.join(OUT, "plot_data.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
