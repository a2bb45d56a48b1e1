"""The job runners' output="pcm": the BRIR files the reference's flow ends with (core/pipeline.py:865-906), from PCM words the
device quantises and interleaves (imp_slice_pack_pcm, slice_pack_pcm_kernel), against

  * the host codec: audio_io.pcm_quantise / HRIR.write_wav of the same responses - byte for byte, file for file;
  * the same runner's output="hrir" result written by HRIR.write_wav, and (without virtual bass) the staged run_slice
    result's files: byte for byte.

CPU tests cover BrirFrames' files, the TrueHD skips, the refusals and the ABI table; GPU tests the kernel alone, the runners,
the flagged (staged) path, a capacity re-make and run_measurement_dirs(write_brirs=True)."""
import os
import sys
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEVEN_ONE = ["FL", "FR", "FC", "BL", "BR", "SL", "SR"]                         # 7.1 without LFE (never measured)
SEVEN_ONE_FOUR = SEVEN_ONE + ["TFL", "TFR", "TBL", "TBR"]


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def _special_rows(R, n, seed):
    """fp32 rows [R, n] (what the device leaves) with the codec's edge cases among ordinary samples: +-1, beyond +-1, exact
    half-way points at the 2^31 scale (round half to even), fp32 denormals, zeros"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, n)) * 0.3).astype(np.float32)
    special = np.array([1.0, -1.0, 1.5, -1.5, 2.5 / 2 ** 31, 3.5 / 2 ** 31, -2.5 / 2 ** 31, -0.5 / 2 ** 31, 0.5 / 2 ** 31,
                        1e-40, -1e-40, 0.0, 1 - 2 ** -24, 0.99999994, -0.99999994, 2 ** -16 * 1.5, 2 ** -8 * 0.5],
                       dtype=np.float32)
    for r in range(R):
        k = min(n, len(special))
        x[r, (np.arange(k) * 7 + r) % n] = np.roll(special, r)[:k]
    return x


def _host_hrir(speakers, rows, fs):
    """an HRIR whose responses are the given float64 rows on the host (row 2 q + s = speaker q, side s)"""
    from impulse_hip.hrir import HRIR
    from impulse_hip.impulse_response import ImpulseResponse
    h = HRIR(types.SimpleNamespace(fs=fs))
    for q, sp in enumerate(speakers):
        h.irs[sp] = {sd: ImpulseResponse(np.asarray(rows[2 * q + s], dtype=np.float64), fs) for s, sd in enumerate(("left", "right"))}
    return h


def _frames_of(speakers, rows, fs, bits):
    from impulse_hip.audio_io import pcm_quantise
    from impulse_hip.brir_frames import BrirFrames
    from impulse_hip.constants import track_name
    words = pcm_quantise(np.asarray(rows, dtype=np.float64).T, bits).astype(np.int32)
    return BrirFrames(fs, bits, [track_name(sp, sd) for sp in speakers for sd in ("left", "right")], words)


def _orders(speakers):
    """(file name, track order) of every file write_brirs(truehd=True) writes for these speakers"""
    from impulse_hip.brir_frames import TRUEHD_LAYOUTS
    from impulse_hip.constants import HESUVI_TRACK_ORDER, HEXADECAGONAL_TRACK_ORDER, track_name
    out = [("hrir.wav", HEXADECAGONAL_TRACK_ORDER), ("hesuvi.wav", HESUVI_TRACK_ORDER)]
    for name, order, least in TRUEHD_LAYOUTS:
        avail = [ch for ch in order if ch in speakers]
        if len(avail) >= least:
            out.append((f"truehd_{name}_{len(avail)}ch.wav", [track_name(ch, sd) for ch in avail for sd in ("left", "right")]))
    return out


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def assert_files_as_hrir(frames, hrir, tmp, bits, truehd=True):
    """every file frames.write_brirs writes = HRIR.write_wav(path, order, bits) of `hrir`, byte for byte"""
    got_dir, want_dir = os.path.join(tmp, "pcm"), os.path.join(tmp, "hrir")
    os.makedirs(got_dir, exist_ok=True)
    os.makedirs(want_dir, exist_ok=True)
    paths = frames.write_brirs(got_dir, truehd=truehd)
    expected = _orders(list(hrir.irs)) if truehd else _orders(list(hrir.irs))[:2]
    assert [os.path.basename(p) for p in paths] == [nm for nm, _ in expected]
    for (nm, order), p in zip(expected, paths):
        want = os.path.join(want_dir, nm)
        hrir.write_wav(want, track_order=order, bit_depth=bits)
        assert _read(p) == _read(want), nm
    return paths


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [16, 24, 32])
@pytest.mark.parametrize("speakers", [["FL", "FR"], SEVEN_ONE, SEVEN_ONE_FOUR, "13ch"])
def test_brir_frames_files_are_the_host_codec_bytes(tmp_path, bits, speakers):
    """BrirFrames.write_wav / write_brirs from compact frames = HRIR.write_wav of the same responses (the host codec, with
    np.zeros tracks for absent channels), for the hexadecagonal, HESUVI and TrueHD orders and every bit depth"""
    from impulse_hip.audio_io import write_wav
    from impulse_hip.constants import HEXADECAGONAL_TRACK_ORDER, TRUEHD_13CH_ORDER
    if speakers == "13ch":
        speakers = list(TRUEHD_13CH_ORDER)
    fs, n = 48000, 1237
    rows = _special_rows(2 * len(speakers), n, bits + len(speakers)).astype(np.float64)
    fr = _frames_of(speakers, rows, fs, bits)
    assert fr.frames.shape == (n, 2 * len(speakers)) and len(fr) == n
    hrir = _host_hrir(speakers, rows, fs)
    assert_files_as_hrir(fr, hrir, str(tmp_path), bits)
    # the expanded data chunk: the slice's columns where the order names them, zeros (silence) elsewhere
    chunk = fr.data_chunk()
    assert chunk.shape == (n, len(HEXADECAGONAL_TRACK_ORDER)) and chunk.dtype == np.int32
    names = fr.tracks
    for t, name in enumerate(HEXADECAGONAL_TRACK_ORDER):
        if name in names:
            assert np.array_equal(chunk[:, t], fr.frames[:, names.index(name)])
        else:
            assert not chunk[:, t].any()
    # ... and the same bytes as the writer of float rows in the file's order (np.zeros(reference_len) for absent tracks)
    by_name = dict(zip(names, rows))
    a, b = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    write_wav(a, fs, np.vstack([by_name.get(ch, np.zeros(n)) for ch in HEXADECAGONAL_TRACK_ORDER]), bit_depth=bits)
    fr.write_wav(b)
    assert _read(a) == _read(b)


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_fewer_frames_than_tracks_take_the_host_codec(tmp_path, bits):
    """The reference's writer transposes data with fewer frames than tracks (core/audio_io.py:82-97); BrirFrames does not
    assume that cannot happen: the bytes are still HRIR.write_wav's"""
    fs = 48000
    for n in (5, 32):
        rows = _special_rows(4, n, n).astype(np.float64)
        d = tmp_path / f"n{n}"
        d.mkdir()
        assert_files_as_hrir(_frames_of(["FL", "FR"], rows, fs, bits), _host_hrir(["FL", "FR"], rows, fs), str(d), bits,
                             truehd=False)


def test_truehd_layouts_with_too_few_channels_are_skipped(tmp_path):
    """core/pipeline.py:878-906: 7.0.4 needs 8 of its 11 channels, 7.0.6 10 of its 13; a layout below the minimum writes no
    file for it and does not fail; the file names carry the channel count present"""
    fs, n = 48000, 300
    cases = [(["FL", "FR"], []), (SEVEN_ONE, []), (SEVEN_ONE + ["TFL"], ["truehd_11ch_8ch.wav"]),
             (SEVEN_ONE + ["TFL", "TFR", "TSL"], ["truehd_11ch_9ch.wav", "truehd_13ch_10ch.wav"]),
             (SEVEN_ONE_FOUR, ["truehd_11ch_11ch.wav", "truehd_13ch_11ch.wav"])]
    for k, (speakers, truehd) in enumerate(cases):
        d = tmp_path / f"case{k}"
        d.mkdir()
        rows = _special_rows(2 * len(speakers), n, k).astype(np.float64)
        paths = _frames_of(speakers, rows, fs, 32).write_brirs(str(d), truehd=True)
        assert sorted(os.listdir(d)) == sorted(["hrir.wav", "hesuvi.wav"] + truehd)
        assert [os.path.basename(p) for p in paths] == ["hrir.wav", "hesuvi.wav"] + truehd
        e = tmp_path / f"plain{k}"
        e.mkdir()
        _frames_of(speakers, rows, fs, 32).write_brirs(str(e))
        assert sorted(os.listdir(e)) == ["hesuvi.wav", "hrir.wav"]


def test_pcm_output_refusals_come_before_any_device_work():
    """An unknown output, a bad bit_depth and output='pcm' with to_host=False are refused with ValueError in the caller's
    thread - before a runner touches a device (here: before a device error could be raised at all)"""
    from impulse_hip.brir_frames import BrirFrames
    from impulse_hip.pipeline_slice import run_measurement_dirs
    from impulse_hip.resident_slice import SliceFleet, SlicePipeline, SliceRunner, run_slice_jobs
    stub = types.SimpleNamespace(estimator=types.SimpleNamespace(fs=48000))
    for run in (SlicePipeline.run, SliceRunner.run, SliceFleet.run):
        with pytest.raises(ValueError, match="output must be"):
            run(stub, [[None]], {}, output="wav")
        for bad in (8, 20, 64, True, "32"):
            with pytest.raises(ValueError, match="bit_depth"):
                run(stub, [[None]], {}, output="pcm", bit_depth=bad)
        with pytest.raises(ValueError, match="to_host"):
            run(stub, [[None]], {}, output="pcm", to_host=False)
    est = types.SimpleNamespace(fs=48000)
    with pytest.raises(ValueError, match="output must be"):
        run_slice_jobs(est, None, [[None]], {}, output="f64")
    with pytest.raises(ValueError, match="bit_depth"):
        run_slice_jobs(est, None, [[None]], {}, output="pcm", bit_depth=12)
    with pytest.raises(ValueError, match="bit_depth"):
        run_measurement_dirs(est, ["/nonexistent/measurement"], write_brirs=True, bit_depth=20)
    with pytest.raises(ValueError, match="bit_depth"):
        BrirFrames(48000, 20, ["FL-left"], np.zeros((4, 1), dtype=np.int32))
    with pytest.raises(ValueError, match="int32"):
        BrirFrames(48000, 32, ["FL-left", "FL-right"], np.zeros((4, 2)))


def test_abi_table_has_the_pcm_entries():
    import re
    from impulse_hip import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "impulse_hip.h")).read(), flags=re.S)
    lib = _native.load_library()
    for name in ("imp_slice_pack_pcm", "imp_pack_pcm_device"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _native.SIGNATURES and hasattr(lib, name)
    assert callable(_native.Slice.pack_pcm) and callable(_native.Context.pack_pcm_device)


# ---- GPU: the kernel alone ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("R", [2, 3, 16, 26])
def test_pack_pcm_kernel_against_the_host_codec(gpu_ctx, R):
    """slice_pack_pcm_kernel over M measurements of different lengths (odd, shorter than a tile, not multiples of it, one of
    length 0): words = audio_io.pcm_quantise of the same fp32 samples for 16 / 24 / 32 bits; the slot of the empty
    measurement and everything past R * len in each slot are left as they were"""
    from impulse_hip import _native
    from impulse_hip.audio_io import pcm_quantise
    ctx = _native.default_context()
    lens = np.array([1237, 0, 3, 257, 513, 64], dtype=np.int64)
    M, max_len = len(lens), int(lens.max())
    pitch = (max_len + 63) // 64 * 64
    stride = R * max_len + 5
    rows = np.zeros((M, R, pitch), dtype=np.float32)
    for m in range(M):
        rows[m, :, :lens[m]] = _special_rows(R, max(int(lens[m]), 1), 100 * m + R)[:, :lens[m]]
    rows[:, :, max_len:] = np.nan                                        # never read
    d_rows, d_len, d_out = ctx.malloc(rows.nbytes), ctx.malloc(lens.nbytes), ctx.malloc(M * stride * 4)
    try:
        ctx.h2d(d_rows, rows)
        ctx.h2d(d_len, lens)
        sentinel = np.full(M * stride, 0x5A5A5A5A, dtype=np.int32)
        for bits in (16, 24, 32):
            ctx.h2d(d_out, sentinel)
            ctx.pack_pcm_device(d_rows, pitch, d_len, R, M, max_len, bits, d_out, stride)
            got = np.empty(M * stride, dtype=np.int32)
            ctx.d2h(got, d_out)
            for m in range(M):
                n = int(lens[m])
                slot = got[m * stride:(m + 1) * stride]
                want = pcm_quantise(rows[m, :, :n].astype(np.float64).T, bits)
                assert np.array_equal(slot[:R * n].reshape(n, R), want), (R, m, bits)
                assert np.all(slot[R * n:] == 0x5A5A5A5A), (R, m, bits)
        with pytest.raises(_native.NativeError):
            ctx.pack_pcm_device(d_rows, pitch, d_len, R, M, max_len, 20, d_out, stride)
        with pytest.raises(_native.NativeError):
            ctx.pack_pcm_device(d_rows, pitch, d_len, R, M, max_len, 32, d_out, R * max_len - 1)
    finally:
        ctx.synchronize()
        for p in (d_rows, d_len, d_out):
            ctx.free(p)


@pytest.mark.gpu
def test_slice_pack_pcm_on_the_slice_rows_and_on_rows_written_into_d_out():
    """Slice.pack_pcm after a call of M = 3 measurements (three out_len): the words of the finished rows = pcm_quantise of
    what pack_f64 brings over; then with the edge cases written into d_out over every row, the same against the host codec"""
    from test_resident_slice import synth_firs, synth_frames
    from impulse_hip import _native
    from impulse_hip.audio_io import pcm_quantise
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.resident_slice import Layout, ResidentSlice
    fs = 48000
    e = ImpulseResponseEstimator(min_duration=1.0, fs=fs)
    spk = ["FL", "FR", "FC"]
    meas = [[synth_frames(e, spk, 2400 + m, rt60=0.15 + 0.1 * m)] for m in range(3)]
    layout = Layout(e, [(meas[0][0].shape[0], 2, spk)])
    rs = ResidentSlice(e, layout, max_measurements=3)
    rs.set_firs(synth_firs(layout.tasks, rs.taps, 9))
    ctx, R, M = rs.ctx, rs.slice.rows, 3
    d_rec = ctx.malloc(M * layout.samples * 4)
    d_f64 = d_pcm = 0
    try:
        for m in range(M):
            rs.upload(d_rec + m * layout.samples * 4, meas[m])
        block = _quiet(rs.execute_device, d_rec, M)
        rows, res = rs.slice.results()
        if np.any(res["flags"] & _native.SLICE_KEEP_CAP) and rs.grow_for(rows):
            block = _quiet(rs.execute_device, d_rec, M)                    # once more, with room for the longest response
            _, res = rs.slice.results()
        cap, pitch, d_out = rs.slice.out_len_max, rs.out_pitch, block.ptr
        d_f64, d_pcm = ctx.malloc(M * R * cap * 8), ctx.malloc(M * R * cap * 4)
        lens = [int(x) for x in res["out_len"]]
        assert not np.any(res["flags"] & _native.SLICE_REDO), res["flags"]
        assert len(set(lens)) > 1, lens
        rs.slice.pack_f64(d_out, pitch, M, d_f64, R * cap)
        f64 = np.empty(M * R * cap)
        ctx.d2h(f64, d_f64)
        special = np.stack([_special_rows(R, pitch, 7 + m) for m in range(M)]).reshape(M * R, pitch)
        for bits in (32, 24, 16):
            rs.slice.pack_pcm(d_out, pitch, M, bits, d_pcm, R * cap)
            words = np.empty(M * R * cap, dtype=np.int32)
            ctx.d2h(words, d_pcm)
            for m in range(M):
                n = lens[m]
                host = f64[m * R * cap:m * R * cap + R * n].reshape(R, n)
                assert np.array_equal(words[m * R * cap:m * R * cap + R * n].reshape(n, R), pcm_quantise(host.T, bits)), (m, bits)
        ctx.h2d(d_out, special)
        for bits in (32, 24, 16):
            rs.slice.pack_pcm(d_out, pitch, M, bits, d_pcm, R * cap)
            words = np.empty(M * R * cap, dtype=np.int32)
            ctx.d2h(words, d_pcm)
            for m in range(M):
                n = lens[m]
                want = pcm_quantise(special[m * R:(m + 1) * R, :n].astype(np.float64).T, bits)
                assert np.array_equal(words[m * R * cap:m * R * cap + R * n].reshape(n, R), want), (m, bits)
        with pytest.raises(_native.NativeError):
            rs.slice.pack_pcm(d_out, pitch, 2, 32, d_pcm, R * cap)             # M must be the last call's
        with pytest.raises(_native.NativeError):
            rs.slice.pack_pcm(d_out, pitch, M, 8, d_pcm, R * cap)
        with pytest.raises(_native.NativeError):
            rs.slice.pack_pcm(d_out, pitch, M, 32, d_pcm, R * cap - 1)
    finally:
        ctx.synchronize()
        for p in (d_rec, d_f64, d_pcm):
            if p:
                ctx.free(p)
        rs.close()


# ---- GPU: the runners ---------------------------------------------------------------------------------------------------------

CONFIGS = {"plain": (dict(), 32), "align": (dict(align=True), 24), "decay": (dict(decay=0.3), 16),
           "vbass": (dict(align=True, vbass={}), 32)}


def _job(spk, M, seed, seconds=1.0, fs=48000):
    from test_resident_slice import synth_firs, synth_frames
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.resident_slice import Layout, _fir_taps
    e = ImpulseResponseEstimator(min_duration=seconds, fs=fs)
    meas = [[synth_frames(e, spk, seed + m, rt60=0.18 + 0.03 * m)] for m in range(M)]
    layout = Layout(e, [(meas[0][0].shape[0], 2, spk)])
    return e, meas, layout, synth_firs(layout.tasks, _fir_taps(e.fs), seed)


def _staged(e, meas_m, spk, firs, head_ms=1, **kw):
    from impulse_hip.pipeline_slice import run_slice
    return _quiet(run_slice, e, [((e.fs, meas_m[0]), spk)], firs=firs, head_ms=head_ms, **kw)


def assert_pcm_as_hrir(pcm, hrir_res, tmp, bits, tag, staged=None):
    """(BrirFrames, gain) of output='pcm' against (HRIR, gain) of output='hrir': equal gains, byte-identical files"""
    from impulse_hip.brir_frames import BrirFrames
    (fr, g1), (h, g2) = pcm, hrir_res
    assert isinstance(fr, BrirFrames) and fr.bit_depth == bits and fr.frames.dtype == np.int32
    assert g1 == g2, tag
    d = os.path.join(tmp, tag)
    assert_files_as_hrir(fr, h, d, bits)
    if staged is not None:
        assert_files_as_hrir(fr, staged[0], os.path.join(d, "staged"), bits)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_runners_pcm_files_are_the_hrir_files(tmp_path, config):
    """SlicePipeline, SliceRunner and run_slice_jobs with output='pcm': every file write_brirs writes (hrir, hesuvi, the
    7.0.4 TrueHD layout with 8 channels) is byte-identical to HRIR.write_wav of the same runner's output='hrir' result, in
    job order, with equal gains; without virtual bass also to the staged run_slice result's files"""
    from impulse_hip.resident_slice import SlicePipeline, SliceRunner, run_slice_jobs
    kw, bits = CONFIGS[config]
    spk = SEVEN_ONE + ["TFL"]
    e, meas, layout, firs = _job(spk, 3, 4100 + 10 * list(CONFIGS).index(config))
    staged = None if "vbass" in kw else [_staged(e, meas[m], spk, firs, **kw) for m in range(3)]
    pipe = SlicePipeline(e, layout)
    lanes = SliceRunner(e, layout, workers=2)
    try:
        for name, runner in (("pipeline", pipe), ("lanes", lanes)):
            want = _quiet(runner.run, meas, firs, **kw)
            got = _quiet(runner.run, meas, firs, output="pcm", bit_depth=bits, **kw)
            assert len(got) == 3
            for m in range(3):
                assert_pcm_as_hrir(got[m], want[m], str(tmp_path), bits, f"{name}{m}", staged and staged[m])
        times = pipe.times()
        assert times["measurements"] >= 6 and "to_host" in times
    finally:
        pipe.close()
        lanes.close()
    want = _quiet(run_slice_jobs, e, layout, meas, firs, **kw)
    got = _quiet(run_slice_jobs, e, layout, meas, firs, output="pcm", bit_depth=bits, **kw)
    for m in range(3):
        assert_pcm_as_hrir(got[m], want[m], str(tmp_path), bits, f"jobs{m}", staged and staged[m])


@pytest.mark.gpu
def test_full_size_c2_pcm_files(tmp_path):
    """BASELINE C2 (7.1 layout x 2 ears, 6.15 s sweep at 48 kHz) with the alignments on, through SlicePipeline: the PCM
    files are the HRIR files and the staged path's, and the words per measurement are half the float64 bytes"""
    from impulse_hip.resident_slice import SlicePipeline
    spk = ["FL", "FR", "FC", "BL", "BR", "SL", "SR", "WL"]
    e, meas, layout, firs = _job(spk, 3, 0xC2, seconds=5.0)
    pipe = SlicePipeline(e, layout)
    try:
        want = _quiet(pipe.run, meas, firs, align=True)
        got = _quiet(pipe.run, meas, firs, align=True, output="pcm")
        for m in range(3):
            assert got[m][0].frames.nbytes * 2 == sum(ir.data.nbytes for pair in want[m][0].irs.values() for ir in pair.values())
            assert_pcm_as_hrir(got[m], want[m], str(tmp_path), 32, f"c2_{m}", _staged(e, meas[m], spk, firs, align=True))
    finally:
        pipe.close()


@pytest.mark.gpu
def test_pcm_files_at_44k1(tmp_path):
    """run_slice_jobs with output='pcm' at 44.1 kHz with the alignments on (30 ms segments of 1323 samples): the files are
    HRIR.write_wav's of the same runner's output='hrir' result and of the staged run_slice result, byte for byte"""
    from impulse_hip.resident_slice import run_slice_jobs
    spk = ["FL", "FR", "FC", "SL", "SR"]
    e, meas, layout, firs = _job(spk, 2, 4410, fs=44100)
    want = _quiet(run_slice_jobs, e, layout, meas, firs, align=True)
    got = _quiet(run_slice_jobs, e, layout, meas, firs, output="pcm", bit_depth=24, align=True)
    for m in range(2):
        assert got[m][0].fs == 44100
        assert_pcm_as_hrir(got[m], want[m], str(tmp_path), 24, f"fs44100_{m}", _staged(e, meas[m], spk, firs, align=True))


@pytest.mark.gpu
def test_flagged_measurements_give_the_same_bytes(tmp_path):
    """A measurement the device flags (IMP_SLICE_ALIGN_GUARD: head_ms = 0, alignments on - as
    test_resident_slice.test_alignment_guard_flags_take_the_staged_path builds it) takes the staged path in PCM mode too: its
    BrirFrames are the host codec's words of the staged rows, in the same column order - the files cannot tell"""
    from test_resident_slice import synth_frames
    from impulse_hip.resident_slice import SlicePipeline, SliceRunner
    spk = ["FL", "FR", "SL", "SR"]
    e, _, layout, firs = _job(spk, 1, 3)
    meas = [[synth_frames(e, spk, 1300 + m)] for m in range(2)]
    for cls, kw in ((SlicePipeline, {}), (SliceRunner, dict(workers=1))):
        runner = cls(e, layout, head_ms=0, **kw)
        try:
            want = _quiet(runner.run, meas, firs, align=True)
            rs = runner.rs if cls is SlicePipeline else runner.lanes[0]["rs"]
            staged_before = rs.stats["staged"]
            got = _quiet(runner.run, meas, firs, align=True, output="pcm", bit_depth=24)
            assert rs.stats["staged"] - staged_before == 2, rs.stats
            for m in range(2):
                assert_pcm_as_hrir(got[m], want[m], str(tmp_path), 24, f"{cls.__name__}{m}",
                                   _staged(e, meas[m], spk, firs, head_ms=0, align=True))
        finally:
            runner.close()


@pytest.mark.gpu
def test_capacity_growth_in_pcm_mode(tmp_path):
    """A job whose knees ask for more than the slice was sized for re-makes the slice and the hand-over ring in mid-job in PCM
    mode: the same bytes as a runner made large enough from the start"""
    from test_resident_slice import synth_frames
    from impulse_hip.resident_slice import SlicePipeline
    spk = ["FL", "FR"]
    e, _, layout, firs = _job(spk, 1, 700)
    rt = [0.18, 0.75, 0.2, 0.22]
    meas = [[synth_frames(e, spk, 700 + m, rt60=rt[m], noise_db=-100.0 if rt[m] > 0.5 else -85.0)] for m in range(4)]
    small, large = SlicePipeline(e, layout, keep_cap=4000), SlicePipeline(e, layout)
    try:
        got = _quiet(small.run, meas, firs, output="pcm")
        assert small.rs.stats["regrown"] >= 1, small.rs.stats
        want = _quiet(large.run, meas, firs, output="pcm")
        ref = _quiet(large.run, meas, firs)
        assert len({len(g[0]) for g in got}) > 1
        for m in range(4):
            assert got[m][1] == want[m][1] and np.array_equal(got[m][0].frames, want[m][0].frames)
            assert_pcm_as_hrir(got[m], ref[m], str(tmp_path), 32, f"grow{m}")
    finally:
        small.close()
        large.close()


@pytest.mark.gpu
def test_run_measurement_dirs_writes_the_brirs(tmp_path):
    """run_measurement_dirs(write_brirs=True) over two measurement directories: each receives hrir.wav and hesuvi.wav
    byte-identical to HRIR.write_wav of that directory's run_measurement_dirs(...) result; without it nothing is written"""
    from test_resident_slice import synth_frames
    from impulse_hip.audio_io import write_wav_frames
    from impulse_hip.brir_frames import BrirFrames
    from impulse_hip.constants import HESUVI_TRACK_ORDER
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from impulse_hip.pipeline_slice import run_measurement_dirs
    fs = 48000
    e = ImpulseResponseEstimator(min_duration=1.0, fs=fs)
    dirs = []
    for m in range(2):
        d = tmp_path / f"measurement{m}"
        d.mkdir()
        write_wav_frames(str(d / "FL,FR.wav"), fs, synth_frames(e, ["FL", "FR"], 5100 + m), 32)
        write_wav_frames(str(d / "FC.wav"), fs, synth_frames(e, ["FC"], 5150 + m), 32)
        dirs.append(str(d))
    whole = _quiet(run_measurement_dirs, e, dirs, decay={"FC": 0.4})
    for d in dirs:
        assert sorted(os.listdir(d)) == ["FC.wav", "FL,FR.wav"]
    out = _quiet(run_measurement_dirs, e, dirs, decay={"FC": 0.4}, write_brirs=True, truehd=True)
    assert len(out) == 2
    for m, d in enumerate(dirs):
        fr, g = out[m]
        assert isinstance(fr, BrirFrames) and g == whole[m][1]
        assert sorted(os.listdir(d)) == ["FC.wav", "FL,FR.wav", "hesuvi.wav", "hrir.wav"]       # too few channels for TrueHD
        for name, order in (("hrir.wav", None), ("hesuvi.wav", HESUVI_TRACK_ORDER)):
            want = str(tmp_path / f"want{m}_{name}")
            whole[m][0].write_wav(want, track_order=order)
            assert _read(os.path.join(d, name)) == _read(want), (m, name)
    again = _quiet(run_measurement_dirs, e, dirs, decay={"FC": 0.4}, write_brirs=True, bit_depth=16)      # the files are not recordings
    for m, d in enumerate(dirs):
        want = str(tmp_path / f"want16_{m}.wav")
        whole[m][0].write_wav(want, bit_depth=16)
        assert again[m][0].bit_depth == 16 and _read(os.path.join(d, "hrir.wav")) == _read(want)
