"""K10, the lag search (xcorr_argmax_kernel): the dynamic LDS its launch requests against what the kernel indexes (CPU,
every residue of the two lengths mod 4 and the 16 384-sample edge), and a shape sweep on the device in which each pair is
launched ALONE, so that no longer pair of a batch pads the request, against scipy.signal.correlate in fp64.

The kernel keeps a in four padded planes of (na + 523) / 4 + 1 slots each and b behind them: the doubles it needs are not
a function of na + nb, and a request sized from the sum alone falls up to 3 doubles short.  The missing doubles are the
last samples of b; an LDS access past the allocation neither faults nor returns the data, so the inputs of the sweep put
the largest sample of b in its last three and the argmax moves if one of them is lost."""
import numpy as np
import pytest

MAX_SAMPLES = 16384                       # a_len + b_len of one pair
LDS_BYTES = 160 * 1024                    # per workgroup on gfx950
STATIC_LDS_BYTES = 256 * (8 + 4)          # the block reduction's rv / rk
LDS_CAP_DOUBLES = 16911                   # the size the kernel is opted in to: (1, 16383) needs the most


def _sizing_pairs():
    """every pair up to 260 + 260 (all 16 residue pairs mod 4, many times over), every split of 16 384 and of 16 383,
    the resident slice's (segment, segment) for 22.05 - 192 kHz and a strided sample of the rest"""
    pairs = set()
    for na in range(1, 261):
        for nb in range(1, 261):
            pairs.add((na, nb))
    for s in (MAX_SAMPLES, MAX_SAMPLES - 1):
        for na in range(1, s):
            pairs.add((na, s - na))
    for fs in (22050, 44100, 48000, 88200, 96000, 176400, 192000):
        seg = fs * 30 // 1000
        pairs.add((seg, seg))
    for na in range(1, MAX_SAMPLES, 61):
        for nb in range(1 + na % 4, MAX_SAMPLES - na + 1, 97):
            pairs.add((na, nb))
    return sorted(pairs)


def test_k10_launch_requests_the_lds_the_kernel_indexes():
    """imp_debug_xcorr_lds for a call whose only pair is (na, nb): requested >= needed, and needed within the opt-in cap
    (the hook fails where the request would exceed it).  The cap plus the static LDS fits one workgroup's 160 KB."""
    from impulse_hip import _native
    pairs = _sizing_pairs()
    assert {(a % 4, b % 4) for a, b in pairs} == {(i, j) for i in range(4) for j in range(4)}
    short = []
    most = 0
    for na, nb in pairs:
        req, need = _native.xcorr_lds(na, nb)
        assert need == 4 * ((na + 523) // 4 + 1) + nb         # the kernel's layout: a's four padded planes, then b
        if req < need:
            short.append((na, nb, req, need))
        most = max(most, need)
    assert not short, f"{len(short)} pairs short, e.g. {short[:4]}"
    assert most == LDS_CAP_DOUBLES
    assert LDS_CAP_DOUBLES * 8 + STATIC_LDS_BYTES <= LDS_BYTES
    # the cases that fell short when the request was sized from na + nb
    for na, nb in ((26, 26), (661, 661), (2646, 2646), (1, 16383)):
        req, need = _native.xcorr_lds(na, nb)
        assert req >= need, (na, nb, req, need)
    # the lag search refuses what it cannot hold, with the reason
    for na, nb, word in ((0, 5, "empty"), (5, 0, "empty"), (8192, 8193, "16384")):
        with pytest.raises(_native.NativeError, match=word):
            _native.xcorr_lds(na, nb)


def _sweep_shapes():
    shapes = [(n, n) for n in range(1, 601)]
    shapes += [(n, n) for n in (661, 1323, 2646, 5292)]                 # 30 ms at 22.05, 44.1, 88.2, 176.4 kHz
    for base in (40, 1000, 8000):                                         # short, medium, long: all 16 residue pairs
        shapes += [(base + ra, base + 16 + rb) for ra in range(4) for rb in range(4)]
    shapes += [(1, 16383), (16383, 1), (8191, 8193), (8192, 8192)]      # the LDS edges
    return shapes


def _pair(rng, na, nb):
    """a: one unit spike over -60 dB noise; b: spikes of 0.8, 0.9 and 1.0 as its last three samples, one of 0.5 before
    them, noise.  The true maximum pairs the two unit spikes; if b's last sample, or its last two or three, read back as
    0 it moves to another of b's spikes (for every shape here but (1, 1), whose single lag cannot move)."""
    a = rng.standard_normal(na) * 1e-3
    b = rng.standard_normal(nb) * 1e-3
    a[int(rng.integers(0, na))] = 1.0
    b[-3:] = (0.8, 0.9, 1.0)[-min(nb, 3):]
    if nb > 3:
        b[int(rng.integers(0, nb - 3))] = 0.5
    return a, b


@pytest.mark.gpu
def test_k10_shape_sweep_one_pair_per_launch(gpu_ctx):
    """Every shape of _sweep_shapes (600 equal pairs 1..600, the 30 ms segments 661 / 1323 / 2646 / 5292, 48 unequal pairs
    covering all residues mod 4 at ~40, ~1000 and ~8000 samples, the LDS edges (1, 16383), (16383, 1), (8191, 8193),
    (8192, 8192)): 656 pairs, each launched on its own through imp_xcorr_argmax (fp64 host rows) and imp_xcorr_argmax_device
    (the fp32 rows on the device) - 1312 calls.  The argmax is scipy's exactly (first maximum), the value within 1e-12 of
    the largest |corr|."""
    from scipy import signal
    rng = np.random.default_rng(1010)
    shapes = _sweep_shapes()
    assert len(shapes) == 656
    rows = [_pair(rng, na, nb) for na, nb in shapes]
    # the fp32 copies of every pair in one device buffer; the host path gets their float64 values, so both searches see
    # the same numbers and so does the reference
    rows = [(a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)) for a, b in rows]
    flat = np.concatenate([np.concatenate((a, b)) for a, b in rows]).astype(np.float32)
    d_rows = gpu_ctx.malloc(flat.nbytes)
    try:
        gpu_ctx.h2d(d_rows, flat)
        at = 0
        bad = []
        for (na, nb), (a, b) in zip(shapes, rows):
            corr = signal.correlate(a, b, mode="full", method="direct")
            want_k, tol = int(np.argmax(corr)), 1e-12 * max(1.0, float(np.abs(corr).max()))
            k_h, v_h = gpu_ctx.xcorr_argmax([a], [b])
            k_d, v_d = gpu_ctx.xcorr_argmax_device(d_rows, [at], [na], [at + na], [nb])
            at += na + nb
            for path, k, v in (("host", k_h[0], v_h[0]), ("device", k_d[0], v_d[0])):
                if int(k) != want_k or abs(v - corr[want_k]) > tol:
                    bad.append((path, na, nb, int(k), want_k, float(v), float(corr[want_k])))
        assert not bad, f"{len(bad)} wrong: {bad[:6]}"
    finally:
        gpu_ctx.free(d_rows)
