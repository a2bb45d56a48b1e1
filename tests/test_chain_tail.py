"""The chain's K5 as blocks of 16 384 samples (fir_block_kernel<2>: two four-step rows, 512 threads, 68 KiB of LDS) for
FIRs of up to 12 289 taps, the FIR plan's 32 768-sample blocks (fir_block_kernel<4>) beyond.  Against the oracle as
tests/test_hip_parity.py checks the chain (same tolerance), against the forced 4-row tail (IMPULSE_HIP_CHAIN_K5=block4),
and with several chains in flight."""
import numpy as np
import pytest

TIME_TOL = 1e-6            # max |dy| / max |y|, as tests/test_hip_parity.py
TAIL2_MAX_TAPS = 12289     # history 12 288 = 16 384 - 4 096


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))


def test_chain_tail_geometry_needs_no_gpu():
    from impulse_hip._native import chain_tail_geometry
    # the everyday job: 0.68 s response (*) 9 600-tap FIR at 48 kHz, 42 239 outputs: 6 784 per block, seven blocks
    assert chain_tail_geometry(9600, 32640) == (9600, 6784, 7)
    assert chain_tail_geometry(1, 32640) == (0, 16384, 2)
    assert chain_tail_geometry(4097, 32640) == (4096, 12288, 3)
    assert chain_tail_geometry(TAIL2_MAX_TAPS, 32640) == (12288, 4096, 11)
    assert chain_tail_geometry(TAIL2_MAX_TAPS + 1, 32640) is None
    assert chain_tail_geometry(19200, 65280) is None                           # C3 at 96 kHz: the 4-row tail


def _recording(e, rng, B, L):
    N = len(e)
    rec = np.zeros((B, L), dtype=np.float32)
    delays = [100, 777, 0, 60000, 155000][:B]                  # channel 2 stays silent; channel 4 peaks near the end
    for c, d in enumerate(delays):
        if c != 2:
            rec[c, d:d + N] += (0.5 * e.test_signal).astype(np.float32)[: L - d]
            rec[c, d + 300:d + 300 + N] += (0.1 * e.test_signal).astype(np.float32)[: L - d - 300]
    rec[B - 1] += (rng.standard_normal(L) * 1e-4).astype(np.float32)
    return rec, delays


def _firs(rng, B, K):
    return rng.standard_normal((B, K)) * np.exp(-np.arange(K) / max(K / 10.0, 1.0))


def _run(ctx, chain, d_x, L, d_out, d_pk, B, po):
    chain.execute_device(d_x, L, d_out, po, d_pk)
    ctx.synchronize()
    y, pk = np.empty((B, po), dtype=np.float32), np.empty(B, dtype=np.int64)
    ctx.d2h(y, d_out)
    ctx.d2h(pk, d_pk)
    return y, pk


@pytest.mark.gpu
@pytest.mark.parametrize("n,K", [(32640, 1), (32640, 4097), (32640, 9600), (32640, TAIL2_MAX_TAPS),
                                 (32640, TAIL2_MAX_TAPS + 1), (65280, 1), (65280, 9600), (65280, TAIL2_MAX_TAPS),
                                 (65280, TAIL2_MAX_TAPS + 1), (65280, 19200)])
def test_chain_tail_against_oracle(gpu_ctx, n, K):
    """Silent channel, a crop clamped at the row's end, a refill of the FIRs between calls; the 2-row tail where the
    filter fits, the 4-row one past it."""
    from impulse_hip import ConvPlan
    from impulse_hip._native import FirChain
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from oracle.estimator import estimate
    from oracle.impulse_response import peak_index
    from oracle.scipy_restated import fft_convolve, hann
    e = ImpulseResponseEstimator(min_duration=1.0, fs=48000)
    N, fs, head, fade, B = len(e), 48000, 48, 400, 5
    L = N + 2 * fs
    rng = np.random.default_rng(K)
    rec, delays = _recording(e, rng, B, L)
    firs = _firs(rng, B, K)
    plan1 = ConvPlan(gpu_ctx, np.asarray(e.inverse_filter), L, "same", ws_channels=B)
    plan5 = ConvPlan(gpu_ctx, firs, n, "full", ws_channels=B)
    chain = FirChain(plan1, plan5, B, head, head, fade)
    po = n + K - 1 + 3
    d_x, d_out, d_pk = gpu_ctx.malloc(rec.nbytes), gpu_ctx.malloc(B * po * 4), gpu_ctx.malloc(B * 8)
    gpu_ctx.h2d(d_x, rec)
    w = np.ones(n)
    w[:head] *= hann(2 * head)[:head]
    w[n - fade:] *= hann(2 * fade)[fade:]
    irs = [estimate(rec[c].astype(np.float64), e.inverse_filter) for c in range(B)]
    try:
        assert chain.tail_rows() == (2 if K <= TAIL2_MAX_TAPS else 4)
        for taps in (firs, firs[::-1].copy()):
            plan5.set_filters(taps)
            assert chain.tail_rows() == (2 if K <= TAIL2_MAX_TAPS else 4)
            y, pk = _run(gpu_ctx, chain, d_x, L, d_out, d_pk, B, po)
            for c in range(B):
                want_pk = peak_index(irs[c])
                assert int(pk[c]) == want_pk
                s0 = min(max(want_pk - head, 0), L - n)
                ref = fft_convolve(irs[c][s0:s0 + n] * w, taps[c], "full")
                if c == 2:
                    assert not np.any(y[c, :n + K - 1])
                else:
                    assert rel(y[c, :n + K - 1], ref) <= TIME_TOL
        assert delays[4] + N // 2 - head > L - n                  # the clamp was exercised
    finally:
        chain.close()
        plan1.close()
        plan5.close()
        for p in (d_x, d_out, d_pk):
            gpu_ctx.free(p)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [9600, TAIL2_MAX_TAPS])
def test_chain_tail_matches_forced_4row_tail(gpu_ctx, monkeypatch, K):
    """The 2-row tail equals the 4-row one (IMPULSE_HIP_CHAIN_K5=block4) within TIME_TOL, peaks exactly, and is
    bit-identical across reruns."""
    from impulse_hip import ConvPlan
    from impulse_hip._native import FirChain
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    e = ImpulseResponseEstimator(min_duration=1.0, fs=48000)
    N, fs, n, head, fade, B = len(e), 48000, 32640, 48, 200, 5
    L = N + 2 * fs
    rng = np.random.default_rng(3)
    rec, _ = _recording(e, rng, B, L)
    firs = _firs(rng, B, K)
    plan1 = ConvPlan(gpu_ctx, np.asarray(e.inverse_filter), L, "same", ws_channels=B)
    plan5 = ConvPlan(gpu_ctx, firs, n, "full", ws_channels=B)
    chain2 = FirChain(plan1, plan5, B, head, head, fade)
    monkeypatch.setenv("IMPULSE_HIP_CHAIN_K5", "block4")
    chain4 = FirChain(plan1, plan5, B, head, head, fade)
    monkeypatch.delenv("IMPULSE_HIP_CHAIN_K5")
    po = n + K - 1
    d_x, d_out, d_pk = gpu_ctx.malloc(rec.nbytes), gpu_ctx.malloc(B * po * 4), gpu_ctx.malloc(B * 8)
    gpu_ctx.h2d(d_x, rec)
    try:
        assert chain2.tail_rows() == 2 and chain4.tail_rows() == 4
        y4, pk4 = _run(gpu_ctx, chain4, d_x, L, d_out, d_pk, B, po)
        y2, pk2 = _run(gpu_ctx, chain2, d_x, L, d_out, d_pk, B, po)
        y2b, pk2b = _run(gpu_ctx, chain2, d_x, L, d_out, d_pk, B, po)
        assert np.array_equal(pk2, pk4) and np.array_equal(pk2, pk2b)
        assert np.array_equal(y2, y2b)
        for c in range(B):
            if c == 2:
                assert not np.any(y2[c]) and not np.any(y4[c])
            else:
                assert rel(y2[c], y4[c].astype(np.float64)) <= TIME_TOL
    finally:
        chain2.close()
        chain4.close()
        plan1.close()
        plan5.close()
        for p in (d_x, d_out, d_pk):
            gpu_ctx.free(p)


@pytest.mark.gpu
def test_chain_tail_with_lanes_and_tail_stream():
    """The 2-row tail on a tail context of its own behind a deconvolution plan on two lanes, seven calls in flight with
    distinct inputs and outputs, every one against the oracle."""
    from impulse_hip import Context, ConvPlan
    from impulse_hip._native import FirChain
    from impulse_hip.impulse_response_estimator import ImpulseResponseEstimator
    from oracle.estimator import estimate
    from oracle.impulse_response import peak_index
    from oracle.scipy_restated import fft_convolve, hann
    e = ImpulseResponseEstimator(min_duration=1.0, fs=48000)
    N, fs = len(e), 48000
    L, n, K, head, fade, B, calls = N + 2 * fs, 32640, 9600, 48, 400, 4, 7
    rng = np.random.default_rng(78)
    firs = _firs(rng, B, K)
    main, tail = Context(0), Context(0)
    plan1 = ConvPlan(main, np.asarray(e.inverse_filter), L, "same", ws_channels=2 * B, fused=False)
    plan1.set_overlap(2)
    plan5 = ConvPlan(tail, firs, n, "full", ws_channels=B)
    chain = FirChain(plan1, plan5, B, head, head, fade)
    po = n + K - 1 + 1
    recs, bufs = [], []
    for j in range(calls):
        rec = (rng.standard_normal((B, L)) * 1e-4).astype(np.float32)
        for c in range(B):
            d = 50 + 211 * j + 37 * c
            rec[c, d:d + N] += (0.5 * e.test_signal).astype(np.float32)
        d_x, d_out, d_pk = main.malloc(rec.nbytes), main.malloc(B * po * 4), main.malloc(B * 8)
        main.h2d(d_x, rec)
        recs.append(rec)
        bufs.append((d_x, d_out, d_pk))
    w = np.ones(n)
    w[:head] *= hann(2 * head)[:head]
    w[n - fade:] *= hann(2 * fade)[fade:]
    try:
        assert chain.tail_rows() == 2
        for d_x, d_out, d_pk in bufs:                               # all in flight: nothing waits between the calls
            chain.execute_device(d_x, L, d_out, po, d_pk)
        main.synchronize()
        tail.synchronize()
        for j, (d_x, d_out, d_pk) in enumerate(bufs):
            y, pk = np.empty((B, po), dtype=np.float32), np.empty(B, dtype=np.int64)
            main.d2h(y, d_out)
            main.d2h(pk, d_pk)
            for c in range(B):
                ir = estimate(recs[j][c].astype(np.float64), e.inverse_filter)
                want_pk = peak_index(ir)
                assert int(pk[c]) == want_pk == N // 2 + 50 + 211 * j + 37 * c
                s0 = min(max(want_pk - head, 0), L - n)
                assert rel(y[c, :n + K - 1], fft_convolve(ir[s0:s0 + n] * w, firs[c], "full")) <= TIME_TOL
    finally:
        chain.close()
        plan1.close()
        plan5.close()
        tail.close()
        main.close()
