// K6 - batched minimum-phase FIR design on the GPU, in fp64.
//
// Replaces, for B channels at once, the tail of FrequencyResponse.minimum_phase_impulse_response
// (reference autoeq/frequency_response.py:676-680):
//     ir = scipy.signal.firwin2(2n, f, gain, fs=fs)          # f = linspace(0, fs//2, n)
//     ir = scipy.signal.minimum_phase(ir, n_fft=len(ir))     # homomorphic, half=True  -> n taps
// as called per channel by core/parallel_workers.py:129 (n = 9 600 @48 kHz, 19 200 @96 kHz).
//
// firwin2 : fx = interp(linspace(0, nyq, 1 + 2^ceil(log2 2n)), f, gain) ; irfft(fx * linear-phase
//           shift)[:2n] * hamming(2n)
// minimum_phase : |FFT_2n| -> + 1e-7 min>0 -> 0.5 log -> IFFT -> causal cepstral window -> FFT -> exp
//           -> IFFT -> real[:n]
//
// Why fp64: the design forces a zero at Nyquist, so |H| there is rounding noise (1e-12) that the log
// turns into a -27 spike; SciPy's own result moves by 5e-9 of the FIR peak for a 1-ulp change of the
// input (tests/test_oracle_golden.py).  In fp32 that bin would be 1e-7 noise and the taps would move
// by ~1e-4.  The work is tiny (4 transforms of 19 200/38 400 points + one of 2^16/2^17 per channel):
// the batched fp64 transform of fft64_host.hip.h, whose load hooks carry the elementwise steps between
// the transforms, ping-ponging two global buffers, and a few elementwise kernels.
// Also here: imp_debug_fft64, the test hook of that transform.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>

#include "fft64_host.hip.h"

namespace {

// firwin2 front: fx = np.interp(x_i, f, gain) on the two uniform grids, times the linear-phase
// shift, extended to the Hermitian spectrum of length nirf = 2 (nfreqs - 1) for a complex IFFT.
__global__ __launch_bounds__(256) void firwin2_spectrum(const double* __restrict__ gain, cdbl* __restrict__ spec,
                                                        int n, int nfreqs, double nyq_f /* fs//2 grid end */,
                                                        double nyq /* fs/2 */, int numtaps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nfreqs) return;
  const double* g = gain + (long long)blockIdx.y * n;
  cdbl* out = spec + (long long)blockIdx.y * (2 * (nfreqs - 1));
  // np.linspace(0, stop, num): arange(num) * (stop / (num - 1)), last element forced to stop
  const double step_x = nyq / (double)(nfreqs - 1);
  const double step_f = nyq_f / (double)(n - 1);
  const double xi = (i == nfreqs - 1) ? nyq : (double)i * step_x;
  // np.interp: j = last index with f[j] <= x ; f[j] = j * step_f (f[n-1] = nyq_f)
  double val;
  if (xi >= nyq_f) {
    val = g[n - 1];
  } else {
    int j = (int)(xi / step_f);
    if (j > n - 2) j = n - 2;
    auto fj = [&](int jj) { return (jj == n - 1) ? nyq_f : (double)jj * step_f; };
    while (j > 0 && fj(j) > xi) --j;
    while (j < n - 2 && fj(j + 1) <= xi) ++j;
    const double slope = (g[j + 1] - g[j]) / (fj(j + 1) - fj(j));
    val = slope * (xi - fj(j)) + g[j];
  }
  // shift = exp(-(numtaps - 1)/2 * 1j * pi * x / nyq).  NumPy divides a complex array by a real
  // scalar as a multiplication by the reciprocal (scl = 1/nyq), so the phase is (c pi x) * (1/nyq);
  // a true division differs by 1 ulp of a ~3e4 rad angle (3.6e-12) in ~20 % of the bins, which is
  // enough to move the taps' alternating sum (= |H| at the forced Nyquist zero, 1e-11) by 25 %.
  const double scl = 1.0 / nyq;
  const double ang = (-((double)(numtaps - 1) / 2.0) * M_PI * xi) * scl;
  double sn, cs;
  sincos(ang, &sn, &cs);
  const cdbl v = make_double2(val * cs, val * sn);
  const int nirf = 2 * (nfreqs - 1);
  // irfft ignores the imaginary parts of the DC and Nyquist bins
  if (i == 0 || i == nfreqs - 1) {
    out[i] = make_double2(v.x, 0.0);
  } else {
    out[i] = v;
    out[nirf - i] = make_double2(v.x, -v.y);
  }
}

// ir[k] = Re(ifft)[k] / nirf * hamming(numtaps)[k], as a complex sequence of length numtaps
__global__ __launch_bounds__(256) void firwin2_window(const cdbl* __restrict__ time, cdbl* __restrict__ ir, int nirf,
                                                      int numtaps) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= numtaps) return;
  const double w = 0.54 - 0.46 * cos(2.0 * M_PI * (double)k / (double)(numtaps - 1));
  const double v = time[(long long)blockIdx.y * nirf + k].x / (double)nirf;
  ir[(long long)blockIdx.y * numtaps + k] = make_double2(v * w, 0.0);
}

// mag = |H| in place (.x), per-transform minimum of the strictly positive magnitudes.  The minima of all transforms sit
// in ONE cache line, and every operation on it - atomic or plain load - is served by one L2 channel at ~10 ns apiece:
// one per wave (4 800 at 16 x 19 200 points) took 43 - 60 us.  A workgroup now covers kMagPerThread x 256 points, folds
// its four waves in LDS and sends one atomic, after a plain read that lets all but a few skip even that.
constexpr int kMagPerThread = 8;
__global__ __launch_bounds__(256) void magnitude_and_min(cdbl* __restrict__ h, unsigned long long* __restrict__ minbits,
                                                         int N) {
  double m = INFINITY;
#pragma unroll
  for (int u = 0; u < kMagPerThread; ++u) {
    const int k = (blockIdx.x * kMagPerThread + u) * 256 + threadIdx.x;
    if (k < N) {
      cdbl* p = h + (long long)blockIdx.y * N + k;
      const double mag = hypot(p->x, p->y);
      *p = make_double2(mag, 0.0);
      if (mag > 0.0) m = fmin(m, mag);
    }
  }
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) m = fmin(m, __shfl_xor(m, sft, 64));
  __shared__ double s_m[4];
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmin(fmin(s_m[0], s_m[1]), fmin(s_m[2], s_m[3]));
    // positive doubles order like their bit patterns; a stale plain read only means an atomic that changes nothing
    if (m != INFINITY &&
        (unsigned long long)__double_as_longlong(m) < __atomic_load_n(&minbits[blockIdx.y], __ATOMIC_RELAXED))
      atomicMin(&minbits[blockIdx.y], (unsigned long long)__double_as_longlong(m));
  }
}

// x = 0.5 * log(mag + 1e-7 * min)
__global__ __launch_bounds__(256) void half_log(cdbl* __restrict__ h, const unsigned long long* __restrict__ minbits, int N) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const double mn = __longlong_as_double((long long)minbits[blockIdx.y]);
  cdbl* p = h + (long long)blockIdx.y * N + k;
  *p = make_double2(0.5 * log(p->x + 1e-7 * mn), 0.0);
}

// cepstrum (unnormalised IFFT output) -> real part / N * homomorphic window (1, 2.., 0..)
__global__ __launch_bounds__(256) void cepstral_window(cdbl* __restrict__ c, int N) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  const int stop = N / 2;
  double w = 0.0;
  if (k == 0) w = 1.0;
  else if (k < stop) w = 2.0;
  else if (k == stop && (N & 1)) w = 1.0;
  cdbl* p = c + (long long)blockIdx.y * N + k;
  *p = make_double2(p->x / (double)N * w, 0.0);
}

__global__ __launch_bounds__(256) void complex_exp(cdbl* __restrict__ c, int N) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  cdbl* p = c + (long long)blockIdx.y * N + k;
  const double e = exp(p->x);
  double sn, cs;
  sincos(p->y, &sn, &cs);
  *p = make_double2(e * cs, e * sn);
}

__global__ __launch_bounds__(256) void take_real(const cdbl* __restrict__ c, double* __restrict__ out, int N, int ntaps) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ntaps) return;
  out[(long long)blockIdx.y * ntaps + k] = c[(long long)blockIdx.y * N + k].x / (double)N;
}

// The same elementwise steps as load hooks of the tile transform (fft64.hip.h): op(value read, transform, index within it).
struct WindowIn {                    // firwin2_window: the value comes from the [B][nirf] time-domain buffer
  int nirf, numtaps;
  __device__ __forceinline__ cdbl operator()(cdbl t, long long, long long k) const {
    const double w = 0.54 - 0.46 * cos(2.0 * M_PI * (double)k / (double)(numtaps - 1));
    const double v = t.x / (double)nirf;
    return make_double2(v * w, 0.0);
  }
};
struct HalfLogIn {                   // half_log
  const unsigned long long* __restrict__ minbits;
  __device__ __forceinline__ cdbl operator()(cdbl h, long long b, long long) const {
    const double mn = __longlong_as_double((long long)minbits[b]);
    return make_double2(0.5 * log(h.x + 1e-7 * mn), 0.0);
  }
};
struct CepstralIn {                  // cepstral_window
  int N;
  __device__ __forceinline__ cdbl operator()(cdbl c, long long, long long k) const {
    const int stop = N / 2;
    double w = 0.0;
    if (k == 0) w = 1.0;
    else if (k < stop) w = 2.0;
    else if (k == stop && (N & 1)) w = 1.0;
    return make_double2(c.x / (double)N * w, 0.0);
  }
};
struct ExpIn {                       // complex_exp
  __device__ __forceinline__ cdbl operator()(cdbl c, long long, long long) const {
    const double e = exp(c.x);
    double sn, cs;
    sincos(c.y, &sn, &cs);
    return make_double2(e * cs, e * sn);
  }
};

}  // namespace

struct MinPhasePlan {
  int n = 0;            // taps out
  int numtaps = 0;      // 2n
  int nfreqs = 0;       // 1 + 2^ceil(log2 numtaps)
  int nirf = 0;         // 2 (nfreqs - 1)
  double nyq = 0, nyq_f = 0;
  std::vector<int> fac_tap, fac_irf;
  cdbl* roots_tap = nullptr;
  cdbl* roots_irf = nullptr;
  // work buffers for up to cap channels
  int64_t cap = 0;
  cdbl *a = nullptr, *b = nullptr;
  double* gain = nullptr;
  double* out = nullptr;
  unsigned long long* minbits = nullptr;
};

static void plan_free(MinPhasePlan* p) {
  if (!p) return;
  (void)hipFree(p->roots_tap);
  (void)hipFree(p->roots_irf);
  (void)hipFree(p->a);
  (void)hipFree(p->b);
  (void)hipFree(p->gain);
  (void)hipFree(p->out);
  (void)hipFree(p->minbits);
  delete p;
}

void minphase_plans_destroy(imp_ctx* ctx) {
  for (auto& kv : ctx->minphase_plans) plan_free(kv.second);
  ctx->minphase_plans.clear();
}

static int minphase_run(imp_ctx* ctx, const double* gain, const double* d_gain, int64_t B, int64_t n, double fs,
                        double* fir_out, int stage, double* d_fir_out = nullptr);

extern "C" int imp_minphase_fir(imp_ctx* ctx, const double* gain, int64_t B, int64_t n, double fs, double* fir_out) {
  return minphase_run(ctx, gain, nullptr, B, n, fs, fir_out, 2);
}

// the gains are already on the device (curves.hip: the FIR design grid computed from the equalisation curves there;
// its last column is zero by construction).  fir_out_host: the taps come back and the call waits for them;
// d_fir_out (device, [B][n]): they stay on the device and the call returns without waiting.
int minphase_fir_from_device_gain(imp_ctx* ctx, const double* d_gain, int64_t B, int64_t n, double fs, double* fir_out_host,
                                  double* d_fir_out) {
  return minphase_run(ctx, nullptr, d_gain, B, n, fs, fir_out_host, 2, d_fir_out);
}

extern "C" int imp_debug_minphase_stage(imp_ctx* ctx, const double* gain, int64_t B, int64_t n, double fs, int stage,
                                        double* out) {
  if (stage < 0 || stage > 1) return fail(IMP_ERR_INVALID, "stage must be 0 (firwin2 taps) or 1 (|FFT| of the taps)");
  return minphase_run(ctx, gain, nullptr, B, n, fs, out, stage);
}

// stage 0: out[B][2n] = firwin2 taps; stage 1: out[B][2n] = |FFT_2n(taps)|; stage 2: out[B][n] = FIR
static int minphase_run(imp_ctx* ctx, const double* gain, const double* d_gain, int64_t B, int64_t n, double fs,
                        double* fir_out, int stage, double* d_fir_out) {
  if (!ctx || (B && ((!gain && !d_gain) || (!fir_out && !d_fir_out)))) return fail(IMP_ERR_INVALID, "imp_minphase_fir: null argument");
  if (B < 0 || n < 2 || n > (1 << 20)) return fail(IMP_ERR_INVALID, "imp_minphase_fir: bad B or n");
  if (!(fs > 0)) return fail(IMP_ERR_INVALID, "imp_minphase_fir: fs must be positive");
  if (B == 0) return IMP_OK;
  for (int64_t b = 0; gain && b < B; ++b)
    if (gain[b * n + n - 1] != 0.0)
      return fail(IMP_ERR_INVALID, "A Type II filter must have zero gain at the Nyquist frequency (channel %lld)", (long long)b);
  IMP_CTX_LOCK(ctx);                               // plan buffers are shared by all callers of this context
  int rc = ctx_bind(ctx);
  if (rc) return rc;

  MinPhasePlan* p = nullptr;
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const auto key = std::make_pair((long long)n, (long long)std::llround(fs * 1000.0));
    auto it = ctx->minphase_plans.find(key);
    if (it != ctx->minphase_plans.end()) {
      p = it->second;
    } else {
      p = new (std::nothrow) MinPhasePlan();
      if (!p) return fail(IMP_ERR_ALLOC, "out of host memory");
      p->n = (int)n;
      p->numtaps = 2 * (int)n;
      int lg = 0;
      while ((1 << lg) < p->numtaps) ++lg;
      p->nfreqs = 1 + (1 << lg);
      p->nirf = 2 * (p->nfreqs - 1);
      p->nyq = 0.5 * fs;
      p->nyq_f = std::floor(fs / 2.0);                 // the reference's grid ends at fs // 2
      p->fac_tap = factorise(p->numtaps);
      p->fac_irf = factorise(p->nirf);
      if (p->fac_tap.empty() || p->fac_irf.empty()) {
        delete p;
        return fail(IMP_ERR_UNSUPPORTED, "2n = %d is not of the form 2^a 3^b 5^c", 2 * (int)n);
      }
      if ((rc = upload_roots(&p->roots_tap, p->numtaps, ctx->stream)) ||
          (rc = upload_roots(&p->roots_irf, p->nirf, ctx->stream))) {
        plan_free(p);
        return rc;
      }
      ctx->minphase_plans[key] = p;
    }
  }
  if (p->nyq_f != p->nyq)
    return fail(IMP_ERR_INVALID, "freq must start with 0 and end with fs/2. (odd fs %g: grid ends at %g)", fs, p->nyq_f);
  if (p->cap < B) {
    (void)hipFree(p->a); (void)hipFree(p->b); (void)hipFree(p->gain); (void)hipFree(p->out); (void)hipFree(p->minbits);
    p->a = p->b = nullptr; p->gain = p->out = nullptr; p->minbits = nullptr; p->cap = 0;
    const size_t len = (size_t)std::max(p->nirf, p->numtaps);
    if (hipMalloc((void**)&p->a, (size_t)B * len * sizeof(cdbl)) != hipSuccess ||
        hipMalloc((void**)&p->b, (size_t)B * len * sizeof(cdbl)) != hipSuccess ||
        hipMalloc((void**)&p->gain, (size_t)B * n * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&p->out, (size_t)B * n * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&p->minbits, (size_t)B * sizeof(unsigned long long)) != hipSuccess)
      return fail(IMP_ERR_ALLOC, "imp_minphase_fir: device allocation for %lld channels failed", (long long)B);
    p->cap = B;
  }
  hipStream_t s = ctx->stream;
  if (gain) HIP_TRY(hipMemcpyAsync(p->gain, gain, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, s));
  else HIP_TRY(hipMemcpyAsync(p->gain, d_gain, (size_t)B * n * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemsetAsync(p->minbits, 0xFF, (size_t)B * sizeof(unsigned long long), s));
  auto grid_for = [&](int count) { return dim3((unsigned)((count + 255) / 256), (unsigned)B); };
  cdbl *cur = p->a, *oth = p->b;

  // firwin2
  hipLaunchKernelGGL(firwin2_spectrum, grid_for(p->nfreqs), dim3(256), 0, s, p->gain, cur, p->n, p->nfreqs, p->nyq_f,
                     p->nyq, p->numtaps);
  HIP_TRY(hipGetLastError());
  if ((rc = run_fft(ctx, p->fac_irf, p->roots_irf, p->nirf, B, +1, &cur, &oth))) return rc;
  // minimum_phase (homomorphic, half = True)
  const int N = p->numtaps;
  auto dump_real = [&](const cdbl* src) -> int {       // debug stages: real parts of [B][N]
    std::vector<cdbl> h((size_t)B * N);
    HIP_TRY(hipMemcpyAsync(h.data(), src, h.size() * sizeof(cdbl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < h.size(); ++i) fir_out[i] = h[i].x;
    return IMP_OK;
  };
  // The elementwise steps between the transforms are the LOAD hooks of the transform that follows them (same arithmetic,
  // same values - one launch and one pass over memory less each); the debug stages and lengths the tile transform does
  // not take keep them as kernels of their own.
  const bool fused = stage == 2 && fft64_wanted() && fft64::make_plan(N).ok;
  if (fused) {
    if ((rc = run_fft_ops(ctx, p->fac_tap, p->roots_tap, N, B, -1, &cur, &oth, WindowIn{p->nirf, p->numtaps}, fft64::NoOp{}, nullptr,
                          p->nirf)))
      return rc;
    hipLaunchKernelGGL(magnitude_and_min, dim3((unsigned)((N + 256 * kMagPerThread - 1) / (256 * kMagPerThread)), (unsigned)B),
                       dim3(256), 0, s, cur, p->minbits, N);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft_ops(ctx, p->fac_tap, p->roots_tap, N, B, +1, &cur, &oth, HalfLogIn{p->minbits}, fft64::NoOp{}))) return rc;
    if ((rc = run_fft_ops(ctx, p->fac_tap, p->roots_tap, N, B, -1, &cur, &oth, CepstralIn{N}, fft64::NoOp{}))) return rc;
    if ((rc = run_fft_ops(ctx, p->fac_tap, p->roots_tap, N, B, +1, &cur, &oth, ExpIn{}, fft64::NoOp{}))) return rc;
  } else {
    hipLaunchKernelGGL(firwin2_window, grid_for(p->numtaps), dim3(256), 0, s, cur, oth, p->nirf, p->numtaps);
    HIP_TRY(hipGetLastError());
    std::swap(cur, oth);
    if (stage == 0) return dump_real(cur);
    if ((rc = run_fft(ctx, p->fac_tap, p->roots_tap, N, B, -1, &cur, &oth))) return rc;
    hipLaunchKernelGGL(magnitude_and_min, dim3((unsigned)((N + 256 * kMagPerThread - 1) / (256 * kMagPerThread)), (unsigned)B),
                       dim3(256), 0, s, cur, p->minbits, N);
    HIP_TRY(hipGetLastError());
    if (stage == 1) return dump_real(cur);
    hipLaunchKernelGGL(half_log, grid_for(N), dim3(256), 0, s, cur, p->minbits, N);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft(ctx, p->fac_tap, p->roots_tap, N, B, +1, &cur, &oth))) return rc;
    hipLaunchKernelGGL(cepstral_window, grid_for(N), dim3(256), 0, s, cur, N);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft(ctx, p->fac_tap, p->roots_tap, N, B, -1, &cur, &oth))) return rc;
    hipLaunchKernelGGL(complex_exp, grid_for(N), dim3(256), 0, s, cur, N);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft(ctx, p->fac_tap, p->roots_tap, N, B, +1, &cur, &oth))) return rc;
  }
  hipLaunchKernelGGL(take_real, grid_for(p->n), dim3(256), 0, s, cur, d_fir_out ? d_fir_out : p->out, N, p->n);
  HIP_TRY(hipGetLastError());
  if (fir_out) {
    HIP_TRY(hipMemcpyAsync(fir_out, d_fir_out ? d_fir_out : p->out, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return IMP_OK;
}


// Test hook: the batched fp64 transform the fp64 kernels share (K6, K2, filter spectra), on host data.
extern "C" int imp_debug_fft64(imp_ctx* ctx, const double* x, int64_t B, int64_t N, int dir, double* y, int* used_tiles) {
  if (!ctx || !x || !y) return fail(IMP_ERR_INVALID, "imp_debug_fft64: null argument");
  if (B < 1 || N < 2 || N > (1 << 22) || (dir != 1 && dir != -1)) return fail(IMP_ERR_INVALID, "imp_debug_fft64: bad B, N or dir");
  const std::vector<int> fac = factorise((int)N);
  if (fac.empty()) return fail(IMP_ERR_UNSUPPORTED, "imp_debug_fft64: N = %lld is not 2^a 3^b 5^c 11^d", (long long)N);
  IMP_CTX_LOCK(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  cdbl *a = nullptr, *b = nullptr, *roots = nullptr;
  const size_t bytes = (size_t)B * N * sizeof(cdbl);
  hipStream_t s = ctx->stream;
  auto cleanup = [&](int code) {
    (void)hipStreamSynchronize(s);
    (void)ctx_block_put(ctx, a);
    (void)ctx_block_put(ctx, b);
    (void)hipFree(roots);
    return code;
  };
  if (ctx_block_get(ctx, bytes, (void**)&a) || ctx_block_get(ctx, bytes, (void**)&b)) return cleanup(IMP_ERR_ALLOC);
  if ((rc = upload_roots(&roots, (int)N, s))) return cleanup(rc);
  if (hipMemcpyAsync(a, x, bytes, hipMemcpyHostToDevice, s) != hipSuccess) return cleanup(fail(IMP_ERR_HIP, "imp_debug_fft64: upload failed"));
  cdbl *cur = a, *oth = b;
  bool tiles = false;
  if ((rc = run_fft_ops(ctx, fac, roots, (int)N, B, dir, &cur, &oth, fft64::NoOp{}, fft64::NoOp{}, &tiles))) return cleanup(rc);
  if (used_tiles) *used_tiles = tiles ? 1 : 0;
  if (hipMemcpyAsync(y, cur, bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return cleanup(fail(IMP_ERR_HIP, "imp_debug_fft64: download failed"));
  return cleanup(IMP_OK);
}
