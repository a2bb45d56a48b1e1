// K2 - magnitude responses in fp64: 20 log10 |rfft(x)| of rows of any length (core/audio_io.py:100-113), by the n-point
// transform itself where n is a product of the radices of fft64_host.hip.h and by Bluestein's chirp-z identity elsewhere.
// Two forms: MagPlan (imp_magnitude_db*: row length known to the host, plans cached per length) and SliceNorm (K2 of
// imp_slice: row lengths known only on the device).  They share the transform, pointwise_mul and rows_max_kernel; their
// pre / post / chirp kernels do different work (pair packing, a device-side chirp) and stay apart.
#include <cstring>
#include <new>

#include "fft64_host.hip.h"

namespace {

// ---- K2 when n is a product of the transform's radices (crop_tails leaves next_fast_len lengths): the DFT itself ----
__global__ __launch_bounds__(256) void real_to_complex(const double* __restrict__ x, cdbl* __restrict__ a, int n) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  a[(long long)blockIdx.y * n + m] = make_double2(x[(long long)blockIdx.y * n + m], 0.0);
}

// out = 20 log10 |X[k]| for k < half (no epsilon: -inf for exact zeros)
__global__ __launch_bounds__(256) void direct_post_db(const cdbl* __restrict__ X, double* __restrict__ out, int n, int half) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= half) return;
  const cdbl v = X[(long long)blockIdx.y * n + k];
  out[(long long)blockIdx.y * half + k] = 20.0 * log10(hypot(v.x, v.y));
}

// ---- K2: arbitrary-length DFT by Bluestein's chirp-z identity --------------------------------
// a[m] = x[m] c[m] (zero padded to Mfft), c[m] = exp(-i pi m^2 / n)
__global__ __launch_bounds__(256) void bluestein_pre(const double* __restrict__ x, const cdbl* __restrict__ chirp,
                                                     cdbl* __restrict__ a, int n, int mfft) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= mfft) return;
  cdbl v = make_double2(0.0, 0.0);
  if (m < n) {
    const double xv = x[(long long)blockIdx.y * n + m];
    const cdbl c = chirp[m];
    v = make_double2(xv * c.x, xv * c.y);
  }
  a[(long long)blockIdx.y * mfft + m] = v;
}

// a[r][m] *= b[r b_pitch + m]: b_pitch = 0 for one b shared by every row, mfft for a b per row
__global__ __launch_bounds__(256) void pointwise_mul(cdbl* __restrict__ a, const cdbl* __restrict__ b, int mfft, int b_pitch) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= mfft) return;
  cdbl* p = a + (long long)blockIdx.y * mfft + m;
  *p = zmul(*p, b[(long long)blockIdx.y * b_pitch + m]);
}

// X[k] = c[k] * conv[k] / Mfft ; out = 20 log10 |X[k]| for k < half (no epsilon: -inf for exact zeros)
__global__ __launch_bounds__(256) void bluestein_post_db(const cdbl* __restrict__ conv, const cdbl* __restrict__ chirp,
                                                         double* __restrict__ out, int mfft, int half) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= half) return;
  const cdbl v = zmul(conv[(long long)blockIdx.y * mfft + k], chirp[k]);
  out[(long long)blockIdx.y * half + k] = 20.0 * log10(hypot(v.x, v.y) / (double)mfft);
}

// np.max of each row of out (NaN if the row holds one, as np.max; -inf for an empty row): one workgroup of 1024 per row,
// eight loads in flight per thread (256 threads walking the row one load at a time took 37 us for two rows of 32 448).
// n_of == nullptr: rows of `half` values, `half` apart.  Otherwise (the slice: two rows per measurement) row g holds
// ceil(min(n_of[g / 2], n_max) / 2) values and the rows are `half` apart.
__global__ __launch_bounds__(1024) void rows_max_kernel(const double* __restrict__ out, int half, const long long* __restrict__ n_of,
                                                        int n_max, double* __restrict__ peak) {
  const double* row = out + (long long)blockIdx.x * half;
  if (n_of) {
    long long n = n_of[blockIdx.x >> 1];
    n = n < n_max ? n : n_max;
    half = (int)((n + 1) / 2);
  }
  double m = -INFINITY;
  bool nan = false;
  for (int k0 = 0; k0 < half; k0 += 8 * 1024) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + u * 1024 + (int)threadIdx.x;
      v[u] = k < half ? row[k] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      nan = nan || v[u] != v[u];
      m = v[u] > m ? v[u] : m;
    }
  }
  __shared__ double s_m[1024];
  __shared__ int s_nan;
  if (threadIdx.x == 0) s_nan = 0;
  __syncthreads();
  s_m[threadIdx.x] = m;
  if (nan) s_nan = 1;
  __syncthreads();
  for (int st = 512; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) s_m[threadIdx.x] = s_m[threadIdx.x] > s_m[threadIdx.x + st] ? s_m[threadIdx.x] : s_m[threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x == 0) peak[blockIdx.x] = s_nan ? __longlong_as_double(0x7ff8000000000000ll) : s_m[0];
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// K2: magnitude response of arbitrary-length rows (core/audio_io.py:100-113), fp64 Bluestein
// ------------------------------------------------------------------------------------------------
struct MagPlan {
  int n = 0, mfft = 0;
  bool direct = false;          // n factorises over the Stockham radices: one n-point transform, no chirp
  std::vector<int> fac;
  cdbl *roots = nullptr, *chirp = nullptr, *bhat = nullptr;
  int64_t cap = 0;
  cdbl *a = nullptr, *b = nullptr;
  double *x = nullptr, *out = nullptr;
};

static std::map<long long, MagPlan*>& mag_plans(imp_ctx* ctx) { return ctx->magnitude_plans; }

static void mag_plan_free(MagPlan* p) {
  if (!p) return;
  (void)hipFree(p->roots); (void)hipFree(p->chirp); (void)hipFree(p->bhat);
  (void)hipFree(p->a); (void)hipFree(p->b); (void)hipFree(p->x); (void)hipFree(p->out);
  delete p;
}

void magnitude_plans_destroy(imp_ctx* ctx) {
  std::lock_guard<std::recursive_mutex> lk(ctx->mu);
  auto& m = mag_plans(ctx);
  for (auto& kv : m) mag_plan_free(kv.second);
  m.clear();
}

namespace {
// out[g][i] = sum over the rows of group g (in row order, zero beyond a row's end) - np.sum(np.vstack(padded), axis=0)
__global__ __launch_bounds__(256) void rows_group_sum_kernel(const float* __restrict__ src, const int64_t* __restrict__ off,
                                                             const int64_t* __restrict__ len, const int64_t* __restrict__ group,
                                                             int B, double* __restrict__ out, int64_t n) {
  const int g = blockIdx.y;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int b = 0; b < B; ++b)
      if (group[b] == g && i < len[b]) acc += (double)src[off[b] + i];
    out[(int64_t)g * n + i] = acc;
  }
}

}  // namespace

static int magnitude_db_core(imp_ctx* ctx, const double* x, const float* d_rows, const int64_t* off, const int64_t* len,
                             const int64_t* group, int64_t n_rows, int64_t B, int64_t n, double* db_out, bool peak_only);

extern "C" int imp_magnitude_db(imp_ctx* ctx, const double* x, int64_t B, int64_t n, double* db_out) {
  return magnitude_db_core(ctx, x, nullptr, nullptr, nullptr, nullptr, 0, B, n, db_out, false);
}

// Device-resident rows (fp32 at d_rows + off[r], len[r] samples, r < n_rows) are summed per group (group[r] in
// [0, n_groups), rows of a group added in row order in fp64, zero beyond a row's end: np.sum(np.vstack(padded), axis=0)
// of core/hrir.py:496-503) and the magnitude response of every sum (n points) is returned: HRIR.normalize without
// bringing the responses back to the host.
extern "C" int imp_magnitude_db_sum_device(imp_ctx* ctx, const float* d_rows, const int64_t* off, const int64_t* len,
                                           const int64_t* group, int64_t n_rows, int64_t n_groups, int64_t n,
                                           double* db_out) {
  if (!ctx || !d_rows || !off || !len || !group || n_rows < 1 || n_groups < 1)
    return fail(IMP_ERR_INVALID, "imp_magnitude_db_sum_device: bad argument");
  for (int64_t r = 0; r < n_rows; ++r)
    if (off[r] < 0 || len[r] < 0 || len[r] > n || group[r] < 0 || group[r] >= n_groups)
      return fail(IMP_ERR_INVALID, "imp_magnitude_db_sum_device: row %lld out of range", (long long)r);
  return magnitude_db_core(ctx, nullptr, d_rows, off, len, group, n_rows, n_groups, n, db_out, false);
}

// the maximum of each of those spectra only (HRIR.normalize with peak_target, core/hrir.py:505: np.max of the stacked
// spectra): peak_db_out[n_groups]; NaN if a spectrum holds one, -inf for an all-zero sum - what np.max returns
extern "C" int imp_magnitude_db_sum_peak_device(imp_ctx* ctx, const float* d_rows, const int64_t* off, const int64_t* len,
                                                const int64_t* group, int64_t n_rows, int64_t n_groups, int64_t n,
                                                double* peak_db_out) {
  if (!ctx || !d_rows || !off || !len || !group || n_rows < 1 || n_groups < 1)
    return fail(IMP_ERR_INVALID, "imp_magnitude_db_sum_peak_device: bad argument");
  for (int64_t r = 0; r < n_rows; ++r)
    if (off[r] < 0 || len[r] < 0 || len[r] > n || group[r] < 0 || group[r] >= n_groups)
      return fail(IMP_ERR_INVALID, "imp_magnitude_db_sum_peak_device: row %lld out of range", (long long)r);
  return magnitude_db_core(ctx, nullptr, d_rows, off, len, group, n_rows, n_groups, n, peak_db_out, true);
}

static int magnitude_db_core(imp_ctx* ctx, const double* x, const float* d_rows, const int64_t* off, const int64_t* len,
                             const int64_t* group, int64_t n_rows, int64_t B, int64_t n, double* db_out, bool peak_only) {
  if (!ctx || (B && n && ((!x && !d_rows) || !db_out))) return fail(IMP_ERR_INVALID, "imp_magnitude_db: null argument");
  IMP_CTX_LOCK(ctx);
  if (B < 0 || n < 0 || n > (1 << 22)) return fail(IMP_ERR_INVALID, "imp_magnitude_db: bad B or n");
  if (B == 0 || n == 0) return IMP_OK;
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  const int half = (int)((n + 1) / 2);
  MagPlan* p = nullptr;
  {
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    auto& plans = mag_plans(ctx);
    auto it = plans.find((long long)n);
    if (it != plans.end()) {
      p = it->second;
    } else {
      p = new (std::nothrow) MagPlan();
      if (!p) return fail(IMP_ERR_ALLOC, "out of host memory");
      p->n = (int)n;
      if (n >= 2 && !ctx->k2_bluestein_only && !factorise((int)n).empty()) {
        p->direct = true;
        p->mfft = (int)n;
        p->fac = factorise((int)n);
        if (upload_roots(&p->roots, (int)n, ctx->stream) != IMP_OK || hipStreamSynchronize(ctx->stream) != hipSuccess) {
          mag_plan_free(p);
          return fail(IMP_ERR_HIP, "imp_magnitude_db: plan set-up for n = %lld failed", (long long)n);
        }
        plans[(long long)n] = p;
      }
    }
    if (!p->direct && !p->chirp) {
      int mf = 1;
      while (mf < 2 * (int)n - 1) mf <<= 1;
      if (mf < 4) mf = 4;
      p->mfft = mf;
      p->fac = factorise(mf);
      // chirp c[m] = exp(-i pi m^2 / n), phase reduced exactly: m^2 mod 2n
      std::vector<cdbl> c((size_t)n), bb((size_t)mf, make_double2(0.0, 0.0));
      for (int64_t m = 0; m < n; ++m) {
        const double ang = -M_PI * (double)((m * m) % (2 * n)) / (double)n;
        c[(size_t)m] = make_double2(std::cos(ang), std::sin(ang));
      }
      // b[j] = conj(c[|j|]) placed circularly at j mod mfft, j in (-n, n)
      for (int64_t j = 0; j < n; ++j) {
        const cdbl v = make_double2(c[(size_t)j].x, -c[(size_t)j].y);
        bb[(size_t)j] = v;
        if (j) bb[(size_t)(mf - j)] = v;
      }
      hipStream_t s = ctx->stream;
      bool ok = upload_roots(&p->roots, mf, s) == IMP_OK &&
                hipMalloc((void**)&p->chirp, (size_t)n * sizeof(cdbl)) == hipSuccess &&
                hipMalloc((void**)&p->bhat, (size_t)mf * sizeof(cdbl)) == hipSuccess &&
                hipMalloc((void**)&p->b, (size_t)mf * sizeof(cdbl)) == hipSuccess &&
                hipMemcpyAsync(p->chirp, c.data(), (size_t)n * sizeof(cdbl), hipMemcpyHostToDevice, s) == hipSuccess &&
                hipMemcpyAsync(p->bhat, bb.data(), (size_t)mf * sizeof(cdbl), hipMemcpyHostToDevice, s) == hipSuccess;
      if (ok) {
        cdbl *cur = p->bhat, *oth = p->b;
        ok = run_fft(ctx, p->fac, p->roots, mf, 1, -1, &cur, &oth) == IMP_OK && hipStreamSynchronize(s) == hipSuccess;
        if (ok && cur != p->bhat) std::swap(p->bhat, p->b);       // result may sit in the other buffer
      }
      if (p->b) { (void)hipFree(p->b); p->b = nullptr; }
      if (!ok) {
        mag_plan_free(p);
        return fail(IMP_ERR_HIP, "imp_magnitude_db: plan set-up for n = %lld failed", (long long)n);
      }
      plans[(long long)n] = p;
    }
  }
  if (p->cap < B) {
    (void)hipFree(p->a); (void)hipFree(p->b); (void)hipFree(p->x); (void)hipFree(p->out);
    p->a = p->b = nullptr; p->x = p->out = nullptr; p->cap = 0;
    if (hipMalloc((void**)&p->a, (size_t)B * p->mfft * sizeof(cdbl)) != hipSuccess ||
        hipMalloc((void**)&p->b, (size_t)B * p->mfft * sizeof(cdbl)) != hipSuccess ||
        hipMalloc((void**)&p->x, (size_t)B * n * sizeof(double)) != hipSuccess ||
        hipMalloc((void**)&p->out, (size_t)B * half * sizeof(double)) != hipSuccess)
      return fail(IMP_ERR_ALLOC, "imp_magnitude_db: device allocation failed");
    p->cap = B;
  }
  hipStream_t s = ctx->stream;
  if (x) {
    HIP_TRY(hipMemcpyAsync(p->x, x, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, s));
  } else {
    // row tables through the staging ring: one copy in stream order, no wait before the transform
    const size_t meta = (size_t)n_rows * sizeof(int64_t);
    int64_t *h_meta = nullptr, *d_meta = nullptr;
    if ((rc = ctx_stage(ctx, 3 * meta, (void**)&h_meta, (void**)&d_meta))) return rc;
    std::memcpy(h_meta, off, meta);
    std::memcpy(h_meta + n_rows, len, meta);
    std::memcpy(h_meta + 2 * n_rows, group, meta);
    if ((rc = ctx_stage_push(ctx, h_meta, d_meta, 3 * meta))) return rc;
    hipLaunchKernelGGL(rows_group_sum_kernel, dim3((unsigned)std::min<int64_t>(256, (n + 255) / 256), (unsigned)B),
                       dim3(256), 0, s, d_rows, d_meta, d_meta + n_rows, d_meta + 2 * n_rows, (int)n_rows, p->x, n);
    if (hipGetLastError() != hipSuccess) return fail(IMP_ERR_HIP, "imp_magnitude_db_sum_device: row sum failed");
  }
  auto grid_for = [&](int count) { return dim3((unsigned)((count + 255) / 256), (unsigned)B); };
  cdbl *cur = p->a, *oth = p->b;
  if (p->direct) {                                       // n = 2^a 3^b 5^c 11^d: the n-point transform itself
    hipLaunchKernelGGL(real_to_complex, grid_for(p->n), dim3(256), 0, s, p->x, cur, p->n);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft(ctx, p->fac, p->roots, p->n, B, -1, &cur, &oth))) return rc;
    hipLaunchKernelGGL(direct_post_db, grid_for(half), dim3(256), 0, s, cur, p->out, p->n, half);
    HIP_TRY(hipGetLastError());
  } else {
    hipLaunchKernelGGL(bluestein_pre, grid_for(p->mfft), dim3(256), 0, s, p->x, p->chirp, cur, p->n, p->mfft);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft(ctx, p->fac, p->roots, p->mfft, B, -1, &cur, &oth))) return rc;
    hipLaunchKernelGGL(pointwise_mul, grid_for(p->mfft), dim3(256), 0, s, cur, (const cdbl*)p->bhat, p->mfft, 0);
    HIP_TRY(hipGetLastError());
    if ((rc = run_fft(ctx, p->fac, p->roots, p->mfft, B, +1, &cur, &oth))) return rc;
    hipLaunchKernelGGL(bluestein_post_db, grid_for(half), dim3(256), 0, s, cur, p->chirp, p->out, p->mfft, half);
    HIP_TRY(hipGetLastError());
  }
  if (peak_only) {                                       // db_out[B]: the maximum of each spectrum (p->x is free again)
    hipLaunchKernelGGL(rows_max_kernel, dim3((unsigned)B), dim3(1024), 0, s, (const double*)p->out, half, (const long long*)nullptr, 0, p->x);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(db_out, p->x, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, s));
  } else {
    HIP_TRY(hipMemcpyAsync(db_out, p->out, (size_t)B * half * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return IMP_OK;
}


// ------------------------------------------------------------------------------------------------
// K2 for imp_slice (HRIR.normalize, core/hrir.py:496-505): np.max of the magnitude response of each ear's sum, for M
// measurements whose row length n_m is known ONLY ON THE DEVICE (crop_tails decided it there).  Same chirp-z identity as
// above, but the chirp of each measurement is formed on the device from its n_m and the convolution length is fixed by
// the slice's capacity (mfft >= 2 n_max - 1), so the launch sequence does not depend on any n_m: nothing is read back.
// The two ear sums are real: they go through ONE complex transform, z = x_L + i x_R, and are separated afterwards.
// ------------------------------------------------------------------------------------------------
struct SliceNorm {
  int n_max = 0, mfft = 0, half_max = 0;
  int64_t m_cap = 0;
  std::vector<int> fac;
  cdbl* roots = nullptr;
  double* x = nullptr;       // [2 m_cap][n_max]   ear sums
  cdbl* chirp = nullptr;     // [m_cap][n_max]
  cdbl* bhat = nullptr;      // [m_cap][mfft]      transform of the conjugate chirp
  cdbl* bwork = nullptr;
  cdbl *a = nullptr, *b = nullptr;     // [m_cap][mfft]: the two ears of a measurement share a transform
  double* out = nullptr;     // [2 m_cap][half_max]
};

namespace {

// x[2 m + ear][i] = sum over the pairs q of rows[(m R + 2 q + ear) pitch + i], i < n_m, added in row order in fp64
// (np.sum(np.vstack(...), axis=0) of core/hrir.py:496-503; the rows of a measurement are equally long after crop_tails)
__global__ __launch_bounds__(256) void sn_sum_kernel(const float* __restrict__ rows, long long pitch, int rows_per_meas,
                                                     const long long* __restrict__ n_of, double* __restrict__ x, int n_max) {
  const int g = blockIdx.y, m = g >> 1, ear = g & 1;
  long long n = n_of[m];
  n = n < n_max ? n : n_max;
  const float* base = rows + ((long long)m * rows_per_meas + ear) * pitch;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    double acc = 0.0;
    for (int q = 0; 2 * q < rows_per_meas; ++q) acc += (double)base[(long long)(2 * q) * pitch + i];
    x[(long long)g * n_max + i] = acc;
  }
}

// chirp[m][j] = exp(-i pi j^2 / n_m) (phase reduced exactly: j^2 mod 2 n_m), j < n_m; bb[m][j] = conj chirp[|j|] placed
// circularly at j mod mfft, zero elsewhere
__global__ __launch_bounds__(256) void sn_chirp_kernel(const long long* __restrict__ n_of, cdbl* __restrict__ chirp,
                                                       cdbl* __restrict__ bb, int n_max, int mfft) {
  const int m = blockIdx.y;
  long long n = n_of[m];
  n = n < n_max ? n : n_max;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= mfft) return;
  auto c_at = [&](long long k) {
    const double ang = -M_PI * (double)((k * k) % (2 * n)) / (double)n;
    double sn, cs;
    sincos(ang, &sn, &cs);
    return make_double2(cs, sn);
  };
  cdbl v = make_double2(0.0, 0.0);
  if (j < n) {
    const cdbl c = c_at(j);
    chirp[(long long)m * n_max + j] = c;
    v = make_double2(c.x, -c.y);
  } else if (j > 0 && mfft - j < n) {
    const cdbl c = c_at(mfft - j);
    v = make_double2(c.x, -c.y);
  }
  bb[(long long)m * mfft + j] = v;
}

// the two ears of a measurement travel as ONE complex signal z = x_L + i x_R (both real): a[m][j] = z[j] chirp[j]
__global__ __launch_bounds__(256) void sn_pre_kernel(const double* __restrict__ x, const cdbl* __restrict__ chirp,
                                                     const long long* __restrict__ n_of, cdbl* __restrict__ a, int n_max,
                                                     int mfft) {
  const int m = blockIdx.y;
  long long n = n_of[m];
  n = n < n_max ? n : n_max;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= mfft) return;
  cdbl v = make_double2(0.0, 0.0);
  if (j < n) {
    const cdbl z = make_double2(x[(long long)(2 * m) * n_max + j], x[(long long)(2 * m + 1) * n_max + j]);
    v = zmul(z, chirp[(long long)m * n_max + j]);
  }
  a[(long long)m * mfft + j] = v;
}

// Z[k] = chirp[k] conv[k] / mfft is the n-point transform of z; the ears' transforms are its Hermitian parts:
// X_L[k] = (Z[k] + conj Z[n - k]) / 2, X_R[k] = (Z[k] - conj Z[n - k]) / 2i; out[2 m + ear][k] = 20 log10 |X_ear[k]|, k < ceil(n / 2)
__global__ __launch_bounds__(256) void sn_post_kernel(const cdbl* __restrict__ conv, const cdbl* __restrict__ chirp,
                                                      const long long* __restrict__ n_of, double* __restrict__ out, int n_max,
                                                      int mfft, int half_max) {
  const int m = blockIdx.y;
  long long n = n_of[m];
  n = n < n_max ? n : n_max;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (n + 1) / 2) return;
  const cdbl* cv = conv + (long long)m * mfft;
  const cdbl* ch = chirp + (long long)m * n_max;
  const int kk = k == 0 ? 0 : (int)(n - k);
  const cdbl zk = zmul(cv[k], ch[k]), zn = zmul(cv[kk], ch[kk]);
  const double s = 0.5 / (double)mfft;
  const cdbl xl = make_double2((zk.x + zn.x) * s, (zk.y - zn.y) * s);
  const cdbl xr = make_double2((zk.y + zn.y) * s, (zn.x - zk.x) * s);
  out[(long long)(2 * m) * half_max + k] = 20.0 * log10(hypot(xl.x, xl.y));
  out[(long long)(2 * m + 1) * half_max + k] = 20.0 * log10(hypot(xr.x, xr.y));
}

}  // namespace

void slice_norm_destroy(SliceNorm* p) {
  if (!p) return;
  (void)hipFree(p->roots); (void)hipFree(p->x); (void)hipFree(p->chirp); (void)hipFree(p->bhat); (void)hipFree(p->bwork);
  (void)hipFree(p->a); (void)hipFree(p->b); (void)hipFree(p->out);
  delete p;
}

int slice_norm_create(imp_ctx* ctx, int64_t n_max, int64_t m_cap, SliceNorm** out) {
  *out = nullptr;
  if (n_max < 1 || n_max > (1 << 22) || m_cap < 1) return fail(IMP_ERR_INVALID, "slice normalisation: bad n_max / capacity");
  SliceNorm* p = new (std::nothrow) SliceNorm();
  if (!p) return fail(IMP_ERR_ALLOC, "out of host memory");
  p->n_max = (int)n_max;
  p->half_max = (int)((n_max + 1) / 2);
  p->m_cap = m_cap;
  int mf = 4;
  while (mf < 2 * (int)n_max - 1) mf <<= 1;
  p->mfft = mf;
  p->fac = factorise(mf);
  const size_t M = (size_t)m_cap;
  bool ok = upload_roots(&p->roots, mf, ctx->stream) == IMP_OK &&
            hipMalloc((void**)&p->x, 2 * M * (size_t)n_max * sizeof(double)) == hipSuccess &&
            hipMalloc((void**)&p->chirp, M * (size_t)n_max * sizeof(cdbl)) == hipSuccess &&
            hipMalloc((void**)&p->bhat, M * (size_t)mf * sizeof(cdbl)) == hipSuccess &&
            hipMalloc((void**)&p->bwork, M * (size_t)mf * sizeof(cdbl)) == hipSuccess &&
            hipMalloc((void**)&p->a, M * (size_t)mf * sizeof(cdbl)) == hipSuccess &&
            hipMalloc((void**)&p->b, M * (size_t)mf * sizeof(cdbl)) == hipSuccess &&
            hipMalloc((void**)&p->out, 2 * M * (size_t)p->half_max * sizeof(double)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    slice_norm_destroy(p);
    return fail(IMP_ERR_ALLOC, "slice normalisation: device allocation failed (n_max %lld, %lld measurements)", (long long)n_max,
                (long long)m_cap);
  }
  *out = p;
  return IMP_OK;
}

int64_t slice_norm_mfft(const SliceNorm* p) { return p->mfft; }

// d_rows: the equalised rows [M R][pitch]; d_n[m] = their length; d_peak_db[2 m + ear] receives the maxima.  Asynchronous
// on the context's stream.
int slice_norm_run(imp_ctx* ctx, SliceNorm* p, const float* d_rows, int64_t pitch, int rows_per_meas, const long long* d_n,
                   int64_t M, double* d_peak_db) {
  if (M < 1 || M > p->m_cap) return fail(IMP_ERR_INVALID, "slice normalisation: %lld measurements exceed the capacity %lld",
                                         (long long)M, (long long)p->m_cap);
  hipStream_t s = ctx->stream;
  const int mf = p->mfft, nm = p->n_max;
  auto grid = [&](int count, int64_t rows) { return dim3((unsigned)((count + 255) / 256), (unsigned)rows); };
  hipLaunchKernelGGL(sn_sum_kernel, dim3((unsigned)std::min<int>(256, (nm + 255) / 256), (unsigned)(2 * M)), dim3(256), 0, s, d_rows,
                     (long long)pitch, rows_per_meas, d_n, p->x, nm);
  hipLaunchKernelGGL(sn_chirp_kernel, grid(mf, M), dim3(256), 0, s, d_n, p->chirp, p->bhat, nm, mf);
  HIP_TRY(hipGetLastError());
  int rc;
  cdbl *cur = p->bhat, *oth = p->bwork;
  if ((rc = run_fft(ctx, p->fac, p->roots, mf, M, -1, &cur, &oth))) return rc;
  const cdbl* bhat = cur;                                  // (either buffer: both belong to the plan)
  hipLaunchKernelGGL(sn_pre_kernel, grid(mf, M), dim3(256), 0, s, p->x, p->chirp, d_n, p->a, nm, mf);
  HIP_TRY(hipGetLastError());
  cdbl *c2 = p->a, *o2 = p->b;
  if ((rc = run_fft(ctx, p->fac, p->roots, mf, M, -1, &c2, &o2))) return rc;
  hipLaunchKernelGGL(pointwise_mul, grid(mf, M), dim3(256), 0, s, c2, bhat, mf, mf);
  HIP_TRY(hipGetLastError());
  if ((rc = run_fft(ctx, p->fac, p->roots, mf, M, +1, &c2, &o2))) return rc;
  hipLaunchKernelGGL(sn_post_kernel, grid(p->half_max, M), dim3(256), 0, s, c2, p->chirp, d_n, p->out, nm, mf, p->half_max);
  hipLaunchKernelGGL(rows_max_kernel, dim3((unsigned)(2 * M)), dim3(1024), 0, s, (const double*)p->out, p->half_max, d_n, nm, d_peak_db);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}
