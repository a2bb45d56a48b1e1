// Filter spectra of convolution plans (alpha/beta planes), fp64 on the device.
// The same arithmetic as host_rfft + host_alpha_beta in impulse_hip.hip (kept there as the debug /
// cross-check path): one packed Nc-point complex FFT per filter, real-FFT unpack, then
//   alpha = (H_k (1+s) + G_k (1-s)) / (2 Nc), beta = i c (H_k - G_k) / (2 Nc),  G_k = conj H[Nc-k],
//   s + i c ... = sin/cos(-pi k / Nc),
// rounded once to fp32 in the row pass's register order.  A 16-filter equalisation plan costs ~8 ms per
// filter on one host core; here the whole batch is a few launches.
#include "fft64_host.hip.h"

namespace {

// z[f][n] = h[f][2n] + i h[f][2n+1], zero beyond M
__global__ __launch_bounds__(256) void pack_filter_kernel(const double* __restrict__ h, cdbl* __restrict__ z, long long M,
                                                          long long ld, int Nc) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= Nc) return;
  const double* row = h + (long long)blockIdx.y * ld;
  const long long i = 2ll * n;
  z[(long long)blockIdx.y * Nc + n] = make_double2(i < M ? row[i] : 0.0, i + 1 < M ? row[i + 1] : 0.0);
}

__device__ __forceinline__ cdbl zconj(cdbl a) { return make_double2(a.x, -a.y); }

// H[k] of the real filter from the packed transform z (k in [0, Nc])
__device__ __forceinline__ cdbl unpack_bin(const cdbl* __restrict__ z, int k, int Nc) {
  const cdbl zk = z[k % Nc];
  const cdbl zm = zconj(z[(Nc - k) % Nc]);
  const cdbl E = make_double2(0.5 * (zk.x + zm.x), 0.5 * (zk.y + zm.y));
  const cdbl d = make_double2(zk.x - zm.x, zk.y - zm.y);
  const cdbl O = make_double2(0.5 * d.y, -0.5 * d.x);                 // -i/2 (zk - zm)
  double sn, cs;
  sincospi(-(double)k / (double)Nc, &sn, &cs);
  const cdbl wO = zmul(make_double2(cs, sn), O);
  return make_double2(E.x + wO.x, E.y + wO.y);
}

__global__ __launch_bounds__(256) void alpha_beta_kernel(const cdbl* __restrict__ zall, float4* __restrict__ ab, int Nc,
                                                         int N1) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;          // position in the plane: k1*4096 + q*256 + u
  if (idx >= Nc) return;
  const cdbl* z = zall + (long long)blockIdx.y * Nc;
  const int k1 = idx >> 12, r = idx & 4095, q = r >> 8, u = r & 255;
  const int k2 = (u >> 4) + 16 * (u & 15) + 256 * q;
  const long long k = (long long)k1 + (long long)N1 * k2;
  const double inv = 1.0 / (double)Nc;
  float4 o;
  if (k == 0) {
    const cdbl z0 = z[0];
    o = make_float4((float)((z0.x + z0.y) * inv), 0.f, (float)((z0.x - z0.y) * inv), 0.f);
  } else {
    const cdbl Hk = unpack_bin(z, (int)k, Nc);
    const cdbl Gk = zconj(unpack_bin(z, Nc - (int)k, Nc));
    double sn, cs;
    sincospi(-(double)k / (double)Nc, &sn, &cs);
    const double a = 0.5 * inv;
    const cdbl alpha = make_double2(a * (Hk.x * (1.0 + sn) + Gk.x * (1.0 - sn)), a * (Hk.y * (1.0 + sn) + Gk.y * (1.0 - sn)));
    const cdbl dd = make_double2(Hk.x - Gk.x, Hk.y - Gk.y);
    const cdbl beta = make_double2(-a * cs * dd.y, a * cs * dd.x);    // i (a c) (Hk - Gk)
    o = make_float4((float)alpha.x, (float)alpha.y, (float)beta.x, (float)beta.y);
  }
  ab[(long long)blockIdx.y * Nc + idx] = o;
}

// pair mode: hs[k1][q*256 + u] = H[k1 + N1 k2] / Nc, k2 = (u >> 4) + 16 (u & 15) + 256 q, over all Nc bins of the
// Nc-point transform of the real filter; z is its packed (Nc / 2)-point transform, H[Nc - k] = conj H[k]
__global__ __launch_bounds__(256) void pair_spectrum_kernel(const cdbl* __restrict__ z, float2* __restrict__ hs, int Nc, int N1) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= Nc) return;
  const int k1 = idx >> 12, r = idx & 4095, q = r >> 8, u = r & 255;
  const int k2 = (u >> 4) + 16 * (u & 15) + 256 * q;
  const long long k = (long long)k1 + (long long)N1 * k2;
  const int half = Nc / 2;
  cdbl H = k <= half ? unpack_bin(z, (int)k, half) : zconj(unpack_bin(z, Nc - (int)k, half));
  const double inv = 1.0 / (double)Nc;
  hs[idx] = make_float2((float)(H.x * inv), (float)(H.y * inv));
}

}  // namespace

void fft_roots_destroy(imp_ctx* ctx) {
  for (auto& kv : ctx->fft_roots) (void)hipFree(kv.second);
  ctx->fft_roots.clear();
}

int spectrum_alpha_beta_device(imp_ctx* ctx, const double* filters, int64_t M, int64_t n_filters, int64_t filter_ld,
                               int64_t Nc, int N1, float4* d_ab, bool filters_on_device) {
  const std::vector<int> fac = factorise((int)Nc);
  if (fac.empty()) return fail(IMP_ERR_UNSUPPORTED, "spectrum length %lld is not 2^a 3^b 5^c 11^d", (long long)Nc);
  hipStream_t s = ctx->stream;
  cdbl* roots = nullptr;
  int rc = ctx_fft_roots(ctx, Nc, &roots);
  if (rc) return rc;
  const int64_t chunk = fft_chunk(n_filters, Nc, (int64_t)64 << 20);     // filters go through in chunks
  cdbl *a = nullptr, *b = nullptr;
  double* d_h = nullptr;
  auto cleanup = [&](int code) {
    (void)hipStreamSynchronize(s);
    (void)ctx_block_put(ctx, a);
    (void)ctx_block_put(ctx, b);
    (void)ctx_block_put(ctx, d_h);
    return code;
  };
  // (filters already on the device are read where they are and nothing below waits: the blocks go back to the pool in
  // stream order)
  auto cleanup_async = [&](int code) {
    (void)ctx_block_put(ctx, a);
    (void)ctx_block_put(ctx, b);
    return code;
  };
  if (ctx_block_get(ctx, (size_t)chunk * Nc * sizeof(cdbl), (void**)&a) ||
      ctx_block_get(ctx, (size_t)chunk * Nc * sizeof(cdbl), (void**)&b) ||
      (!filters_on_device && ctx_block_get(ctx, (size_t)chunk * M * sizeof(double), (void**)&d_h)))
    return cleanup(fail(IMP_ERR_ALLOC, "device buffers for the filter spectra (%lld filters of %lld points)",
                        (long long)chunk, (long long)Nc));
  for (int64_t f0 = 0; f0 < n_filters; f0 += chunk) {
    const int64_t nf = std::min(chunk, n_filters - f0);
    if (!filters_on_device &&
        hipMemcpy2DAsync(d_h, (size_t)M * sizeof(double), filters + f0 * filter_ld, (size_t)filter_ld * sizeof(double),
                         (size_t)M * sizeof(double), (size_t)nf, hipMemcpyHostToDevice, s) != hipSuccess)
      return cleanup(fail(IMP_ERR_HIP, "filter upload failed"));
    const dim3 grid((unsigned)((Nc + 255) / 256), (unsigned)nf);
    if (filters_on_device)
      hipLaunchKernelGGL(pack_filter_kernel, grid, dim3(256), 0, s, filters + f0 * filter_ld, a, (long long)M, (long long)filter_ld, (int)Nc);
    else
      hipLaunchKernelGGL(pack_filter_kernel, grid, dim3(256), 0, s, (const double*)d_h, a, (long long)M, (long long)M, (int)Nc);
    cdbl *cur = a, *oth = b;
    if ((rc = run_fft(ctx, fac, roots, (int)Nc, nf, -1, &cur, &oth))) return cleanup(rc);
    hipLaunchKernelGGL(alpha_beta_kernel, grid, dim3(256), 0, s, cur, d_ab + f0 * Nc, (int)Nc, N1);
    if (hipGetLastError() != hipSuccess) return cleanup(fail(IMP_ERR_HIP, "alpha/beta launch failed"));
    // the host rows of this chunk may be reused by the caller after return: drain before the next upload
    if (!filters_on_device && hipStreamSynchronize(s) != hipSuccess) return cleanup(fail(IMP_ERR_HIP, "filter spectrum: stream error"));
  }
  return filters_on_device ? cleanup_async(IMP_OK) : cleanup(IMP_OK);
}

int spectrum_pair_device(imp_ctx* ctx, const double* filter, int64_t M, int64_t Nc, int N1, cf* d_hs) {
  if (Nc % 2) return fail(IMP_ERR_UNSUPPORTED, "pair spectrum: odd circular length %lld", (long long)Nc);
  const int64_t half = Nc / 2;
  const std::vector<int> fac = factorise((int)half);
  if (fac.empty()) return fail(IMP_ERR_UNSUPPORTED, "spectrum length %lld is not 2^a 3^b 5^c 11^d", (long long)half);
  if (M > Nc) return fail(IMP_ERR_INVALID, "filter of %lld taps longer than the circular length %lld", (long long)M, (long long)Nc);
  hipStream_t s = ctx->stream;
  cdbl* roots = nullptr;
  int rc = ctx_fft_roots(ctx, half, &roots);
  if (rc) return rc;
  cdbl *a = nullptr, *b = nullptr;
  double* d_h = nullptr;
  auto cleanup = [&](int code) {
    (void)hipStreamSynchronize(s);
    (void)ctx_block_put(ctx, a);
    (void)ctx_block_put(ctx, b);
    (void)ctx_block_put(ctx, d_h);
    return code;
  };
  if (ctx_block_get(ctx, (size_t)half * sizeof(cdbl), (void**)&a) || ctx_block_get(ctx, (size_t)half * sizeof(cdbl), (void**)&b) ||
      ctx_block_get(ctx, (size_t)M * sizeof(double), (void**)&d_h))
    return cleanup(fail(IMP_ERR_ALLOC, "device buffers for the pair spectrum (%lld points)", (long long)Nc));
  if (hipMemcpyAsync(d_h, filter, (size_t)M * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
    return cleanup(fail(IMP_ERR_HIP, "filter upload failed"));
  hipLaunchKernelGGL(pack_filter_kernel, dim3((unsigned)((half + 255) / 256), 1), dim3(256), 0, s, d_h, a, (long long)M,
                     (long long)M, (int)half);
  cdbl *cur = a, *oth = b;
  if ((rc = run_fft(ctx, fac, roots, (int)half, 1, -1, &cur, &oth))) return cleanup(rc);
  hipLaunchKernelGGL(pair_spectrum_kernel, dim3((unsigned)((Nc + 255) / 256)), dim3(256), 0, s, cur,
                     reinterpret_cast<float2*>(d_hs), (int)Nc, N1);
  if (hipGetLastError() != hipSuccess) return cleanup(fail(IMP_ERR_HIP, "pair spectrum launch failed"));
  return cleanup(IMP_OK);
}
