// Host driver of the batched fp64 transform that K6, K2, the filter spectra, K15 and K16 share: the tile transform of
// fft64.hip.h in one or two launches (run_fft_ops), and a Stockham autosort transform with one launch per radix pass through
// global memory (radix 8/4/2/3/5/7/11, generic O(R^2) butterflies with exact table twiddles) for lengths the tiles do not
// hold and as their cross-check (IMPULSE_HIP_FFT64_GENERIC=1).
//
// Everything here is static or in an anonymous namespace: every translation unit that includes the header gets its own
// copies, which is how the load / store hooks of a stage are instantiated next to the stage that defines them.
//
// Two sources of roots, which may differ in the last place and are kept apart: host cos / sin (upload_roots: K6, K2 and the
// slice's K2, whose goldens and bit identities sit on them) and device sincospi cached per context (ctx_fft_roots: the
// filter spectra, K15, K16).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <utility>

#include "internal.h"
#include "fft64.hip.h"

typedef double2 cdbl;

namespace {

__device__ __forceinline__ cdbl zmul(cdbl a, cdbl b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// One Stockham pass of radix R over `batch` transforms of length N (blockIdx.y = transform).
//   n = current sub-transform length, s = N / n interleaved sub-transforms, m = n / R
//   a_k = x[q + s (p + k m)] ; b_j = sum_k a_k w_R^(j k) ; y[q + s (R p + j)] = b_j w_n^(p j)
// roots[k] = exp(-2 pi i k / N); dir = +1 uses the conjugates.
template <int R>
__global__ __launch_bounds__(256) void stockham_pass(const cdbl* __restrict__ x, cdbl* __restrict__ y,
                                                     const cdbl* __restrict__ roots, int N, int n, int s, int dir) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = n / R;
  if (i >= s * m) return;
  const int q = i % s, p = i / s;
  const long long base = (long long)blockIdx.y * N;
  cdbl a[R];
#pragma unroll
  for (int k = 0; k < R; ++k) a[k] = x[base + q + (long long)s * (p + k * m)];
  const int step_r = N / R;        // w_R = roots[step_r]
  const int step_n = N / n;        // w_n = roots[step_n]
  cdbl wr[R];                      // the R-th roots once per thread; (j k) % R is a compile-time index below
#pragma unroll
  for (int k = 0; k < R; ++k) {
    wr[k] = roots[k * step_r];
    if (dir > 0) wr[k].y = -wr[k].y;
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    cdbl acc = a[0];
#pragma unroll
    for (int k = 1; k < R; ++k) {
      const cdbl w = wr[(j * k) % R];
      const cdbl t = zmul(a[k], w);
      acc.x += t.x;
      acc.y += t.y;
    }
    cdbl tw = roots[(int)(((long long)p * j * step_n) % N)];
    if (dir > 0) tw.y = -tw.y;
    y[base + q + (long long)s * (R * p + j)] = zmul(acc, tw);
  }
}

// roots[k] = exp(-2 pi i k / N) on the device (ctx_fft_roots)
__global__ __launch_bounds__(256) void roots_kernel(cdbl* __restrict__ roots, int N) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= N) return;
  double sn, cs;
  sincospi(-2.0 * (double)k / (double)N, &sn, &cs);
  roots[k] = make_double2(cs, sn);
}

// The radix passes of an n-point transform, empty when n is not 2^a 3^b 5^c 11^d (seven: 7^e as well, what
// scipy.fft.next_fast_len gives K15).
std::vector<int> factorise(int n, bool seven = false) {
  std::vector<int> f;
  // Every pass is one launch at the launch floor (~6 us at these sizes): radix 8 passes shorten the power-of-two part
  // (78 VGPRs; the O(R^2) butterfly of radix 16 needs 256 at occupancy 1 and gained nothing: whole slice, radix 4 / 8 / 16:
  // 3.47 / 3.38 / 3.45 ms, so it is no longer built).  Two-level butterflies (16 = 4 x 4, 25 = 5 x 5 inside the thread,
  // 126 / 155 VGPRs) were tried in round 3: 34 passes per slice instead of 47, and the same 300 us - 9.4 us per radix-16 pass
  // against 6 - 7 us per radix-8 pass.  IMPULSE_HIP_FFT_MAX_RADIX below 8 (2, 4) keeps radix 8 out; 8 and above act as 8.
  static const int max_radix = [] {
    const char* e = std::getenv("IMPULSE_HIP_FFT_MAX_RADIX");
    return e ? std::atoi(e) : 8;
  }();
  for (int r : {8, 4, 2, 3, 5, 7, 11}) {                   // 11: 66-row convolution plans (filter spectrum preparation)
    if ((r == 8 && max_radix < 8) || (r == 7 && !seven)) continue;
    while (n % r == 0) { f.push_back(r); n /= r; }
  }
  if (n != 1) f.clear();
  return f;
}

// n = 2^a 3^b 5^c 7^d 11^e: the lengths scipy.fft.next_fast_len returns
bool smooth_11(int64_t n) {
  if (n < 1) return false;
  for (int64_t p : {2, 3, 5, 7, 11})
    while (n % p == 0) n /= p;
  return n == 1;
}

// Transforms of `points` points that go through one pair of ping-pong buffers at a time: at most `bytes` per buffer, at
// least one, at most `want`
int64_t fft_chunk(int64_t want, int64_t points, int64_t bytes = (int64_t)128 << 20) {
  return std::max<int64_t>(1, std::min<int64_t>(want, bytes / (points * (int64_t)sizeof(cdbl))));
}

}  // namespace

// roots from host cos / sin, in a block of their own (the caller frees it)
static int upload_roots(cdbl** dptr, int N, hipStream_t s) {
  std::vector<cdbl> h((size_t)N);
  for (int k = 0; k < N; ++k) {
    const double ang = -2.0 * M_PI * (double)k / (double)N;
    h[(size_t)k] = make_double2(std::cos(ang), std::sin(ang));
  }
  HIP_TRY(hipMalloc((void**)dptr, (size_t)N * sizeof(cdbl)));
  HIP_TRY(hipMemcpyAsync(*dptr, h.data(), (size_t)N * sizeof(cdbl), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return IMP_OK;
}

// roots from device sincospi, made once per context and length (fft_roots_destroy frees them); stream ordered, no wait
static int ctx_fft_roots(imp_ctx* ctx, int64_t N, cdbl** roots) {
  auto it = ctx->fft_roots.find((long long)N);
  if (it != ctx->fft_roots.end()) {
    *roots = (cdbl*)it->second;
    return IMP_OK;
  }
  HIP_TRY(hipMalloc((void**)roots, (size_t)N * sizeof(cdbl)));
  hipLaunchKernelGGL(roots_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, *roots, (int)N);
  HIP_TRY(hipGetLastError());
  ctx->fft_roots[(long long)N] = *roots;
  return IMP_OK;
}

// one launch per radix pass through global memory
static int run_fft_passes(imp_ctx* ctx, const std::vector<int>& fac, const cdbl* roots, int N, int64_t B, int dir, cdbl** cur,
                          cdbl** other) {
  int n = N, s = 1;
  for (int r : fac) {
    const int threads = N / r;
    dim3 grid((unsigned)((threads + 255) / 256), (unsigned)B), block(256);
    switch (r) {
      case 8: hipLaunchKernelGGL(stockham_pass<8>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      case 4: hipLaunchKernelGGL(stockham_pass<4>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      case 2: hipLaunchKernelGGL(stockham_pass<2>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      case 3: hipLaunchKernelGGL(stockham_pass<3>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      case 5: hipLaunchKernelGGL(stockham_pass<5>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      case 7: hipLaunchKernelGGL(stockham_pass<7>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      case 11: hipLaunchKernelGGL(stockham_pass<11>, grid, block, 0, ctx->stream, *cur, *other, roots, N, n, s, dir); break;
      default: return fail(IMP_ERR_UNSUPPORTED, "radix %d", r);
    }
    HIP_TRY(hipGetLastError());
    std::swap(*cur, *other);
    n /= r;
    s *= r;
  }
  return IMP_OK;
}

// one pass of the tile transform (fft64.hip.h)
template <int T, class InOp, class OutOp>
static int fft64_launch(imp_ctx* ctx, const fft64::Args& a, InOp in_op, OutOp out_op) {
  auto kern = fft64::tile_kernel<T, InOp, OutOp>;
  const size_t lds = fft64::tile_lds(a.P, T);
  int rc = ctx_kernel_lds(ctx, reinterpret_cast<const void*>(kern), (size_t)160 * 1024);
  if (rc) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((a.n_groups + T - 1) / T)), dim3(256), lds, ctx->stream, a, in_op, out_op);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

template <class InOp, class OutOp>
static int fft64_pass(imp_ctx* ctx, fft64::Args a, int64_t B, InOp in_op, OutOp out_op) {
  a.n_groups = (long long)B * a.nvec;
  if ((double)a.n_groups * (double)a.nvec >= 4294967296.0)
    return fail(IMP_ERR_UNSUPPORTED, "fp64 transform batch of %lld vectors: beyond the kernel's 32-bit index arithmetic", (long long)a.n_groups);
  a.m_nvec = fft64::magic_of((unsigned)a.nvec);
  for (int st = 0, blk = a.P; st < a.nstages; ++st) {
    blk /= a.radix[st];
    a.m_blk[st] = fft64::magic_of((unsigned)blk);
  }
  switch (fft64::tile_vectors(a.P, a.n_groups)) {
    case 16: return fft64_launch<16>(ctx, a, in_op, out_op);
    case 8: return fft64_launch<8>(ctx, a, in_op, out_op);
    default: return fft64_launch<4>(ctx, a, in_op, out_op);
  }
}

static bool fft64_wanted() {
  static const bool generic = [] { const char* e = std::getenv("IMPULSE_HIP_FFT64_GENERIC"); return e && e[0] == '1'; }();
  return !generic;
}

// Batched N-point transforms of B rows ([B][N], roots = exp(-2 pi i k / N)): the tile transform in one or two launches
// where N splits into factors it holds (every length of the path does), else one launch per radix pass.  The result ends
// in *cur.  in_op is applied to every value read from *cur, out_op to every value of the result (elementwise hooks, so
// that the kernels between two transforms need no launch and no pass over memory of their own).
// tiles_required: for a load hook that SUPPLIES the input (nothing has been written to *cur): IMPULSE_HIP_FFT64_GENERIC is
// not consulted, and a length without a tile plan is IMP_ERR_UNSUPPORTED - never the radix passes, which know no hooks.
template <class InOp, class OutOp>
static int run_fft_ops(imp_ctx* ctx, const std::vector<int>& fac, const cdbl* roots, int N, int64_t B, int dir, cdbl** cur,
                       cdbl** other, InOp in_op, OutOp out_op, bool* used_tiles = nullptr, int64_t in_pitch = 0, bool seven = false,
                       bool tiles_required = false) {
  const fft64::Plan pl = tiles_required || fft64_wanted() ? fft64::make_plan(N, seven) : fft64::Plan();
  if (used_tiles) *used_tiles = pl.ok;
  if (!pl.ok && tiles_required) return fail(IMP_ERR_UNSUPPORTED, "transform length %d has no tile plan", N);
  if (!pl.ok) return run_fft_passes(ctx, fac, roots, N, B, dir, cur, other);
  fft64::Args a = {};
  a.roots = roots;
  a.n_roots = N;
  a.dir = dir;
  a.in_batch = in_pitch > 0 ? in_pitch : N;              // rows of the input may be further apart than N (hooks that read a
  a.out_batch = N;                                       // longer buffer: the FIR design's window step)
  int rc;
  if (pl.P2 == 1) {
    a.in = *cur;
    a.out = *other;
    a.nvec = 1;
    a.P = N;
    a.in_vec = a.out_vec = N;
    a.in_elem = a.out_elem = 1;
    a.twiddle = 0;
    a.nstages = (int)pl.r1.size();
    for (int i = 0; i < a.nstages; ++i) a.radix[i] = pl.r1[(size_t)i];
    if ((rc = fft64_pass(ctx, a, B, in_op, out_op))) return rc;
    std::swap(*cur, *other);
    return IMP_OK;
  }
  // pass 1: the P2 columns, P1 points each, x w_N^(n2 k1) -> Y[k1][n2]
  a.in = *cur;
  a.out = *other;
  a.nvec = pl.P2;
  a.P = pl.P1;
  a.in_vec = 1;
  a.in_elem = pl.P2;
  a.out_vec = 1;
  a.out_elem = pl.P2;
  a.twiddle = 1;
  a.nstages = (int)pl.r1.size();
  for (int i = 0; i < a.nstages; ++i) a.radix[i] = pl.r1[(size_t)i];
  if ((rc = fft64_pass(ctx, a, B, in_op, fft64::NoOp{}))) return rc;
  // pass 2: the P1 rows of Y, P2 points each -> X[k1 + P1 k2]
  a.in = *other;
  a.out = *cur;
  a.in_batch = N;
  a.nvec = pl.P1;
  a.P = pl.P2;
  a.in_vec = pl.P2;
  a.in_elem = 1;
  a.out_vec = 1;
  a.out_elem = pl.P1;
  a.twiddle = 0;
  a.nstages = (int)pl.r2.size();
  for (int i = 0; i < a.nstages; ++i) a.radix[i] = pl.r2[(size_t)i];
  return fft64_pass(ctx, a, B, fft64::NoOp{}, out_op);
}

// batched FFT: result ends in *cur (either buf0 or buf1)
static int run_fft(imp_ctx* ctx, const std::vector<int>& fac, const cdbl* roots, int N, int64_t B, int dir, cdbl** cur,
                   cdbl** other) {
  return run_fft_ops(ctx, fac, roots, N, B, dir, cur, other, fft64::NoOp{}, fft64::NoOp{});
}
