// K17: rational resampling of finished rows (resample_kernels.hip.h), the --fs stage of the reference
// (core/pipeline.py:851-863 -> core/hrir.py:890-919 -> core/impulse_response.py:121-124): the polyphase arithmetic of
// scipy.signal.resample_poly with the filter handed in.  Like K14-K16 the entry exists twice: device-resident fp32 rows, and
// fp64 host rows that are uploaded as they are (ragged_rows.h).  The taps are a host table in both; they go to the device
// once per call, re-laid phase-major, through the staging ring next to the row table.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

#include "ragged_rows.h"
#include "resample_kernels.hip.h"

namespace {

constexpr int64_t kRsMaxTaps = 65536;
constexpr int64_t kRsMaxIndex = (int64_t)1 << 62;      // len up + down + L stays below this: every index fits 63 bits

// ceil(n up / down), or -1 where n up (+ down + L) leaves the index range
int64_t rs_len(int64_t n, int64_t up, int64_t down, int64_t L) {
  const __int128 top = (__int128)n * up + down + L;
  if (top >= (__int128)kRsMaxIndex) return -1;
  return (int64_t)(((__int128)n * up + down - 1) / down);
}

// tile and chunk of (up, down, L), both reduced: the staged span (k0 of the tile's last output - k0 of its first) + chunk is
// at most floor((tile - 1) down / up) + 1 + chunk <= kRsSpan
imp::RsPlan rs_plan(int64_t up, int64_t down, int64_t L) {
  imp::RsPlan p;
  p.up = up;
  p.down = down;
  p.half = (L - 1) / 2;
  p.nph = (L + up - 1) / up;
  p.phases = std::min(up, L);
  auto tspan = [&](int64_t tile) { return (int64_t)(((__int128)(tile - 1) * down) / up) + 2; };
  int64_t tile = imp::kRsThreads;
  const __int128 wide = ((__int128)(tile - 1) * down) / up + 2;
  if (wide > imp::kRsSpan / 2)
    tile = std::min<int64_t>(imp::kRsThreads, 1 + (int64_t)(((__int128)(imp::kRsSpan / 2 - 2) * up) / down));
  p.tile = (int)tile;
  p.chunk = (int)std::min<int64_t>(p.nph, imp::kRsSpan - tspan(tile));
  p.uniform = up <= 2 && tile == imp::kRsThreads;
  return p;
}

// what both entries refuse, with the reason; *sp = what the rows span, n_out[b] = the result's length
int rs_check(const char* who, const void* x, const int64_t* off, const int64_t* len, int64_t B, int64_t up, int64_t down,
             const double* taps, int64_t L, const void* out, const int64_t* out_off, RowSpan* sp, std::vector<int64_t>& n_out) {
  if (up <= 0 || down <= 0) return fail(IMP_ERR_INVALID, "%s: up = %lld, down = %lld (need both positive)", who, (long long)up, (long long)down);
  if (L < 1 || !taps) return fail(IMP_ERR_INVALID, "%s: a filter of %lld taps (need at least 1, and the table)", who, (long long)L);
  if (L > kRsMaxTaps) return fail(IMP_ERR_UNSUPPORTED, "%s: a filter of %lld taps (limit %lld)", who, (long long)L, (long long)kRsMaxTaps);
  if (B > 65535) return fail(IMP_ERR_UNSUPPORTED, "%s: B = %lld rows (limit 65535)", who, (long long)B);
  int rc = rows_check(who, off, len, B, kAnyLen, sp);
  if (rc) return rc;
  if (B > 0 && !out_off) return fail(IMP_ERR_INVALID, "%s: null output table", who);
  const int64_t g = std::gcd(up, down);
  n_out.assign((size_t)B, 0);
  int64_t total = 0;
  for (int64_t b = 0; b < B; ++b) {
    if (out_off[b] < 0) return fail(IMP_ERR_INVALID, "%s: negative output offset in row %lld", who, (long long)b);
    const int64_t n = rs_len(len[b], up / g, down / g, L);
    if (n < 0)
      return fail(IMP_ERR_UNSUPPORTED, "%s: row %lld of %lld samples times up = %lld does not fit 63 bits", who, (long long)b,
                  (long long)len[b], (long long)(up / g));
    n_out[(size_t)b] = n;
    total += n;
  }
  if ((sp->extent > 0 && !x) || (total > 0 && !out)) return fail(IMP_ERR_INVALID, "%s: null rows or output", who);
  return IMP_OK;
}

// One launch for all rows: d_x rows in, d_out + dst[b] rows out.  Nothing here waits.
template <class T, class O>
int rs_launch(imp_ctx* ctx, const char* who, const T* d_x, const int64_t* off, const int64_t* len, int64_t B, int64_t up,
              int64_t down, const double* taps, int64_t L, const std::vector<int64_t>& n_out, const int64_t* dst, O* d_out) {
  const int64_t g = std::gcd(up, down);
  up /= g;
  down /= g;
  const double one = 1.0;
  if (up == down) {                                                      // scipy: a copy of the row
    taps = &one;
    L = 1;
  }
  const imp::RsPlan pl = rs_plan(up, down, L);
  std::vector<imp::RsRow> rows((size_t)B);
  int64_t longest = 0;
  for (int64_t b = 0; b < B; ++b) {
    rows[(size_t)b] = {off[b], len[b], n_out[(size_t)b], dst[b]};
    longest = std::max(longest, n_out[(size_t)b]);
  }
  if (longest == 0) return IMP_OK;
  if ((longest + pl.tile - 1) / pl.tile > (int64_t)0x7fffffff)
    return fail(IMP_ERR_UNSUPPORTED, "%s: a result of %lld samples is more than one launch holds", who, (long long)longest);
  std::vector<double> ph((size_t)(pl.phases * pl.nph), 0.0);              // phase p: taps[p], taps[p + up], ... and zeros
  for (int64_t p = 0; p < pl.phases; ++p)
    for (int64_t i = 0, j = p; j < L; ++i, j += up) ph[(size_t)(p * pl.nph + i)] = taps[j];
  void* tab[2];
  int rc = ctx_stage_tables(ctx, {{rows.data(), rows.size() * sizeof(imp::RsRow)}, {ph.data(), ph.size() * sizeof(double)}}, tab);
  if (rc) return rc;
  const dim3 grid((unsigned)((longest + pl.tile - 1) / pl.tile), (unsigned)B);
  if (pl.uniform)
    hipLaunchKernelGGL((imp::resample_poly_kernel<T, O, true>), grid, dim3(imp::kRsThreads), 0, ctx->stream, d_x,
                       (const imp::RsRow*)tab[0], (const double*)tab[1], pl, d_out);
  else
    hipLaunchKernelGGL((imp::resample_poly_kernel<T, O, false>), grid, dim3(imp::kRsThreads), 0, ctx->stream, d_x,
                       (const imp::RsRow*)tab[0], (const double*)tab[1], pl, d_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(IMP_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(e));
  return IMP_OK;
}

}  // namespace

extern "C" int imp_resample_poly_len(int64_t n_in, int64_t up, int64_t down, int64_t* n_out) {
  if (!n_out) return fail(IMP_ERR_INVALID, "imp_resample_poly_len: null output");
  if (up <= 0 || down <= 0 || n_in < 0)
    return fail(IMP_ERR_INVALID, "imp_resample_poly_len: n_in = %lld, up = %lld, down = %lld (need n_in >= 0 and both factors positive)",
                (long long)n_in, (long long)up, (long long)down);
  const int64_t g = std::gcd(up, down);
  const int64_t n = rs_len(n_in, up / g, down / g, 0);
  if (n < 0)
    return fail(IMP_ERR_UNSUPPORTED, "imp_resample_poly_len: %lld samples times up = %lld does not fit 63 bits", (long long)n_in,
                (long long)(up / g));
  *n_out = n;
  return IMP_OK;
}

extern "C" int imp_resample_poly_device(imp_ctx* ctx, const float* d_x, const int64_t* off, const int64_t* len, int64_t B, int64_t up,
                                        int64_t down, const double* taps, int64_t L, float* d_dst, const int64_t* dst_off) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_resample_poly_device: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  std::vector<int64_t> n_out;
  int rc = rs_check("imp_resample_poly_device", d_x, off, len, B, up, down, taps, L, d_dst, dst_off, &sp, n_out);
  if (rc || B == 0 || (rc = ctx_bind(ctx))) return rc;
  return rs_launch<float, float>(ctx, "imp_resample_poly_device", d_x, off, len, B, up, down, taps, L, n_out, dst_off, d_dst);
}

// fp64 host rows: uploaded as they are, then the same kernel on Sample = Out = double
extern "C" int imp_resample_poly(imp_ctx* ctx, const double* x, const int64_t* off, const int64_t* len, int64_t B, int64_t up,
                                 int64_t down, const double* taps, int64_t L, double* out, const int64_t* out_off) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_resample_poly: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  std::vector<int64_t> n_out;
  int rc = rs_check("imp_resample_poly", x, off, len, B, up, down, taps, L, out, out_off, &sp, n_out);
  if (rc || B == 0 || (rc = ctx_bind(ctx))) return rc;
  std::vector<int64_t> pos((size_t)B);                                   // the results packed on the device
  int64_t total = 0;
  for (int64_t b = 0; b < B; ++b) {
    pos[(size_t)b] = total;
    total += n_out[(size_t)b];
  }
  if (total == 0) return IMP_OK;
  BlockHold rows(ctx), res(ctx);
  if ((rc = upload_rows(ctx, "imp_resample_poly", x, sp.extent, rows)) || (rc = res.get((size_t)total * sizeof(double)))) return rc;
  if ((rc = rs_launch<double, double>(ctx, "imp_resample_poly", (const double*)rows.p, off, len, B, up, down, taps, L, n_out,
                                      pos.data(), (double*)res.p)))
    return rc;
  std::vector<double> packed((size_t)total);
  const hipError_t e = hipMemcpyAsync(packed.data(), res.p, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return fail(IMP_ERR_HIP, "imp_resample_poly: %s", hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(IMP_ERR_HIP, "imp_resample_poly: %s", hipGetErrorString(e2));
  for (int64_t b = 0; b < B; ++b)
    if (n_out[(size_t)b]) std::memcpy(out + out_off[b], packed.data() + pos[(size_t)b], (size_t)n_out[(size_t)b] * sizeof(double));
  return IMP_OK;
}
