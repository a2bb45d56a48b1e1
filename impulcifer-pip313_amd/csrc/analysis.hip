// Analysis stages on finished rows, each next to the fp64 transform it takes (fft64_host.hip.h):
//   K14  microphone-deviation analysis   micdev_kernels.hip.h
//   K15  binaural analysis metrics       analysis_kernels.hip.h   band cross-spectra through PairIn, IACF, energy decay
//   K16  short-time spectra              stft_kernels.hip.h       spectrogram / waterfall data through StftIn
// Every entry exists twice: device-resident fp32 rows, and fp64 host rows that are uploaded as they are (ragged_rows.h).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "fft64_host.hip.h"
#include "ragged_rows.h"
#include "block_scan.hip.h"
// The kernel headers below are compiled with fp contraction off, as they were after decay_kernels.hip.h in impulse_hip.hip;
// the transform and the scan above them with contraction on, as everywhere else.
#pragma clang fp contract(off)
#include "micdev_kernels.hip.h"
#include "analysis_kernels.hip.h"
#include "stft_kernels.hip.h"

// ------------------------------------------------------------------------------------------------
// K14 microphone-deviation analysis: direct-sound power on the log grid, interaural mismatch per group
// ------------------------------------------------------------------------------------------------
// scipy.fft.next_fast_len(n) (real=False): the smallest 2^a 3^b 5^c 7^d 11^e >= n
static int64_t next_fast_len_11(int64_t n) {
  int64_t m = n < 1 ? 1 : n;
  while (!smooth_11(m)) ++m;
  return m;
}

// the bins np.interp(grid, rfftfreq(nfft, 1 / fs), mag, left=mag[0], right=mag[-1]) reads, and its brackets
static void mic_tables(int64_t nfft, double fs, const double* grid, int64_t M, std::vector<long long>& bins,
                       std::vector<imp::MicInterp>& interp) {
  const int64_t nxp = nfft / 2 + 1;
  const double val = 1.0 / ((double)nfft * (1.0 / fs));            // rfftfreq: k * (1 / (n d))
  auto xp = [&](int64_t k) { return (double)k * val; };
  std::vector<int64_t> lo((size_t)M), hi((size_t)M);
  std::vector<int> lerp((size_t)M, 0);
  std::vector<double> xd((size_t)M, 0.0), dd((size_t)M, 1.0);
  std::vector<int64_t> used;
  for (int64_t g = 0; g < M; ++g) {
    const double x = grid[g];
    int64_t j;                                                       // binary_search_with_guess: xp[j] <= x < xp[j + 1]
    if (x < xp(0)) j = -1;
    else if (x > xp(nxp - 1)) j = nxp;
    else {
      j = std::min<int64_t>(std::max<int64_t>((int64_t)std::floor(x / val), 0), nxp - 1);
      while (j > 0 && xp(j) > x) --j;
      while (j + 1 < nxp && xp(j + 1) <= x) ++j;
    }
    int64_t a = j, b = j;
    if (j < 0) a = b = 0;
    else if (j >= nxp - 1) a = b = nxp - 1;                          // right value, or the last bin itself
    else if (xp(j) != x) {
      b = j + 1;
      lerp[(size_t)g] = 1;
      xd[(size_t)g] = x - xp(j);
      dd[(size_t)g] = xp(j + 1) - xp(j);
    }
    lo[(size_t)g] = a;
    hi[(size_t)g] = b;
    used.push_back(a);
    used.push_back(b);
  }
  std::sort(used.begin(), used.end());
  used.erase(std::unique(used.begin(), used.end()), used.end());
  bins.assign(used.begin(), used.end());
  interp.resize((size_t)M);
  for (int64_t g = 0; g < M; ++g) {
    imp::MicInterp& e = interp[(size_t)g];
    e.ia = (int)(std::lower_bound(used.begin(), used.end(), lo[(size_t)g]) - used.begin());
    e.ib = (int)(std::lower_bound(used.begin(), used.end(), hi[(size_t)g]) - used.begin());
    e.lerp = lerp[(size_t)g];
    e.pad = 0;
    e.xd = xd[(size_t)g];
    e.dd = dd[(size_t)g];
  }
}

template <class T>
static int mic_mismatch_impl(imp_ctx* ctx, const char* who, const T* d_x, const int64_t* off, const int64_t* len,
                             const int64_t* peak, const int32_t* group, const int32_t* side, const int32_t* anchor, int64_t B,
                             int64_t G, int64_t win, int64_t pre, double fs, const double* grid, int64_t M, double* raw_out,
                             double* power_out) {
  // rows: the reference's segment and fades; one table set per distinct nfft
  std::vector<imp::MicRow> rows((size_t)B);
  std::map<int64_t, size_t> set_of;                                  // nfft -> set
  std::vector<std::vector<long long>> set_bins;
  std::vector<std::vector<imp::MicInterp>> set_interp;
  for (int64_t b = 0; b < B; ++b) {
    imp::MicRow& r = rows[(size_t)b];
    const int64_t n = len[b];
    const int64_t pk = std::min<int64_t>(std::max<int64_t>(peak[b], 0), std::max<int64_t>(n - 1, 0));   // np.clip(peak, 0, n - 1)
    const int64_t start = std::max<int64_t>(pk - pre, 0), end = std::min<int64_t>(pk + win, n);
    const int64_t L = n > 0 ? std::max<int64_t>(end - start, 0) : 0;
    r.off = off[b];
    r.start = start;
    r.L = L;
    r.fade_in = std::min<int64_t>(pre, L / 4);
    r.fade_out = std::max<int64_t>(L / 4, 1);
    r.nfft = next_fast_len_11(std::max<int64_t>(L, 8192));
    r.group = group[b];
    r.side = side[b];
    r.anchor = anchor[b] != 0;
    r.pad = 0;
    if (L >= imp::kMicMinSeg && !set_of.count(r.nfft)) {
      set_of[r.nfft] = set_bins.size();
      set_bins.emplace_back();
      set_interp.emplace_back();
      mic_tables(r.nfft, fs, grid, M, set_bins.back(), set_interp.back());
    }
  }
  std::vector<long long> bin_off(set_bins.size());
  int64_t n_bins = 0, pitch = 1;
  for (size_t s = 0; s < set_bins.size(); ++s) {
    bin_off[s] = n_bins;
    n_bins += (int64_t)set_bins[s].size();
    pitch = std::max<int64_t>(pitch, (int64_t)set_bins[s].size());
  }
  int64_t max_nb = 0;
  for (auto& r : rows) {
    if (r.L >= imp::kMicMinSeg) {
      const size_t s = set_of[r.nfft];
      r.bin_off = bin_off[s];
      r.nb = (int64_t)set_bins[s].size();
      r.interp_off = (long long)s * M;
    } else {
      r.bin_off = r.nb = r.interp_off = 0;
    }
    max_nb = std::max<int64_t>(max_nb, r.nb);
  }
  // staged tables: rows | bins | interp (each 256-byte aligned)
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t rows_b = up((size_t)B * sizeof(imp::MicRow)), bins_b = up((size_t)std::max<int64_t>(n_bins, 1) * sizeof(long long));
  const size_t interp_b = up(std::max<size_t>(set_bins.size(), 1) * (size_t)M * sizeof(imp::MicInterp));
  char *h_tab = nullptr, *d_tab = nullptr;
  int rc = ctx_stage(ctx, rows_b + bins_b + interp_b, (void**)&h_tab, (void**)&d_tab);
  if (rc) return rc;
  std::memcpy(h_tab, rows.data(), (size_t)B * sizeof(imp::MicRow));
  for (size_t s = 0; s < set_bins.size(); ++s) {
    std::memcpy(h_tab + rows_b + (size_t)bin_off[s] * sizeof(long long), set_bins[s].data(), set_bins[s].size() * sizeof(long long));
    std::memcpy(h_tab + rows_b + bins_b + s * (size_t)M * sizeof(imp::MicInterp), set_interp[s].data(),
                (size_t)M * sizeof(imp::MicInterp));
  }
  if ((rc = ctx_stage_push(ctx, h_tab, d_tab, rows_b + bins_b + interp_b))) return rc;
  const imp::MicRow* d_rows = (const imp::MicRow*)d_tab;
  const long long* d_bins = (const long long*)(d_tab + rows_b);
  const imp::MicInterp* d_interp = (const imp::MicInterp*)(d_tab + rows_b + bins_b);
  // work: mag [B][pitch] | power [B][M] | raw [G][M]
  const size_t mag_n = (size_t)B * (size_t)pitch, pow_n = (size_t)B * (size_t)M, raw_n = (size_t)G * (size_t)M;
  BlockHold work(ctx);
  if ((rc = work.get((mag_n + pow_n + raw_n) * sizeof(double)))) return rc;
  double *d_mag = (double*)work.p, *d_pow = d_mag + mag_n, *d_raw = d_pow + pow_n;
  hipStream_t s = ctx->stream;
  const unsigned mblocks = (unsigned)((M + imp::kMicThreads - 1) / imp::kMicThreads);
  hipError_t e = hipSuccess;
  if (max_nb > 0) {
    hipLaunchKernelGGL(imp::micdev_mag_kernel<T>, dim3((unsigned)((max_nb + imp::kMicThreads - 1) / imp::kMicThreads), (unsigned)B),
                       dim3(imp::kMicThreads), 0, s, d_x, d_rows, d_bins, d_mag, (long long)pitch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(imp::micdev_power_kernel, dim3(mblocks, (unsigned)B), dim3(imp::kMicThreads), 0, s, d_rows, d_interp,
                       (const double*)d_mag, (long long)pitch, (long long)M, d_pow);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(imp::micdev_ratio_kernel, dim3(mblocks, (unsigned)G), dim3(imp::kMicThreads), 0, s, d_rows, (long long)B,
                       (const double*)d_pow, (long long)M, d_raw);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(raw_out, d_raw, raw_n * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && power_out) e = hipMemcpyAsync(power_out, d_pow, pow_n * sizeof(double), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e2));
  return IMP_OK;
}

// the arguments both entries share, refused with the reason; *sp = what the rows span
static int mic_check(const char* who, const void* x, const int64_t* off, const int64_t* len, const int64_t* peak,
                     const int32_t* group, const int32_t* side, const int32_t* anchor, int64_t B, int64_t G, int64_t win,
                     int64_t pre, double fs, const double* grid, int64_t M, const double* raw_out, RowSpan* sp) {
  if (!off || !len || !peak || !group || !side || !anchor || !grid || !raw_out)
    return fail(IMP_ERR_INVALID, "%s: null argument", who);
  if (B < 2 || G < 1 || G > 65535 || B > 65535) return fail(IMP_ERR_INVALID, "%s: B = %lld rows in G = %lld groups (need 2 <= B, 1 <= G, both <= 65535)", who, (long long)B, (long long)G);
  if (M < 2 || M > (1 << 20)) return fail(IMP_ERR_INVALID, "%s: grid of %lld points (need 2 .. 2^20)", who, (long long)M);
  if (!(fs > 0.0) || !std::isfinite(fs)) return fail(IMP_ERR_INVALID, "%s: fs must be positive and finite (got %g)", who, fs);
  if (win < 1 || pre < 0 || win > ((int64_t)1 << 30) || pre > ((int64_t)1 << 30))
    return fail(IMP_ERR_INVALID, "%s: win = %lld, pre = %lld (need win >= 1, pre >= 0, both <= 2^30)", who, (long long)win, (long long)pre);
  for (int64_t g = 0; g < M; ++g)
    if (!std::isfinite(grid[g]) || !(grid[g] > 0.0) || (g && !(grid[g] > grid[g - 1])))
      return fail(IMP_ERR_INVALID, "%s: grid must be positive, finite and increasing (point %lld)", who, (long long)g);
  int rc = rows_check(who, off, len, B, kAnyLen, sp);
  if (rc) return rc;
  std::vector<int> seen((size_t)G * 2, 0);
  for (int64_t b = 0; b < B; ++b) {
    if (group[b] < 0 || group[b] >= G) return fail(IMP_ERR_INVALID, "%s: row %lld names group %d of %lld", who, (long long)b, group[b], (long long)G);
    if (side[b] != 0 && side[b] != 1) return fail(IMP_ERR_INVALID, "%s: row %lld has side %d (0 left, 1 right)", who, (long long)b, side[b]);
    if (anchor[b]) seen[(size_t)group[b] * 2 + side[b]] = 1;
  }
  for (int64_t g = 0; g < G; ++g)
    if (!seen[(size_t)g * 2] || !seen[(size_t)g * 2 + 1])
      return fail(IMP_ERR_INVALID, "%s: group %lld has no anchor row for the %s ear", who, (long long)g, seen[(size_t)g * 2] ? "right" : "left");
  if (sp->extent > 0 && !x) return fail(IMP_ERR_INVALID, "%s: null rows", who);
  return IMP_OK;
}

extern "C" int imp_mic_mismatch_device(imp_ctx* ctx, const float* d_x, const int64_t* off, const int64_t* len, const int64_t* peak,
                                       const int32_t* group, const int32_t* side, const int32_t* anchor, int64_t B, int64_t G,
                                       int64_t win, int64_t pre, double fs, const double* grid, int64_t M, double* raw_out,
                                       double* power_out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_mic_mismatch_device: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = mic_check("imp_mic_mismatch_device", d_x, off, len, peak, group, side, anchor, B, G, win, pre, fs, grid, M, raw_out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  return mic_mismatch_impl<float>(ctx, "imp_mic_mismatch_device", d_x, off, len, peak, group, side, anchor, B, G, win, pre, fs, grid,
                                  M, raw_out, power_out);
}

// fp64 host rows: uploaded as they are, then the same kernels on Sample = double
extern "C" int imp_mic_mismatch(imp_ctx* ctx, const double* x, const int64_t* off, const int64_t* len, const int64_t* peak,
                                const int32_t* group, const int32_t* side, const int32_t* anchor, int64_t B, int64_t G, int64_t win,
                                int64_t pre, double fs, const double* grid, int64_t M, double* raw_out, double* power_out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_mic_mismatch: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = mic_check("imp_mic_mismatch", x, off, len, peak, group, side, anchor, B, G, win, pre, fs, grid, M, raw_out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  BlockHold rows(ctx);
  if ((rc = upload_rows(ctx, "imp_mic_mismatch", x, sp.extent, rows))) return rc;
  return mic_mismatch_impl<double>(ctx, "imp_mic_mismatch", (const double*)rows.p, off, len, peak, group, side, anchor, B, G, win, pre,
                                   fs, grid, M, raw_out, power_out);
}

// ------------------------------------------------------------------------------------------------
// K15 binaural analysis metrics: band cross-spectra and IACF per speaker pair, energy decay curves per row
// ------------------------------------------------------------------------------------------------
// the arguments both metric entries share; *sp = what the rows span
static int binaural_check(const char* who, const void* x, const int64_t* off, const int64_t* len, int64_t P, const int64_t* nfft,
                          const int64_t* bins, int64_t bands, int64_t D, const double* band_out, const double* iacf_out,
                          const int64_t* peak_out, const double* energy_out, RowSpan* sp) {
  if (!off || !len || !iacf_out || !peak_out || !energy_out || (bands > 0 && (!nfft || !bins || !band_out)))
    return fail(IMP_ERR_INVALID, "%s: null argument", who);
  if (P < 1 || P > 65535) return fail(IMP_ERR_INVALID, "%s: P = %lld pairs (need 1 .. 65535)", who, (long long)P);
  if (bands < 0 || bands > 65535) return fail(IMP_ERR_INVALID, "%s: %lld bands (need 0 .. 65535)", who, (long long)bands);
  if (D < 0) return fail(IMP_ERR_INVALID, "%s: negative maximum lag %lld", who, (long long)D);
  if (D > imp::kIacfMaxD)
    return fail(IMP_ERR_UNSUPPORTED, "%s: maximum lag of %lld samples is above the limit of %d (10 ms at 192 kHz is 1920)", who,
                (long long)D, imp::kIacfMaxD);
  int rc = rows_check(who, off, len, 2 * P, (int64_t)1 << 22, sp);
  if (rc) return rc;
  for (int64_t p = 0; bands > 0 && p < P; ++p) {
    const int64_t n = nfft[p];
    if (n < 1 || n > ((int64_t)1 << 22) || n < len[2 * p] || n < len[2 * p + 1])
      return fail(IMP_ERR_INVALID, "%s: nfft = %lld of pair %lld (need 1 .. 2^22 and at least both rows' lengths %lld, %lld)", who,
                  (long long)n, (long long)p, (long long)len[2 * p], (long long)len[2 * p + 1]);
    if (!smooth_11(n)) return fail(IMP_ERR_UNSUPPORTED, "%s: nfft = %lld of pair %lld is not 2^a 3^b 5^c 7^d 11^e", who, (long long)n, (long long)p);
    for (int64_t b = 0; b < bands; ++b) {
      const int64_t k0 = bins[(p * bands + b) * 2], k1 = bins[(p * bands + b) * 2 + 1];
      if (k0 < 0 || k1 < k0 || k1 > n / 2 + 1)
        return fail(IMP_ERR_INVALID, "%s: bins [%lld, %lld) of pair %lld, band %lld (need 0 <= k0 <= k1 <= nfft / 2 + 1 = %lld)", who,
                    (long long)k0, (long long)k1, (long long)p, (long long)b, (long long)(n / 2 + 1));
    }
  }
  if (sp->extent > 0 && !x) return fail(IMP_ERR_INVALID, "%s: null rows", who);
  return IMP_OK;
}

// K15 (a): Z[p] = FFT_nfft(x_L + i x_R) of `count` pairs (analysis_kernels.hip.h), 11-smooth nfft as scipy.fft.next_fast_len
// gives it (the factor 7 included).  a, b: [count][nfft] each; *z: whichever of them holds the result.  The tile transform
// forms z in its load hook; lengths it does not hold go through plain radix passes after pair_pack_kernel, which also
// serves nfft = 1.  Nothing here waits.
template <class T>
static int analysis_pair_spectra(imp_ctx* ctx, const T* d_x, const imp::AnPair* d_pairs, int64_t count, int64_t nfft, cdbl* a,
                                 cdbl* b, cdbl** z) {
  hipStream_t s = ctx->stream;
  auto pack = [&]() {
    hipLaunchKernelGGL(imp::pair_pack_kernel<T>, dim3((unsigned)((nfft + imp::kAnThreads - 1) / imp::kAnThreads), (unsigned)count),
                       dim3(imp::kAnThreads), 0, s, d_x, d_pairs, a, (long long)nfft);
    return hipGetLastError();
  };
  *z = a;
  if (nfft == 1) {
    HIP_TRY(pack());
    return IMP_OK;
  }
  const std::vector<int> fac = factorise((int)nfft, true);
  if (fac.empty()) return fail(IMP_ERR_UNSUPPORTED, "transform length %lld is not 2^a 3^b 5^c 7^d 11^e", (long long)nfft);
  cdbl* roots = nullptr;
  int rc = ctx_fft_roots(ctx, nfft, &roots);
  if (rc) return rc;
  cdbl *cur = a, *oth = b;
  const bool tiles = fft64_wanted() && fft64::make_plan((int)nfft, true).ok;
  if (!tiles) HIP_TRY(pack());
  rc = run_fft_ops(ctx, fac, roots, (int)nfft, count, -1, &cur, &oth, imp::PairIn<T>{d_x, d_pairs}, fft64::NoOp{}, nullptr, 0, true);
  if (rc) return rc;
  *z = cur;
  return IMP_OK;
}

template <class T>
static int binaural_metrics_impl(imp_ctx* ctx, const char* who, const T* d_x, const int64_t* off, const int64_t* len, int64_t P,
                                 const int64_t* nfft, const int64_t* bins, int64_t bands, int64_t D, double* band_out,
                                 double* iacf_out, int64_t* peak_out, double* energy_out) {
  const int64_t nlag = 2 * D + 1;
  // pairs in the order the spectra are taken: grouped by nfft (a std::map: ascending), call order inside a group
  std::map<int64_t, std::vector<int64_t>> by_nfft;
  int64_t tiles_pitch = 1;
  std::vector<imp::AnPair> pairs((size_t)P);
  for (int64_t p = 0; p < P; ++p) {
    pairs[(size_t)p] = {off[2 * p], len[2 * p], off[2 * p + 1], len[2 * p + 1]};
    tiles_pitch = std::max<int64_t>(tiles_pitch, (std::max(len[2 * p], len[2 * p + 1]) + imp::kIacfTile - 1) / imp::kIacfTile);
    if (bands > 0) by_nfft[nfft[p]].push_back(p);
  }
  // longer groups go through in chunks (fft_chunk)
  struct Chunk { int64_t nfft, first, count; };
  std::vector<Chunk> chunks;
  std::vector<int64_t> order;                                          // pair of sorted position
  size_t z_elems = 1;
  for (auto& kv : by_nfft) {
    for (int64_t i = 0, count, n = (int64_t)kv.second.size(); i < n; i += count) {
      count = fft_chunk(n - i, kv.first);
      chunks.push_back({kv.first, (int64_t)order.size(), count});
      for (int64_t k = 0; k < count; ++k) order.push_back(kv.second[(size_t)(i + k)]);
      z_elems = std::max(z_elems, (size_t)count * (size_t)kv.first);
    }
  }
  // staged tables: pairs in call order | pairs in sorted order | bins in sorted order
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t pairs_b = up((size_t)P * sizeof(imp::AnPair));
  const size_t bins_b = up(std::max<size_t>((size_t)P * (size_t)bands * 2, 1) * sizeof(long long));
  char *h_tab = nullptr, *d_tab = nullptr;
  int rc = ctx_stage(ctx, 2 * pairs_b + bins_b, (void**)&h_tab, (void**)&d_tab);
  if (rc) return rc;
  std::memcpy(h_tab, pairs.data(), (size_t)P * sizeof(imp::AnPair));
  for (size_t i = 0; i < order.size(); ++i) {
    const int64_t p = order[i];
    reinterpret_cast<imp::AnPair*>(h_tab + pairs_b)[i] = pairs[(size_t)p];
    for (int64_t q = 0; q < bands * 2; ++q)
      reinterpret_cast<long long*>(h_tab + 2 * pairs_b)[(int64_t)i * bands * 2 + q] = (long long)bins[p * bands * 2 + q];
  }
  if ((rc = ctx_stage_push(ctx, h_tab, d_tab, 2 * pairs_b + bins_b))) return rc;
  const imp::AnPair* d_pairs = (const imp::AnPair*)d_tab;
  const imp::AnPair* d_sorted = (const imp::AnPair*)(d_tab + pairs_b);
  const long long* d_bins = (const long long*)(d_tab + 2 * pairs_b);
  // work: part [P][tiles_pitch][nlag + 2] | iacf [P][nlag] | energy [P][2] | peak [P] | band sums [P][bands][4] (sorted order)
  const size_t part_n = (size_t)P * (size_t)tiles_pitch * (size_t)(nlag + 2), iacf_n = (size_t)P * (size_t)nlag;
  const size_t band_n = (size_t)P * (size_t)bands * 4;
  hipStream_t s = ctx->stream;
  BlockHold work(ctx), spec_a(ctx), spec_b(ctx);
  if ((rc = work.get((part_n + iacf_n + 3 * (size_t)P + band_n + 1) * sizeof(double)))) return rc;
  double *d_part = (double*)work.p, *d_iacf = d_part + part_n, *d_energy = d_iacf + iacf_n;
  long long* d_peak = reinterpret_cast<long long*>(d_energy + 2 * (size_t)P);
  double* d_band = d_energy + 3 * (size_t)P;
  if (bands > 0 && ((rc = spec_a.get(z_elems * sizeof(double2))) || (rc = spec_b.get(z_elems * sizeof(double2))))) return rc;
  double2 *za = (double2*)spec_a.p, *zb = (double2*)spec_b.p;
  hipLaunchKernelGGL(imp::iacf_kernel<T>, dim3((unsigned)tiles_pitch, (unsigned)P), dim3(imp::kAnThreads), 0, s, d_x, d_pairs, (int)D,
                     (long long)tiles_pitch, d_part);
  if (hipGetLastError() != hipSuccess) return fail(IMP_ERR_HIP, "%s: IACF launch failed", who);
  hipLaunchKernelGGL(imp::iacf_finish_kernel, dim3((unsigned)P), dim3(imp::kAnThreads), 0, s, d_pairs, (int)D, (long long)tiles_pitch,
                     (const double*)d_part, d_iacf, d_peak, d_energy);
  if (hipGetLastError() != hipSuccess) return fail(IMP_ERR_HIP, "%s: IACF reduction launch failed", who);
  for (const Chunk& c : chunks) {
    double2* z = nullptr;
    if ((rc = analysis_pair_spectra(ctx, d_x, d_sorted + c.first, c.count, c.nfft, za, zb, &z))) return rc;
    hipLaunchKernelGGL(imp::band_cross_kernel, dim3((unsigned)bands, (unsigned)c.count), dim3(imp::kAnThreads), 0, s, (const double2*)z,
                       (long long)c.nfft, d_bins + c.first * bands * 2, (int)bands, d_band + c.first * bands * 4);
    if (hipGetLastError() != hipSuccess) return fail(IMP_ERR_HIP, "%s: band sums launch failed", who);
  }
  std::vector<double> h_band(band_n);
  hipError_t e = hipMemcpyAsync(iacf_out, d_iacf, iacf_n * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(energy_out, d_energy, 2 * (size_t)P * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(peak_out, d_peak, (size_t)P * sizeof(long long), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && band_n) e = hipMemcpyAsync(h_band.data(), d_band, band_n * sizeof(double), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e2));
  for (size_t i = 0; i < order.size(); ++i)
    std::memcpy(band_out + order[i] * bands * 4, h_band.data() + i * (size_t)bands * 4, (size_t)bands * 4 * sizeof(double));
  return IMP_OK;
}

extern "C" int imp_binaural_metrics_device(imp_ctx* ctx, const float* d_x, const int64_t* off, const int64_t* len, int64_t P,
                                           const int64_t* nfft, const int64_t* bins, int64_t bands, int64_t D, double* band_out,
                                           double* iacf_out, int64_t* peak_out, double* energy_out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_binaural_metrics_device: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = binaural_check("imp_binaural_metrics_device", d_x, off, len, P, nfft, bins, bands, D, band_out, iacf_out, peak_out,
                          energy_out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  return binaural_metrics_impl<float>(ctx, "imp_binaural_metrics_device", d_x, off, len, P, nfft, bins, bands, D, band_out, iacf_out,
                                      peak_out, energy_out);
}

// fp64 host rows: uploaded as they are, then the same kernels on Sample = double
extern "C" int imp_binaural_metrics(imp_ctx* ctx, const double* x, const int64_t* off, const int64_t* len, int64_t P,
                                    const int64_t* nfft, const int64_t* bins, int64_t bands, int64_t D, double* band_out,
                                    double* iacf_out, int64_t* peak_out, double* energy_out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_binaural_metrics: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = binaural_check("imp_binaural_metrics", x, off, len, P, nfft, bins, bands, D, band_out, iacf_out, peak_out, energy_out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  BlockHold rows(ctx);
  if ((rc = upload_rows(ctx, "imp_binaural_metrics", x, sp.extent, rows))) return rc;
  return binaural_metrics_impl<double>(ctx, "imp_binaural_metrics", (const double*)rows.p, off, len, P, nfft, bins, bands, D, band_out,
                                       iacf_out, peak_out, energy_out);
}

static int edc_check(const char* who, const void* x, const int64_t* off, const int64_t* len, int64_t B, double floor_db,
                     const double* out, RowSpan* sp) {
  if (!off || !len) return fail(IMP_ERR_INVALID, "%s: null argument", who);
  if (B < 1 || B > 65535) return fail(IMP_ERR_INVALID, "%s: B = %lld rows (need 1 .. 65535)", who, (long long)B);
  if (std::isnan(floor_db)) return fail(IMP_ERR_INVALID, "%s: floor_db is NaN", who);
  int rc = rows_check(who, off, len, B, (int64_t)1 << 26, sp);
  if (rc) return rc;
  if (sp->extent > 0 && (!x || !out)) return fail(IMP_ERR_INVALID, "%s: null rows or output", who);
  return IMP_OK;
}

template <class T>
static int edc_impl(imp_ctx* ctx, const char* who, const T* d_x, const int64_t* off, const int64_t* len, int64_t B, double floor_db,
                    int64_t total, double* out) {
  if (total == 0) return IMP_OK;
  std::vector<int64_t> pos((size_t)B);                                 // where row b's curve starts in out
  for (int64_t b = 0, at = 0; b < B; ++b) {
    pos[(size_t)b] = at;
    at += len[b];
  }
  const size_t meta = (size_t)B * sizeof(int64_t);
  void* tab[3];
  int rc = ctx_stage_tables(ctx, {{off, meta}, {len, meta}, {pos.data(), meta}}, tab);
  if (rc) return rc;
  BlockHold work(ctx);                                                 // scan [total] | curves [total]
  if ((rc = work.get(2 * (size_t)total * sizeof(double)))) return rc;
  double* d_work = (double*)work.p;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(imp::edc_kernel<T>, dim3((unsigned)B), dim3(imp::kDecayThreads), 0, s, d_x, (const long long*)tab[0],
                     (const long long*)tab[1], (const long long*)tab[2], floor_db, d_work, d_work + total);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_work + total, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e2));
  return IMP_OK;
}

extern "C" int imp_energy_decay_db_device(imp_ctx* ctx, const float* d_x, const int64_t* off, const int64_t* len, int64_t B,
                                          double floor_db, double* out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_energy_decay_db_device: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = edc_check("imp_energy_decay_db_device", d_x, off, len, B, floor_db, out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  return edc_impl<float>(ctx, "imp_energy_decay_db_device", d_x, off, len, B, floor_db, sp.total, out);
}

extern "C" int imp_energy_decay_db(imp_ctx* ctx, const double* x, const int64_t* off, const int64_t* len, int64_t B, double floor_db,
                                   double* out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_energy_decay_db: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = edc_check("imp_energy_decay_db", x, off, len, B, floor_db, out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  BlockHold rows(ctx);
  if ((rc = upload_rows(ctx, "imp_energy_decay_db", x, sp.extent, rows))) return rc;
  return edc_impl<double>(ctx, "imp_energy_decay_db", (const double*)rows.p, off, len, B, floor_db, sp.total, out);
}

// ------------------------------------------------------------------------------------------------
// K16 short-time spectra: the spectrogram and waterfall data of the plot stage
// ------------------------------------------------------------------------------------------------
// K16 (b): Z[b] = FFT_nfft of `count` transforms, each two windowed, mean-free segments as one complex signal
// (stft_kernels.hip.h; StftIn forms them in the tile transform's load hook).  Only lengths the tile plans hold: a
// segment length is fs / 10 at the rates of the path (2205 .. 19 200), and there is no other route.  a, b: [count][nfft]
// each (a is never read: the hook supplies every point); *z: whichever of them holds the result.  Nothing here waits.
static bool stft_length_ok(int64_t nfft) { return nfft >= 2 && nfft <= ((int64_t)1 << 20) && fft64::make_plan((int)nfft, true).ok; }

template <class T>
static int stft_spectra(imp_ctx* ctx, const T* d_x, const imp::StftXf* d_xf, int64_t count, int64_t nfft, cdbl* a, cdbl* b,
                        cdbl** z) {
  if (!stft_length_ok(nfft)) return fail(IMP_ERR_UNSUPPORTED, "segment length %lld has no tile plan", (long long)nfft);
  cdbl* roots = nullptr;
  int rc = ctx_fft_roots(ctx, nfft, &roots);
  if (rc) return rc;
  *z = a;
  return run_fft_ops(ctx, std::vector<int>(), roots, (int)nfft, count, -1, z, &b, imp::StftIn<T>{d_x, d_xf, roots}, fft64::NoOp{},
                     nullptr, 0, true, true);
}

static int stft_check(const char* who, const void* x, const int64_t* off, const int64_t* len, int64_t B, int64_t nfft, int64_t hop,
                      double fs, int mode, const void* out, RowSpan* sp) {
  if (!off || !len) return fail(IMP_ERR_INVALID, "%s: null argument", who);
  if (B < 1 || B > 65535) return fail(IMP_ERR_INVALID, "%s: B = %lld rows (need 1 .. 65535)", who, (long long)B);
  if (nfft < 2) return fail(IMP_ERR_INVALID, "%s: segment length nfft = %lld (need at least 2)", who, (long long)nfft);
  if (hop < 1 || hop > nfft) return fail(IMP_ERR_INVALID, "%s: hop = %lld (need 1 .. nfft = %lld)", who, (long long)hop, (long long)nfft);
  if (!(fs > 0.0) || std::isinf(fs)) return fail(IMP_ERR_INVALID, "%s: fs = %g", who, fs);
  if (mode != IMP_STFT_PSD_DB && mode != IMP_STFT_MAGNITUDE) return fail(IMP_ERR_INVALID, "%s: mode %d", who, mode);
  if (!stft_length_ok(nfft))
    return fail(IMP_ERR_UNSUPPORTED, "%s: segment length nfft = %lld is not a product of the radices 2, 3, 5, 7, 11 that is at most "
                "%d or splits into two such factors of at most %d", who, (long long)nfft, fft64::kMaxPoints, fft64::kMaxPoints);
  int rc = rows_check(who, off, len, B, (int64_t)1 << 26, sp);
  if (rc) return rc;
  int64_t total = 0;
  for (int64_t b = 0; b < B; ++b)
    if (len[b] >= nfft) total += (nfft / 2) * ((len[b] - (nfft - hop)) / hop);
  if (total > ((int64_t)1 << 32)) return fail(IMP_ERR_UNSUPPORTED, "%s: %lld output values (limit 2^32)", who, (long long)total);
  if ((sp->extent > 0 && !x) || (total > 0 && !out)) return fail(IMP_ERR_INVALID, "%s: null rows or output", who);
  return IMP_OK;
}

template <class T>
static int stft_impl(imp_ctx* ctx, const char* who, const T* d_x, const int64_t* off, const int64_t* len, int64_t B, int64_t nfft,
                     int64_t hop, double fs, int mode, int out_is_f32, void* out) {
  const int64_t nb = nfft / 2;
  // scipy's scale 1 / (fs sum w^2) of the periodic Hann window, the sum in index order; its square root for the magnitudes
  double w2 = 0.0;
  for (int64_t n = 0; n < nfft; ++n) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)n / (double)nfft);
    w2 += w * w;
  }
  double scale = 1.0 / (fs * w2);
  if (mode == IMP_STFT_MAGNITUDE) scale = std::sqrt(scale);
  std::vector<imp::StftRow> rows((size_t)B);
  int64_t n_xf = 0, total = 0, max_xf = 0;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t S = len[b] >= nfft ? (len[b] - (nfft - hop)) / hop : 0;
    rows[(size_t)b] = {off[b], len[b], total, n_xf, S};
    n_xf += (S + 1) / 2;
    max_xf = std::max(max_xf, (S + 1) / 2);
    total += nb * S;
  }
  if (total == 0) return IMP_OK;
  void* tab[1];
  int rc = ctx_stage_tables(ctx, {{rows.data(), (size_t)B * sizeof(imp::StftRow)}}, tab);
  if (rc) return rc;
  const int64_t cap = fft_chunk(n_xf, nfft);                             // more transforms go through in chunks
  const size_t out_bytes = (size_t)total * (out_is_f32 ? sizeof(float) : sizeof(double));
  BlockHold h_xf(ctx), h_za(ctx), h_zb(ctx), h_out(ctx);
  if ((rc = h_xf.get((size_t)n_xf * sizeof(imp::StftXf))) || (rc = h_za.get((size_t)cap * (size_t)nfft * sizeof(double2))) ||
      (rc = h_zb.get((size_t)cap * (size_t)nfft * sizeof(double2))) || (rc = h_out.get(out_bytes)))
    return rc;
  imp::StftXf* d_xf = (imp::StftXf*)h_xf.p;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(imp::stft_mean_kernel<T>, dim3((unsigned)max_xf, (unsigned)B), dim3(imp::kStftThreads), 0, s, d_x,
                     (const imp::StftRow*)tab[0], (long long)nfft, (long long)hop, d_xf);
  if (hipGetLastError() != hipSuccess) return fail(IMP_ERR_HIP, "%s: segment mean launch failed", who);
  for (int64_t first = 0; first < n_xf; first += cap) {
    const int64_t count = std::min(cap, n_xf - first);
    double2* z = nullptr;
    if ((rc = stft_spectra(ctx, d_x, d_xf + first, count, nfft, (double2*)h_za.p, (double2*)h_zb.p, &z))) return rc;
    const dim3 grid((unsigned)((count + imp::kStftTileXf - 1) / imp::kStftTileXf), (unsigned)((nb + imp::kStftTileBins - 1) / imp::kStftTileBins));
    if (out_is_f32)
      hipLaunchKernelGGL(imp::stft_out_kernel<float>, grid, dim3(imp::kStftThreads), 0, s, (const double2*)z,
                         (const imp::StftXf*)(d_xf + first), (long long)count, (long long)nfft, mode, scale, (float*)h_out.p);
    else
      hipLaunchKernelGGL(imp::stft_out_kernel<double>, grid, dim3(imp::kStftThreads), 0, s, (const double2*)z,
                         (const imp::StftXf*)(d_xf + first), (long long)count, (long long)nfft, mode, scale, (double*)h_out.p);
    if (hipGetLastError() != hipSuccess) return fail(IMP_ERR_HIP, "%s: epilogue launch failed", who);
  }
  const hipError_t e = hipMemcpyAsync(out, h_out.p, out_bytes, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  if (e != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
  if (e2 != hipSuccess) return fail(IMP_ERR_HIP, "%s: %s", who, hipGetErrorString(e2));
  return IMP_OK;
}

extern "C" int imp_stft_db_device(imp_ctx* ctx, const float* d_x, const int64_t* off, const int64_t* len, int64_t B, int64_t nfft,
                                  int64_t hop, double fs, int mode, int out_is_f32, void* out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_stft_db_device: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = stft_check("imp_stft_db_device", d_x, off, len, B, nfft, hop, fs, mode, out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  return stft_impl<float>(ctx, "imp_stft_db_device", d_x, off, len, B, nfft, hop, fs, mode, out_is_f32, out);
}

extern "C" int imp_stft_db(imp_ctx* ctx, const double* x, const int64_t* off, const int64_t* len, int64_t B, int64_t nfft, int64_t hop,
                           double fs, int mode, int out_is_f32, void* out) {
  if (!ctx) return fail(IMP_ERR_INVALID, "imp_stft_db: null ctx");
  IMP_CTX_LOCK(ctx);
  RowSpan sp;
  int rc = stft_check("imp_stft_db", x, off, len, B, nfft, hop, fs, mode, out, &sp);
  if (rc || (rc = ctx_bind(ctx))) return rc;
  BlockHold rows(ctx);
  if ((rc = upload_rows(ctx, "imp_stft_db", x, sp.extent, rows))) return rc;
  return stft_impl<double>(ctx, "imp_stft_db", (const double*)rows.p, off, len, B, nfft, hop, fs, mode, out_is_f32, out);
}
