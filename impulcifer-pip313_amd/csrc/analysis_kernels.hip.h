// K15: binaural analysis metrics of finished rows (core/plotting/analysis.py:31-58 _band_cross_spectra, :90-100
// energy_decay_curve_db, :103-138 interaural_cross_correlation; called on every speaker pair by
// core/plotting/hrir_plotter.py:574-860).
//
// A pair = the left and the right row of one speaker.  Pairs are independent: a result never depends on what else is in the call.
//   (a) band cross-spectra   the two ears travel as z = x_L + i x_R, zero padded to nfft, through the fp64 tile transform
//                            (fft64::tile_kernel with PairIn as its load hook; pair_pack_kernel where the transform runs as
//                            plain radix passes).  band_cross_kernel, grid (bands, pairs): the threads stride over the bins
//                            k0 <= k < k1 of the host's table, split L = (Z[k] + conj Z[nfft - k]) / 2 and
//                            R = (Z[k] - conj Z[nfft - k]) / (2i), and add |L|^2, |R|^2 and L conj R; a tree of fixed shape
//                            joins the threads.  An empty range gives NaN.  The device never sees a frequency.
//   (b) IACF                 iacf_kernel<Sample>, grid (tiles, pairs): kIacfTile samples of the right row and the same stretch
//                            of the left row with D samples either side in LDS as fp64; thread t owns the lags t, t + 256, ...
//                            (consecutive lanes read consecutive left samples, the right sample is a broadcast: no bank
//                            conflict) and adds sum_n l[n + lag] r[n] over the tile in sample order; the tile's sum l^2 and
//                            sum r^2 by a fixed tree.  iacf_finish_kernel, grid (pairs): the tiles in tile order, divided by
//                            sqrt(E_l E_r); the first index of max |iacf| among the lags scipy's 'full' mode has.
//   (c) EDC                  edc_kernel<Sample>, grid (rows): block_scan (block_scan.hip.h) over the squares from the row's
//                            end, then 10 log10(e / (e[0] + 1e-12) + 1e-12), or floor_db when e[0] <= 1e-12.
// fp64 throughout; Sample = float rows are widened exactly on load.  Contraction is off except for the explicit fma of the
// lag sums.  No scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "block_scan.hip.h"

namespace imp {

constexpr int kAnThreads = 256;
constexpr int kIacfTile = 1024;          // right-row samples per workgroup
constexpr int kIacfMaxD = 2048;          // largest lag: 10 ms at 192 kHz is 1 920
constexpr int kIacfLagBlock = 4;         // lags a thread carries through one sweep of the tile

struct AnPair {
  long long off_l, n_l, off_r, n_r;      // rows in the input (elements)
};

// load hook of fft64::tile_kernel: point e of transform b is x_L[e] + i x_R[e], zero beyond a row's end
template <class T>
struct PairIn {
  const T* __restrict__ x;
  const AnPair* __restrict__ pairs;
  __device__ __forceinline__ double2 operator()(double2, long long b, long long e) const {
    const AnPair p = pairs[b];
    return make_double2(e < p.n_l ? (double)x[p.off_l + e] : 0.0, e < p.n_r ? (double)x[p.off_r + e] : 0.0);
  }
};

// the same values written out, for transform lengths the tile kernel does not hold (and nfft = 1, which is its own transform)
template <class T>
__global__ __launch_bounds__(kAnThreads) void pair_pack_kernel(const T* __restrict__ x, const AnPair* __restrict__ pairs,
                                                               double2* __restrict__ z, long long nfft) {
  const long long e = (long long)blockIdx.x * kAnThreads + threadIdx.x;
  if (e >= nfft) return;
  z[(long long)blockIdx.y * nfft + e] = PairIn<T>{x, pairs}(make_double2(0.0, 0.0), blockIdx.y, e);
}

// bins: [pairs][bands][2] = (k0, k1), 0 <= k0 <= k1 <= nfft / 2 + 1 checked by the host; out: [pairs][bands][4]
static __global__ __launch_bounds__(kAnThreads) void band_cross_kernel(const double2* __restrict__ z, long long nfft,
                                                                       const long long* __restrict__ bins, int bands,
                                                                       double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[4][kAnThreads];
  const int t = threadIdx.x;
  const long long slot = (long long)blockIdx.y * bands + blockIdx.x;
  const long long k0 = bins[2 * slot], k1 = bins[2 * slot + 1];
  double* o = out + 4 * slot;
  if (k0 >= k1) {                                                      // uniform per workgroup
    if (t < 4) o[t] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const double2* zr = z + (long long)blockIdx.y * nfft;
  double pl = 0.0, pr = 0.0, cr = 0.0, ci = 0.0;
  for (long long k = k0 + t; k < k1; k += kAnThreads) {
    const double2 a = zr[k], b = zr[k ? nfft - k : 0];
    const double lx = (a.x + b.x) * 0.5, ly = (a.y - b.y) * 0.5;
    const double rx = (a.y + b.y) * 0.5, ry = (b.x - a.x) * 0.5;
    pl += lx * lx + ly * ly;
    pr += rx * rx + ry * ry;
    cr += lx * rx + ly * ry;
    ci += ly * rx - lx * ry;
  }
  red[0][t] = pl;
  red[1][t] = pr;
  red[2][t] = cr;
  red[3][t] = ci;
  __syncthreads();
  for (int s = kAnThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + s];
    }
    __syncthreads();
  }
  if (t < 4) o[t] = red[t][0];
}

// part: [pairs][tiles_pitch][2 D + 3]: the lag sums of the tile, then its sum l^2 and sum r^2
template <class T>
__global__ __launch_bounds__(kAnThreads) void iacf_kernel(const T* __restrict__ x, const AnPair* __restrict__ pairs, int D,
                                                          long long tiles_pitch, double* __restrict__ part) {
  __shared__ double sl[kIacfTile + 2 * kIacfMaxD];
  __shared__ double sr[kIacfTile];
  __shared__ double red[2][kAnThreads];
  const AnPair p = pairs[blockIdx.y];
  const long long t0 = (long long)blockIdx.x * kIacfTile;
  const long long nmax = p.n_l > p.n_r ? p.n_l : p.n_r;
  if (t0 >= nmax) return;                                              // uniform per workgroup
  const int t = threadIdx.x;
  const int nlag = 2 * D + 1;
  const T* xl = x + p.off_l;
  const T* xr = x + p.off_r;
  for (int i = t; i < kIacfTile; i += kAnThreads) sr[i] = t0 + i < p.n_r ? (double)xr[t0 + i] : 0.0;
  for (int i = t; i < kIacfTile + 2 * D; i += kAnThreads) {
    const long long j = t0 - D + i;
    sl[i] = (j >= 0 && j < p.n_l) ? (double)xl[j] : 0.0;
  }
  __syncthreads();
  double* o = part + ((long long)blockIdx.y * tiles_pitch + blockIdx.x) * (nlag + 2);
  // lag index j = lag + D: sum_n l[t0 + n + lag] r[t0 + n] = sum_n sl[n + j] sr[n]
  for (int j0 = 0; j0 < nlag; j0 += kAnThreads * kIacfLagBlock) {      // uniform trip count
    int j[kIacfLagBlock];
    double acc[kIacfLagBlock];
#pragma unroll
    for (int u = 0; u < kIacfLagBlock; ++u) {
      const int want = j0 + u * kAnThreads + t;
      j[u] = want < nlag ? want : nlag - 1;                            // reads stay inside sl; only `want < nlag` is stored
      acc[u] = 0.0;
    }
    const int live = (nlag - j0 + kAnThreads - 1) / kAnThreads;        // blocks of 256 lags left: uniform
    if (live >= kIacfLagBlock) {
      for (int n = 0; n < kIacfTile; ++n) {
        const double r = sr[n];
#pragma unroll
        for (int u = 0; u < kIacfLagBlock; ++u) acc[u] = fma(sl[n + j[u]], r, acc[u]);
      }
    } else {
      for (int n = 0; n < kIacfTile; ++n) {
        const double r = sr[n];
#pragma unroll
        for (int u = 0; u < kIacfLagBlock; ++u)
          if (u < live) acc[u] = fma(sl[n + j[u]], r, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kIacfLagBlock; ++u) {
      const int want = j0 + u * kAnThreads + t;
      if (want < nlag) o[want] = acc[u];
    }
  }
  {
#pragma clang fp contract(off)
    double el = 0.0, er = 0.0;
    for (int n = t; n < kIacfTile; n += kAnThreads) {
      const double a = sl[D + n], b = sr[n];
      el += a * a;
      er += b * b;
    }
    red[0][t] = el;
    red[1][t] = er;
    __syncthreads();
    for (int s = kAnThreads / 2; s > 0; s >>= 1) {
      if (t < s) {
        red[0][t] += red[0][t + s];
        red[1][t] += red[1][t + s];
      }
      __syncthreads();
    }
    if (t < 2) o[nlag + t] = red[t][0];
  }
}

// iacf: [pairs][2 D + 1]; peak: index into that row of the first max |iacf| among the lags -(n_r - 1) .. n_l - 1 (-1: none,
// or nothing comparable); energy: [pairs][2]
static __global__ __launch_bounds__(kAnThreads) void iacf_finish_kernel(const AnPair* __restrict__ pairs, int D, long long tiles_pitch,
                                                                        const double* __restrict__ part, double* __restrict__ iacf,
                                                                        long long* __restrict__ peak, double* __restrict__ energy) {
#pragma clang fp contract(off)
  __shared__ double s_e[2];
  __shared__ double s_v[kAnThreads];
  __shared__ int s_i[kAnThreads];
  const AnPair p = pairs[blockIdx.x];
  const int t = threadIdx.x;
  const int nlag = 2 * D + 1;
  const long long nmax = p.n_l > p.n_r ? p.n_l : p.n_r;
  const long long tiles = (nmax + kIacfTile - 1) / kIacfTile;
  const double* pp = part + (long long)blockIdx.x * tiles_pitch * (nlag + 2);
  if (t < 2) {
    double e = 0.0;
    for (long long k = 0; k < tiles; ++k) e += pp[k * (nlag + 2) + nlag + t];
    s_e[t] = e;
    energy[2 * (long long)blockIdx.x + t] = e;
  }
  __syncthreads();
  const double denom = sqrt(s_e[0] * s_e[1]);
  const long long lo = (p.n_r - 1 < D ? -(p.n_r - 1) : -(long long)D) + D;      // valid lag indices lo .. hi
  const long long hi = (p.n_l - 1 < D ? p.n_l - 1 : (long long)D) + D;
  double best = -1.0;
  int best_i = -1;
  for (int j = t; j < nlag; j += kAnThreads) {
    double s = 0.0;
    for (long long k = 0; k < tiles; ++k) s += pp[k * (nlag + 2) + j];
    const double v = s / denom;
    iacf[(long long)blockIdx.x * nlag + j] = v;
    if (p.n_l > 0 && p.n_r > 0 && j >= lo && j <= hi && fabs(v) > best) {       // ascending j: the first of equals stays
      best = fabs(v);
      best_i = j;
    }
  }
  s_v[t] = best;
  s_i[t] = best_i;
  __syncthreads();
  for (int s = kAnThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      const double v = s_v[t + s];
      const int i = s_i[t + s];
      if (i >= 0 && (s_i[t] < 0 || v > s_v[t] || (v == s_v[t] && i < s_i[t]))) {
        s_v[t] = v;
        s_i[t] = i;
      }
    }
    __syncthreads();
  }
  if (t == 0) peak[blockIdx.x] = s_i[0];
}

// rows at x + off[b] (len[b] samples); out and scratch packed at out_off[b]; one workgroup per row
template <class T>
__global__ __launch_bounds__(kDecayThreads) void edc_kernel(const T* __restrict__ x, const long long* __restrict__ off,
                                                            const long long* __restrict__ len, const long long* __restrict__ out_off,
                                                            double floor_db, double* __restrict__ scratch, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[kDecayThreads / 64];
  const long long n = len[blockIdx.x];
  if (n < 1) return;
  const T* xr = x + off[blockIdx.x];
  double* sc = scratch + out_off[blockIdx.x];
  double* o = out + out_off[blockIdx.x];
  // sc[j] = sum of the last j + 1 squares = e[n - 1 - j]
  block_scan([&](long long j) { const double v = (double)xr[n - 1 - j]; return v * v; }, n, sc, red);
  const double total = sc[n - 1];                                      // np.max(energy): the sums never fall
  if (total <= 1e-12) {
    for (long long i = threadIdx.x; i < n; i += kDecayThreads) o[i] = floor_db;
    return;
  }
  const double den = total + 1e-12;
  for (long long i = threadIdx.x; i < n; i += kDecayThreads) o[i] = 10.0 * log10(sc[n - 1 - i] / den + 1e-12);
}

}  // namespace imp
