// K17: rational resampling of rows, what ImpulseResponse.resample computes (core/impulse_response.py:121-124, per response
// from core/hrir.py:890-919): scipy.signal.resample_poly(x, up, down, window=taps), whose pre-pad, post-pad and trim collapse to
//   y[m] = up * sum_k taps[m down + half - k up] x[k],   half = (L - 1) / 2,  0 <= m < n_out = ceil(n_in up / down),
// with up / down reduced, the tap index inside [0, L) and x zero beyond the row.
//
// With t = m down + half, phase p = t mod up and k0 = t div up, output m is the dot product of ONE contiguous run of the
// phase-major tap table, ph[p][i] = taps[p + i up] (i < nph = ceil(L / up), zero where p + i up >= L), with x[k0 - i]:
//   y[m] = up * sum_{i = 0}^{nph - 1} ph[p][i] x[k0 - i]
// One thread owns one output and adds its terms in the order i = 0, 1, ..., each as one fma: the order is a function of
// (m, up, down, L) and of nothing else - not of the batch, the row's place in it, the tile or the grid.  (A workgroup skips a
// span that lies wholly outside the row: every term there is an exact +-0 and leaves the sum as it is, bit for bit.)
//
// A workgroup owns `tile` consecutive outputs of one row.  The terms go through in chunks of `chunk`; per chunk the input
// span the tile needs, (k0 of its last output - k0 of its first) + chunk samples, is staged in LDS as fp64 (Sample = float is
// widened exactly) and read from there.  tile and chunk are chosen on the host (RsPlan, a function of up, down, L) so that the
// span never exceeds kRsSpan samples = 32 KiB: five workgroups per CU, whatever the ratio and the filter.
//   up > 2   thread t has output m0 + t: neighbouring lanes have different phases and each walks its own run of the table
//            (16 001 taps: 128 KB, L2 resident); their inputs lie k0-close: consecutive, shared or a few apart.
//   up <= 2  wave w has the outputs m0 + (w mod up) + up j: one phase per wave, so a tap is ONE address per wave
//            instruction (the phase comes from readfirstlane and the tap loads are scalar), and lane j reads input
//            k0 + j down - i: consecutive doubles for down = 1 (ds_read_b64: 32 lanes on 32 different 8-byte banks).
// fp64 products and sums; the output is rounded once to Out.  No atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace imp {

constexpr int kRsThreads = 256;
constexpr int kRsSpan = 4096;            // staged input samples per workgroup

struct RsPlan {                          // a function of (up, down, L) alone
  long long up, down;                    // reduced
  long long half;                        // (L - 1) / 2
  long long nph;                         // terms per output, ceil(L / up)
  long long phases;                      // phases the table holds, min(up, L): an output of a later phase is zero
  int tile;                              // outputs per workgroup, 1 .. kRsThreads
  int chunk;                             // terms per staged span
  int uniform;                           // up <= 2 and a full tile: one phase per wave
};

struct RsRow {
  long long off, len;                    // the row in the input (elements)
  long long n_out;                       // ceil(len up / down)
  long long dst;                         // its place in the output (elements)
};

template <class T, class O, bool UNI>
__global__ __launch_bounds__(kRsThreads) void resample_poly_kernel(const T* __restrict__ x, const RsRow* __restrict__ rows,
                                                                   const double* __restrict__ ph, const RsPlan pl,
                                                                   O* __restrict__ dst) {
  __shared__ double xs[kRsSpan];
  const RsRow r = rows[blockIdx.y];
  const long long m0 = (long long)blockIdx.x * pl.tile;
  if (m0 >= r.n_out) return;                                           // uniform per workgroup
  const int t = threadIdx.x;
  const T* row = x + r.off;
  // the tile's first and last k0
  const long long kmin = (m0 * pl.down + pl.half) / pl.up;
  const long long kmax = ((m0 + pl.tile - 1) * pl.down + pl.half) / pl.up;
  long long m, k0, p;
  bool mine;
  if (UNI) {
    const int up = (int)pl.up;                                         // 1 or 2
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int res = w % up, j = (w / up) * 64 + (t & 63);
    const long long tt = (m0 + res) * pl.down + pl.half;               // uniform per wave
    const long long q = tt / up;
    p = tt - q * up;
    k0 = q + (long long)j * pl.down;
    m = m0 + res + (long long)up * j;
    mine = m < r.n_out;
  } else {
    m = m0 + t;
    const long long tt = m * pl.down + pl.half;
    k0 = tt / pl.up;
    p = tt - k0 * pl.up;
    mine = t < pl.tile && m < r.n_out;
  }
  const bool live = mine && p < pl.phases;
  const double* tp = ph + (p < pl.phases ? p : 0) * pl.nph;            // UNI: one pointer per wave
  double acc = 0.0;
  for (long long c0 = 0; c0 < pl.nph; c0 += pl.chunk) {
    const int cl = (int)(pl.nph - c0 < pl.chunk ? pl.nph - c0 : pl.chunk);
    const long long base = kmin - c0 - cl + 1;                         // the sample xs[0] holds
    const int span = (int)(kmax - kmin) + cl;                          // <= kRsSpan by the plan
    if (base + span <= 0 || base >= r.len) continue;                   // all zeros; uniform per workgroup
    __syncthreads();
    for (int s = t; s < span; s += kRsThreads) {
      const long long k = base + s;
      xs[s] = (k >= 0 && k < r.len) ? (double)row[k] : 0.0;
    }
    __syncthreads();
    if (live) {
      const double* xp = xs + (int)(k0 - kmin) + cl - 1;               // x[k0 - c0]; term i reads xp[-i]
      const double* tq = tp + c0;
#pragma unroll 8
      for (int i = 0; i < cl; ++i) acc = fma(tq[i], xp[-i], acc);
    }
  }
  if (mine) dst[r.dst + m] = (O)((double)pl.up * acc);
}

}  // namespace imp
