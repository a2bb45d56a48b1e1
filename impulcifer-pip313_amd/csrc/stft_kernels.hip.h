// K16: short-time spectra of rows, the data behind ImpulseResponse.plot() (core/plotting/impulse_response_plotter.py:114-293
// plot_spectrogram, :459-609 plot_waterfall): what scipy.signal.spectrogram(x, fs, window=get_window("hann", nfft),
// nperseg=nfft, noverlap=nfft - hop, mode="psd" | "magnitude") computes, bin 0 dropped, "psd" as 10 log10(|p| + 1e-9).
//
// Row r has S_r = (len_r - (nfft - hop)) / hop segments (0 when it is shorter than nfft); segment s is x[s hop .. s hop + nfft).
// Two consecutive segments of a row travel as one complex signal, transform j of the row = segments 2 j and 2 j + 1; the
// last transform of a row with odd S carries one segment and zeros.  The transforms of all rows are numbered in row order.
//   (a) stft_mean_kernel<Sample>   grid (transforms of the longest row, rows), one workgroup per transform: the mean of each
//                                  of its two segments (scipy's detrend="constant"): every thread adds the samples
//                                  t, t + 256, ... in that order, a tree of fixed shape joins the threads.  It also writes
//                                  the transform's record (StftXf: where its segments start, their means, where its
//                                  columns go), so that nothing later needs to know the rows.
//   (b) fft64::tile_kernel         with StftIn as its load hook: point e of transform b is
//                                  (x_a[e] - mean_a) w[e] + i (x_b[e] - mean_b) w[e], w[e] = 0.5 - 0.5 cos(2 pi e / nfft) (the
//                                  periodic Hann window; the cosine is the real part of the transform's own table of roots).
//   (c) stft_out_kernel<Out>       grid (tiles of 32 transforms, tiles of 64 bins): splits A = (Z[k] + conj Z[nfft - k]) / 2,
//                                  B = (Z[k] - conj Z[nfft - k]) / (2 i), takes |.|^2 scale (doubled except at Nyquist) in dB, or
//                                  |.| scale, and writes [nfft / 2][S_r] per row through an LDS tile: the reads run along
//                                  the bins, the writes along the segments, both contiguous.
// fp64 throughout; Sample = float rows are widened exactly on load, Out = float is rounded once on store.  No atomics, no
// scratch, contraction off.  A row's values depend on that row alone.
#pragma once
#include <hip/hip_runtime.h>

namespace imp {

constexpr int kStftThreads = 256;
constexpr int kStftTileXf = 32;          // transforms (64 segments) per workgroup of the epilogue
constexpr int kStftTileBins = 64;

struct StftRow {
  long long off, len;                    // the row in the input (elements)
  long long out_off;                     // its [nfft / 2][S] block in the output (elements)
  long long xf0;                         // number of its first transform
  long long S;                           // segments
};

struct StftXf {
  long long off_a, off_b;                // first sample of either segment in the input; off_b < 0: no second segment
  double mean_a, mean_b;
  long long out;                         // output element of (bin 1, segment 2 j); bin k, segment 2 j + h at out + (k - 1) S + h
  long long S;
};

// load hook of fft64::tile_kernel
template <class T>
struct StftIn {
  const T* __restrict__ x;
  const StftXf* __restrict__ xf;
  const double2* __restrict__ roots;     // exp(-2 pi i e / nfft)
  __device__ __forceinline__ double2 operator()(double2, long long b, long long e) const {
#pragma clang fp contract(off)
    const StftXf* r = xf + b;
    const long long oa = r->off_a, ob = r->off_b;
    const double w = 0.5 - 0.5 * roots[e].x;
    const double re = ((double)x[oa + e] - r->mean_a) * w;
    const double im = ob >= 0 ? ((double)x[ob + e] - r->mean_b) * w : 0.0;
    return make_double2(re, im);
  }
};

template <class T>
__global__ __launch_bounds__(kStftThreads) void stft_mean_kernel(const T* __restrict__ x, const StftRow* __restrict__ rows,
                                                                 long long nfft, long long hop, StftXf* __restrict__ xf) {
#pragma clang fp contract(off)
  __shared__ double red[2][kStftThreads];
  const StftRow r = rows[blockIdx.y];
  const long long j = blockIdx.x;
  if (2 * j >= r.S) return;                                            // uniform per workgroup
  const int t = threadIdx.x;
  const bool two = 2 * j + 1 < r.S;
  const T* xa = x + r.off + 2 * j * hop;
  const T* xb = xa + hop;
  double sa = 0.0, sb = 0.0;
  for (long long i = t; i < nfft; i += kStftThreads) {
    sa += (double)xa[i];
    if (two) sb += (double)xb[i];
  }
  red[0][t] = sa;
  red[1][t] = sb;
  __syncthreads();
  for (int s = kStftThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    StftXf o;
    o.off_a = r.off + 2 * j * hop;
    o.off_b = two ? o.off_a + hop : -1;
    o.mean_a = red[0][0] / (double)nfft;
    o.mean_b = red[1][0] / (double)nfft;
    o.out = r.out_off + 2 * j;
    o.S = r.S;
    xf[r.xf0 + j] = o;
  }
}

// mode 0: 10 log10(|p| + 1e-9), p = |X|^2 scale, doubled unless `single`; mode 1: |X| scale
__device__ __forceinline__ double stft_value(double re, double im, int mode, double scale, bool single) {
#pragma clang fp contract(off)
  if (mode == 0) {
    double p = (re * re + im * im) * scale;
    if (!single) p *= 2.0;
    return 10.0 * log10(fabs(p) + 1e-9);
  }
  return hypot(re, im) * scale;
}

// z: [count][nfft] spectra of the transforms xf[0 .. count); out: the whole output
template <class O>
__global__ __launch_bounds__(kStftThreads) void stft_out_kernel(const double2* __restrict__ z, const StftXf* __restrict__ xf,
                                                                long long count, long long nfft, int mode, double scale,
                                                                O* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double tile[kStftTileBins][2 * kStftTileXf + 1];
  const int t = threadIdx.x;
  const long long nb = nfft / 2;                                       // bins 1 .. nb
  const long long b0 = (long long)blockIdx.x * kStftTileXf;
  const long long k0 = 1 + (long long)blockIdx.y * kStftTileBins;
  {
    const int kk = t % kStftTileBins;
    const long long k = k0 + kk;
    const bool single = 2 * k == nfft;                                 // Nyquist of an even length
    for (int tb = t / kStftTileBins; tb < kStftTileXf; tb += kStftThreads / kStftTileBins) {
      const long long b = b0 + tb;
      if (b < count && k <= nb) {
        const double2* zr = z + b * nfft;
        const double2 a = zr[k], c = zr[nfft - k];
        tile[kk][2 * tb] = stft_value((a.x + c.x) * 0.5, (a.y - c.y) * 0.5, mode, scale, single);
        tile[kk][2 * tb + 1] = stft_value((a.y + c.y) * 0.5, (c.x - a.x) * 0.5, mode, scale, single);
      }
    }
  }
  __syncthreads();
  {
    const int ss = t % (2 * kStftTileXf);
    const long long b = b0 + ss / 2;
    const int h = ss & 1;
    if (b >= count) return;
    const StftXf* r = xf + b;
    if (h && r->off_b < 0) return;
    const long long S = r->S;
    O* o = out + r->out + h;
    for (int kk = t / (2 * kStftTileXf); kk < kStftTileBins; kk += kStftThreads / (2 * kStftTileXf)) {
      const long long k = k0 + kk;
      if (k <= nb) o[(k - 1) * S] = (O)tile[kk][ss];
    }
  }
}
}  // namespace imp
