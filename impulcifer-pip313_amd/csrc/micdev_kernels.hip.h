// K14: direct-sound power spectra and the interaural mismatch of microphone-deviation correction
// (core/microphone_deviation_correction.py:106-140 _windowed_power, :195-218 estimate_interaural_mismatch up to raw_delta).
//
// Per row: the segment [max(peak - pre, 0), min(peak + win, n)) with the reference's two half-Hann fades, zero-padded to
// nfft = scipy.fft.next_fast_len(max(L, 8192)) (11-smooth), |X[k]| at the bins np.interp needs for the log grid, the
// interpolation, squared.  Per group (one HRIR): the mean power of its anchor rows per ear and 10 log10 of their ratio.
//   micdev_mag_kernel     grid (ceil(nb / 256), rows): the tapered segment in LDS tiles as fp64, one needed bin per thread,
//                         direct summation with the angle (k n) mod nfft reduced exactly as an integer before sincospi (as
//                         K13's single-bin DFTs); |X| = hypot(re, im)
//   micdev_power_kernel   grid (ceil(M / 256), rows): numpy's interp formula slope * (x - xp[j]) + fp[j] from the host's
//                         (bin pair, x - xp[j], xp[j+1] - xp[j]) table of the row's nfft; power = value * value
//   micdev_ratio_kernel   grid (ceil(M / 256), groups): sums of the anchor rows in row order (what np.mean over axis 0 adds),
//                         divided by their count; raw = 10 log10((left + 1e-20) / (right + 1e-20))
// The bin table and the interpolation brackets depend on (fs, nfft, grid) only; the host builds them (one set per distinct
// nfft of the call).  fp64 throughout, contraction off (numpy rounds every product and sum); no scratch.
namespace imp {

constexpr int kMicThreads = 256;
constexpr int kMicTile = 2048;          // fp64 samples per LDS tile (16 KiB)
constexpr int kMicMinSeg = 8;           // shorter segments: the row's power is all zeros

struct MicRow {                         // one analysed row
  long long off;                        // row start in the input (elements)
  long long start;                      // segment start within the row
  long long L;                          // segment length (< kMicMinSeg: zeros)
  long long fade_in, fade_out;          // half-Hann lengths (applied when > 1)
  long long nfft;
  long long bin_off;                    // this row's table set: needed bins at bins[bin_off ..], nb of them
  long long nb;
  long long interp_off;                 // MicInterp entries at interp[interp_off ..], M of them
  int group, side, anchor, pad;
};

struct MicInterp {                      // one grid point of np.interp(grid, rfftfreq(nfft, 1 / fs), mag, mag[0], mag[-1])
  int ia, ib;                           // positions in the row's needed-bin list of xp[j], xp[j + 1]
  int lerp, pad;                        // 0: fp[j] itself (left / right / last bin / x == xp[j]); 1: the formula
  double xd, dd;                        // x - xp[j], xp[j + 1] - xp[j]
};

// np.hanning(2 f): 0.5 + 0.5 cos(pi m / (2 f - 1)), m = 1 - 2 f + 2 i
__device__ __forceinline__ double mic_hann(long long i, long long f) {
#pragma clang fp contract(off)
  const double m = (double)(1 - 2 * f + 2 * i);
  return 0.5 + 0.5 * cos(M_PI * m / (double)(2 * f - 1));
}

__device__ __forceinline__ double mic_taper(const MicRow& r, long long i) {
  if (r.fade_out > 1 && i >= r.L - r.fade_out) return mic_hann(r.fade_out + (i - (r.L - r.fade_out)), r.fade_out);
  if (r.fade_in > 1 && i < r.fade_in) return mic_hann(i, r.fade_in);
  return 1.0;
}

template <class T>
__global__ __launch_bounds__(kMicThreads) void micdev_mag_kernel(const T* __restrict__ x, const MicRow* __restrict__ rows,
                                                                 const long long* __restrict__ bins, double* __restrict__ mag,
                                                                 long long mag_pitch) {
#pragma clang fp contract(off)
  __shared__ double seg[kMicTile];
  const MicRow r = rows[blockIdx.y];
  const long long j = (long long)blockIdx.x * kMicThreads + threadIdx.x;
  if (r.L < kMicMinSeg || (long long)blockIdx.x * kMicThreads >= r.nb) return;      // uniform per workgroup
  const bool live = j < r.nb;
  const long long k = live ? bins[r.bin_off + j] : 0;
  const long long nfft = r.nfft;
  const double inv = 2.0 / (double)nfft;
  const T* xr = x + r.off + r.start;
  double re = 0.0, im = 0.0;
  for (long long t0 = 0; t0 < r.L; t0 += kMicTile) {
    const long long tn = r.L - t0 < kMicTile ? r.L - t0 : kMicTile;
    __syncthreads();
    for (long long i = threadIdx.x; i < tn; i += kMicThreads) seg[i] = (double)xr[t0 + i] * mic_taper(r, t0 + i);
    __syncthreads();
    if (live) {
      long long q = (k * t0) % nfft;
      for (long long i = 0; i < tn; ++i) {
        double sn, cs;
        sincospi((double)q * inv, &sn, &cs);
        re += seg[i] * cs;
        im -= seg[i] * sn;
        q += k;
        if (q >= nfft) q -= nfft;
      }
    }
  }
  if (live) mag[(long long)blockIdx.y * mag_pitch + j] = hypot(re, im);
}

__global__ __launch_bounds__(kMicThreads) void micdev_power_kernel(const MicRow* __restrict__ rows, const MicInterp* __restrict__ interp,
                                                                   const double* __restrict__ mag, long long mag_pitch, long long M,
                                                                   double* __restrict__ power) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * kMicThreads + threadIdx.x;
  if (g >= M) return;
  const MicRow r = rows[blockIdx.y];
  double v = 0.0;
  if (r.L >= kMicMinSeg) {
    const MicInterp e = interp[r.interp_off + g];
    const double* mr = mag + (long long)blockIdx.y * mag_pitch;
    const double fa = mr[e.ia];
    if (e.lerp) {
      const double slope = (mr[e.ib] - fa) / e.dd;
      v = slope * e.xd + fa;
    } else {
      v = fa;
    }
  }
  power[(long long)blockIdx.y * M + g] = v * v;
}

__global__ __launch_bounds__(kMicThreads) void micdev_ratio_kernel(const MicRow* __restrict__ rows, long long B,
                                                                   const double* __restrict__ power, long long M,
                                                                   double* __restrict__ raw) {
#pragma clang fp contract(off)
  const long long g = (long long)blockIdx.x * kMicThreads + threadIdx.x;
  if (g >= M) return;
  const int grp = blockIdx.y;
  double sl = 0.0, sr = 0.0;
  long long nl = 0, nr = 0;
  for (long long b = 0; b < B; ++b) {
    const MicRow& r = rows[b];
    if (r.group != grp || !r.anchor) continue;
    const double p = power[b * M + g];
    if (r.side == 0) {
      sl += p;
      ++nl;
    } else {
      sr += p;
      ++nr;
    }
  }
  const double left = sl / (double)nl, right = sr / (double)nr;
  raw[(long long)grp * M + g] = 10.0 * log10((left + 1e-20) / (right + 1e-20));
}

}  // namespace imp
