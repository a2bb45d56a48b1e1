// K13: virtual bass as a resident-slice stage (core/virtual_bass.py:82-176), and the chunk-parallel fp64 cascade IIR under it.
//
// A cascade of up to 8 second-order sections (the reference's crossover high-pass: 4) over a row of n samples is a linear
// recurrence on a state of 2 doubles per section (16 at most):
//     s[i+1] = A s[i] + b x[i],   y[i] = c s[i] + d x[i]
// so a row cut into chunks of kIirChunk samples runs as a two-pass scan:
//   pass 1   every chunk filtered from ZERO state, in parallel over chunks and rows; only its end state e[c] is kept
//   carry    per row, serial over chunks: init[0] = 0, init[c+1] = P init[c] + e[c] with P = A^kIirChunk (16 x 16, made on
//            the host by running the cascade with zero input from every unit state) - each chunk's true initial state
//   pass 2/3 every chunk re-run from init[c]: pass 2 accumulates the single-bin DFT of the output, pass 3 adds the synthesised
//            bass and writes the fp32 row (or fp64 rows: imp_sosfilt_chunked)
// The recurrence is reassociated (and contracted to FMAs), so the outputs are NOT bit-identical to scipy.signal.sosfilt / K11;
// they agree within 1e-12 of the row's peak.  One thread per chunk: the sections' state lives in
// VGPRs, the coefficients are kernel arguments (scalar registers); no scratch.
namespace imp {

constexpr int kIirChunk = 128;          // samples per chunk (IMP_IIR_CHUNK)
constexpr int kIirState = 2 * kMaxSections;
constexpr int kVbRefSpan = 4096;        // samples per workgroup of the reference bin's DFT
constexpr int kCarryTile = 64;          // chunks per LDS tile of the carry (2 x 8 KiB)

struct IirSos {                         // a cascade of n <= kMaxSections sections (the rest: identity, skipped)
  double b0[kMaxSections], b1[kMaxSections], b2[kMaxSections], a1[kMaxSections], a2[kMaxSections];
  int n;
};

struct VbRow {                          // what pass 3 adds to row b: gp * sig[i - delay] where 0 <= i - delay < n
  long long delay;
  int cross;                            // 0: g mpbass (direct), 1: g ild_mpbass (cross)
  int pad;
};

// one sample through the cascade (direct form II transposed, as K11), fused multiply-adds allowed
__device__ __forceinline__ double iir_step(const IirSos& f, double (&z0)[kMaxSections], double (&z1)[kMaxSections], double cur) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int s = 0; s < kMaxSections; ++s) {            // compile-time indices keep the state in registers; n is uniform
    if (s < f.n) {
      const double out = f.b0[s] * cur + z0[s];
      z0[s] = (f.b1[s] * cur - f.a1[s] * out) + z1[s];
      z1[s] = f.b2[s] * cur - f.a2[s] * out;
      cur = out;
    }
  }
  return cur;
}

// the samples [i0, i1) of a chunk through f(i, x): loads issued a block of kIirPrefetch samples ahead (one thread walks a chunk
// alone, so without them every sample would wait for its own load)
constexpr int kIirPrefetch = 8;
template <class T, class F>
__device__ __forceinline__ void chunk_loop(const T* xr, long long i0, long long i1, F&& f) {   // (xr may be written by f)
  T cur[kIirPrefetch], nxt[kIirPrefetch];
#pragma unroll
  for (int j = 0; j < kIirPrefetch; ++j) cur[j] = i0 + j < i1 ? xr[i0 + j] : T(0);
  for (long long base = i0; base < i1; base += kIirPrefetch) {
#pragma unroll
    for (int j = 0; j < kIirPrefetch; ++j) nxt[j] = base + kIirPrefetch + j < i1 ? xr[base + kIirPrefetch + j] : T(0);
#pragma unroll
    for (int j = 0; j < kIirPrefetch; ++j)
      if (base + j < i1) f(base + j, (double)cur[j]);
#pragma unroll
    for (int j = 0; j < kIirPrefetch; ++j) cur[j] = nxt[j];
  }
}

// pass 1: the end state of every chunk filtered from zero state.  grid (ceil(chunks / 64), rows), 64 threads; chunk c of row
// b covers samples [c L, min((c + 1) L, len[b])); chunks past the row's end do nothing.
template <class T>
__global__ __launch_bounds__(64) void iir_chunk_end_kernel(IirSos f, const T* __restrict__ x, const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ len, double* __restrict__ end_state,
                                                           long long chunk_pitch) {
  const int b = blockIdx.y;
  const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
  const long long n = len[b];
  const long long i0 = c * kIirChunk;
  if (c >= chunk_pitch || i0 >= n) return;
  const long long i1 = i0 + kIirChunk < n ? i0 + kIirChunk : n;
  const T* xr = x + off[b];
  double z0[kMaxSections], z1[kMaxSections];
#pragma unroll
  for (int s = 0; s < kMaxSections; ++s) z0[s] = z1[s] = 0.0;
  chunk_loop(xr, i0, i1, [&](long long, double v) { (void)iir_step(f, z0, z1, v); });
  double* e = end_state + ((long long)b * chunk_pitch + c) * kIirState;
#pragma unroll
  for (int s = 0; s < kMaxSections; ++s) {
    e[2 * s] = z0[s];
    e[2 * s + 1] = z1[s];
  }
}

// carry: per row (one wave), init[c] = the state before chunk c.  Lane 4 i + q holds component i of the state and sums the
// products of P row i with state components 4 q .. 4 q + 3; two butterflies complete the dot product.  The end states come in
// and the initial states go out through LDS, kCarryTile chunks at a time (coalesced), so the serial chain waits on LDS only.
__global__ __launch_bounds__(64) void iir_carry_kernel(const double* __restrict__ P /*[16][16]*/, const int64_t* __restrict__ len,
                                                       const double* __restrict__ end_state, double* __restrict__ init,
                                                       long long chunk_pitch) {
  const int b = blockIdx.x, lane = threadIdx.x, i = lane >> 2, q = lane & 3;
  const long long n = len[b];
  const long long nch = (n + kIirChunk - 1) / kIirChunk;
  double p[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) p[j] = P[i * kIirState + 4 * q + j];
  const double* e = end_state + (long long)b * chunk_pitch * kIirState;
  double* out = init + (long long)b * chunk_pitch * kIirState;
  __shared__ double te[kCarryTile * kIirState], to[kCarryTile * kIirState];
  double s = 0.0;
  for (long long c0 = 0; c0 < nch; c0 += kCarryTile) {
    const int cnt = (int)(nch - c0 < kCarryTile ? nch - c0 : kCarryTile);
    __syncthreads();
    for (int k = lane; k < cnt * kIirState; k += 64) te[k] = e[c0 * kIirState + k];
    __syncthreads();
    for (int cc = 0; cc < cnt; ++cc) {
      if (q == 0) to[cc * kIirState + i] = s;
      if (c0 + cc + 1 == nch) break;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fma(p[j], __shfl(s, 4 * (4 * q + j), 64), acc);
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      s = acc + te[cc * kIirState + i];
    }
    __syncthreads();
    for (int k = lane; k < cnt * kIirState; k += 64) out[c0 * kIirState + k] = to[k];
  }
}

__device__ __forceinline__ void iir_load_init(const double* __restrict__ init, long long b, long long c, long long chunk_pitch,
                                              double (&z0)[kMaxSections], double (&z1)[kMaxSections]) {
  const double* s0 = init + (b * chunk_pitch + c) * kIirState;
#pragma unroll
  for (int s = 0; s < kMaxSections; ++s) {
    z0[s] = s0[2 * s];
    z1[s] = s0[2 * s + 1];
  }
}

// pass 3 of imp_sosfilt_chunked: the filtered rows as fp64 (y: same offsets as x)
template <class T>
__global__ __launch_bounds__(64) void iir_chunk_out_kernel(IirSos f, const T* __restrict__ x, const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ len, const double* __restrict__ init,
                                                           long long chunk_pitch, double* __restrict__ y) {
  const int b = blockIdx.y;
  const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
  const long long n = len[b];
  const long long i0 = c * kIirChunk;
  if (c >= chunk_pitch || i0 >= n) return;
  const long long i1 = i0 + kIirChunk < n ? i0 + kIirChunk : n;
  double z0[kMaxSections], z1[kMaxSections];
  iir_load_init(init, b, c, chunk_pitch, z0, z1);
  const T* xr = x + off[b];
  double* yr = y + off[b];
  chunk_loop(xr, i0, i1, [&](long long i, double v) { yr[i] = iir_step(f, z0, z1, v); });
}

// ---- the virtual-bass stage of imp_slice ---------------------------------------------------------------------------------

// the bin np.argmin(np.abs(np.fft.rfftfreq(n, 1 / fs) - xo)) picks: rfftfreq's values are k * (1.0 / (n * (1.0 / fs))); the
// candidates around round(xo / val) are compared with the same fp64 expression, the first of equal distances wins
__device__ inline long long vbass_bin(long long n, double fs, double xo) {
  if (n < 1) return 0;
  const double val = 1.0 / ((double)n * (1.0 / fs));
  const long long kmax = n / 2;
  long long k0 = (long long)rint(xo / val) - 2;
  if (k0 < 0) k0 = 0;
  long long best = k0;
  double dbest = fabs((double)k0 * val - xo);
  for (long long k = k0 + 1; k <= k0 + 4 && k <= kmax; ++k) {
    const double d = fabs((double)k * val - xo);
    if (d < dbest) {
      dbest = d;
      best = k;
    }
  }
  return best > kmax ? kmax : best;
}

// per row: where the cropped row goes (its own pitch), its length and crop_tails' fade-out; per measurement: the bin
__global__ __launch_bounds__(64) void vbass_tables_kernel(const long long* __restrict__ keep, int rows_per_meas, int n_rows,
                                                          long long pitch, long long fade_out, double fs, double xo,
                                                          int64_t* __restrict__ off, int64_t* __restrict__ len,
                                                          WindowParams* __restrict__ par, long long* __restrict__ bin) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_rows) return;
  const int m = b / rows_per_meas;
  const long long n = keep[m];
  off[b] = (int64_t)b * pitch;
  len[b] = n;
  WindowParams p;
  p.gain = 1.0f;
  p.fade_in = 0;
  p.fade_out = fade_out <= n ? fade_out : 0;         // (longer: flagged IMP_SLICE_FADE by crop_tails)
  p.decay_start = 0;
  p.decay_half = -1;
  p.decay_knee = 0;
  p.decay_level_db = 0.0f;
  par[b] = p;
  if (b % rows_per_meas == 0) bin[m] = vbass_bin(n, fs, xo);
}

// pass 2: per chunk, sum_i hi[i] (cos, sin)(2 pi k i / n) with (k i) mod n reduced exactly as an integer before sincospi
__global__ __launch_bounds__(64) void vbass_dft_kernel(IirSos f, const float* __restrict__ x, const int64_t* __restrict__ off,
                                                       const int64_t* __restrict__ len, const double* __restrict__ init,
                                                       long long chunk_pitch, const long long* __restrict__ bin, int rows_per_meas,
                                                       double* __restrict__ part /*[rows][chunk_pitch][2]*/) {
  const int b = blockIdx.y;
  const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
  const long long n = len[b];
  const long long i0 = c * kIirChunk;
  if (c >= chunk_pitch || i0 >= n) return;
  const long long i1 = i0 + kIirChunk < n ? i0 + kIirChunk : n;
  const long long k = bin[b / rows_per_meas];
  double z0[kMaxSections], z1[kMaxSections];
  iir_load_init(init, b, c, chunk_pitch, z0, z1);
  const float* xr = x + off[b];
  long long r = (k * i0) % n;
  const double inv_n = 2.0 / (double)n;
  double re = 0.0, im = 0.0;
  chunk_loop(xr, i0, i1, [&](long long, double v) {
    const double h = iir_step(f, z0, z1, v);
    double sn, cs;
    sincospi((double)r * inv_n, &sn, &cs);
    re = fma(h, cs, re);
    im = fma(h, sn, im);
    r += k;
    if (r >= n) r -= n;
  });
  part[(b * chunk_pitch + c) * 2] = re;
  part[(b * chunk_pitch + c) * 2 + 1] = im;
}

// the same bin of mpbass[:n] (the reference's |rfft(mpbass)[k]|), kVbRefSpan samples per workgroup of 256 threads
__global__ __launch_bounds__(256) void vbass_ref_dft_kernel(const double* __restrict__ mp, const long long* __restrict__ keep,
                                                            const long long* __restrict__ bin, double* __restrict__ part,
                                                            int spans) {
  __shared__ double red[2][256];
  const int m = blockIdx.y, t = threadIdx.x;
  const long long n = keep[m], k = bin[m];
  const long long a = (long long)blockIdx.x * kVbRefSpan;
  const long long e = a + kVbRefSpan < n ? a + kVbRefSpan : n;
  const double inv_n = n > 0 ? 2.0 / (double)n : 0.0;
  double re = 0.0, im = 0.0;
  for (long long i = a + t; i < e; i += 256) {
    double sn, cs;
    sincospi((double)((k * i) % n) * inv_n, &sn, &cs);
    re = fma(mp[i], cs, re);
    im = fma(mp[i], sn, im);
  }
  red[0][t] = re;
  red[1][t] = im;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    part[((long long)m * spans + blockIdx.x) * 2] = red[0][0];
    part[((long long)m * spans + blockIdx.x) * 2 + 1] = red[1][0];
  }
}

// per measurement (256 threads): |hi[k]| of every row, g = mean / (|mpbass[:n] bin| + 1e-20) (polarity applied), the pairs'
// ITDs from the first peaks of the cropped rows, and what pass 3 adds to every row
__global__ __launch_bounds__(256) void vbass_gain_kernel(const double* __restrict__ part, long long chunk_pitch,
                                                         const double* __restrict__ ref_part, int spans, const long long* __restrict__ keep,
                                                         const long long* __restrict__ bin, const RowPeak* __restrict__ peaks,
                                                         const int* __restrict__ on_left, int rows_per_meas, long long head,
                                                         double polarity, double* __restrict__ gp, VbRow* __restrict__ vrow,
                                                         SliceRowOut* __restrict__ rows, SliceMeasOut* __restrict__ meas,
                                                         int* __restrict__ meas_flags) {
  __shared__ double red[2][256];
  const int m = blockIdx.x, t = threadIdx.x;
  const long long n = keep[m];
  const long long nch = (n + kIirChunk - 1) / kIirChunk;
  auto sum2 = [&](double re, double im) {
    __syncthreads();
    red[0][t] = re;
    red[1][t] = im;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) {
        red[0][t] += red[0][t + s];
        red[1][t] += red[1][t + s];
      }
      __syncthreads();
    }
    return hypot(red[0][0], red[1][0]);
  };
  double total = 0.0;
  bool finite = true;
  for (int r = 0; r < rows_per_meas; ++r) {
    const long long b = (long long)m * rows_per_meas + r;
    double re = 0.0, im = 0.0;
    for (long long c = t; c < nch; c += 256) {
      re += part[(b * chunk_pitch + c) * 2];
      im += part[(b * chunk_pitch + c) * 2 + 1];
    }
    const double mag = sum2(re, im);
    finite = finite && isfinite(mag);
    total += mag;
    if (t == 0) rows[b].vbass_mag = mag;
  }
  double re = 0.0, im = 0.0;
  for (int j = t; j < spans; j += 256) {
    re += ref_part[((long long)m * spans + j) * 2];
    im += ref_part[((long long)m * spans + j) * 2 + 1];
  }
  const double ref = sum2(re, im);
  if (t != 0) return;
  const double mean = total / (double)rows_per_meas;
  const double den = ref + 1e-20;
  const double g = mean / den;
  // a gain the relative contract cannot speak for (zero: nothing at the crossover) or that is not a number: the host decides
  if (!finite || !isfinite(ref) || den == 0.0 || !isfinite(g) || !(mean > 0.0)) meas_flags[m] |= SLICE_VBASS_GUARD;
  meas[m].vbass_gain = g;
  meas[m].vbass_bin = bin[m];
  gp[m] = g * polarity;
  for (int q = 0; 2 * q < rows_per_meas; ++q) {
    const long long bl = (long long)m * rows_per_meas + 2 * q;
    const RowPeak pl = peaks[bl], pr = peaks[bl + 1];
    const long long kl = (long long)(pl.first_peak != ~0ull ? pl.first_peak : pl.first_max);
    const long long kr = (long long)(pr.first_peak != ~0ull ? pr.first_peak : pr.first_max);
    const long long itd = kr - kl;
    const bool left = on_left[q] != 0;
    const long long cross = head + (left ? itd : -itd);
    vrow[bl] = VbRow{left ? head : cross, left ? 0 : 1, 0};
    vrow[bl + 1] = VbRow{left ? cross : head, left ? 1 : 0, 0};
    rows[bl].vbass_itd = itd;
    rows[bl + 1].vbass_itd = itd;
  }
}

// pass 3: hi + g * (mpbass | ild_mpbass)[i - delay], rounded to fp32 once, in place (each thread reads only its own chunk);
// hi64 (optional): the fp64 high-passed rows as well, [rows][hi_pitch]
__global__ __launch_bounds__(64) void vbass_synth_kernel(IirSos f, float* x, const int64_t* __restrict__ off,
                                                         const int64_t* __restrict__ len, const double* __restrict__ init,
                                                         long long chunk_pitch, int rows_per_meas, const double* __restrict__ gp,
                                                         const VbRow* __restrict__ vrow, const double* __restrict__ mp,
                                                         const double* __restrict__ ild, double* __restrict__ hi64, long long hi_pitch) {
  const int b = blockIdx.y;
  const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
  const long long n = len[b];
  const long long i0 = c * kIirChunk;
  if (c >= chunk_pitch || i0 >= n) return;
  const long long i1 = i0 + kIirChunk < n ? i0 + kIirChunk : n;
  double z0[kMaxSections], z1[kMaxSections];
  iir_load_init(init, b, c, chunk_pitch, z0, z1);
  float* xr = x + off[b];
  const VbRow v = vrow[b];
  const long long v_delay = v.delay;
  const double* sig = v.cross ? ild : mp;
  const double g = gp[b / rows_per_meas];
  chunk_loop((const float*)xr, i0, i1, [&](long long i, double v) {
    const double h = iir_step(f, z0, z1, v);
    const long long j = i - v_delay;
    // the reference: hi + (mpbass * gain * polarity)[j] - separately rounded (contraction is off here)
    const double add = (j >= 0 && j < n) ? sig[j] * g : 0.0;
    if (hi64) hi64[(long long)b * hi_pitch + i] = h;
    xr[i] = (float)(h + add);                        // (the prefetch has read past i already: in place is safe)
  });
}

}  // namespace imp
