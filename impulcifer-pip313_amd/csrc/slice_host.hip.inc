// imp_slice: host side (included at the end of impulse_hip.hip; kernels in slice_kernels.hip.h).
// One stream-ordered sequence of launches for M measurements; see include/impulse_hip.h for the contract.

struct imp_slice {
  imp_ctx* ctx = nullptr;
  imp_plan* deconv = nullptr;        // K1 'same' plan of the column length (the caller's, must outlive the slice)
  imp_plan* fir = nullptr;           // K5: fused 'full' plan with one filter per row of a measurement (owned)
  SliceNorm* norm = nullptr;         // K2 of the ear sums (owned)
  int64_t n_pairs = 0, R = 0, L = 0, elem_stride = 1, m_cap = 0;
  int bits = 32;
  std::vector<int64_t> pair_offset, delay;
  int64_t head = 0, fade_out = 0, taps = 0, keep_cap = 0;
  double fs = 0, peak_height = 0.12589, peak_target = -0.1, guard_rel = 1e-10;
  int64_t row_len = 0, pitch_ir = 0, pitch_crop = 0, out_len_max = 0;
  int tiles = 0;
  int64_t chunks = 0, knee_chunks = 0;
  bool firs_set = false;
  // device state, all sized for m_cap measurements (B = m_cap R rows)
  char* d_block = nullptr;           // one allocation for the small tables below
  float* d_ir = nullptr;             // [B][pitch_ir]   deconvolved columns; crop_heads fades them in place
  double* d_win = nullptr;           // hann(2 fade_out)[fade_out:] as a table (K5's loader fades on load)
  unsigned* d_tile = nullptr;        // [B][tiles][chunks] chunk maxima left by pass C (pair-mode plans)
  unsigned* d_chunk = nullptr;       // [B][knee_chunks] chunk maxima of the cropped rows
  imp::RowPeak *d_res = nullptr, *d_res2 = nullptr;
  int64_t *d_meta = nullptr, *d_off2 = nullptr, *d_len2 = nullptr, *d_fade_len = nullptr;
  imp::WindowParams *d_fade_par = nullptr, *d_g_par = nullptr;
  long long* d_delay = nullptr;
  imp::KneeRow* d_knee = nullptr;
  unsigned long long* d_max = nullptr;
  double* d_means = nullptr;
  int64_t *d_g_off = nullptr, *d_g_len = nullptr;
  long long *d_keep = nullptr, *d_outlen = nullptr;
  double* d_peak_db = nullptr;
  imp::SliceRowOut* d_rows = nullptr;
  imp::SliceMeasOut* d_meas = nullptr;
  int* d_flags = nullptr;
  // decay adjustment (imp_slice_set_decay): targets per row of a measurement and the tables of its launches
  bool decay_on = false;
  int64_t dchunks = 0, dscratch = 0;
  double* d_target = nullptr;        // [R] target RT60 in seconds, NaN = leave the row alone
  char* d_dblock = nullptr;          // one allocation: the tables below
  int64_t *d_off3 = nullptr, *d_len3 = nullptr, *d_dlen = nullptr;
  imp::RowPeak* d_res3 = nullptr;
  imp::DecayJob* d_jobs = nullptr;
  double* d_rt = nullptr;            // [B][4]
  imp::WindowParams* d_dpar = nullptr;
  unsigned* d_dchunk = nullptr;      // [B][dchunks]
  double* d_dscr = nullptr;          // [B][dscratch] decay_times' Schroeder / prefix-sum rows
  // alignment between crop_heads and crop_tails (imp_slice_set_alignment)
  bool align_on = false;
  int n_ipsi = 0, ref_pair = 0;
  int64_t segment = 0;
  float* d_ir2 = nullptr;            // [B][pitch_ir] the aligned rows
  char* d_ablock = nullptr;          // one allocation: the tables below
  int *d_ipsi_a = nullptr, *d_ipsi_b = nullptr, *d_leader = nullptr, *d_leads = nullptr;   // leads[q]: q's left ear gives a group (or the reference) its peak
  int64_t *d_xa_off = nullptr, *d_xa_len = nullptr, *d_xb_off = nullptr, *d_xb_len = nullptr, *d_len1 = nullptr;
  long long *d_xarg = nullptr, *d_d1 = nullptr, *d_s2 = nullptr, *d_xpart_k = nullptr;
  int64_t* d_off_al = nullptr;       // [B] where the later stages read row b: crop_heads' place or its materialised copy
  double *d_xval = nullptr, *d_xpart_val = nullptr;
  imp::RowPeak* d_res1 = nullptr;
  // virtual bass between crop_tails and equalize (imp_slice_set_virtual_bass)
  bool vb_on = false;
  imp::IirSos vb_sos{};
  double vb_xo = 0, vb_pol = 1;
  int64_t vb_head = 0, vb_chunks = 0, vb_spans = 0, vb_hi_pitch = 0;
  char* d_vbblock = nullptr;         // one allocation: the tables below
  float* d_vb = nullptr;             // [B][pitch_crop] the cropped rows, then hi + synth: what K5 reads
  double *d_vb_end = nullptr, *d_vb_init = nullptr;   // [B][vb_chunks][16] chunk states of the IIR scan
  double *d_vb_part = nullptr, *d_vb_refp = nullptr;  // DFT partial sums: [B][vb_chunks][2], [m_cap][vb_spans][2]
  double *d_vb_mp = nullptr, *d_vb_ild = nullptr;     // [keep_cap] mpbass, ild_mpbass
  double *d_vb_P = nullptr, *d_vb_gp = nullptr;       // A^L [16][16]; g * polarity per measurement
  int* d_vb_left = nullptr;          // [n_pairs]
  int64_t *d_vb_off = nullptr, *d_vb_len = nullptr;
  imp::WindowParams* d_vb_par = nullptr;
  long long* d_vb_bin = nullptr;
  imp::VbRow* d_vb_rows = nullptr;
  imp::RowPeak* d_vb_res = nullptr;
  double* d_vb_hi = nullptr;         // the caller's: fp64 high-passed rows of the next calls (imp_slice_vbass_hi_device)
  // pinned host copies of the results of the last call
  imp::SliceRowOut* h_rows = nullptr;
  imp::SliceMeasOut* h_meas = nullptr;
  int64_t last_M = 0;
};

// One block of small device tables, 256-byte aligned each.  A block's tables stand in ONE list of (pointer member, element
// count): run with no base it only sizes the block (`need`), run with the allocation it points the members into it.
struct TableCarver {
  char* base = nullptr;
  size_t need = 0;
  template <class T>
  void operator()(T*& p, size_t count) {
    if (base) p = (T*)(base + need);
    need += (count * sizeof(T) + 255) & ~(size_t)255;
  }
};
// sizes the block of `tables` (a callable over a TableCarver&), allocates it into `block` and places the tables
template <class F>
static bool carve_tables(char*& block, size_t* need, F&& tables) {
  TableCarver size, place;
  tables(size);
  *need = size.need;
  if (hipMalloc((void**)&block, size.need) != hipSuccess) return false;
  place.base = block;
  tables(place);
  return true;
}

static_assert(sizeof(imp::SliceRowOut) == sizeof(imp_slice_row_result), "imp_slice_row_result layout");
static_assert(sizeof(imp::SliceMeasOut) == sizeof(imp_slice_result), "imp_slice_result layout");
static_assert(sizeof(imp::WindowParams) == sizeof(imp_window_params), "imp_window_params layout");

extern "C" void imp_slice_destroy(imp_slice* s) {
  if (!s) return;
  IMP_CTX_LOCK(s->ctx);
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);
  if (s->fir) imp_plan_destroy(s->fir);
  slice_norm_destroy(s->norm);
  (void)hipFree(s->d_block);
  (void)hipFree(s->d_ir);
  (void)hipFree(s->d_win);
  (void)hipFree(s->d_tile);
  (void)hipFree(s->d_chunk);
  (void)hipFree(s->d_means);
  (void)hipFree(s->d_target);
  (void)hipFree(s->d_dblock);
  (void)hipFree(s->d_dchunk);
  (void)hipFree(s->d_dscr);
  (void)hipFree(s->d_ir2);
  (void)hipFree(s->d_ablock);
  (void)hipFree(s->d_vbblock);
  if (s->h_rows) (void)hipHostFree(s->h_rows);
  if (s->h_meas) (void)hipHostFree(s->h_meas);
  delete s;
}

extern "C" int imp_slice_create(imp_plan* deconv, const imp_slice_geometry* g, int64_t max_measurements, imp_slice** out) {
  if (!deconv || !g || !out) return fail(IMP_ERR_INVALID, "imp_slice_create: null argument");
  *out = nullptr;
  imp_ctx* ctx = deconv->ctx;
  IMP_CTX_LOCK(ctx);
  if (deconv->mode != IMP_MODE_SAME || deconv->ola || deconv->fused || deconv->lanes != 1 || deconv->n_filters != 1)
    return fail(IMP_ERR_INVALID, "imp_slice_create: the deconvolution stage is a 'same' plan with one shared filter, in stream order "
                                 "(no overlap-add, no lanes)");
  if (g->n_pairs < 1 || g->n_pairs > 4096 || !g->pair_offset || !g->delay || max_measurements < 1 || max_measurements > 4096)
    return fail(IMP_ERR_INVALID, "imp_slice_create: bad pair count or capacity");
  if (g->bits != 16 && g->bits != 32) return fail(IMP_ERR_INVALID, "imp_slice_create: bits must be 16 or 32 (PCM frames)");
  if (g->elem_stride < 1 || g->head < 0 || g->fade_out < 0 || !(g->fs > 0) || !(g->peak_height > 0))
    return fail(IMP_ERR_INVALID, "imp_slice_create: bad stride, head, fade or fs");
  if (g->taps < 1 || g->taps > kFusedMaxTaps)
    return fail(IMP_ERR_UNSUPPORTED, "imp_slice_create: FIRs of 1 .. %lld taps (the fused overlap-save kernel); got %lld", (long long)kFusedMaxTaps,
                (long long)g->taps);
  if (g->keep_cap < 1 || g->keep_cap > deconv->out_len)
    return fail(IMP_ERR_INVALID, "imp_slice_create: keep_cap must be in [1, %lld]", (long long)deconv->out_len);
  for (int64_t q = 0; q < g->n_pairs; ++q)
    if (g->pair_offset[q] < 0 || g->delay[q] < 0) return fail(IMP_ERR_INVALID, "imp_slice_create: negative offset / delay of pair %lld", (long long)q);
  int rc = check_input_span(deconv, g->elem_stride, g->bits == 16 ? 2 : 4);
  if (rc) return rc;
  if ((deconv->paired ? deconv->N1 / 2 : deconv->N1) > imp::kMaxPlanRows)
    return fail(IMP_ERR_UNSUPPORTED, "imp_slice_create: deconvolution plan of %d rows", deconv->N1);
  if ((rc = ctx_bind(ctx))) return rc;
  imp_slice* s = new (std::nothrow) imp_slice();
  if (!s) return fail(IMP_ERR_ALLOC, "out of host memory");
  s->ctx = ctx;
  s->deconv = deconv;
  s->n_pairs = g->n_pairs;
  s->R = 2 * g->n_pairs;
  s->L = deconv->L;
  s->elem_stride = g->elem_stride;
  s->bits = g->bits;
  s->m_cap = max_measurements;
  s->pair_offset.assign(g->pair_offset, g->pair_offset + g->n_pairs);
  s->delay.assign(g->delay, g->delay + g->n_pairs);
  s->head = g->head;
  s->fade_out = g->fade_out;
  s->taps = g->taps;
  s->keep_cap = g->keep_cap;
  s->fs = g->fs;
  s->peak_height = g->peak_height;
  s->peak_target = g->peak_target_db;
  s->guard_rel = g->gain_guard_rel > 0 ? g->gain_guard_rel : 1e-10;
  s->row_len = deconv->out_len;
  s->pitch_ir = (deconv->out_len + 63) / 64 * 64;
  s->pitch_crop = (g->keep_cap + 63) / 64 * 64;
  s->out_len_max = g->keep_cap + g->taps - 1;
  s->tiles = plan_col_tiles(deconv);
  s->chunks = deconv->paired ? deconv->N1 / 2 : deconv->N1;
  s->knee_chunks = std::max<int64_t>(1, (s->row_len + imp::kPeakChunk - 1) / imp::kPeakChunk);
  auto bail = [&](int code) {
    imp_slice_destroy(s);
    return code;
  };
  const int64_t B = s->m_cap * s->R, M = s->m_cap;
  // K5: one filter per row of a measurement, the longest row the slice allows
  if ((rc = plan_create_empty_impl(ctx, g->taps, s->R, g->keep_cap, IMP_MODE_FULL, B, false, &s->fir, true))) return bail(rc);
  if (!s->fir->fused) return bail(fail(IMP_ERR_UNSUPPORTED, "imp_slice_create: fused FIR plans are switched off (IMPULSE_HIP_NO_FUSED_FIR)"));
  if ((rc = slice_norm_create(ctx, s->out_len_max, M, &s->norm))) return bail(rc);
  // the small tables as one block
  size_t need = 0;
  bool ok = carve_tables(s->d_block, &need, [&](TableCarver& t) {
              t(s->d_res, B), t(s->d_res2, B), t(s->d_meta, 2 * B), t(s->d_off2, B), t(s->d_len2, B), t(s->d_fade_len, B);
              t(s->d_fade_par, B), t(s->d_g_par, B), t(s->d_delay, s->n_pairs), t(s->d_knee, B), t(s->d_max, B);
              t(s->d_g_off, B), t(s->d_g_len, B), t(s->d_keep, M), t(s->d_outlen, M), t(s->d_peak_db, 2 * M);
              t(s->d_rows, B), t(s->d_meas, M), t(s->d_flags, M);
            }) &&
            hipMalloc((void**)&s->d_ir, (size_t)(B * s->pitch_ir) * sizeof(float)) == hipSuccess &&
            hipMalloc((void**)&s->d_win, (size_t)std::max<int64_t>(s->fade_out, 1) * sizeof(double)) == hipSuccess &&
            hipMalloc((void**)&s->d_tile, (size_t)std::max<int64_t>(B * s->tiles * s->chunks, 1) * sizeof(unsigned)) == hipSuccess &&
            hipMalloc((void**)&s->d_chunk, (size_t)(B * s->knee_chunks) * sizeof(unsigned)) == hipSuccess &&
            hipMalloc((void**)&s->d_means, (size_t)B * kKneeMeanPitch * sizeof(double)) == hipSuccess &&
            hipHostMalloc((void**)&s->h_rows, (size_t)B * sizeof(imp::SliceRowOut), hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&s->h_meas, (size_t)M * sizeof(imp::SliceMeasOut), hipHostMallocDefault) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    return bail(fail(IMP_ERR_ALLOC, "imp_slice_create: device allocation for %lld measurements of %lld rows failed", (long long)M, (long long)s->R));
  }
  std::vector<int64_t> meta((size_t)(2 * B));
  for (int64_t b = 0; b < B; ++b) {
    meta[(size_t)b] = b * s->pitch_ir;
    meta[(size_t)(B + b)] = s->row_len;
  }
  std::vector<long long> dl(s->delay.begin(), s->delay.end());
  if (s->fade_out > 0) {
    hipLaunchKernelGGL(imp::fade_table_kernel, dim3((unsigned)((s->fade_out + 255) / 256)), dim3(256), 0, ctx->stream, s->d_win,
                       (long long)0, (long long)s->fade_out);
    if (hipGetLastError() != hipSuccess) return bail(fail(IMP_ERR_HIP, "imp_slice_create: fade table launch failed"));
  }
  ok = hipMemsetAsync(s->d_block, 0, need, ctx->stream) == hipSuccess &&
       hipMemcpyAsync(s->d_meta, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
       hipMemcpyAsync(s->d_delay, dl.data(), dl.size() * 8, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
       hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) return bail(fail(IMP_ERR_HIP, "imp_slice_create: table upload failed"));
  *out = s;
  return IMP_OK;
}

extern "C" int imp_slice_info(const imp_slice* s, int64_t* rows_per_measurement, int64_t* max_measurements, int64_t* out_len_max,
                              int64_t* norm_fft_len) {
  if (!s) return fail(IMP_ERR_INVALID, "null slice");
  if (rows_per_measurement) *rows_per_measurement = s->R;
  if (max_measurements) *max_measurements = s->m_cap;
  if (out_len_max) *out_len_max = s->out_len_max;
  if (norm_fft_len) *norm_fft_len = slice_norm_mfft(s->norm);
  return IMP_OK;
}

extern "C" int imp_slice_set_firs(imp_slice* s, const double* firs, int64_t ld) {
  if (!s || !firs) return fail(IMP_ERR_INVALID, "imp_slice_set_firs: null argument");
  IMP_CTX_LOCK(s->ctx);
  int rc = imp_plan_set_filters(s->fir, firs, ld);
  if (!rc) s->firs_set = true;
  return rc;
}

extern "C" int imp_slice_set_firs_device(imp_slice* s, const double* d_firs, int64_t ld) {
  if (!s || !d_firs) return fail(IMP_ERR_INVALID, "imp_slice_set_firs_device: null argument");
  IMP_CTX_LOCK(s->ctx);
  int rc = imp_plan_set_filters_device(s->fir, d_firs, ld);
  if (!rc) s->firs_set = true;
  return rc;
}

extern "C" int imp_slice_set_alignment(imp_slice* s, int64_t n_ipsi, const int32_t* ipsi_first, const int32_t* ipsi_second,
                                       const int32_t* leader_of_pair, int32_t ref_pair, int64_t segment) {
  if (!s) return fail(IMP_ERR_INVALID, "imp_slice_set_alignment: null slice");
  imp_ctx* ctx = s->ctx;
  IMP_CTX_LOCK(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  const int64_t B = s->m_cap * s->R;
  if (n_ipsi <= 0 && !leader_of_pair) {
    if (s->align_on) HIP_TRY(hipMemsetAsync(s->d_rows, 0, (size_t)B * sizeof(imp::SliceRowOut), ctx->stream));   // no stale shift fields
    s->align_on = false;
    return IMP_OK;
  }
  if (n_ipsi < 0 || n_ipsi > s->n_pairs || (n_ipsi && (!ipsi_first || !ipsi_second)) || !leader_of_pair)
    return fail(IMP_ERR_INVALID, "imp_slice_set_alignment: bad tables");
  if (ref_pair < 0 || ref_pair >= s->n_pairs) return fail(IMP_ERR_INVALID, "imp_slice_set_alignment: reference pair %d of %lld", ref_pair, (long long)s->n_pairs);
  if (segment < 1 || 2 * segment > 16384)
    return fail(IMP_ERR_UNSUPPORTED, "imp_slice_set_alignment: the lag search holds two segments of up to 8192 samples in LDS; got %lld", (long long)segment);
  std::vector<char> used((size_t)s->n_pairs, 0);
  for (int64_t p = 0; p < n_ipsi; ++p) {
    const int32_t a = ipsi_first[p], b = ipsi_second[p];
    if (a < 0 || a >= s->n_pairs || b < 0 || b >= s->n_pairs) return fail(IMP_ERR_INVALID, "imp_slice_set_alignment: ipsilateral pair %lld out of range", (long long)p);
    // the searches of a measurement run as one batch on the rows crop_heads left: no speaker may sit in two pairs
    if (used[(size_t)a] || (b != a && used[(size_t)b])) return fail(IMP_ERR_UNSUPPORTED, "imp_slice_set_alignment: a speaker in two ipsilateral pairs");
    used[(size_t)a] = used[(size_t)b] = 1;
  }
  for (int64_t q = 0; q < s->n_pairs; ++q)
    if (leader_of_pair[q] >= s->n_pairs) return fail(IMP_ERR_INVALID, "imp_slice_set_alignment: leader of pair %lld out of range", (long long)q);
  if (!s->d_ablock) {
    const int64_t J = s->m_cap * s->n_pairs;                  // jobs: at most one per pair and measurement
    const int64_t S_max = xcorr_slices(16384);
    size_t need = 0;
    bool ok = carve_tables(s->d_ablock, &need, [&](TableCarver& t) {
                t(s->d_ipsi_a, s->n_pairs), t(s->d_ipsi_b, s->n_pairs), t(s->d_leader, s->n_pairs), t(s->d_leads, s->n_pairs);
                t(s->d_xa_off, J), t(s->d_xa_len, J), t(s->d_xb_off, J), t(s->d_xb_len, J), t(s->d_xarg, J), t(s->d_xval, J);
                t(s->d_xpart_k, J * S_max), t(s->d_xpart_val, J * S_max);
                t(s->d_len1, B), t(s->d_d1, B), t(s->d_s2, B), t(s->d_res1, B), t(s->d_off_al, B);
              }) &&
              hipMalloc((void**)&s->d_ir2, (size_t)(B * s->pitch_ir) * sizeof(float)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      (void)hipFree(s->d_ablock);
      (void)hipFree(s->d_ir2);
      s->d_ablock = nullptr;
      s->d_ir2 = nullptr;
      return fail(IMP_ERR_ALLOC, "imp_slice_set_alignment: device allocation for %lld rows of %lld samples failed", (long long)B, (long long)s->pitch_ir);
    }
    HIP_TRY(hipMemsetAsync(s->d_ablock, 0, need, ctx->stream));
  }
  if (n_ipsi) {
    HIP_TRY(hipMemcpyAsync(s->d_ipsi_a, ipsi_first, (size_t)n_ipsi * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->d_ipsi_b, ipsi_second, (size_t)n_ipsi * 4, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(hipMemcpyAsync(s->d_leader, leader_of_pair, (size_t)s->n_pairs * 4, hipMemcpyHostToDevice, ctx->stream));
  std::vector<int> leads((size_t)s->n_pairs, 0);
  leads[(size_t)ref_pair] = 1;
  for (int64_t q = 0; q < s->n_pairs; ++q)
    if (leader_of_pair[q] >= 0) leads[(size_t)leader_of_pair[q]] = 1;
  HIP_TRY(hipMemcpyAsync(s->d_leads, leads.data(), (size_t)s->n_pairs * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));             // the caller's arrays may go
  s->n_ipsi = (int)n_ipsi;
  s->ref_pair = ref_pair;
  s->segment = segment;
  s->align_on = true;
  return IMP_OK;
}

extern "C" int imp_slice_set_decay(imp_slice* s, const double* target_rt60) {
  if (!s) return fail(IMP_ERR_INVALID, "imp_slice_set_decay: null slice");
  imp_ctx* ctx = s->ctx;
  IMP_CTX_LOCK(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  const int64_t B = s->m_cap * s->R;
  bool any = false;
  if (target_rt60)
    for (int64_t r = 0; r < s->R; ++r) {
      const double t = target_rt60[r];
      if (t != t) continue;
      if (!(t > 0) || !(t < 1e300)) return fail(IMP_ERR_INVALID, "imp_slice_set_decay: target of row %lld must be a positive time or NaN", (long long)r);
      any = true;
    }
  if (!any) {
    if (s->decay_on) HIP_TRY(hipMemsetAsync(s->d_rows, 0, (size_t)B * sizeof(imp::SliceRowOut), ctx->stream));   // no stale decay fields
    s->decay_on = false;
    return IMP_OK;
  }
  if (!s->d_dblock) {
    s->dchunks = std::max<int64_t>(1, (s->out_len_max + imp::kPeakChunk - 1) / imp::kPeakChunk);
    s->dscratch = 2 * (s->out_len_max + 2);
    size_t need = 0;
    bool ok = hipMalloc((void**)&s->d_target, (size_t)s->R * 8) == hipSuccess &&
              carve_tables(s->d_dblock, &need, [&](TableCarver& t) {
                t(s->d_off3, B), t(s->d_len3, B), t(s->d_dlen, B), t(s->d_res3, B), t(s->d_jobs, B), t(s->d_rt, 4 * B), t(s->d_dpar, B);
              }) &&
              hipMalloc((void**)&s->d_dchunk, (size_t)(B * s->dchunks) * sizeof(unsigned)) == hipSuccess &&
              hipMalloc((void**)&s->d_dscr, (size_t)(B * s->dscratch) * sizeof(double)) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      (void)hipFree(s->d_target);
      (void)hipFree(s->d_dblock);
      (void)hipFree(s->d_dchunk);
      (void)hipFree(s->d_dscr);
      s->d_target = nullptr;
      s->d_dblock = nullptr;
      s->d_dchunk = nullptr;
      s->d_dscr = nullptr;
      return fail(IMP_ERR_ALLOC, "imp_slice_set_decay: device allocation for %lld rows of %lld samples failed", (long long)B, (long long)s->out_len_max);
    }
    HIP_TRY(hipMemsetAsync(s->d_dblock, 0, need, ctx->stream));
  }
  HIP_TRY(hipMemcpyAsync(s->d_target, target_rt60, (size_t)s->R * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));             // the caller's array may go
  s->decay_on = true;
  return IMP_OK;
}

extern "C" int imp_slice_set_virtual_bass(imp_slice* s, const double* sos_hp, int64_t n_sections, const double* mpbass,
                                          const double* ild_mpbass, int64_t len, double crossover_freq, int64_t head,
                                          int32_t invert_polarity, const int32_t* pair_on_left) {
  if (!s) return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: null slice");
  imp_ctx* ctx = s->ctx;
  IMP_CTX_LOCK(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  const int64_t B = s->m_cap * s->R;
  // off: no sections, or a crossover at or above Nyquist (core/virtual_bass.py:93-95 returns without touching the rows)
  if (!sos_hp || n_sections == 0 || !(crossover_freq < s->fs / 2)) {
    if (crossover_freq != crossover_freq) return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: crossover frequency is NaN");
    if (s->vb_on) {                                        // no stale virtual-bass fields
      HIP_TRY(hipMemsetAsync(s->d_rows, 0, (size_t)B * sizeof(imp::SliceRowOut), ctx->stream));
      HIP_TRY(hipMemsetAsync(s->d_meas, 0, (size_t)s->m_cap * sizeof(imp::SliceMeasOut), ctx->stream));
    }
    s->vb_on = false;
    return IMP_OK;
  }
  imp::IirSos f;
  if ((rc = iir_sos_from(sos_hp, n_sections, &f, "imp_slice_set_virtual_bass"))) return rc;
  if (!mpbass || !ild_mpbass || !pair_on_left) return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: null signal or side table");
  if (len < s->keep_cap)
    return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: mpbass / ild_mpbass of %lld samples, the slice keeps up to %lld", (long long)len,
                (long long)s->keep_cap);
  if (!(crossover_freq > 0)) return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: crossover frequency must be positive");
  if (head < -(int64_t(1) << 40) || head > (int64_t(1) << 40)) return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: head out of range");
  for (int64_t i = 0; i < s->keep_cap; ++i)
    if (!std::isfinite(mpbass[i]) || !std::isfinite(ild_mpbass[i]))
      return fail(IMP_ERR_INVALID, "imp_slice_set_virtual_bass: non-finite synth sample %lld", (long long)i);
  if (!s->d_vbblock) {
    s->vb_chunks = (s->keep_cap + imp::kIirChunk - 1) / imp::kIirChunk;
    s->vb_spans = (s->keep_cap + imp::kVbRefSpan - 1) / imp::kVbRefSpan;
    const int64_t M = s->m_cap, C = s->vb_chunks;
    size_t need = 0;
    if (!carve_tables(s->d_vbblock, &need, [&](TableCarver& t) {
          t(s->d_vb, B * s->pitch_crop), t(s->d_vb_end, B * C * imp::kIirState), t(s->d_vb_init, B * C * imp::kIirState);
          t(s->d_vb_part, B * C * 2), t(s->d_vb_refp, M * s->vb_spans * 2), t(s->d_vb_mp, s->keep_cap), t(s->d_vb_ild, s->keep_cap);
          t(s->d_vb_P, 256), t(s->d_vb_gp, M), t(s->d_vb_left, s->n_pairs), t(s->d_vb_off, B), t(s->d_vb_len, B), t(s->d_vb_par, B);
          t(s->d_vb_bin, M), t(s->d_vb_rows, B), t(s->d_vb_res, B);
        })) {
      (void)hipGetLastError();
      s->d_vbblock = nullptr;
      return fail(IMP_ERR_ALLOC, "imp_slice_set_virtual_bass: device allocation for %lld rows of %lld samples failed", (long long)B,
                  (long long)s->pitch_crop);
    }
    HIP_TRY(hipMemsetAsync(s->d_vbblock, 0, need, ctx->stream));
  }
  std::vector<double> P(256);
  iir_transition(f, imp::kIirChunk, P.data());
  std::vector<int> left((size_t)s->n_pairs);
  for (int64_t q = 0; q < s->n_pairs; ++q) left[(size_t)q] = pair_on_left[q] ? 1 : 0;
  HIP_TRY(hipMemcpyAsync(s->d_vb_mp, mpbass, (size_t)s->keep_cap * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(s->d_vb_ild, ild_mpbass, (size_t)s->keep_cap * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(s->d_vb_P, P.data(), 256 * 8, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(s->d_vb_left, left.data(), left.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));             // the caller's arrays may go
  s->vb_sos = f;
  s->vb_xo = crossover_freq;
  s->vb_pol = invert_polarity ? -1.0 : 1.0;
  s->vb_head = head;
  s->vb_on = true;
  return IMP_OK;
}

extern "C" int imp_slice_vbass_hi_device(imp_slice* s, double* d_hi, int64_t pitch) {
  if (!s) return fail(IMP_ERR_INVALID, "imp_slice_vbass_hi_device: null slice");
  IMP_CTX_LOCK(s->ctx);
  if (d_hi && pitch < s->keep_cap)
    return fail(IMP_ERR_INVALID, "imp_slice_vbass_hi_device: pitch %lld < keep_cap %lld", (long long)pitch, (long long)s->keep_cap);
  s->d_vb_hi = d_hi;
  s->vb_hi_pitch = d_hi ? pitch : 0;
  return IMP_OK;
}

// the virtual-bass stage of M measurements: the cropped rows materialised (crop_tails' truncation + fade-out, as the staged
// imp_apply_window_device), their first peaks, the IIR scan with the crossover bin's DFT, the gain, hi + synth in place
static int slice_vbass_run(imp_slice* s, hipStream_t st, int64_t M, const float* rows_al, const int64_t* off_al) {
  const int64_t R = s->R, B = M * R, C = s->vb_chunks;
  hipLaunchKernelGGL(imp::vbass_tables_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const long long*)s->d_keep, (int)R, (int)B,
                     (long long)s->pitch_crop, (long long)s->fade_out, s->fs, s->vb_xo, s->d_vb_off, s->d_vb_len, s->d_vb_par, s->d_vb_bin);
  int rc;
  if ((rc = launch_window_copy(st, rows_al, off_al, s->d_vb, s->d_vb_off, s->d_vb_len, s->d_vb_par, s->keep_cap, B)) ||
      (rc = launch_first_peaks(st, s->d_vb, s->d_vb_off, s->d_vb_len, B, s->d_chunk, s->knee_chunks, s->d_vb_res, s->peak_height, nullptr)))
    return rc;
  const dim3 grid((unsigned)((C + 63) / 64), (unsigned)B);
  hipLaunchKernelGGL(imp::iir_chunk_end_kernel<float>, grid, dim3(64), 0, st, s->vb_sos, (const float*)s->d_vb, (const int64_t*)s->d_vb_off,
                     (const int64_t*)s->d_vb_len, s->d_vb_end, (long long)C);
  hipLaunchKernelGGL(imp::iir_carry_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)s->d_vb_P, (const int64_t*)s->d_vb_len,
                     (const double*)s->d_vb_end, s->d_vb_init, (long long)C);
  hipLaunchKernelGGL(imp::vbass_ref_dft_kernel, dim3((unsigned)s->vb_spans, (unsigned)M), dim3(256), 0, st, (const double*)s->d_vb_mp,
                     (const long long*)s->d_keep, (const long long*)s->d_vb_bin, s->d_vb_refp, (int)s->vb_spans);
  hipLaunchKernelGGL(imp::vbass_dft_kernel, grid, dim3(64), 0, st, s->vb_sos, (const float*)s->d_vb, (const int64_t*)s->d_vb_off,
                     (const int64_t*)s->d_vb_len, (const double*)s->d_vb_init, (long long)C, (const long long*)s->d_vb_bin, (int)R, s->d_vb_part);
  hipLaunchKernelGGL(imp::vbass_gain_kernel, dim3((unsigned)M), dim3(256), 0, st, (const double*)s->d_vb_part, (long long)C,
                     (const double*)s->d_vb_refp, (int)s->vb_spans, (const long long*)s->d_keep, (const long long*)s->d_vb_bin,
                     (const imp::RowPeak*)s->d_vb_res, (const int*)s->d_vb_left, (int)R, (long long)s->vb_head, s->vb_pol, s->d_vb_gp,
                     s->d_vb_rows, s->d_rows, s->d_meas, s->d_flags);
  hipLaunchKernelGGL(imp::vbass_synth_kernel, grid, dim3(64), 0, st, s->vb_sos, s->d_vb, (const int64_t*)s->d_vb_off, (const int64_t*)s->d_vb_len,
                     (const double*)s->d_vb_init, (long long)C, (int)R, (const double*)s->d_vb_gp, (const imp::VbRow*)s->d_vb_rows,
                     (const double*)s->d_vb_mp, (const double*)s->d_vb_ild, s->d_vb_hi, (long long)s->vb_hi_pitch);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

// K1 of one measurement: the pairs in runs of equal spacing, a run in launch groups of at most the plan's capacity
template <class Sample>
static int slice_ingest_typed(imp_slice* s, const Sample* rec, int64_t m, float scale) {
  imp_plan* p = s->deconv;
  int rc = IMP_OK;
  const int64_t row0 = m * s->R;
  int64_t q = 0;
  while (q < s->n_pairs && !rc) {
    int64_t q1 = q + 1;
    const int64_t stride = q1 < s->n_pairs ? s->pair_offset[(size_t)q1] - s->pair_offset[(size_t)q] : 0;
    while (q1 < s->n_pairs && stride > 0 && s->pair_offset[(size_t)q1] - s->pair_offset[(size_t)(q1 - 1)] == stride) ++q1;
    if (stride <= 0) q1 = q + 1;
    // pairs [q, q1) are `stride` samples apart
    const int64_t cap_pairs = std::max<int64_t>(1, (p->ws_channels / p->lanes) / 2);
    for (int64_t a = q; a < q1 && !rc; a += cap_pairs) {
      const int64_t nq = std::min(cap_pairs, q1 - a);
      const Sample* base = rec + s->pair_offset[(size_t)a];
      float* y = s->d_ir + (row0 + 2 * a) * s->pitch_ir;
      if (p->paired) {
        p->tile_max = s->d_tile + (row0 + 2 * a) * s->tiles * s->chunks;
        rc = run_group_pair(p, imp::LoadPair<Sample>{base, stride, 1, s->elem_stride, p->L, (int)(2 * nq), scale}, 2 * nq, y,
                            s->pitch_ir, 2);
        p->tile_max = nullptr;
      } else {
        // one channel per transform: the left ears of the run, then the right ears (rows 2 q + ear)
        for (int ear = 0; ear < 2 && !rc; ++ear) {
          imp::LoadPcmPacked<Sample> ld{base + ear, stride, s->elem_stride, p->L, scale};
          rc = run_group_with(p, ld, nq, y + ear * s->pitch_ir, 2 * s->pitch_ir, 0, 2);
        }
      }
    }
    q = q1;
  }
  return rc;
}

// ---- the stages of imp_slice_execute_device, in the order of core/pipeline.py; B = M R rows throughout
// K1: every column of every measurement -> d_ir (pair mode: pass C also leaves the chunk maxima)
static int slice_ingest(imp_slice* s, const void* d_rec, int64_t rec_stride, int64_t M) {
  for (int64_t m = 0; m < M; ++m) {
    const int rc = s->bits == 32 ? slice_ingest_typed<int>(s, (const int*)d_rec + m * rec_stride, m, 1.0f / 2147483648.0f)
                                 : slice_ingest_typed<short>(s, (const short*)d_rec + m * rec_stride, m, 1.0f / 32768.0f);
    if (rc) return rc;
  }
  return IMP_OK;
}

// K3: first peaks of the deconvolved columns
static int slice_first_peaks(imp_slice* s, hipStream_t st, int64_t M) {
  const int64_t* len = s->d_meta + s->m_cap * s->R;
  if (s->deconv->paired)
    return launch_first_peaks(st, s->d_ir, s->d_meta, len, M * s->R, nullptr, s->chunks, s->d_res, s->peak_height, nullptr,
                              s->deconv->out_start, s->d_tile, s->tiles);
  return launch_first_peaks(st, s->d_ir, s->d_meta, len, M * s->R, s->d_chunk, s->knee_chunks, s->d_res, s->peak_height, nullptr);
}

// crop_heads: offsets and lengths on the device, Hann fade-in in place
static int slice_crop_heads(imp_slice* s, hipStream_t st, int64_t M) {
  const int n_pairs_total = (int)(M * s->n_pairs);
  hipLaunchKernelGGL(imp::slice_crop_heads_kernel, dim3((unsigned)((n_pairs_total + 63) / 64)), dim3(64), 0, st, (const imp::RowPeak*)s->d_res,
                     (const long long*)s->d_delay, (int)s->n_pairs, n_pairs_total, (long long)s->pitch_ir, (long long)s->row_len,
                     (long long)s->head, s->d_off2, s->d_len2, s->d_fade_len, s->d_fade_par, s->d_rows, s->d_flags);
  if (s->head > 0) return launch_window_copy(st, s->d_ir, s->d_off2, s->d_ir, s->d_off2, s->d_fade_len, s->d_fade_par, s->head, M * s->R);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

// alignment (core/pipeline.py:593-597): ipsilateral lags (K10), onset shifts from the leaders' peaks, the rows materialised.
// The later stages read row b at d_ir + d_off_al[b]: crop_heads' place, or the copy in d_ir2.
static int slice_align(imp_slice* s, hipStream_t st, int64_t M) {
  const int64_t R = s->R, B = M * R;
  const int n_jobs = (int)(M * s->n_ipsi);
  int rc;
  HIP_TRY(hipMemsetAsync(s->d_xarg, 0, (size_t)std::max(n_jobs, 1) * 8, st));
  if (n_jobs) {
    hipLaunchKernelGGL(imp::slice_align_jobs_kernel, dim3((unsigned)((n_jobs + 63) / 64)), dim3(64), 0, st, (const int64_t*)s->d_off2,
                       (const int64_t*)s->d_len2, (const int*)s->d_ipsi_a, (const int*)s->d_ipsi_b, s->n_ipsi, (int)R, n_jobs, (long long)s->segment,
                       s->d_xa_off, s->d_xa_len, s->d_xb_off, s->d_xb_len, s->d_flags);
    if ((rc = launch_xcorr<float>(s->ctx, st, (const float*)s->d_ir, (const int64_t*)s->d_xa_off, (const int64_t*)s->d_xa_len, (const float*)s->d_ir,
                                  (const int64_t*)s->d_xb_off, (const int64_t*)s->d_xb_len, n_jobs, imp::xcorr_lds_doubles(s->segment, s->segment), 2 * s->segment - 1,
                                  s->d_xpart_k, s->d_xpart_val, s->d_xarg, s->d_xval)))
      return rc;
  }
  hipLaunchKernelGGL(imp::slice_align_delays_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, (const long long*)s->d_xarg,
                     (const int64_t*)s->d_xa_len, (const int*)s->d_ipsi_a, (const int*)s->d_ipsi_b, s->n_ipsi, (int)R, (int)M,
                     (const int64_t*)s->d_len2, (const int*)s->d_leads, s->d_d1, s->d_len1);
  if ((rc = launch_first_peaks(st, s->d_ir, s->d_off2, s->d_len1, B, s->d_chunk, s->knee_chunks, s->d_res1, s->peak_height, nullptr))) return rc;
  hipLaunchKernelGGL(imp::slice_align_onset_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, (const imp::RowPeak*)s->d_res1,
                     (const long long*)s->d_d1, (const int64_t*)s->d_len1, (const float*)s->d_ir, (const int64_t*)s->d_off2,
                     (const int*)s->d_leader, s->ref_pair, (int)R, (int)M, s->d_s2, (long long)(s->d_ir2 - s->d_ir), (long long)s->pitch_ir,
                     s->d_off_al, s->d_rows, s->d_flags);
  hipLaunchKernelGGL(imp::shift_rows_kernel, rows_grid(s->row_len, B), dim3(256), 0, st, (const float*)s->d_ir, (const int64_t*)s->d_off2,
                     (const int64_t*)s->d_len2, (const long long*)s->d_d1, (const long long*)s->d_s2, s->d_ir2, (const int64_t*)s->d_meta);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

// crop_tails: peak + Lundeby knee search of the cropped rows (K7c), the common length (truncation + fade-out: K5's loader)
static int slice_crop_tails(imp_slice* s, hipStream_t st, int64_t M, const int64_t* off_al) {
  const int64_t B = M * s->R;
  int rc;
  if ((rc = launch_first_peaks(st, s->d_ir, off_al, s->d_len2, B, s->d_chunk, s->knee_chunks, s->d_res2, s->peak_height, nullptr)) ||
      (rc = launch_knee_search(st, s->d_ir, off_al, s->d_len2, B, s->row_len, s->fs, KneeScratch{s->d_res2, s->d_max, s->d_knee, s->d_means})))
    return rc;
  hipLaunchKernelGGL(imp::slice_keep_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, (const imp::KneeRow*)s->d_knee,
                     off_al, (const int64_t*)s->d_len2, (int)s->R, (int)M, (long long)s->fade_out, (long long)s->keep_cap,
                     (long long)s->taps, s->d_keep, s->d_outlen, s->d_rows, s->d_meas, s->d_flags);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

// equalize: K5 over every row, straight from the rows it is given - offsets, lengths and the fade-out from the device
static int slice_equalize(imp_slice* s, hipStream_t st, int64_t M, const float* rows, const int64_t* off, long long fade_out, float* d_out,
                          int64_t out_pitch) {
  imp_plan* f = s->fir;
  f->cur_stream = st;
  imp::LoadRowsDeviceLen ld{rows, off, (const long long*)s->d_keep, (int)s->R, (long long)s->taps, fade_out, (const double*)s->d_win};
  return launch_fir_block(f, ld, M * s->R, d_out, out_pitch, 0);
}

// adjust decay: decay_params (K3 + K7c) + decay_times of the equalized rows that have a target, the window in place
static int slice_decay(imp_slice* s, hipStream_t st, int64_t M, float* d_out, int64_t out_pitch) {
  const int64_t R = s->R, B = M * R;
  int rc;
  hipLaunchKernelGGL(imp::slice_decay_rows_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const long long*)s->d_outlen, (int)R, (int)B,
                     (long long)out_pitch, s->d_off3, s->d_len3);
  if ((rc = launch_first_peaks(st, d_out, s->d_off3, s->d_len3, B, s->d_dchunk, s->dchunks, s->d_res3, s->peak_height, nullptr)) ||
      (rc = launch_knee_search(st, d_out, s->d_off3, s->d_len3, B, s->out_len_max, s->fs, KneeScratch{s->d_res3, s->d_max, s->d_knee, s->d_means})))
    return rc;
  hipLaunchKernelGGL(imp::slice_decay_jobs_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const imp::KneeRow*)s->d_knee,
                     (const double*)s->d_target, (int)R, (int)B, (long long)s->dscratch, s->d_jobs);
  hipLaunchKernelGGL(imp::decay_times_kernel<float>, dim3((unsigned)B), dim3(imp::kDecayThreads), 0, st, (const float*)d_out, (const imp::DecayJob*)s->d_jobs, s->d_dscr,
                     s->fs, s->d_rt);
  hipLaunchKernelGGL(imp::slice_decay_params_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, (const imp::KneeRow*)s->d_knee,
                     (const double*)s->d_rt, (const double*)s->d_target, (const int64_t*)s->d_len3, (int)R, (int)M, s->fs, s->d_dlen, s->d_dpar,
                     s->d_rows, s->d_flags);
  return launch_window_copy(st, d_out, s->d_off3, d_out, s->d_off3, s->d_dlen, s->d_dpar, s->out_len_max, B);
}

// normalize: maxima of the ear sums' spectra, gain on the device, applied in place
static int slice_normalize(imp_slice* s, hipStream_t st, int64_t M, float* d_out, int64_t out_pitch) {
  const int64_t R = s->R;
  int rc;
  if ((rc = slice_norm_run(s->ctx, s->norm, d_out, out_pitch, (int)R, (const long long*)s->d_outlen, M, s->d_peak_db))) return rc;
  hipLaunchKernelGGL(imp::slice_gain_kernel, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, st, (const double*)s->d_peak_db,
                     (const long long*)s->d_outlen, (int)R, (int)M, s->peak_target, s->guard_rel, (long long)out_pitch, s->d_g_off, s->d_g_len,
                     s->d_g_par, s->d_meas, s->d_flags);
  return launch_window_copy(st, d_out, s->d_g_off, d_out, s->d_g_off, s->d_g_len, s->d_g_par, s->out_len_max, M * R);
}

extern "C" int imp_slice_execute_device(imp_slice* s, const void* d_rec, int64_t rec_stride, int64_t M, float* d_out,
                                        int64_t out_pitch) {
  if (!s || !d_rec || !d_out) return fail(IMP_ERR_INVALID, "imp_slice_execute_device: null argument");
  imp_ctx* ctx = s->ctx;
  IMP_CTX_LOCK(ctx);
  if (M < 1 || M > s->m_cap) return fail(IMP_ERR_INVALID, "imp_slice_execute_device: %lld measurements, capacity %lld", (long long)M, (long long)s->m_cap);
  if (out_pitch < s->out_len_max) return fail(IMP_ERR_INVALID, "imp_slice_execute_device: out_pitch %lld < %lld (keep_cap + taps - 1)",
                                              (long long)out_pitch, (long long)s->out_len_max);
  if (M > 1 && rec_stride < 1) return fail(IMP_ERR_INVALID, "imp_slice_execute_device: rec_stride must be positive");
  if (!s->firs_set) return fail(IMP_ERR_INVALID, "imp_slice_execute_device: no FIRs yet (imp_slice_set_firs)");
  if (s->deconv->lanes != 1) return fail(IMP_ERR_INVALID, "imp_slice_execute_device: the deconvolution plan's overlap setting changed");
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  HIP_TRY(hipMemsetAsync(s->d_flags, 0, (size_t)M * sizeof(int), st));
  if ((rc = slice_ingest(s, d_rec, rec_stride, M)) || (rc = slice_first_peaks(s, st, M)) || (rc = slice_crop_heads(s, st, M))) return rc;
  if (s->align_on && (rc = slice_align(s, st, M))) return rc;
  const int64_t* off_al = s->align_on ? s->d_off_al : s->d_off2;
  if ((rc = slice_crop_tails(s, st, M, off_al))) return rc;
  if (s->vb_on) {                                          // its rows are truncated and faded already: K5 reads them as they are
    if ((rc = slice_vbass_run(s, st, M, s->d_ir, off_al)) || (rc = slice_equalize(s, st, M, s->d_vb, s->d_vb_off, 0, d_out, out_pitch))) return rc;
  } else if ((rc = slice_equalize(s, st, M, s->d_ir, off_al, s->fade_out, d_out, out_pitch))) {
    return rc;
  }
  if (s->decay_on && (rc = slice_decay(s, st, M, d_out, out_pitch))) return rc;
  if ((rc = slice_normalize(s, st, M, d_out, out_pitch))) return rc;
  // ---- the scalars, once
  const int64_t B = M * s->R;
  HIP_TRY(hipMemcpyAsync(s->h_rows, s->d_rows, (size_t)B * sizeof(imp::SliceRowOut), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_meas, s->d_meas, (size_t)M * sizeof(imp::SliceMeasOut), hipMemcpyDeviceToHost, st));
  s->last_M = M;
  return IMP_OK;
}

extern "C" int imp_slice_results(imp_slice* s, imp_slice_row_result* rows_out, imp_slice_result* meas_out) {
  if (!s) return fail(IMP_ERR_INVALID, "null slice");
  IMP_CTX_LOCK(s->ctx);
  int rc = ctx_bind(s->ctx);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  if (rows_out) std::memcpy(rows_out, s->h_rows, (size_t)(s->last_M * s->R) * sizeof(imp::SliceRowOut));
  if (meas_out) std::memcpy(meas_out, s->h_meas, (size_t)s->last_M * sizeof(imp::SliceMeasOut));
  return IMP_OK;
}

extern "C" int imp_slice_pack_f64(imp_slice* s, const float* d_out, int64_t out_pitch, int64_t M, double* d_packed, int64_t meas_stride) {
  if (!s || !d_out || !d_packed) return fail(IMP_ERR_INVALID, "imp_slice_pack_f64: null argument");
  IMP_CTX_LOCK(s->ctx);
  if (M < 1 || M > s->m_cap || M != s->last_M)
    return fail(IMP_ERR_INVALID, "imp_slice_pack_f64: %lld measurements, the last call had %lld", (long long)M, (long long)s->last_M);
  if (out_pitch < s->out_len_max || meas_stride < s->R * s->out_len_max)
    return fail(IMP_ERR_INVALID, "imp_slice_pack_f64: out_pitch %lld / meas_stride %lld too small for %lld rows of %lld", (long long)out_pitch,
                (long long)meas_stride, (long long)s->R, (long long)s->out_len_max);
  int rc = ctx_bind(s->ctx);
  if (rc) return rc;
  const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (s->out_len_max + 2047) / 2048));
  hipLaunchKernelGGL(imp::slice_pack_f64_kernel, dim3(bx, (unsigned)(M * s->R)), dim3(256), 0, s->ctx->stream, d_out, (long long)out_pitch,
                     (const long long*)s->d_outlen, (int)s->R, d_packed, (long long)meas_stride);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

// slice_pack_pcm_kernel over M measurements of R rows (pitch apart) whose lengths are on the device, at most max_len
static int pack_pcm_launch(hipStream_t st, const float* d_rows, int64_t pitch, const long long* d_len, int64_t R, int64_t M,
                           int64_t max_len, int bits, int32_t* d_packed, int64_t meas_stride) {
  int64_t tile = 1;                                  // frames per workgroup: a [tile][R] block of about 16 KiB, at most 512 frames
  while (tile < 512 && 2 * tile * R <= 4096) tile *= 2;
  const size_t lds = (size_t)(tile * (R | 1)) * sizeof(int32_t);
  const unsigned bx = (unsigned)std::max<int64_t>(1, (max_len + tile - 1) / tile);
  hipLaunchKernelGGL(imp::slice_pack_pcm_kernel, dim3(bx, (unsigned)M), dim3(256), lds, st, d_rows, (long long)pitch, d_len, (int)R,
                     (int)tile, 32 - bits, (int*)d_packed, (long long)meas_stride);
  HIP_TRY(hipGetLastError());
  return IMP_OK;
}

extern "C" int imp_slice_pack_pcm(imp_slice* s, const float* d_out, int64_t out_pitch, int64_t M, int bits, int32_t* d_packed,
                                  int64_t meas_stride) {
  if (!s || !d_out || !d_packed) return fail(IMP_ERR_INVALID, "imp_slice_pack_pcm: null argument");
  if (bits != 16 && bits != 24 && bits != 32) return fail(IMP_ERR_INVALID, "imp_slice_pack_pcm: %d bits (16, 24 or 32)", bits);
  IMP_CTX_LOCK(s->ctx);
  if (M < 1 || M > s->m_cap || M != s->last_M)
    return fail(IMP_ERR_INVALID, "imp_slice_pack_pcm: %lld measurements, the last call had %lld", (long long)M, (long long)s->last_M);
  if (out_pitch < s->out_len_max || meas_stride < s->R * s->out_len_max)
    return fail(IMP_ERR_INVALID, "imp_slice_pack_pcm: out_pitch %lld / meas_stride %lld too small for %lld rows of %lld", (long long)out_pitch,
                (long long)meas_stride, (long long)s->R, (long long)s->out_len_max);
  int rc = ctx_bind(s->ctx);
  if (rc) return rc;
  return pack_pcm_launch(s->ctx->stream, d_out, out_pitch, (const long long*)s->d_outlen, s->R, M, s->out_len_max, bits, d_packed,
                         meas_stride);
}

extern "C" int imp_pack_pcm_device(imp_ctx* ctx, const float* d_rows, int64_t pitch, const int64_t* d_len, int64_t rows_per_meas,
                                   int64_t M, int64_t max_len, int bits, int32_t* d_packed, int64_t meas_stride) {
  if (!ctx || !d_rows || !d_len || !d_packed) return fail(IMP_ERR_INVALID, "imp_pack_pcm_device: null argument");
  if (bits != 16 && bits != 24 && bits != 32) return fail(IMP_ERR_INVALID, "imp_pack_pcm_device: %d bits (16, 24 or 32)", bits);
  if (rows_per_meas < 1 || rows_per_meas > 8192 || M < 1 || M > 65535 || max_len < 0 || pitch < max_len ||
      meas_stride < rows_per_meas * max_len)
    return fail(IMP_ERR_INVALID, "imp_pack_pcm_device: bad sizes");
  IMP_CTX_LOCK(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  return pack_pcm_launch(ctx->stream, d_rows, pitch, (const long long*)d_len, rows_per_meas, M, max_len, bits, d_packed, meas_stride);
}

extern "C" int imp_host_alloc(imp_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out) return fail(IMP_ERR_INVALID, "imp_host_alloc: null argument");
  *out = nullptr;
  IMP_CTX_LOCK(ctx);
  int rc = ctx_bind(ctx);
  if (rc) return rc;
  if (!bytes) return IMP_OK;
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable));
  return IMP_OK;
}

extern "C" int imp_host_free(void* p) {
  if (!p) return IMP_OK;
  HIP_TRY(hipHostFree(p));
  return IMP_OK;
}
