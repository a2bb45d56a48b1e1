// Ragged rows: a base pointer plus off[B] / len[B].  What the entry points of the row stages share (impulse_hip.hip,
// analysis.hip): the check of the row table, the way of small tables to the device, and the pooled block that holds
// uploaded rows for a call.  Uses only what internal.h exports.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "internal.h"

struct RowSpan {
  int64_t extent = 0, total = 0, maxlen = 0;      // max(off + len), sum of len, longest row
};
static constexpr int64_t kAnyLen = INT64_MAX;     // rows_check: no limit on a row's length

// the row table of `who`: refused when B < 0, a table is missing, an entry is negative or a row is longer than max_len
static int rows_check(const char* who, const int64_t* off, const int64_t* len, int64_t B, int64_t max_len, RowSpan* out) {
  *out = RowSpan();
  if (B < 0) return fail(IMP_ERR_INVALID, "%s: B < 0", who);
  if (B > 0 && (!off || !len)) return fail(IMP_ERR_INVALID, "%s: null row table", who);
  for (int64_t b = 0; b < B; ++b) {
    if (off[b] < 0 || len[b] < 0) return fail(IMP_ERR_INVALID, "%s: negative offset/length in row %lld", who, (long long)b);
    if (len[b] > max_len)
      return fail(IMP_ERR_UNSUPPORTED, "%s: row %lld has %lld samples (limit %lld)", who, (long long)b, (long long)len[b],
                  (long long)max_len);
    out->extent = std::max(out->extent, off[b] + len[b]);
    out->total += len[b];
    out->maxlen = std::max(out->maxlen, len[b]);
  }
  return IMP_OK;
}

// N host tables through the staging ring: laid out 8-byte aligned in ONE allocation and sent with ONE copy in stream
// order; dev[i] = where piece i lies on the device (valid as ctx_stage says)
struct TablePiece {
  const void* host;
  size_t bytes;
};
template <size_t N>
static int ctx_stage_tables(imp_ctx* ctx, const TablePiece (&piece)[N], void* (&dev)[N]) {
  size_t at[N], bytes = 0;
  for (size_t i = 0; i < N; ++i) {
    at[i] = bytes;
    bytes += (piece[i].bytes + 7) & ~(size_t)7;
  }
  bytes = std::max<size_t>(bytes, 8);
  char *h = nullptr, *d = nullptr;
  int rc = ctx_stage(ctx, bytes, (void**)&h, (void**)&d);
  if (rc) return rc;
  for (size_t i = 0; i < N; ++i) {
    if (piece[i].bytes) std::memcpy(h + at[i], piece[i].host, piece[i].bytes);
    dev[i] = d + at[i];
  }
  return ctx_stage_push(ctx, h, d, bytes);
}

// A pooled block for the length of a call: whichever way the call ends, the stream is drained and the block handed back.
// release(): the block lives on with a new owner (a segment set).
struct BlockHold {
  imp_ctx* ctx;
  void* p = nullptr;
  explicit BlockHold(imp_ctx* c) : ctx(c) {}
  BlockHold(const BlockHold&) = delete;
  BlockHold& operator=(const BlockHold&) = delete;
  ~BlockHold() {
    if (!p) return;
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx_block_put(ctx, p);
  }
  int get(size_t bytes) { return ctx_block_get(ctx, bytes, &p); }
  void* release() {
    void* q = p;
    p = nullptr;
    return q;
  }
};

// host rows x[0, extent) into a pooled block, as they are (the kernels read Sample = T)
template <class T>
static int upload_rows(imp_ctx* ctx, const char* who, const T* x, int64_t extent, BlockHold& rows) {
  int rc = rows.get((size_t)std::max<int64_t>(extent, 1) * sizeof(T));
  if (rc) return rc;
  if (extent > 0) {
    const hipError_t e = hipMemcpyAsync(rows.p, x, (size_t)extent * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return fail(IMP_ERR_HIP, "%s: h2d: %s", who, hipGetErrorString(e));
  }
  return IMP_OK;
}
