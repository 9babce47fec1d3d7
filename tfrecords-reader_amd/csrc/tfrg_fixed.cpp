// tfrg_fixed.cpp -- the fixed-shape views of the last result (include/tfrg.h): dense tensors on
// result_dense; raw tensors, resized images and log-mel spectrograms for a list of rows on one frame,
// result_fixed_rows; and the tables of a mel transform. The context and the setup shared with the other
// views are in tfrg_ctx.h.
#include <string.h>

#include <cmath>

#include "tfrg_ctx.h"
#include "tfrg_mel.h"
#include "tfrg_raw.h"
#include "tfrg_resize.h"

// The row list of tfrg_result_dense_rows (d_rows null: tfrg_result_dense, every record in order)
struct DenseRows {
  const void* d_rows = nullptr;
  uint32_t dtype = 0, m = 0;
  int64_t row0 = 0;
  uint32_t* d_skipped = nullptr;
};

static int result_dense(const char* fn, bool by_rows, tfrg_ctx* c, const tfrg_dense_spec* specs, uint32_t n_specs,
                        const DenseRows& rows, uint32_t* d_stats, void* consumer_stream) {
  auto bad = [fn](const std::string& why) {
    set_error(std::string(fn) + ": " + why);
    return TFRG_E_ARG;
  };
  if (const int rc = check_specs(c, specs, n_specs, TFRG_DENSE_MAX_SPECS, bad)) return rc;
  static_assert(TFRG_DENSE_MAX_SPECS == kDenseMaxSpecs && TFRG_DENSE_MAX_WIDTH == kDenseMaxWidth &&
                    TFRG_DENSE_I64 == kDenseI64 && TFRG_DENSE_I32 == kDenseI32 && TFRG_DENSE_F32 == kDenseF32 &&
                    TFRG_DENSE_U8 == kDenseU8,
                "tfrg.h mirrors tfrg_dense.h");
  for (uint32_t i = 0; i < n_specs; ++i) {
    const tfrg_dense_spec& s = specs[i];
    const std::string at = "spec " + std::to_string(i) + ": ";
    if (const int rc = check_slot_dtype(c, at, s.slot, s.dtype, bad)) return rc;
    if (s.width == 0 || s.width > TFRG_DENSE_MAX_WIDTH)
      return bad(at + "width must be 1.." + std::to_string(TFRG_DENSE_MAX_WIDTH));
    if (!s.out) return bad(at + "out is NULL");
    if (s.reserved) return bad(at + "reserved must be 0");
  }
  if (by_rows) {
    if (const int rc = check_rows_dtype(rows.d_rows, rows.dtype, true, bad)) return rc;
    if (const int rc = check_rows_m(rows.d_rows, rows.m, true, bad)) return rc;
  }
  if (!by_rows && c->res.req.n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = confirm_pending(c)) return rc;
  // the rows of every output
  const uint32_t out_rows = by_rows ? rows.m : c->res.req.n;
  DenseArgs a{};
  if (by_rows) {
    a.rows = rows.d_rows;
    a.rows64 = rows.dtype == TFRG_ROWS_I64;
    a.m = rows.m;
    a.row0 = rows.row0;
    a.skipped = rows.d_skipped;
  }
  fill_columns(c, a);
  fill_bytes_source(c, a);
  a.stats = d_stats;
  a.n_specs = n_specs;
  a.nt = (uint32_t)c->sw.dense_nt;
  // workgroups per spec: one per chunk of its output, within an even share of 16 per CU
  const uint64_t cap = std::max<uint64_t>(1, (uint64_t)c->num_cus * 16u / n_specs);
  uint32_t blocks = 0;
  for (uint32_t i = 0; i < n_specs; ++i) {
    const tfrg_dense_spec& s = specs[i];
    DenseSpec& d = a.sp[i];
    d.out = s.out;
    d.lengths = s.lengths;
    d.fill = s.fill;
    d.slot = s.slot;
    d.dtype = s.dtype;
    d.width = s.width;
    d.const_len = const_len_of(c, s.slot, s.dtype == TFRG_DENSE_U8);
    d.const_off = const_off_of(c, s.slot, s.dtype == TFRG_DENSE_U8);
    const uint64_t isz = s.dtype == TFRG_DENSE_I64 ? 8 : s.dtype == TFRG_DENSE_U8 ? 1 : 4;
    const uint64_t total = (uint64_t)out_rows * s.width * isz;
    // 16-byte units, or single elements where the output's base is not 16-byte aligned
    const uint64_t work = ((uintptr_t)s.out & 15u) ? total / isz : (total >> 4) + 16;
    d.blk0 = blocks;
    d.nblk = (uint32_t)std::min<uint64_t>(cap, (work + kDenseChunk - 1) / kDenseChunk);
    blocks += d.nblk;
  }
  hipStream_t st, cs;
  if (const int rc = fence_open(c, consumer_stream, &st, &cs)) return rc;
  // (counters that lie back to back, stats first, are zeroed by one memset: one launch less per step)
  const bool one_memset = by_rows && c->res.req.n && d_stats && rows.d_skipped == d_stats + 4 * (size_t)n_specs;
  if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_specs * (one_memset ? 20 : 16), st));
  // (a row list over an empty result: no record to read, every row is skipped)
  if (by_rows && rows.d_skipped && !one_memset)
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rows.d_skipped), c->res.req.n ? 0 : (int)rows.m, n_specs, st));
  if (out_rows && c->res.req.n) HIP_TRY(launch_dense(a, blocks, st));
  return fence_close(c, st, cs);
}

int tfrg_result_dense(tfrg_ctx* c, const tfrg_dense_spec* specs, uint32_t n_specs, uint32_t* d_stats,
                      void* consumer_stream) {
  return result_dense("tfrg_result_dense", false, c, specs, n_specs, DenseRows{}, d_stats, consumer_stream);
}

int tfrg_result_dense_rows(tfrg_ctx* c, const tfrg_dense_spec* specs, uint32_t n_specs, const void* d_rows,
                           uint32_t rows_dtype, uint32_t m, int64_t row0, uint32_t* d_stats, uint32_t* d_skipped,
                           void* consumer_stream) {
  DenseRows rows;
  rows.d_rows = d_rows;
  rows.dtype = rows_dtype;
  rows.m = m;
  rows.row0 = row0;
  rows.d_skipped = d_skipped;
  return result_dense("tfrg_result_dense_rows", true, c, specs, n_specs, rows, d_stats, consumer_stream);
}

// ---- The frame of the entry points that write one fixed-shape output per spec for a list of rows
// (tfrg_result_raw_rows, _raw_resize, _mel): the checks in the one order all three make them, the
// confirmation, the consumer fence and the counters, the row list and the column view of the argument
// struct, around what an entry point brings as its own.
// check(spec, at, bad): the spec's own checks.
// call_check(bad): what the call checks beyond its specs and its row list, after both.
// launch(a, st): the spec table of `a` and its own fields (the common ones are filled), then its kernels;
// called only where there is a row and a record.
// Nothing is written on the device before every check has passed.
template <class Args, class Spec, class Check, class CallCheck, class Launch>
static int result_fixed_rows(const char* fn, uint32_t max_specs, tfrg_ctx* c, const Spec* specs, uint32_t n_specs,
                             const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0, uint32_t* d_stats,
                             uint32_t* d_skipped, void* consumer_stream, const Check& check,
                             const CallCheck& call_check, const Launch& launch) {
  auto bad = [fn](const std::string& why) {
    set_error(std::string(fn) + ": " + why);
    return TFRG_E_ARG;
  };
  if (const int rc = check_specs(c, specs, n_specs, max_specs, bad)) return rc;
  for (uint32_t i = 0; i < n_specs; ++i)
    if (const int rc = check(specs[i], "spec " + std::to_string(i) + ": ", bad)) return rc;
  if (const int rc = check_rows_dtype(d_rows, rows_dtype, false, bad)) return rc;
  if (const int rc = check_rows_m(d_rows, m, false, bad)) return rc;
  if (const int rc = call_check(bad)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = confirm_pending(c)) return rc;
  hipStream_t st, cs;
  if (const int rc = fence_open(c, consumer_stream, &st, &cs)) return rc;
  if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_specs * 16, st));
  // (a row list over an empty result: no record to read, every row is skipped)
  if (d_skipped)
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_skipped), c->res.req.n ? 0 : (int)m, n_specs, st));
  if (m && c->res.req.n) {
    Args a{};
    a.rows = d_rows;
    a.rows64 = d_rows && rows_dtype == TFRG_ROWS_I64;
    a.m = m;
    a.row0 = row0;
    a.skipped = d_skipped;
    fill_columns(c, a);
    fill_bytes_source(c, a);
    a.stats = d_stats;
    a.n_specs = n_specs;
    if (const int rc = launch(a, st)) return rc;
  }
  return fence_close(c, st, cs);
}
static const auto no_call_check = [](const auto&) { return 0; };

// The checks and the fill word that the specs of the three share (tfrg_raw.h has the types)
template <class Bad>
static int check_src_out(const std::string& at, uint32_t src, uint32_t out, const Bad& bad) {
  if (src >= kRawSrcs) return bad(at + "unknown src " + std::to_string(src));
  if (out >= kRawOuts) return bad(at + "unknown out " + std::to_string(out));
  return 0;
}
template <class Bad>
static int check_out_ptr(const std::string& at, const void* out_ptr, uint32_t src, uint32_t out, const Bad& bad) {
  if (!out_ptr) return bad(at + "out_ptr is NULL");
  if ((uintptr_t)out_ptr & (raw_out_size(src, out) - 1u)) return bad(at + "out_ptr must be aligned to the output element size");
  return 0;
}
// (the fill's bits, masked to the width of an output element)
static uint32_t fill_bits(uint32_t src, uint32_t out, uint32_t fill) {
  const uint32_t osz = raw_out_size(src, out);
  return osz == 4 ? fill : fill & ((1u << (8 * osz)) - 1u);
}

// Raw tensors from bytes features for a list of rows (tfrg_raw.h): one launch, all specs. Its own are the
// spec table and the split into work items.
int tfrg_result_raw_rows(tfrg_ctx* c, const tfrg_raw_spec* specs, uint32_t n_specs, const void* d_rows,
                         uint32_t rows_dtype, uint32_t m, int64_t row0, uint32_t* d_stats, uint32_t* d_skipped,
                         void* consumer_stream) {
  static_assert(TFRG_RAW_MAX_SPECS == kRawMaxSpecs && TFRG_RAW_MAX_COUNT == kRawMaxCount &&
                    TFRG_RAW_MAX_CHANNELS == kRawMaxChannels && TFRG_RAW_U8 == kRawU8 && TFRG_RAW_I8 == kRawI8 &&
                    TFRG_RAW_U16 == kRawU16 && TFRG_RAW_I16 == kRawI16 && TFRG_RAW_I32 == kRawI32 &&
                    TFRG_RAW_F16 == kRawF16 && TFRG_RAW_BF16 == kRawBF16 && TFRG_RAW_F32 == kRawF32 &&
                    TFRG_RAW_OUT_F32 == kRawOutF32 && TFRG_RAW_OUT_F16 == kRawOutF16 &&
                    TFRG_RAW_OUT_BF16 == kRawOutBF16 && TFRG_RAW_OUT_SAME == kRawOutSame,
                "tfrg.h mirrors tfrg_raw.h");
  static_assert(sizeof(tfrg_raw_spec) == 176, "tfrg.h states the size");
  static_assert(kRawNoLen == kDenseNoLen && kRawOffStored == kDenseOffStored, "const_len_of / const_off_of serve k_raw");
  return result_fixed_rows<RawArgs>(
      "tfrg_result_raw_rows", TFRG_RAW_MAX_SPECS, c, specs, n_specs, d_rows, rows_dtype, m, row0, d_stats, d_skipped,
      consumer_stream,
      [c](const tfrg_raw_spec& s, const std::string& at, const auto& bad) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (const int rc = check_src_out(at, s.src, s.out, bad)) return rc;
        if (s.count == 0 || s.count > TFRG_RAW_MAX_COUNT) return bad(at + "count must be 1.." + std::to_string(TFRG_RAW_MAX_COUNT));
        if (s.channels == 0 || s.channels > TFRG_RAW_MAX_CHANNELS)
          return bad(at + "channels must be 1.." + std::to_string(TFRG_RAW_MAX_CHANNELS));
        if (s.count % s.channels) return bad(at + "count must be a multiple of channels");
        if (s.planar > 1) return bad(at + "planar must be 0 or 1");
        if (const int rc = check_out_ptr(at, s.out_ptr, s.src, s.out, bad)) return rc;
        if (s.reserved) return bad(at + "reserved must be 0");
        return 0;
      },
      no_call_check,
      [c, specs](RawArgs& a, hipStream_t st) -> int {
        a.nt = (uint32_t)c->sw.dense_nt;
        // workgroups per spec: one per work item (wide rows: kRawSpan tiles; narrow rows: four rows, a wave
        // each), within an even share of 32 per CU; they stride over what is left
        const uint64_t cap = std::max<uint64_t>(1, (uint64_t)c->num_cus * 32u / a.n_specs);
        uint32_t blocks = 0;
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_raw_spec& s = specs[i];
          RawSpec& d = a.sp[i];
          d.out = s.out_ptr;
          d.lengths = s.lengths;
          d.fill = fill_bits(s.src, s.out, s.fill);
          d.slot = s.slot;
          d.src = s.src;
          d.outt = s.out;
          d.count = s.count;
          d.channels = s.channels;
          d.planar = s.planar;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
          const uint32_t tp = raw_tile_pixels(s.channels), tiles = (s.count / s.channels + tp - 1) / tp;
          d.spans = (tiles + kRawSpan - 1) / kRawSpan;
          const uint64_t work = s.count > kRawNarrow ? (uint64_t)a.m * d.spans : ((uint64_t)a.m + 3) / 4;
          d.blk0 = blocks;
          d.nblk = (uint32_t)std::min<uint64_t>(cap, work);
          blocks += d.nblk;
          memcpy(d.scale, s.scale, sizeof d.scale);
          memcpy(d.bias, s.bias, sizeof d.bias);
        }
        HIP_TRY(launch_raw(a, blocks, st));
        return 0;
      });
}

// Resized raw images for a list of rows (tfrg_resize.h): one launch of k_resize for all plain specs and
// one of k_resize_aa for all antialiased ones. Its own are the int64 slots of the shape, the geometry of
// the outputs, the boxes and flips, the split into bands and each launch's LDS.
int tfrg_result_raw_resize(tfrg_ctx* c, const tfrg_resize_spec* specs, uint32_t n_specs, const void* d_rows,
                           uint32_t rows_dtype, uint32_t m, int64_t row0, const int32_t* d_boxes,
                           const uint8_t* d_flip, uint32_t* d_stats, uint32_t* d_skipped, void* consumer_stream) {
  static_assert(TFRG_RESIZE_MAX_SPECS == kResizeMaxSpecs && TFRG_RESIZE_MAX_CHANNELS == kResizeMaxChannels &&
                    TFRG_RESIZE_MAX_OUT == kResizeMaxOut && TFRG_RESIZE_MAX_SRC == kResizeMaxSrc &&
                    TFRG_RESIZE_MAX_ROW_BYTES == kResizeMaxRowBytes && TFRG_RESIZE_CONST == kResizeConst &&
                    TFRG_RESIZE_BILINEAR == kResizeBilinear && TFRG_RESIZE_NEAREST == kResizeNearest &&
                    TFRG_RESIZE_ANTIALIAS == kResizeAntialias,
                "tfrg.h mirrors tfrg_resize.h");
  static_assert(sizeof(tfrg_resize_spec) == 104, "tfrg.h states the size");
  return result_fixed_rows<ResizeArgs>(
      "tfrg_result_raw_resize", TFRG_RESIZE_MAX_SPECS, c, specs, n_specs, d_rows, rows_dtype, m, row0, d_stats, d_skipped,
      consumer_stream,
      [c](const tfrg_resize_spec& s, const std::string& at, const auto& bad) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (const int rc = check_src_out(at, s.src, s.out, bad)) return rc;
        if (s.interp == (TFRG_RESIZE_NEAREST | TFRG_RESIZE_ANTIALIAS))
          return bad(at + "TFRG_RESIZE_ANTIALIAS filters: it goes with TFRG_RESIZE_BILINEAR only");
        if (s.interp >= kResizeInterps && s.interp != (TFRG_RESIZE_BILINEAR | TFRG_RESIZE_ANTIALIAS))
          return bad(at + "unknown interp " + std::to_string(s.interp));
        if (s.out == TFRG_RAW_OUT_SAME && s.interp != TFRG_RESIZE_NEAREST)
          return bad(at + "TFRG_RAW_OUT_SAME copies bits: it goes with TFRG_RESIZE_NEAREST only");
        if (s.channels == 0 || s.channels > TFRG_RESIZE_MAX_CHANNELS)
          return bad(at + "channels must be 1.." + std::to_string(TFRG_RESIZE_MAX_CHANNELS));
        if (s.out_h == 0 || s.out_h > TFRG_RESIZE_MAX_OUT || s.out_w == 0 || s.out_w > TFRG_RESIZE_MAX_OUT)
          return bad(at + "out_h and out_w must be 1.." + std::to_string(TFRG_RESIZE_MAX_OUT));
        if (s.out_w * s.channels > TFRG_RESIZE_MAX_OUT)
          return bad(at + "out_w * channels must be at most " + std::to_string(TFRG_RESIZE_MAX_OUT));
        const struct {
          const char* what;
          uint32_t slot, konst;
        } ext[2] = {{"h_slot", s.h_slot, s.src_h}, {"w_slot", s.w_slot, s.src_w}};
        for (const auto& e : ext) {
          if (e.slot == TFRG_RESIZE_CONST) {
            if (e.konst == 0 || e.konst > TFRG_RESIZE_MAX_SRC)
              return bad(at + "a constant extent must be 1.." + std::to_string(TFRG_RESIZE_MAX_SRC));
          } else if (e.slot >= c->n_slots || (c->slot_kind_h[e.slot] & 3u) != TFRG_KIND_INT64) {
            return bad(at + e.what + " " + std::to_string(e.slot) + " is not an int64_list slot");
          }
        }
        if (s.planar > 1) return bad(at + "planar must be 0 or 1");
        if (const int rc = check_out_ptr(at, s.out_ptr, s.src, s.out, bad)) return rc;
        if ((uintptr_t)s.shapes & 3u) return bad(at + "shapes must be 4-byte aligned");
        if (s.reserved) return bad(at + "reserved must be 0");
        return 0;
      },
      [d_boxes](const auto& bad) -> int { return ((uintptr_t)d_boxes & 3u) ? bad("d_boxes must be 4-byte aligned") : 0; },
      [c, specs, d_boxes, d_flip](ResizeArgs& a, hipStream_t st) -> int {
        a.boxes = d_boxes;
        a.flips = d_flip;
        a.nt = (uint32_t)c->sw.dense_nt;
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_resize_spec& s = specs[i];
          ResizeSpec& d = a.sp[i];
          d.out = s.out_ptr;
          d.shapes = s.shapes;
          d.fill = fill_bits(s.src, s.out, s.fill);
          d.slot = s.slot;
          d.src = s.src;
          d.outt = s.out;
          d.channels = s.channels;
          d.planar = s.planar;
          d.interp = s.interp;
          d.out_h = s.out_h;
          d.out_w = s.out_w;
          d.h_slot = s.h_slot;
          d.w_slot = s.w_slot;
          d.src_h = s.src_h;
          d.src_w = s.src_w;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
          memcpy(d.scale, s.scale, sizeof d.scale);
          memcpy(d.bias, s.bias, sizeof d.bias);
        }
        // Per kernel, the blk0 table of its launch: workgroups per spec of its kind, one per band of a row, within
        // an even share of 8 per CU (what the LDS of the common sizes lets a CU hold, and more); they stride over
        // what is left. A spec of the other kind has no workgroup, so no block index selects it; the spec index,
        // and with it the counters, are the call's in both launches.
        const uint64_t cap = std::max<uint64_t>(1, (uint64_t)c->num_cus * 8u / a.n_specs);
        for (const bool aa : {false, true}) {
          uint32_t blocks = 0, lds_words = 0;
          for (uint32_t i = 0; i < a.n_specs; ++i) {
            ResizeSpec& d = a.sp[i];
            const bool mine = ((d.interp & kResizeAntialias) != 0) == aa;
            const uint32_t band = aa ? resize_aa_band(d.out_w * d.channels) : kResizeBand;
            d.bands = (d.out_h + band - 1) / band;
            d.blk0 = blocks;
            d.nblk = mine ? (uint32_t)std::min<uint64_t>(cap, (uint64_t)a.m * d.bands) : 0u;
            blocks += d.nblk;
            if (mine) lds_words = std::max(lds_words, (aa ? resize_aa_lds_words : resize_lds_words)(d.out_w, d.channels));
          }
          HIP_TRY((aa ? launch_resize_aa : launch_resize)(a, blocks, lds_words * 4u, st));
        }
        return 0;
      });
}

// ---- The tables of a mel transform (tfrg_mel.h has their layout): the windowed cos / -sin basis and the
// filterbank, each in the order the lanes of k_mel load it, built in float64 and rounded once.
int tfrg_mel_create(int device, uint32_t n_fft, const float* window, uint32_t n_mels, const float* fb, tfrg_mel** out) {
  auto bad = [](const std::string& why) {
    set_error("tfrg_mel_create: " + why);
    return TFRG_E_ARG;
  };
  static_assert(TFRG_MEL_MAX_FFT == kMelMaxFft && TFRG_MEL_MAX_MELS == kMelMaxMels && TFRG_MEL_MAX_SAMPLES == kMelMaxSamples &&
                    TFRG_MEL_MAX_FRAMES == kMelMaxFrames && TFRG_MEL_LINEAR == kMelLinear && TFRG_MEL_LN == kMelLn &&
                    TFRG_MEL_LOG10 == kMelLog10,
                "tfrg.h mirrors tfrg_mel.h");
  if (!out) return bad("out is NULL");
  *out = nullptr;
  if (device < 0) return bad("device must be a device ordinal");
  if (n_fft < 2 || n_fft > TFRG_MEL_MAX_FFT || (n_fft & 1u)) return bad("n_fft must be even and in 2.." + std::to_string(TFRG_MEL_MAX_FFT));
  if (n_mels == 0 || n_mels > TFRG_MEL_MAX_MELS) return bad("n_mels must be 1.." + std::to_string(TFRG_MEL_MAX_MELS));
  if (!window || !fb) return bad("window or fb is NULL");
  const uint32_t n_bins = n_fft / 2 + 1, KG = mel_k16(n_fft) / kMelKGroup, NCH = mel_chunks(n_fft), MT = mel_mtiles(n_mels);
  for (uint32_t k = 0; k < n_fft; ++k)
    if (!std::isfinite(window[k])) return bad("window[" + std::to_string(k) + "] is not finite");
  for (uint64_t i = 0; i < (uint64_t)n_mels * n_bins; ++i)
    if (!std::isfinite(fb[i])) return bad("fb[" + std::to_string(i) + "] is not finite");
  const uint64_t nb = mel_basis_words(n_fft), nf = mel_fb_words(n_fft, n_mels);
  std::vector<float> h;
  tfrg_mel* mel = new (std::nothrow) tfrg_mel;
  try {
    h.assign(nb + nf, 0.f);
  } catch (const std::bad_alloc&) {
    delete mel;
    mel = nullptr;
  }
  if (!mel) {
    set_error("tfrg_mel_create: out of memory");
    return TFRG_E_NOMEM;
  }
  const double step = 6.283185307179586476925286766559 / (double)n_fft;
  for (uint32_t bt = 0; bt < NCH * 4u; ++bt)
    for (uint32_t kg = 0; kg < KG; ++kg)
      for (uint32_t lane = 0; lane < 64; ++lane)
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t k = kMelKGroup * kg + 4u * j + lane / 16u, col = lane % 16u, bin = kMelTileBins * bt + col / 2u;
          if (k >= n_fft || bin >= n_bins) continue;
          // (the angle reduced exactly: bin * k mod n_fft, before the trig call)
          const double ang = step * (double)(((uint64_t)bin * k) % n_fft);
          h[(((uint64_t)bt * KG + kg) * 64u + lane) * 4u + j] = (float)((double)window[k] * ((col & 1u) ? -std::sin(ang) : std::cos(ang)));
        }
  for (uint32_t mt = 0; mt < MT; ++mt)
    for (uint32_t ch = 0; ch < NCH; ++ch)
      for (uint32_t hh = 0; hh < 2; ++hh)
        for (uint32_t lane = 0; lane < 64; ++lane)
          for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t f = 16u * mt + lane % 16u, bin = kMelChunkBins * ch + 16u * hh + 4u * j + lane / 16u;
            if (f < n_mels && bin < n_bins) h[nb + ((((uint64_t)mt * NCH + ch) * 2u + hh) * 64u + lane) * 4u + j] = fb[(uint64_t)f * n_bins + bin];
          }
  void* p = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc(&p, h.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(p, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    if (p) (void)hipFree(p);
    delete mel;
    set_error(std::string("tfrg_mel_create: upload: ") + hipGetErrorString(e));
    return TFRG_E_HIP;
  }
  mel->device = device;
  mel->n_fft = n_fft;
  mel->n_mels = n_mels;
  mel->d_mem = p;
  mel->d_basis = static_cast<const float*>(p);
  mel->d_fb = mel->d_basis + nb;
  mel->device_bytes = h.size() * 4;
  *out = mel;
  return 0;
}

int tfrg_mel_destroy(tfrg_mel* mel) {
  if (!mel) return 0;
  HIP_TRY(hipSetDevice(mel->device));
  HIP_TRY(hipDeviceSynchronize());  // (work already queued may still read the tables)
  HIP_TRY(hipFree(mel->d_mem));
  delete mel;
  return 0;
}

int tfrg_mel_info(const tfrg_mel* mel, uint32_t* n_fft, uint32_t* n_mels, uint32_t* n_bins, uint64_t* device_bytes) {
  if (!mel) {
    set_error("tfrg_mel_info: mel is NULL");
    return TFRG_E_ARG;
  }
  if (n_fft) *n_fft = mel->n_fft;
  if (n_mels) *n_mels = mel->n_mels;
  if (n_bins) *n_bins = mel->n_fft / 2 + 1;
  if (device_bytes) *device_bytes = mel->device_bytes;
  return 0;
}

uint32_t tfrg_mel_tile_frames(uint32_t n_fft, uint32_t hop) {
  if (n_fft < 2 || n_fft > TFRG_MEL_MAX_FFT || hop == 0 || hop > n_fft) return 0;
  return mel_tile_frames(n_fft, hop);
}

// Log-mel spectrograms for a list of rows (tfrg_mel.h): one launch of k_mel per tile size among the specs
// (at most three). Its own are the framing checks and the tile of a spec.
int tfrg_result_mel(tfrg_ctx* c, const tfrg_mel_spec* specs, uint32_t n_specs, const void* d_rows, uint32_t rows_dtype,
                    uint32_t m, int64_t row0, uint32_t* d_stats, uint32_t* d_skipped, void* consumer_stream) {
  static_assert(sizeof(tfrg_mel_spec) == 88, "tfrg.h states the size");
  return result_fixed_rows<MelArgs>(
      "tfrg_result_mel", TFRG_RAW_MAX_SPECS, c, specs, n_specs, d_rows, rows_dtype, m, row0, d_stats, d_skipped,
      consumer_stream,
      [c](const tfrg_mel_spec& s, const std::string& at, const auto& bad) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (s.src >= kRawSrcs) return bad(at + "unknown src " + std::to_string(s.src));
        if (s.out >= kRawOutSame) return bad(at + "out must be TFRG_RAW_OUT_F32, _F16 or _BF16, not " + std::to_string(s.out));
        if (!s.mel) return bad(at + "mel is NULL");
        if (s.mel->device != c->device)
          return bad(at + "the tables are on device " + std::to_string(s.mel->device) + ", the context on " + std::to_string(c->device));
        const uint32_t n_fft = s.mel->n_fft;
        if (s.channels == 0 || s.channels > TFRG_RAW_MAX_CHANNELS) return bad(at + "channels must be 1.." + std::to_string(TFRG_RAW_MAX_CHANNELS));
        if (s.channel >= s.channels) return bad(at + "channel must be below channels");
        if (s.samples == 0 || s.samples > TFRG_MEL_MAX_SAMPLES) return bad(at + "samples must be 1.." + std::to_string(TFRG_MEL_MAX_SAMPLES));
        if (s.frames == 0 || s.frames > TFRG_MEL_MAX_FRAMES) return bad(at + "frames must be 1.." + std::to_string(TFRG_MEL_MAX_FRAMES));
        if (s.hop == 0 || s.hop > n_fft) return bad(at + "hop must be 1..n_fft");
        if (s.center > 1) return bad(at + "center must be 0 or 1");
        if (s.power != 1 && s.power != 2) return bad(at + "power must be 1 or 2");
        if (s.log >= kMelLogs) return bad(at + "unknown log " + std::to_string(s.log));
        if (s.log != TFRG_MEL_LINEAR && !(s.floor > 0.f && std::isfinite(s.floor))) return bad(at + "a log needs a finite floor > 0");
        if (!std::isfinite(s.scale) || !std::isfinite(s.bias)) return bad(at + "scale and bias must be finite");
        const uint64_t last = (uint64_t)(s.frames - 1) * s.hop;
        if (s.center) {
          if (s.samples <= n_fft / 2) return bad(at + "center reflects: samples must exceed n_fft / 2");
          if (last > s.samples) return bad(at + "the last frame's centre lies past samples");
        } else if (last + n_fft > s.samples) {
          return bad(at + "the last frame ends past samples");
        }
        if (const int rc = check_out_ptr(at, s.out_ptr, s.src, s.out, bad)) return rc;
        if ((uintptr_t)s.lengths & 3u) return bad(at + "lengths must be 4-byte aligned");
        if (s.reserved) return bad(at + "reserved must be 0");
        return 0;
      },
      no_call_check,
      [c, specs](MelArgs& a, hipStream_t st) -> int {
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_mel_spec& s = specs[i];
          MelSpec& d = a.sp[i];
          d.out = s.out_ptr;
          d.lengths = s.lengths;
          d.basis = s.mel->d_basis;
          d.fb = s.mel->d_fb;
          d.fill = fill_bits(s.src, s.out, s.fill);  // (a 16-bit output unless float32)
          d.slot = s.slot;
          d.src = s.src;
          d.outt = s.out;
          d.channels = s.channels;
          d.channel = s.channel;
          d.samples = s.samples;
          d.frames = s.frames;
          d.hop = s.hop;
          d.n_fft = s.mel->n_fft;
          d.n_mels = s.mel->n_mels;
          d.center = s.center;
          d.power = s.power;
          d.log = s.log;
          d.floor = s.floor;
          d.scale = s.scale;
          d.bias = s.bias;
          d.hop_magic = s.hop >= 2 ? (uint32_t)((0x100000000ull + s.hop - 1) / s.hop) : 0u;
          d.tf = mel_tile_frames(d.n_fft, d.hop);
          d.tiles = (d.frames + d.tf - 1) / d.tf;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
        }
        // Per tile size, the blk0 table of its launch (as tfrg_result_raw_resize's per kernel): a workgroup per
        // work item within an even share of 2 per CU -- what the LDS of a tile lets a CU hold -- striding over the rest.
        const uint64_t cap = std::max<uint64_t>(1, (uint64_t)c->num_cus * 2u / a.n_specs);
        for (const uint32_t tf : {64u, 32u, 16u}) {
          uint32_t blocks = 0, lds_words = 0;
          for (uint32_t i = 0; i < a.n_specs; ++i) {
            MelSpec& d = a.sp[i];
            d.blk0 = blocks;
            d.nblk = d.tf == tf ? (uint32_t)std::min<uint64_t>(cap, (uint64_t)a.m * d.tiles) : 0u;
            blocks += d.nblk;
            if (d.tf == tf) lds_words = std::max(lds_words, mel_lds_words(d.n_fft, d.hop, tf));
          }
          HIP_TRY(launch_mel(a, tf, blocks, lds_words * 4u, st));
        }
        return 0;
      });
}
