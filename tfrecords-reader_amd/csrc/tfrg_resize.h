// tfrg_resize.h — arguments of k_resize (tfrg_resize.hip) and k_resize_aa (tfrg_resize_aa.hip, the
// antialiased specs), the kernels behind tfrg_result_raw_resize:
// element 0 of a bytes_list slot read as an H x W x channels image whose H and W are int64 features of the
// same record, a per-row crop window resampled (bilinear or nearest, optionally mirrored) to a fixed
// out_h x out_w, normalised per channel and written interleaved or planar, for a list of rows.
// Shared with tfrg_fixed.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "tfrg_raw.h"

namespace tfrg {

constexpr uint32_t kResizeMaxSpecs = 16;        // (tfrg.h TFRG_RESIZE_MAX_SPECS)
constexpr uint32_t kResizeMaxChannels = 4;      // (tfrg.h TFRG_RESIZE_MAX_CHANNELS)
constexpr uint32_t kResizeMaxOut = 4096;        // (tfrg.h TFRG_RESIZE_MAX_OUT): out_h, out_w, out_w * channels
constexpr uint32_t kResizeMaxSrc = 16384;       // (tfrg.h TFRG_RESIZE_MAX_SRC): H, W
constexpr uint32_t kResizeMaxRowBytes = 16384;  // (tfrg.h TFRG_RESIZE_MAX_ROW_BYTES): a crop row
constexpr uint32_t kResizeConst = 0xffffffffu;  // (tfrg.h TFRG_RESIZE_CONST)
enum ResizeInterp : uint32_t { kResizeBilinear = 0, kResizeNearest, kResizeInterps };
constexpr uint32_t kResizeAntialias = 0x100u;   // (tfrg.h TFRG_RESIZE_ANTIALIAS): OR-ed into interp; k_resize_aa

// A work item is a band of kResizeBand consecutive output rows of one list entry.
constexpr uint32_t kResizeBand = 16;

// LDS of a workgroup, in words: the row stage (a crop row of kResizeMaxRowBytes, laid out as k_raw's
// tile), then, sized by the launch for its largest spec, the ring of two resampled rows (out_w * channels
// float32 each) and the column table (out_w entries of two words).
constexpr uint32_t kResizeStageWords = 4352;
__host__ __device__ constexpr uint32_t resize_lds_words(uint32_t out_w, uint32_t channels) {
  return kResizeStageWords + 2u * out_w * channels + 2u * out_w;
}

// k_resize_aa (tfrg_resize_aa.hip). A work item is a band of resize_aa_band() output rows; its source rows
// are staged and resampled horizontally in groups of up to resize_aa_group() rows (fewer where fewer crop
// rows fit the stage). Both follow from the output row's length rn = out_w * channels alone, so the
// launcher and the kernel agree without a field: about 24 KiB for the band's accumulators and 12 KiB for
// the group's horizontal results, at most 8 and 4 rows (224 x 3: 8 and 4), at least 2 and 1 (rn = 4096).
constexpr uint32_t kResizeAaMaxBand = 8, kResizeAaMaxGroup = 4;
__host__ __device__ constexpr uint32_t resize_aa_band(uint32_t rn) {
  const uint32_t b = 6144u / rn;
  return b > kResizeAaMaxBand ? kResizeAaMaxBand : b < 2u ? 2u : b;
}
__host__ __device__ constexpr uint32_t resize_aa_group(uint32_t rn) {
  const uint32_t g = 3072u / rn;
  return g > kResizeAaMaxGroup ? kResizeAaMaxGroup : g < 1u ? 1u : g;
}
// LDS of a workgroup, in words: the stage, the group's horizontal results, the band's accumulators, the
// column table (three words per output column) and the band's row table (four words per output row).
__host__ __device__ constexpr uint32_t resize_aa_lds_words(uint32_t out_w, uint32_t channels) {
  const uint32_t rn = out_w * channels;
  return kResizeStageWords + (resize_aa_group(rn) + resize_aa_band(rn)) * rn + 3u * out_w + 4u * kResizeAaMaxBand;
}

// One requested output. Workgroups [blk0, blk0 + nblk) of the launch work inside it and stride over its
// m * bands work items.
struct ResizeSpec {
  void* out;         // [m][out_h * out_w * channels] of the output type
  int32_t* shapes;   // [m][2] or null
  uint32_t fill;     // raw low bits of a bad row's value, in the output type
  uint32_t slot;
  uint32_t src;      // RawSrc
  uint32_t outt;     // RawOut
  uint32_t channels;
  uint32_t planar;
  uint32_t interp;
  uint32_t out_h, out_w;
  uint32_t h_slot, w_slot;  // int64_list slots, or kResizeConst
  uint32_t src_h, src_w;
  uint32_t const_len;  // as DenseSpec's
  int32_t const_off;   // as DenseSpec's
  uint32_t blk0;
  uint32_t nblk;
  uint32_t bands;  // work items per row
  float scale[kResizeMaxChannels];
  float bias[kResizeMaxChannels];
};

// Kernel argument (the common fields are named as DenseArgs's: tfrg_rows.h and fill_columns read them)
struct ResizeArgs {
  const uint32_t* rs;
  const uint64_t* slot_base;
  const int64_t* i64;         // int64 values, or (i64_w 4 / 2) the narrow column of a narrowed decode: read by col_i64
  uint32_t i64_w;             // bytes per element of i64: 8, 4 or 2 (tfrg_info.i64_width)
  const uint32_t* f32;  // (not read)
  const uint32_t* b_off;
  const uint32_t* b_len;
  const uint32_t* end32;
  const uint64_t* b_off64;
  const uint8_t* in;
  const uint32_t* info;
  uint32_t* stats;    // [n_specs][4] or null
  const void* rows;   // [m] int32, or int64 with rows64; null: row k is record k - row0
  uint32_t* skipped;  // [n_specs] or null
  const int32_t* boxes;  // [m][4] top, left, height, width; null: the whole image
  const uint8_t* flips;  // [m]; null: none
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;
  uint32_t n;
  uint32_t n_specs;
  uint32_t nt;
  ResizeSpec sp[kResizeMaxSpecs];
};
static_assert(sizeof(ResizeArgs) <= 4096, "k_resize's spec table travels as the kernel argument");

// lds_bytes: resize_lds_words of the launch's largest spec, in bytes
hipError_t launch_resize(const ResizeArgs& a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st);
// the same for k_resize_aa over the antialiased specs of a call (lds_bytes: resize_aa_lds_words)
hipError_t launch_resize_aa(const ResizeArgs& a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st);

}  // namespace tfrg
