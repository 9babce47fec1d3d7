// tfrg_raw.h — arguments of k_raw (tfrg_raw.hip), the kernel behind tfrg_result_raw_rows: element 0 of
// a bytes_list slot read as a tensor of a fixed element type (tf.io.decode_raw), cast, scaled per
// channel and written as [m][count] rows, interleaved or planar (HWC -> CHW), for a list of rows.
// Shared with tfrg_fixed.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kRawMaxSpecs = 16;        // (tfrg.h TFRG_RAW_MAX_SPECS)
constexpr uint32_t kRawMaxCount = 1u << 24;  // (tfrg.h TFRG_RAW_MAX_COUNT)
constexpr uint32_t kRawMaxChannels = 16;     // (tfrg.h TFRG_RAW_MAX_CHANNELS)
// (TFRG_RAW_*: the source element types, little-endian)
enum RawSrc : uint32_t { kRawU8 = 0, kRawI8, kRawU16, kRawI16, kRawI32, kRawF16, kRawBF16, kRawF32, kRawSrcs };
enum RawOut : uint32_t { kRawOutF32 = 0, kRawOutF16, kRawOutBF16, kRawOutSame, kRawOuts };  // (TFRG_RAW_OUT_*)
constexpr uint32_t kRawNoLen = 0xffffffffu;    // RawSpec::const_len: the bytes_len column is stored
constexpr int32_t kRawOffStored = 0x7fffffff;  // RawSpec::const_off: the bytes_off column is stored

__host__ __device__ constexpr uint32_t raw_src_size(uint32_t src) {
  return src <= kRawI8 ? 1u : (src == kRawI32 || src == kRawF32) ? 4u : 2u;
}
__host__ __device__ constexpr uint32_t raw_out_size(uint32_t src, uint32_t out) {
  return out == kRawOutF32 ? 4u : out == kRawOutSame ? raw_src_size(src) : 2u;
}

// A tile: kRawTile elements of one row at the most, in whole pixels (groups of `channels` elements)
// and a multiple of 16 of them, so that a tile starts a 16-byte unit of every output type in every
// plane. A work item is kRawSpan consecutive tiles of one row; a row of at most kRawNarrow elements is
// one tile that a single wave works on (four rows per workgroup at a time).
constexpr uint32_t kRawTile = 4096;
constexpr uint32_t kRawNarrow = 1024;
constexpr uint32_t kRawSpan = 4;
__host__ __device__ constexpr uint32_t raw_tile_pixels(uint32_t channels) { return (kRawTile / channels) & ~15u; }

// One requested output. Workgroups [blk0, blk0 + nblk) of the launch work inside it and stride over
// its work items (wide rows: m * spans of them; narrow rows: the m rows, a wave each).
struct RawSpec {
  void* out;          // [m][count] of the output type
  int32_t* lengths;   // [m] or null
  uint32_t fill;      // raw low bits of the pad value, in the output type
  uint32_t slot;
  uint32_t src;       // RawSrc
  uint32_t outt;      // RawOut
  uint32_t count;     // elements per row
  uint32_t channels;
  uint32_t planar;
  uint32_t const_len;  // as DenseSpec's
  int32_t const_off;   // as DenseSpec's
  uint32_t blk0;
  uint32_t nblk;
  uint32_t spans;      // work items per wide row
  float scale[kRawMaxChannels];
  float bias[kRawMaxChannels];
};

// Kernel argument (the common fields are named as DenseArgs's: tfrg_rows.h and fill_columns read them)
struct RawArgs {
  const uint32_t* rs;
  const uint64_t* slot_base;
  const int64_t* i64;   // (not read)
  uint32_t i64_w;       // (fill_columns sets it beside i64)
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
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;
  uint32_t n;
  uint32_t n_specs;
  uint32_t nt;
  RawSpec sp[kRawMaxSpecs];
};
static_assert(sizeof(RawArgs) <= 4096, "k_raw's spec table travels as the kernel argument");

hipError_t launch_raw(const RawArgs& a, uint32_t blocks, hipStream_t st);

}  // namespace tfrg
