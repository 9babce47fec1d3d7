// tfrg_ragged.h — arguments of the three kernels of tfrg_ragged.hip behind tfrg_result_ragged_rows:
// the ragged columns of a decoded batch as packed values + offsets ([m + 1], cu_seqlens) for a list of
// rows. Shared with tfrg_capi.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kRaggedMaxSpecs = 64;  // (tfrg.h TFRG_RAGGED_MAX_SPECS)
// rows per workgroup tile (tfrg_ctx_set_ragged_tile): a power of two
constexpr uint32_t kRaggedTileMin = 64, kRaggedTileMax = 4096, kRaggedTileDefault = 1024;
// k_rg_scan's workgroup: it takes that many tile sums per pass and carries across passes
constexpr uint32_t kRaggedScanThreads = 1024;
// A gathering workgroup takes 16-byte units [chunk * kRaggedChunk, + kRaggedChunk) of its tile's span,
// chunk = s, s + S, ... for the s-th of the tile's S workgroups
constexpr uint32_t kRaggedChunk = 1024;
constexpr uint32_t kRaggedMaxSplit = 256;
constexpr uint32_t kRaggedNoLen = 0xffffffffu;  // RaggedSpec::const_len: the bytes_len column is stored
constexpr int32_t kRaggedOffStored = 0x7fffffff;  // RaggedSpec::const_off: the bytes_off column is stored

// One requested output
struct RaggedSpec {
  void* values;        // [cap] of the dtype, or null (offsets and counters only)
  int64_t* offsets;    // [m + 1]
  uint64_t cap;        // elements that values can hold: positions >= cap are not stored
  uint32_t slot;
  uint32_t dtype;      // DenseType
  uint32_t max_len;    // 0: whole rows
  uint32_t const_len;  // bytes slot under TFRG_IMPLICIT_BYTES_LEN: every element's length; else kRaggedNoLen
  int32_t const_off;   // bytes slot under tfrg_info.implicit_off_slots: the element of record g lies at
                       // end32[g] + const_off; else kRaggedOffStored
};

// Kernel argument of all three kernels (read with scalar loads: every field a workgroup uses is
// uniform over it)
struct RaggedArgs {
  const uint32_t* rs;         // [n_slots][n + 1] row splits (rows of placed slots are not read)
  const uint64_t* slot_base;  // [n_slots]
  const int64_t* i64;
  const uint32_t* f32;
  const uint32_t* b_off;      // bytes views into `in` (null: materialized)
  const uint32_t* b_len;
  const uint32_t* end32;      // [n] the decode's u32 record ends (read for specs with a const_off only)
  const uint64_t* b_off64;    // materialized: element e is in[b_off64[e], b_off64[e + 1])
  const uint8_t* in;          // the batch (views) or the materialized byte column
  const uint32_t* info;       // the decode's info words (kInfoPlacedLo / Hi read on the device)
  uint32_t* stats;            // [n_specs][4] truncated, empty, multi, skipped; or null
  uint64_t* totals;           // [n_specs] offsets[m]; or null
  uint64_t* tsum;             // [n_specs][tiles] scratch: the tiles' sums, then their exclusive bases
  const void* rows;           // [m] int32, or int64 with rows64; null: entry k is k
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;          // readable bytes of `in` (a multiple of 4): reads past it give 0
  uint32_t n;
  uint32_t n_specs;
  uint32_t tile;              // rows per tile
  uint32_t tiles;             // ceil(m / tile) >= 1
  uint32_t split;             // S: gathering workgroups per tile
  RaggedSpec sp[kRaggedMaxSpecs];
};
static_assert(sizeof(RaggedArgs) <= 4096, "the spec table travels as the kernel argument");

// (m > 0 and n > 0)
hipError_t launch_ragged(const RaggedArgs& a, hipStream_t st);

}  // namespace tfrg
