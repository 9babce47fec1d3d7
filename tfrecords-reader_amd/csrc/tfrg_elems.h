// tfrg_elems.h — arguments of the four kernels of tfrg_elems.hip behind tfrg_result_ragged_elems: every
// element of a bytes_list slot for a list of rows, as packed bytes + element offsets ([E + 1]) + row
// offsets ([m + 1], in elements). Shared with tfrg_capi.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kElemsMaxSpecs = 32;  // (tfrg.h TFRG_ELEMS_MAX_SPECS)
// k_el_scan's workgroup: it takes that many tile sums per pass and carries across passes
constexpr uint32_t kElemsScanThreads = 1024;
// A copying workgroup takes 16-byte units [chunk * kElemsChunk, + kElemsChunk) of its tile's span, for
// the s-th of S consecutive runs of chunks as the s-th of the tile's S workgroups
constexpr uint32_t kElemsChunk = 1024;
constexpr uint32_t kElemsMaxSplit = 256;
constexpr uint32_t kElemsNoLen = 0xffffffffu;    // ElemsSpec::const_len: the bytes_len column is stored
constexpr int32_t kElemsOffStored = 0x7fffffff;  // ElemsSpec::const_off: the bytes_off column is stored

// One requested output
struct ElemsSpec {
  uint8_t* values;        // [cap], or null (offsets and counters only)
  int64_t* elem_offsets;  // [elem_cap + 1], or null (row offsets and counters only)
  int64_t* row_offsets;   // [m + 1]
  uint64_t elem_cap;      // elements that elem_offsets describes: entries above elem_cap are not stored
  uint64_t cap;           // bytes that values can hold: positions >= cap are not stored
  uint32_t slot;
  uint32_t max_elems;     // 0: every element of a row
  uint32_t max_len;       // 0: whole elements
  uint32_t const_len;     // under TFRG_IMPLICIT_BYTES_LEN: every element's length; else kElemsNoLen
  int32_t const_off;      // under tfrg_info.implicit_off_slots: the element of record g lies at
                          // end32[g] + const_off (such a slot is placed); else kElemsOffStored
  uint32_t pad;
};
static_assert(sizeof(ElemsSpec) == 64, "32 of them and the header fit the kernel argument");

// Kernel argument of all four kernels (read with scalar loads: every field a workgroup uses is
// uniform over it)
struct ElemsArgs {
  const uint32_t* rs;         // [n_slots][n + 1] row splits (rows of placed slots are not read)
  const uint64_t* slot_base;  // [n_slots]
  const uint32_t* b_off;      // bytes views into `in` (null: materialized)
  const uint32_t* b_len;
  const uint32_t* end32;      // [n] the decode's u32 record ends (read for specs with a const_off only)
  const uint64_t* b_off64;    // materialized: element e is in[b_off64[e], b_off64[e + 1])
  const uint8_t* in;          // the batch (views) or the materialized byte column
  const uint32_t* info;       // the decode's info words (kInfoPlacedLo / Hi read on the device)
  uint32_t* stats;            // [n_specs][4] rows truncated, elements truncated, empty, skipped; or null
  uint64_t* totals;           // [n_specs][2] E, B; or null
  uint64_t* tsum;             // [2][n_specs][tiles] scratch: the tiles' element counts, then their byte
                              // sums; after k_el_scan their exclusive bases
  const void* rows;           // [m] int32, or int64 with rows64; null: entry k is k
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;          // readable bytes of `in` (a multiple of 4): reads past it give 0
  uint32_t n;
  uint32_t n_specs;
  uint32_t tile;              // rows per tile
  uint32_t tiles;             // ceil(m / tile) >= 1
  uint32_t split;             // S: copying workgroups per tile; 0: no spec has bytes to store
  // (fill_columns' common view: the numeric columns are not read here)
  const int64_t* i64;
  const uint32_t* f32;
  ElemsSpec sp[kElemsMaxSpecs];
};
static_assert(sizeof(ElemsArgs) <= 4096, "the spec table travels as the kernel argument");

// dynamic LDS of the kernels that hold a tile's row table (every carve a multiple of 16 bytes)
constexpr size_t elems_lds_bytes(uint32_t tile) { return ((size_t)tile + 2u) * 8u + (size_t)tile * 4u + 128u; }

// (m > 0 and n > 0)
hipError_t launch_elems(const ElemsArgs& a, hipStream_t st);

}  // namespace tfrg
