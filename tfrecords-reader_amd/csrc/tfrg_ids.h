// tfrg_ids.h — arguments of the three kernels of tfrg_ids.hip behind tfrg_result_elem_ids: one int64 id
// per element of a bytes_list slot for a list of rows (a vocabulary lookup, hash buckets, or both), with
// the row offsets ([m + 1], in elements) of tfrg_result_ragged_elems. Shared with tfrg_capi.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kIdsMaxSpecs = 32;  // (tfrg.h TFRG_IDS_MAX_SPECS)
// k_id_scan's workgroup: it takes that many tile sums per pass and carries across passes
constexpr uint32_t kIdsScanThreads = 1024;
constexpr uint32_t kIdsNoLen = 0xffffffffu;    // IdsSpec::const_len: the bytes_len column is stored
constexpr int32_t kIdsOffStored = 0x7fffffff;  // IdsSpec::const_off: the bytes_off column is stored

// One requested output
struct IdsSpec {
  int64_t* ids;          // [elem_cap], or null (offsets and counters only)
  int64_t* row_offsets;  // [m + 1]
  uint64_t elem_cap;     // positions >= elem_cap of ids are not stored
  // the vocabulary's device arrays (tfrg_vocab.h); table null: hash buckets only
  const uint32_t* table;   // [mask + 1] word index, or kVocabEmpty
  const uint32_t* w_offs;  // [n_words + 1]
  const uint8_t* blob;
  const int64_t* w_ids;    // [n_words]
  uint64_t n_buckets;      // 0: an unmatched element gets default_id
  int64_t oov_base;
  int64_t default_id;
  uint32_t slot;
  uint32_t max_elems;   // 0: every element of a row
  uint32_t const_len;   // as ElemsSpec::const_len
  int32_t const_off;    // as ElemsSpec::const_off
  uint32_t mask;        // the table's capacity - 1
  uint32_t max_probe;   // no word lies further from its home slot
  uint32_t max_word;    // no word is longer
  uint32_t blob_bound;  // readable bytes of blob (a multiple of 4): reads past it give 0
};
static_assert(sizeof(IdsSpec) == 112, "32 of them and the header fit the kernel argument");

// Kernel argument of all three kernels (read with scalar loads: every field a workgroup uses is
// uniform over it). The first fields are those of ElemsArgs: fill_columns and fill_bytes_source fill them.
struct IdsArgs {
  const uint32_t* rs;         // [n_slots][n + 1] row splits (rows of placed slots are not read)
  const uint64_t* slot_base;  // [n_slots]
  const uint32_t* b_off;      // bytes views into `in` (null: materialized)
  const uint32_t* b_len;
  const uint32_t* end32;      // [n] the decode's u32 record ends (read for specs with a const_off only)
  const uint64_t* b_off64;    // materialized: element e is in[b_off64[e], b_off64[e + 1])
  const uint8_t* in;          // the batch (views) or the materialized byte column
  const uint32_t* info;       // the decode's info words (kInfoPlacedLo / Hi read on the device)
  uint32_t* stats;            // [n_specs][4] rows truncated, elements unmatched, empty, skipped; or null
  uint64_t* totals;           // [n_specs] E; or null
  uint64_t* tsum;             // [n_specs][tiles] scratch: the tiles' element counts; after k_id_scan
                              // their exclusive bases
  const void* rows;           // [m] int32, or int64 with rows64; null: entry k is k
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;          // readable bytes of `in` (a multiple of 4): reads past it give 0
  uint32_t n;
  uint32_t n_specs;
  uint32_t tile;              // rows per tile
  uint32_t tiles;             // ceil(m / tile) >= 1
  uint32_t pad;
  // (fill_columns' common view: the numeric columns are not read here)
  const int64_t* i64;
  const uint32_t* f32;
  IdsSpec sp[kIdsMaxSpecs];
};
static_assert(sizeof(IdsArgs) <= 4096, "the spec table travels as the kernel argument");

// dynamic LDS of the kernels that hold a tile's row table (every carve a multiple of 16 bytes)
constexpr size_t ids_lds_bytes(uint32_t tile) { return ((size_t)tile + 2u) * 8u + (size_t)tile * 4u + 64u; }

// (m > 0 and n > 0)
hipError_t launch_ids(const IdsArgs& a, hipStream_t st);

}  // namespace tfrg
