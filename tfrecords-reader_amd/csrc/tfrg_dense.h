// tfrg_dense.h — arguments of k_dense (tfrg_dense.hip), the collate kernel behind tfrg_result_dense
// and tfrg_result_dense_rows: ragged result columns -> fixed-shape [n][width] outputs, or [m][width]
// outputs whose row k is record rows[k] - row0. Shared with tfrg_capi.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kDenseMaxSpecs = 64;    // (tfrg.h TFRG_DENSE_MAX_SPECS)
constexpr uint32_t kDenseMaxWidth = 4096;  // (tfrg.h TFRG_DENSE_MAX_WIDTH)
enum DenseType : uint32_t { kDenseI64 = 0, kDenseI32 = 1, kDenseF32 = 2, kDenseU8 = 3 };  // (TFRG_DENSE_*)
constexpr uint32_t kDenseNoLen = 0xffffffffu;  // DenseSpec::const_len: the bytes_len column is stored
constexpr int32_t kDenseOffStored = 0x7fffffff;  // DenseSpec::const_off: the bytes_off column is stored (a real
                                                 // offset is negative: the element lies before the record's end)

// A workgroup covers 16-byte units [chunk * kDenseChunk, + kDenseChunk) of one output, 4 per lane
constexpr uint32_t kDenseChunk = 1024;

// One requested output. Workgroups [blk0, blk0 + nblk) of the launch work inside it, workgroup b on
// chunks b - blk0, b - blk0 + nblk, ... of its flat row-major bytes.
struct DenseSpec {
  void* out;           // [n][width] of the dtype ([m][width] with a row list)
  int32_t* lengths;    // [n] ([m]) or null
  uint64_t fill;       // raw low bits of the pad value
  uint32_t slot;
  uint32_t dtype;      // DenseType
  uint32_t width;
  uint32_t const_len;  // bytes slot under TFRG_IMPLICIT_BYTES_LEN: every element's length; else kDenseNoLen
  uint32_t blk0;
  uint32_t nblk;
  int32_t const_off;   // bytes slot under tfrg_info.implicit_off_slots: the element of record g lies at
                       // end32[g] + const_off; else kDenseOffStored
};

// Kernel argument (read with scalar loads: every field a workgroup uses is uniform over it)
struct DenseArgs {
  const uint32_t* rs;          // [n_slots][n + 1] row splits (rows of placed slots are not read)
  const uint64_t* slot_base;   // [n_slots]
  const int64_t* i64;
  const uint32_t* f32;
  const uint32_t* b_off;       // bytes views into `in` (null: materialized)
  const uint32_t* b_len;
  const uint32_t* end32;       // [n] the decode's u32 record ends (read for specs with a const_off only)
  const uint64_t* b_off64;     // materialized: element e is in[b_off64[e], b_off64[e + 1])
  const uint8_t* in;           // the batch (views) or the materialized byte column
  const uint32_t* info;        // the decode's info words (kInfoPlacedLo / Hi read on the device)
  uint32_t* stats;             // [n_specs][4] or null
  // the row list (k_dense_rows only): output row k < m is record rows[k] - row0 where that is
  // in [0, n), and is left unwritten and counted in skipped[spec] where it is not
  const void* rows;            // [m] int32, or int64 with rows64
  uint32_t* skipped;           // [n_specs] or null
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;           // readable bytes of `in` (a multiple of 4): reads past it give 0
  uint32_t n;
  uint32_t n_specs;
  uint32_t nt;                 // nontemporal output stores
  DenseSpec sp[kDenseMaxSpecs];
};
static_assert(sizeof(DenseArgs) <= 4096, "k_dense's spec table travels as the kernel argument");

hipError_t launch_dense(const DenseArgs& a, uint32_t blocks, hipStream_t st);

}  // namespace tfrg
