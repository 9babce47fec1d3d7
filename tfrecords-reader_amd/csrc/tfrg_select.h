// tfrg_select.h — arguments of the three kernels of tfrg_select.hip behind tfrg_result_select_rows and
// tfrg_result_select_match: predicates over the decoded columns of a list of candidate rows in, the
// entries of the passing candidates compacted into a device row list out. Shared with tfrg_capi.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kSelMaxTerms = 32;  // (tfrg.h TFRG_SEL_MAX_TERMS); groups are numbered below 32 too
// candidates per workgroup tile (tfrg_ctx_set_select_tile): a power of two, a multiple of the wave
constexpr uint32_t kSelTileMin = 64, kSelTileMax = 4096, kSelTileDefault = 1024;
// k_sel_scan's workgroup: it takes that many tile sums per pass and carries across passes
constexpr uint32_t kSelScanThreads = 1024;
constexpr uint32_t kSelNoLen = 0xffffffffu;  // SelTerm::const_len: the bytes_len column is stored
constexpr int32_t kSelOffStored = 0x7fffffff;  // SelectBytesArgs::const_off: the bytes_off column is stored
// byte-string operands (tfrg.h TFRG_SEL_MAX_PATTERN, TFRG_SEL_MAX_PATTERN_BYTES)
constexpr uint32_t kSelMaxPattern = 256, kSelMaxPatternBytes = 2048;
// CONTAINS: elements longer than this many bytes are scanned by their wave (tfrg_ctx_set_select_scan)
constexpr uint32_t kSelScanMin = 4, kSelScanMax = 65536, kSelScanDefault = 256;

enum SelSubject : uint32_t {  // (TFRG_SEL_*)
  kSelValue = 0, kSelAny = 1, kSelCount = 2, kSelBytesLen = 3, kSelStatus = 4, kSelBytes = 5, kSelBytesAny = 6
};
enum SelOp : uint32_t {
  kSelEq = 0, kSelNe = 1, kSelLt = 2, kSelLe = 3, kSelGt = 4, kSelGe = 5, kSelPrefix = 6, kSelSuffix = 7, kSelContains = 8
};

// One term, as the kernel takes it. Every subject ends in one signed 64-bit compare `lhs op rhs`:
// floats are compared through sel_float_key (an integer key in the order of the values, -0.0 on
// 0.0), with NaN on either side decided apart (true under NE alone).
struct SelTerm {
  int64_t rhs;         // the operand; float slots: its key; kSelBytes / kSelBytesAny: pattern offset | length << 32
  uint32_t slot;
  uint32_t subject;    // SelSubject
  uint32_t op;         // SelOp
  uint32_t group;      // < 32
  uint32_t index;      // kSelValue: which value of the list
  uint32_t is_float;   // kSelValue / kSelAny on a float_list slot
  uint32_t rhs_nan;    // the float operand is a NaN
  uint32_t const_len;  // kSelBytesLen under TFRG_IMPLICIT_BYTES_LEN: every element's length; else kSelNoLen
};

// the bits of a float that is not a NaN -> a key ordered as the values are (host and device)
__host__ __device__ inline int64_t sel_float_key(uint32_t u) {
  if (u == 0x80000000u) u = 0u;  // -0.0 == 0.0
  return (u & 0x80000000u) ? (int64_t)(int32_t)(0x80000000u - u) : (int64_t)u;
}
__host__ __device__ inline bool sel_float_nan(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u; }

// Kernel argument of all three kernels (read with scalar loads: every field is uniform)
struct SelectArgs {
  const uint32_t* rs;         // [n_slots][n + 1] row splits (rows of placed slots are not read)
  const uint64_t* slot_base;  // [n_slots]
  const int64_t* i64;
  const uint32_t* f32;
  const uint32_t* b_len;      // bytes views' lengths (not read where the length is constant)
  const uint64_t* b_off64;    // materialized: element e is b_off64[e + 1] - b_off64[e] bytes long; else null
  const int32_t* status;      // [n], or null under TFRG_IMPLICIT_STATUS (every status is 0)
  const uint32_t* info;       // the decode's info words (kInfoPlacedLo / Hi read on the device)
  uint32_t* stats;            // [2] selected by this call, skipped; or null
  uint64_t* count;            // *d_count
  uint64_t* words;            // [ceil(m / 64)] scratch: bit l of word w is the verdict of candidate 64 w + l
  uint64_t* tsum;             // [tiles] scratch: the tiles' selected counts, then their first positions
  const void* rows;           // [m] int32, or int64 with rows64; null: entry k is k
  void* out;                  // [cap] int32, or int64 with out64; or null
  uint64_t cap;
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t out64;
  uint32_t n;
  uint32_t n_terms;
  uint32_t all_groups;        // bit g: group g occurs among the terms
  uint32_t tile;              // candidates per tile
  uint32_t tiles;             // ceil(m / tile) >= 1
  uint32_t append;            // positions start at *count as the scan kernel finds it
  uint32_t pad_;
  SelTerm term[kSelMaxTerms];
};
static_assert(sizeof(SelectArgs) <= 4096, "the term table travels as the kernel argument");

// Kernel argument of k_sel_eval's instantiation for term tables with a kSelBytes / kSelBytesAny term
// (the other two kernels take its SelectArgs): the bytes' source, as RaggedArgs has it, and the patterns
struct SelectBytesArgs {
  SelectArgs s;
  const uint32_t* b_off;      // bytes views into `in` (not read where materialized or implicit)
  const uint32_t* end32;      // [n] the decode's u32 record ends (read for terms with a const_off only)
  const uint8_t* in;          // the batch (views) or the materialized byte column
  uint32_t in_bound;          // readable bytes of `in` (a multiple of 16): bytes past it are 0
  uint32_t scan_min;          // CONTAINS: elements longer than this take the wave scan
  int32_t const_off[kSelMaxTerms];  // bytes term under tfrg_info.implicit_off_slots: the element of record g
                                    // lies at end32[g] + const_off; else kSelOffStored
  // the operands back to back, read as aligned dword pairs (hence the words after the last pattern byte)
  uint32_t pat[kSelMaxPatternBytes / 4 + 2];
};
static_assert(sizeof(SelectBytesArgs) <= 4096, "the patterns travel as the kernel argument");

// (m > 0 and n > 0)
hipError_t launch_select(const SelectArgs& a, hipStream_t st);
// the same three launches with the bytes instantiation of the first
hipError_t launch_select_bytes(const SelectBytesArgs& a, hipStream_t st);

}  // namespace tfrg
