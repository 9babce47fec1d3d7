// tfrg_tokens.h — arguments of the three kernels of tfrg_tokens.hip behind tfrg_result_token_ids: the
// elements of a bytes_list slot split into tokens at ASCII delimiter bytes, one int64 id per token (the
// id rule of tfrg_ids.h) and the row offsets ([m + 1], in tokens) for a list of rows. Shared with
// tfrg_rowlist.cpp and, for the default split, tfrg_ctx.h only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kTokMaxSpecs = 16;  // (tfrg.h TFRG_TOK_MAX_SPECS; 28 TokSpecs would still fit the argument)
constexpr uint32_t kTokLowerAscii = 1u;  // (tfrg.h TFRG_TOK_LOWER_ASCII)
// k_tok_scan's workgroup: it takes that many tile sums per pass and carries across passes
constexpr uint32_t kTokScanThreads = 1024;
constexpr uint32_t kTokNoLen = 0xffffffffu;    // TokSpec::const_len: the bytes_len column is stored
constexpr int32_t kTokOffStored = 0x7fffffff;  // TokSpec::const_off: the bytes_off column is stored
// tfrg_ctx_set_token_split: a row of at most that many bytes is one lane's work, a longer one a wave's
constexpr uint32_t kTokSplitMin = 8, kTokSplitMax = 65536, kTokSplitDefault = 256;

// One requested output
struct TokSpec {
  int64_t* ids;          // [tok_cap], or null (offsets and counters only)
  int64_t* row_offsets;  // [m + 1]; between k_tok_count and k_tok_write entry k holds row k's count
  uint64_t tok_cap;      // positions >= tok_cap of ids are not stored
  // the vocabulary's device arrays (tfrg_vocab.h); table null: hash buckets only
  const uint32_t* table;   // [mask + 1] word index, or kVocabEmpty
  const uint32_t* w_offs;  // [n_words + 1]
  const uint8_t* blob;
  const int64_t* w_ids;    // [n_words]
  uint64_t n_buckets;      // 0: an unmatched token gets default_id
  int64_t oov_base;
  int64_t default_id;
  uint64_t delims[2];   // bit b: ASCII byte b separates tokens (never both 0: the host fills the default)
  uint32_t slot;
  uint32_t max_elems;   // 0: every element of a row
  uint32_t max_tokens;  // 0: every token of a row
  uint32_t lower;       // 1: A..Z of a token hash and compare as a..z
  uint32_t const_len;   // as ElemsSpec::const_len
  int32_t const_off;    // as ElemsSpec::const_off
  uint32_t mask;        // the table's capacity - 1
  uint32_t max_probe;   // no word lies further from its home slot
  uint32_t max_word;    // no word is longer
  uint32_t blob_bound;  // readable bytes of blob (a multiple of 4): reads past it give 0
};
static_assert(sizeof(TokSpec) == 136, "16 of them and the header fit the kernel argument");

// Kernel argument of all three kernels (read with scalar loads: every field a workgroup uses is
// uniform over it). The first fields are those of ElemsArgs: fill_columns and fill_bytes_source fill them.
struct TokArgs {
  const uint32_t* rs;         // [n_slots][n + 1] row splits (rows of placed slots are not read)
  const uint64_t* slot_base;  // [n_slots]
  const uint32_t* b_off;      // bytes views into `in` (null: materialized)
  const uint32_t* b_len;
  const uint32_t* end32;      // [n] the decode's u32 record ends (read for specs with a const_off only)
  const uint64_t* b_off64;    // materialized: element e is in[b_off64[e], b_off64[e + 1])
  const uint8_t* in;          // the batch (views) or the materialized byte column
  const uint32_t* info;       // the decode's info words (kInfoPlacedLo / Hi read on the device)
  uint32_t* stats;            // [n_specs][4] rows cut at max_tokens, tokens unmatched, rows without a
                              // token, rows skipped; or null
  uint64_t* totals;           // [n_specs] T; or null
  uint64_t* tsum;             // [n_specs][tiles] scratch: the tiles' token counts; after k_tok_scan
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
  uint32_t split;             // kTokSplitMin .. kTokSplitMax
  // (fill_columns' common view: the numeric columns are not read here)
  const int64_t* i64;   // (not read)
  uint32_t i64_w;       // (fill_columns sets it beside i64)
  const uint32_t* f32;
  TokSpec sp[kTokMaxSpecs];
};
static_assert(sizeof(TokArgs) <= 4096, "the spec table travels as the kernel argument");

// dynamic LDS of the kernels that hold a tile's row table (tfrg_rows.h; every carve a multiple of 16 bytes)
constexpr size_t tok_lds_bytes(uint32_t tile) { return ((size_t)tile + 2u) * 8u + (size_t)tile * 4u + 64u; }

// (m > 0 and n > 0)
hipError_t launch_tokens(const TokArgs& a, hipStream_t st);

}  // namespace tfrg
