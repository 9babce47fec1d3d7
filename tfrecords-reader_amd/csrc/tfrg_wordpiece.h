// tfrg_wordpiece.h — arguments of the three kernels of tfrg_wordpiece.hip behind tfrg_result_wordpiece_ids:
// the elements of a bytes_list slot split into words (delimiters, isolated punctuation), every word cut
// greedily into the longest pieces of two vocabularies, one int64 id per piece and the row offsets
// ([m + 1], in pieces) for a list of rows. Shared with tfrg_rowlist.cpp only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace tfrg {

constexpr uint32_t kWpMaxSpecs = 16;     // (tfrg.h TFRG_WP_MAX_SPECS; 18 WpSpecs would still fit the argument)
constexpr uint32_t kWpLowerAscii = 1u;   // (tfrg.h TFRG_WP_LOWER_ASCII)
constexpr uint32_t kWpSpecial = 2u;      // (tfrg.h TFRG_WP_SPECIAL)
constexpr uint32_t kWpScanThreads = 1024;  // k_wp_scan's workgroup: tile sums per pass
constexpr uint32_t kWpNoLen = 0xffffffffu;    // WpSpec::const_len: the bytes_len column is stored
constexpr int32_t kWpOffStored = 0x7fffffff;  // WpSpec::const_off: the bytes_off column is stored
constexpr uint32_t kWpMaxWordBytes = 1024, kWpDefaultWordBytes = 100;  // (tfrg.h: max_word_bytes)
constexpr uint32_t kWpUnbounded = 0xffffffffu;  // WpSpec::limit: every piece of a row

// Lanes that probe the candidate ends of one piece together: a wave matches 64 / kWpG words a round.
// A build-time constant so that tools/wordpiece_speed.py can time the kernel against G = 1 (one lane
// walks a word's ends one after the other): make WP_G=1 BUILD=build_g1 OUT=.../libtfrg_g1.so
#ifndef TFRG_WP_G
#define TFRG_WP_G 8
#endif
constexpr uint32_t kWpG = TFRG_WP_G;
static_assert(kWpG == 1 || kWpG == 2 || kWpG == 4 || kWpG == 8 || kWpG == 16, "a group divides a wave and its stage");
constexpr uint32_t kWpStage = 16;  // pieces of a word its group holds back in registers (lane j: j, j + G, ...)
// words a sweep step can finish: 64 lanes of 8 bytes each, in which 8 isolated bytes and the end of the
// run that was open on entry make 9
constexpr uint32_t kWpQueue = 64 * 9;

// One vocabulary's device arrays (tfrg_vocab.h); table null: no such vocabulary
struct WpTab {
  const uint32_t* table;   // [mask + 1] word index, or kVocabEmpty
  const uint32_t* w_offs;  // [n_words + 1]
  const uint8_t* blob;
  const int64_t* w_ids;    // [n_words]
  uint32_t mask;           // the table's capacity - 1
  uint32_t max_probe;      // no word lies further from its home slot
  uint32_t max_word;       // no word is longer
  uint32_t blob_bound;     // readable bytes of blob (a multiple of 4): reads past it give 0
};

// One requested output
struct WpSpec {
  int64_t* ids;          // [tok_cap], or null (offsets and counters only)
  int64_t* row_offsets;  // [m + 1]; between k_wp_count and k_wp_write entry k holds row k's count
  uint64_t tok_cap;      // positions >= tok_cap of ids are not stored
  WpTab first;           // the pieces that may begin a word
  WpTab cont;            // the continuation pieces, without their prefix
  uint64_t delims[2];    // bit b: ASCII byte b separates words (never both 0: the host fills the default)
  uint64_t isolate[2];   // bit b: ASCII byte b is a word of its own (the host clears the delimiters from it)
  int64_t cls_id, sep_id, unk_id;
  uint32_t slot;
  uint32_t max_elems;       // 0: every element of a row
  uint32_t limit;           // pieces of a row besides cls / sep; kWpUnbounded: all of them
  uint32_t lower;           // 1: A..Z of a word hash and compare as a..z
  uint32_t special;         // 1: cls before and sep after the pieces of every row that is not skipped
  uint32_t const_len;       // as ElemsSpec::const_len
  int32_t const_off;        // as ElemsSpec::const_off
  uint32_t max_word_bytes;  // a longer word is unk_id (1 .. kWpMaxWordBytes)
};
static_assert(sizeof(WpSpec) == 208, "16 of them and the header fit the kernel argument");

// Kernel argument of all three kernels (read with scalar loads: every field a workgroup uses is
// uniform over it). The fields before `sp` are TokArgs's, name for name: fill_columns,
// fill_bytes_source and result_row_list fill them.
struct WpArgs {
  const uint32_t* rs;
  const uint64_t* slot_base;
  const uint32_t* b_off;
  const uint32_t* b_len;
  const uint32_t* end32;
  const uint64_t* b_off64;
  const uint8_t* in;
  const uint32_t* info;
  uint32_t* stats;   // [n_specs][4] rows cut at the limit, words that became unk, rows without a word,
                     // rows skipped; or null
  uint64_t* totals;  // [n_specs] T; or null
  uint64_t* tsum;    // [n_specs][tiles] scratch: the tiles' piece counts; after k_wp_scan their bases
  const void* rows;
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;
  uint32_t n;
  uint32_t n_specs;
  uint32_t tile;
  uint32_t tiles;
  uint32_t split;  // kTokSplitMin .. kTokSplitMax (tfrg_ctx_set_token_split)
  const int64_t* i64;   // (not read)
  uint32_t i64_w;       // (fill_columns sets it beside i64)
  const uint32_t* f32;
  WpSpec sp[kWpMaxSpecs];
};
static_assert(sizeof(WpArgs) <= 4096, "the spec table travels as the kernel argument");

// (m > 0 and n > 0)
hipError_t launch_wordpiece(const WpArgs& a, hipStream_t st);

}  // namespace tfrg
