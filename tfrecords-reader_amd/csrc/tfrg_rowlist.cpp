// tfrg_rowlist.cpp -- the row-list views of the last result (include/tfrg.h): packed per-spec outputs with
// offsets for a list of rows (ragged, elems, ids, tokens, wordpiece) on one frame, result_row_list; the
// device half of a vocabulary; and select. The context and the setup shared with the other views are in
// tfrg_ctx.h.
#include <string.h>

#include "tfrg_ctx.h"
#include "tfrg_ids.h"
#include "tfrg_vocab.h"
#include "tfrg_wordpiece.h"

// ---- The frame of the entry points that pack per-spec outputs for a list of rows (tfrg_result_ragged_rows,
// _ragged_elems, _elem_ids, _token_ids, _wordpiece_ids): the checks in the one order all five make them, the
// tiles and the split, the scratch, the consumer fence and the counters, around what an entry point brings
// as its own.
struct RowListCall {  // the arguments the five have in common
  const void* d_rows;
  uint32_t rows_dtype, m;
  int64_t row0;
  uint64_t* d_totals;
  uint32_t* d_stats;
  void* consumer_stream;
};
struct RowListKind {
  const char* fn;
  uint32_t max_specs;
  DBuf Arena::*tsum;   // the scratch of the per-tile sums
  uint32_t words;      // u64 words per (spec, tile) in it, and per spec in d_totals
  uint32_t split0;     // workgroups per tile that share its bytes: where no spec has bytes to store,
  uint32_t max_split;  // and at the most (while the launch is below 4 per CU)
};
// check(spec, at, bad, any_values): the spec's own checks; any_values: it has bytes to store.
// launch(a, split, st): the spec table of `a` (its other fields are filled) and the kernels.
// empty(spec, st): the spec's offsets of a result without a row or a record, where all of them are 0.
// Nothing is written on the device before every check has passed.
template <class Args, class Spec, class Check, class Launch, class Empty>
static int result_row_list(const RowListKind& k, tfrg_ctx* c, const Spec* specs, uint32_t n_specs, const RowListCall& q,
                           const Check& check, const Launch& launch, const Empty& empty) {
  auto bad = [&k](const std::string& why) {
    set_error(std::string(k.fn) + ": " + why);
    return TFRG_E_ARG;
  };
  if (const int rc = check_specs(c, specs, n_specs, k.max_specs, bad)) return rc;
  bool any_values = false;
  for (uint32_t i = 0; i < n_specs; ++i)
    if (const int rc = check(specs[i], "spec " + std::to_string(i) + ": ", bad, any_values)) return rc;
  if (const int rc = check_rows_dtype(q.d_rows, q.rows_dtype, false, bad)) return rc;
  if (const int rc = check_rows_m(q.d_rows, q.m, false, bad)) return rc;
  const uint32_t m = q.m, tile = c->ragged_tile;
  const uint64_t tiles = ((uint64_t)m + tile - 1) / tile;
  uint64_t split = k.split0;
  if (any_values && tiles) {
    const uint64_t want = (uint64_t)std::max(c->num_cus, 1) * 4u, have = tiles * n_specs;
    split = std::min<uint64_t>(k.max_split, std::max<uint64_t>(1, (want + have - 1) / have));
  }
  if (tiles * n_specs * std::max<uint64_t>(split, 1) > 0x7fffffffull)
    return bad("too many tiles for one launch: raise the ragged tile");
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = confirm_pending(c)) return rc;
  const bool run = m && c->res.req.n;
  DBuf& tsum = c->*k.tsum;
  if (run) HIP_TRY(tsum.ensure((size_t)(tiles * n_specs) * k.words * 8));
  hipStream_t st, cs;
  if (const int rc = fence_open(c, q.consumer_stream, &st, &cs)) return rc;
  if (q.d_stats) HIP_TRY(hipMemsetAsync(q.d_stats, 0, (size_t)n_specs * 16, st));
  if (run) {
    Args a{};
    fill_columns(c, a);
    fill_bytes_source(c, a);
    a.stats = q.d_stats;
    a.totals = q.d_totals;
    a.tsum = tsum.as<uint64_t>();
    a.rows = q.d_rows;
    a.rows64 = q.rows_dtype == TFRG_ROWS_I64;
    a.row0 = q.row0;
    a.m = m;
    a.n_specs = n_specs;
    a.tile = tile;
    a.tiles = (uint32_t)tiles;
    if (const int rc = launch(a, (uint32_t)split, st)) return rc;
  } else {
    // no row, or no record (every row is skipped): all offsets and totals are 0
    for (uint32_t i = 0; i < n_specs; ++i) {
      if (const int rc = empty(specs[i], st)) return rc;
      if (q.d_stats && m)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(q.d_stats + 4 * (size_t)i + 3), (int)m, 1, st));
    }
    if (q.d_totals) HIP_TRY(hipMemsetAsync(q.d_totals, 0, (size_t)n_specs * k.words * 8, st));
  }
  return fence_close(c, st, cs);
}

// The device view of a vocabulary: what IdsSpec, TokSpec and WpTab have in common (no vocabulary: the
// destination stays zero)
template <class Dst>
static void fill_vocab(const tfrg_vocab* v, Dst& d) {
  if (!v) return;
  d.table = v->d_table;
  d.w_offs = v->d_offs;
  d.blob = v->d_blob;
  d.w_ids = v->d_ids;
  d.mask = (uint32_t)v->table.size() - 1u;
  d.max_probe = v->max_probe;
  d.max_word = v->max_word;
  d.blob_bound = v->d_blob_bound;
}
// The first delimiter word of a spec: both words 0 mean bytes.split()'s set (09 0a 0b 0c 0d 20)
static uint64_t delims0_of(const uint64_t delims[2]) { return !delims[0] && !delims[1] ? 0x100003e00ull : delims[0]; }

// Packed values + offsets for a list of rows (tfrg_ragged.h: lengths, tile scan, gather). Every grid
// size comes from m, n_specs, the tile and the split: nothing is read back from the device.
int tfrg_result_ragged_rows(tfrg_ctx* c, const tfrg_ragged_spec* specs, uint32_t n_specs, const void* d_rows,
                            uint32_t rows_dtype, uint32_t m, int64_t row0, uint64_t* d_totals, uint32_t* d_stats,
                            void* consumer_stream) {
  static_assert(TFRG_RAGGED_MAX_SPECS == kRaggedMaxSpecs, "tfrg.h mirrors tfrg_ragged.h");
  // (the split: workgroups per tile that share its span, 1 where nothing is stored)
  const RowListKind kind{"tfrg_result_ragged_rows", TFRG_RAGGED_MAX_SPECS, &Arena::rg_tsum, 1, 1, kRaggedMaxSplit};
  return result_row_list<RaggedArgs>(
      kind, c, specs, n_specs, RowListCall{d_rows, rows_dtype, m, row0, d_totals, d_stats, consumer_stream},
      [c](const tfrg_ragged_spec& s, const std::string& at, const auto& bad, bool& any_values) -> int {
        if (const int rc = check_slot_dtype(c, at, s.slot, s.dtype, bad)) return rc;
        if (!s.offsets) return bad(at + "offsets is NULL");
        if (s.reserved) return bad(at + "reserved must be 0");
        const uintptr_t isz = s.dtype == TFRG_DENSE_I64 ? 8 : s.dtype == TFRG_DENSE_U8 ? 1 : 4;
        if (((uintptr_t)s.values & (isz - 1)) || ((uintptr_t)s.offsets & 7u))
          return bad(at + "values and offsets must be aligned to their element size");
        any_values |= s.values != nullptr && s.cap != 0;
        return 0;
      },
      [c, specs](RaggedArgs& a, uint32_t split, hipStream_t st) -> int {
        a.split = split;
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_ragged_spec& s = specs[i];
          RaggedSpec& d = a.sp[i];
          d.values = s.values;
          d.offsets = s.offsets;
          d.cap = s.cap;
          d.slot = s.slot;
          d.dtype = s.dtype;
          d.max_len = s.max_len;
          d.const_len = const_len_of(c, s.slot, s.dtype == TFRG_DENSE_U8);
          d.const_off = const_off_of(c, s.slot, s.dtype == TFRG_DENSE_U8);
        }
        HIP_TRY(launch_ragged(a, st));
        return 0;
      },
      [m](const tfrg_ragged_spec& s, hipStream_t st) -> int {
        HIP_TRY(hipMemsetAsync(s.offsets, 0, ((size_t)m + 1) * 8, st));
        return 0;
      });
}

// Every element of a bytes_list slot for a list of rows: bytes + element offsets + row offsets
// (tfrg_elems.h: counts and byte sums, tile scan, offsets, copy). Every grid size comes from m, n_specs,
// the tile and the split: nothing is read back from the device.
int tfrg_result_ragged_elems(tfrg_ctx* c, const tfrg_elems_spec* specs, uint32_t n_specs, const void* d_rows,
                             uint32_t rows_dtype, uint32_t m, int64_t row0, uint64_t* d_totals, uint32_t* d_stats,
                             void* consumer_stream) {
  static_assert(TFRG_ELEMS_MAX_SPECS == kElemsMaxSpecs, "tfrg.h mirrors tfrg_elems.h");
  static_assert(sizeof(tfrg_elems_spec) == 56, "tfrg.h states the size");
  // (the split: workgroups per tile that share its bytes; 0: no spec has bytes to store, and the copy
  // is not launched)
  const RowListKind kind{"tfrg_result_ragged_elems", TFRG_ELEMS_MAX_SPECS, &Arena::el_tsum, 2, 0, kElemsMaxSplit};
  return result_row_list<ElemsArgs>(
      kind, c, specs, n_specs, RowListCall{d_rows, rows_dtype, m, row0, d_totals, d_stats, consumer_stream},
      [c](const tfrg_elems_spec& s, const std::string& at, const auto& bad, bool& any_values) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (!s.row_offsets) return bad(at + "row_offsets is NULL");
        if (((uintptr_t)s.row_offsets & 7u) || ((uintptr_t)s.elem_offsets & 7u))
          return bad(at + "row_offsets and elem_offsets must be 8-byte aligned");
        if (s.values && !s.elem_offsets) return bad(at + "values without elem_offsets");
        if (s.reserved) return bad(at + "reserved must be 0");
        any_values |= s.values != nullptr && s.cap != 0 && s.elem_cap != 0;
        return 0;
      },
      [c, specs](ElemsArgs& a, uint32_t split, hipStream_t st) -> int {
        a.split = split;
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_elems_spec& s = specs[i];
          ElemsSpec& d = a.sp[i];
          d.values = s.values;
          d.elem_offsets = s.elem_offsets;
          d.row_offsets = s.row_offsets;
          d.elem_cap = s.elem_cap;
          d.cap = s.cap;
          d.slot = s.slot;
          d.max_elems = s.max_elems;
          d.max_len = s.max_len;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
        }
        HIP_TRY(launch_elems(a, st));
        return 0;
      },
      [m](const tfrg_elems_spec& s, hipStream_t st) -> int {
        HIP_TRY(hipMemsetAsync(s.row_offsets, 0, ((size_t)m + 1) * 8, st));
        if (s.elem_offsets) HIP_TRY(hipMemsetAsync(s.elem_offsets, 0, 8, st));
        return 0;
      });
}

// ---- The device half of a vocabulary (tfrg_vocab.h; the host half, tfrg_host.cpp, calls it through
// g_vocab_device). One allocation: ids, table, offsets, then the blob and zeros to a multiple of 16.
static int vocab_upload(tfrg_vocab* v) {
  if (v->blob.size() >= 0xfffffff0ull) {  // (the kernels read the blob through a 32-bit buffer bound)
    set_error("tfrg_vocab_create: words of 2^32 - 16 bytes or more in all cannot go to a device");
    return TFRG_E_ARG;
  }
  HIP_TRY(hipSetDevice(v->device));
  const size_t n_ids = v->ids.size() * 8, n_tab = v->table.size() * 4, n_off = v->offs.size() * 4;
  const size_t at_tab = n_ids, at_off = at_tab + n_tab, at_blob = (at_off + n_off + 15) & ~(size_t)15;
  const size_t blob_room = (v->blob.size() + 16) & ~(size_t)15;
  const size_t total = at_blob + blob_room;
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, total));
  uint8_t* const d = static_cast<uint8_t*>(p);
  hipError_t e = hipMemset(d + at_blob, 0, blob_room);
  if (e == hipSuccess && n_ids) e = hipMemcpy(d, v->ids.data(), n_ids, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + at_tab, v->table.data(), n_tab, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + at_off, v->offs.data(), n_off, hipMemcpyHostToDevice);
  if (e == hipSuccess && !v->blob.empty()) e = hipMemcpy(d + at_blob, v->blob.data(), v->blob.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipFree(p);
    v->d_mem = nullptr;
    set_error(std::string("tfrg_vocab_create: upload: ") + hipGetErrorString(e));
    return TFRG_E_HIP;
  }
  v->d_mem = p;
  v->d_ids = reinterpret_cast<const int64_t*>(d);
  v->d_table = reinterpret_cast<const uint32_t*>(d + at_tab);
  v->d_offs = reinterpret_cast<const uint32_t*>(d + at_off);
  v->d_blob = d + at_blob;
  v->d_blob_bound = (uint32_t)std::min<uint64_t>(blob_room, 0xfffffff0ull);
  v->device_bytes = total;
  return 0;
}
static int vocab_release(tfrg_vocab* v) {
  HIP_TRY(hipSetDevice(v->device));
  HIP_TRY(hipDeviceSynchronize());  // (work already queued may still read the table)
  HIP_TRY(hipFree(v->d_mem));
  v->d_mem = nullptr;
  return 0;
}
static const bool g_vocab_device_registered = (tfrg::g_vocab_device = {vocab_upload, vocab_release}, true);

// One id per element of a bytes_list slot for a list of rows (tfrg_ids.h: counts, tile scan, row
// offsets and ids). Every grid size comes from m, n_specs and the tile: nothing is read back.
int tfrg_result_elem_ids(tfrg_ctx* c, const tfrg_ids_spec* specs, uint32_t n_specs, const void* d_rows,
                         uint32_t rows_dtype, uint32_t m, int64_t row0, uint64_t* d_totals, uint32_t* d_stats,
                         void* consumer_stream) {
  static_assert(TFRG_IDS_MAX_SPECS == kIdsMaxSpecs, "tfrg.h mirrors tfrg_ids.h");
  static_assert(sizeof(tfrg_ids_spec) == 72, "tfrg.h states the size");
  static_assert(kIdsNoLen == kElemsNoLen && kIdsOffStored == kElemsOffStored, "const_len_of / const_off_of serve tfrg_ids.h");
  const RowListKind kind{"tfrg_result_elem_ids", TFRG_IDS_MAX_SPECS, &Arena::id_tsum, 1, 0, 0};  // (no split)
  return result_row_list<IdsArgs>(
      kind, c, specs, n_specs, RowListCall{d_rows, rows_dtype, m, row0, d_totals, d_stats, consumer_stream},
      [c](const tfrg_ids_spec& s, const std::string& at, const auto& bad, bool&) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (!s.row_offsets) return bad(at + "row_offsets is NULL");
        if (((uintptr_t)s.row_offsets & 7u) || ((uintptr_t)s.ids & 7u)) return bad(at + "row_offsets and ids must be 8-byte aligned");
        if (s.reserved0 || s.reserved1) return bad(at + "reserved words must be 0");
        if (!s.vocab && !s.num_oov_buckets) return bad(at + "no vocabulary and no hash buckets");
        if (s.vocab && !s.vocab->d_mem) return bad(at + "the vocabulary was built host-only (device -1)");
        if (s.vocab && s.vocab->device != c->device)
          return bad(at + "the vocabulary is on device " + std::to_string(s.vocab->device) + ", the context on " +
                     std::to_string(c->device));
        return 0;
      },
      [c, specs](IdsArgs& a, uint32_t, hipStream_t st) -> int {
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_ids_spec& s = specs[i];
          IdsSpec& d = a.sp[i];
          d.ids = s.ids;
          d.row_offsets = s.row_offsets;
          d.elem_cap = s.elem_cap;
          fill_vocab(s.vocab, d);
          d.n_buckets = s.num_oov_buckets;
          d.oov_base = s.oov_base;
          d.default_id = s.default_id;
          d.slot = s.slot;
          d.max_elems = s.max_elems;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
        }
        HIP_TRY(launch_ids(a, st));
        return 0;
      },
      [m](const tfrg_ids_spec& s, hipStream_t st) -> int {
        HIP_TRY(hipMemsetAsync(s.row_offsets, 0, ((size_t)m + 1) * 8, st));
        return 0;
      });
}

// One id per token of the elements of a bytes_list slot for a list of rows (tfrg_tokens.h: token counts,
// tile scan, row offsets and ids). Every grid size comes from m, n_specs and the tile: nothing is read back.
int tfrg_result_token_ids(tfrg_ctx* c, const tfrg_tok_spec* specs, uint32_t n_specs, const void* d_rows,
                          uint32_t rows_dtype, uint32_t m, int64_t row0, uint64_t* d_totals, uint32_t* d_stats,
                          void* consumer_stream) {
  static_assert(TFRG_TOK_MAX_SPECS == kTokMaxSpecs && TFRG_TOK_LOWER_ASCII == kTokLowerAscii, "tfrg.h mirrors tfrg_tokens.h");
  static_assert(sizeof(tfrg_tok_spec) == 88, "tfrg.h states the size");
  static_assert(sizeof(TokArgs) < 4096, "the kernel argument");
  static_assert(kTokNoLen == kElemsNoLen && kTokOffStored == kElemsOffStored, "const_len_of / const_off_of serve tfrg_tokens.h");
  const RowListKind kind{"tfrg_result_token_ids", TFRG_TOK_MAX_SPECS, &Arena::tk_tsum, 1, 0, 0};  // (no split)
  return result_row_list<TokArgs>(
      kind, c, specs, n_specs, RowListCall{d_rows, rows_dtype, m, row0, d_totals, d_stats, consumer_stream},
      [c](const tfrg_tok_spec& s, const std::string& at, const auto& bad, bool&) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (!s.row_offsets) return bad(at + "row_offsets is NULL");
        if (((uintptr_t)s.row_offsets & 7u) || ((uintptr_t)s.ids & 7u)) return bad(at + "row_offsets and ids must be 8-byte aligned");
        if (s.flags & ~TFRG_TOK_LOWER_ASCII) return bad(at + "unknown flag bits " + std::to_string(s.flags));
        if (!s.vocab && !s.num_oov_buckets) return bad(at + "no vocabulary and no hash buckets");
        if (s.vocab && !s.vocab->d_mem) return bad(at + "the vocabulary was built host-only (device -1)");
        if (s.vocab && s.vocab->device != c->device)
          return bad(at + "the vocabulary is on device " + std::to_string(s.vocab->device) + ", the context on " +
                     std::to_string(c->device));
        return 0;
      },
      [c, specs](TokArgs& a, uint32_t, hipStream_t st) -> int {
        a.split = c->token_split;
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_tok_spec& s = specs[i];
          TokSpec& d = a.sp[i];
          d.ids = s.ids;
          d.row_offsets = s.row_offsets;
          d.tok_cap = s.tok_cap;
          fill_vocab(s.vocab, d);
          d.n_buckets = s.num_oov_buckets;
          d.oov_base = s.oov_base;
          d.default_id = s.default_id;
          d.delims[0] = delims0_of(s.delims);
          d.delims[1] = s.delims[1];
          d.slot = s.slot;
          d.max_elems = s.max_elems;
          d.max_tokens = s.max_tokens;
          d.lower = (s.flags & TFRG_TOK_LOWER_ASCII) ? 1u : 0u;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
        }
        HIP_TRY(launch_tokens(a, st));
        return 0;
      },
      [m](const tfrg_tok_spec& s, hipStream_t st) -> int {
        HIP_TRY(hipMemsetAsync(s.row_offsets, 0, ((size_t)m + 1) * 8, st));
        return 0;
      });
}

// One id per WordPiece of the words of a bytes_list slot for a list of rows (tfrg_wordpiece.h: piece
// counts, tile scan, row offsets and ids). Every grid size comes from m, n_specs and the tile: nothing is
// read back.
int tfrg_result_wordpiece_ids(tfrg_ctx* c, const tfrg_wp_spec* specs, uint32_t n_specs, const void* d_rows,
                              uint32_t rows_dtype, uint32_t m, int64_t row0, uint64_t* d_totals, uint32_t* d_stats,
                              void* consumer_stream) {
  static_assert(TFRG_WP_MAX_SPECS == kWpMaxSpecs && TFRG_WP_LOWER_ASCII == kWpLowerAscii && TFRG_WP_SPECIAL == kWpSpecial &&
                    TFRG_WP_MAX_WORD_BYTES == kWpMaxWordBytes,
                "tfrg.h mirrors tfrg_wordpiece.h");
  static_assert(sizeof(tfrg_wp_spec) == 120, "tfrg.h states the size");
  static_assert(kWpNoLen == kElemsNoLen && kWpOffStored == kElemsOffStored, "const_len_of / const_off_of serve tfrg_wordpiece.h");
  const RowListKind kind{"tfrg_result_wordpiece_ids", TFRG_WP_MAX_SPECS, &Arena::wp_tsum, 1, 0, 0};  // (no split)
  return result_row_list<WpArgs>(
      kind, c, specs, n_specs, RowListCall{d_rows, rows_dtype, m, row0, d_totals, d_stats, consumer_stream},
      [c](const tfrg_wp_spec& s, const std::string& at, const auto& bad, bool&) -> int {
        if (const int rc = check_bytes_slot(c, at, s.slot, bad)) return rc;
        if (!s.row_offsets) return bad(at + "row_offsets is NULL");
        if (((uintptr_t)s.row_offsets & 7u) || ((uintptr_t)s.ids & 7u)) return bad(at + "row_offsets and ids must be 8-byte aligned");
        if (s.flags & ~(TFRG_WP_LOWER_ASCII | TFRG_WP_SPECIAL)) return bad(at + "unknown flag bits " + std::to_string(s.flags));
        if (s.reserved) return bad(at + "reserved must be 0");
        if (!s.vocab) return bad(at + "vocab is NULL");
        for (const tfrg_vocab* v : {s.vocab, s.vocab_cont}) {
          if (v && !v->d_mem) return bad(at + "a vocabulary was built host-only (device -1)");
          if (v && v->device != c->device)
            return bad(at + "a vocabulary is on device " + std::to_string(v->device) + ", the context on " + std::to_string(c->device));
        }
        if (s.max_word_bytes > TFRG_WP_MAX_WORD_BYTES)
          return bad(at + "max_word_bytes must be at most " + std::to_string(TFRG_WP_MAX_WORD_BYTES));
        if ((s.flags & TFRG_WP_SPECIAL) && s.max_pieces == 1) return bad(at + "max_pieces 1 leaves no room for cls and sep");
        return 0;
      },
      [c, specs](WpArgs& a, uint32_t, hipStream_t st) -> int {
        a.split = c->token_split;
        for (uint32_t i = 0; i < a.n_specs; ++i) {
          const tfrg_wp_spec& s = specs[i];
          WpSpec& d = a.sp[i];
          d.ids = s.ids;
          d.row_offsets = s.row_offsets;
          d.tok_cap = s.tok_cap;
          fill_vocab(s.vocab, d.first);
          fill_vocab(s.vocab_cont, d.cont);
          d.delims[0] = delims0_of(s.delims);
          d.delims[1] = s.delims[1];
          d.isolate[0] = s.isolate[0] & ~d.delims[0];  // (a byte in both sets is a delimiter)
          d.isolate[1] = s.isolate[1] & ~d.delims[1];
          d.cls_id = s.cls_id;
          d.sep_id = s.sep_id;
          d.unk_id = s.unk_id;
          d.slot = s.slot;
          d.max_elems = s.max_elems;
          d.special = (s.flags & TFRG_WP_SPECIAL) ? 1u : 0u;
          d.limit = !s.max_pieces ? kWpUnbounded : s.max_pieces - 2u * d.special;
          d.lower = (s.flags & TFRG_WP_LOWER_ASCII) ? 1u : 0u;
          d.const_len = const_len_of(c, s.slot, true);
          d.const_off = const_off_of(c, s.slot, true);
          d.max_word_bytes = s.max_word_bytes ? s.max_word_bytes : kWpDefaultWordBytes;
        }
        HIP_TRY(launch_wordpiece(a, st));
        return 0;
      },
      [m](const tfrg_wp_spec& s, hipStream_t st) -> int {
        HIP_TRY(hipMemsetAsync(s.row_offsets, 0, ((size_t)m + 1) * 8, st));
        return 0;
      });
}

// The WHERE clause over the last result (tfrg_select.h: verdicts, tile scan, write). Every grid size
// comes from m and the tile: nothing is read back from the device. One implementation behind both entry
// points: tfrg_result_select_rows is tfrg_result_select_match without patterns (`match` false: the
// bytes subjects and the ops past GE are unknown to it).
struct SelectCall {
  const void* d_rows;
  uint32_t rows_dtype, m;
  int64_t row0;
  void* d_out;
  uint32_t out_dtype;
  uint64_t cap;
  uint64_t* d_count;
  uint32_t* d_stats;
  uint32_t flags;
  void* consumer_stream;
};

static bool sel_bytes_subject(uint32_t subject) { return subject == TFRG_SEL_BYTES || subject == TFRG_SEL_BYTES_ANY; }

static int result_select(const char* fn, bool match, tfrg_ctx* c, const tfrg_select_term* terms, uint32_t n_terms,
                         const uint8_t* patterns, uint64_t patterns_len, const SelectCall& q) {
  auto bad = [fn](const std::string& why) {
    set_error(std::string(fn) + ": " + why);
    return TFRG_E_ARG;
  };
  if (const int rc = check_result(c, bad)) return rc;
  static_assert(TFRG_SEL_MAX_TERMS == kSelMaxTerms && TFRG_SEL_VALUE == kSelValue && TFRG_SEL_ANY == kSelAny &&
                    TFRG_SEL_COUNT == kSelCount && TFRG_SEL_BYTES_LEN == kSelBytesLen &&
                    TFRG_SEL_STATUS == kSelStatus && TFRG_SEL_BYTES == kSelBytes && TFRG_SEL_BYTES_ANY == kSelBytesAny &&
                    TFRG_SEL_EQ == kSelEq && TFRG_SEL_GE == kSelGe && TFRG_SEL_PREFIX == kSelPrefix &&
                    TFRG_SEL_SUFFIX == kSelSuffix && TFRG_SEL_CONTAINS == kSelContains &&
                    TFRG_SEL_MAX_PATTERN == kSelMaxPattern && TFRG_SEL_MAX_PATTERN_BYTES == kSelMaxPatternBytes &&
                    sizeof(tfrg_select_term) == 32,
                "tfrg.h mirrors tfrg_select.h");
  const uint32_t max_subject = match ? TFRG_SEL_BYTES_ANY : TFRG_SEL_STATUS, max_op = match ? TFRG_SEL_CONTAINS : TFRG_SEL_GE;
  if (n_terms > TFRG_SEL_MAX_TERMS) return bad("n_terms must be at most " + std::to_string(TFRG_SEL_MAX_TERMS));
  if (n_terms && !terms) return bad("terms is NULL");
  if (patterns_len > TFRG_SEL_MAX_PATTERN_BYTES)
    return bad("patterns_len must be at most " + std::to_string(TFRG_SEL_MAX_PATTERN_BYTES));
  if (patterns_len && !patterns) return bad("patterns is NULL");
  bool any_bytes = false;
  for (uint32_t i = 0; i < n_terms; ++i) {
    const tfrg_select_term& t = terms[i];
    const std::string at = "term " + std::to_string(i) + ": ";
    if (t.slot >= c->n_slots) return bad(at + "slot " + std::to_string(t.slot) + " >= n_slots");
    if (t.subject > max_subject) return bad(at + "unknown subject " + std::to_string(t.subject));
    if (t.op > max_op) return bad(at + "unknown op " + std::to_string(t.op));
    if (t.group >= 32) return bad(at + "group must be below 32");
    const uint32_t kind = c->slot_kind_h[t.slot] & 3u;
    const bool list = t.subject == TFRG_SEL_VALUE || t.subject == TFRG_SEL_ANY;
    const bool bytes = sel_bytes_subject(t.subject);
    if ((list && kind != TFRG_KIND_INT64 && kind != TFRG_KIND_FLOAT) ||
        ((t.subject == TFRG_SEL_BYTES_LEN || bytes) && kind != TFRG_KIND_BYTES) ||
        (t.subject == TFRG_SEL_STATUS && t.slot != 0))
      return bad(at + "subject " + std::to_string(t.subject) + " does not fit slot " + std::to_string(t.slot) +
                 " of kind " + std::to_string(kind));
    if (t.op > TFRG_SEL_GE && !bytes)
      return bad(at + "op " + std::to_string(t.op) + " needs TFRG_SEL_BYTES or TFRG_SEL_BYTES_ANY");
    if (t.index && t.subject != TFRG_SEL_VALUE && t.subject != TFRG_SEL_BYTES)
      return bad(at + (match ? "index must be 0 outside TFRG_SEL_VALUE and TFRG_SEL_BYTES" : "index must be 0 outside TFRG_SEL_VALUE"));
    if (t.reserved) return bad(at + "reserved must be 0");
    if (list && kind == TFRG_KIND_FLOAT && (t.operand >> 32)) return bad(at + "a float operand has its high 32 bits set");
    if (bytes) {
      const uint64_t off = t.operand & 0xffffffffull, len = t.operand >> 32;
      if (len > TFRG_SEL_MAX_PATTERN) return bad(at + "a pattern is at most " + std::to_string(TFRG_SEL_MAX_PATTERN) + " bytes long");
      if (off + len > patterns_len) return bad(at + "the pattern lies outside patterns");
      any_bytes = true;
    }
  }
  if (const int rc = check_rows_dtype(q.d_rows, q.rows_dtype, false, bad)) return rc;
  if (q.out_dtype != TFRG_ROWS_I32 && q.out_dtype != TFRG_ROWS_I64)
    return bad("out_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not " + std::to_string(q.out_dtype));
  if (const int rc = check_rows_m(q.d_rows, q.m, false, bad)) return rc;
  if (!q.d_count) return bad("d_count is NULL");
  if (((uintptr_t)q.d_count & 7u) || ((uintptr_t)q.d_out & (q.out_dtype == TFRG_ROWS_I64 ? 7u : 3u)))
    return bad("d_out and d_count must be aligned to their element size");
  if (q.out_dtype == TFRG_ROWS_I32 && c->res.req.n &&
      (q.row0 < (int64_t)INT32_MIN || q.row0 > (int64_t)INT32_MAX - ((int64_t)c->res.req.n - 1)))
    return bad("rows [row0, row0 + n) do not fit an int32 output");
  if (q.flags & ~TFRG_SEL_APPEND) return bad("unknown flag bits");
  const bool append = (q.flags & TFRG_SEL_APPEND) != 0;
  const uint32_t m = q.m;
  uint32_t* const d_stats = q.d_stats;
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = confirm_pending(c)) return rc;
  const uint32_t tile = c->select_tile;
  const uint64_t tiles = ((uint64_t)m + tile - 1) / tile, nwords = ((uint64_t)m + 63) / 64;
  const bool run = m && c->res.req.n;
  if (run) HIP_TRY(c->sel_buf.ensure((size_t)(nwords + tiles) * 8));
  hipStream_t st, cs;
  if (const int rc = fence_open(c, q.consumer_stream, &st, &cs)) return rc;
  if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, 8, st));
  if (run) {
    // (the bytes fields and the patterns are filled, and travel, only where a bytes term asks for them)
    SelectBytesArgs ba{};
    SelectArgs& a = ba.s;
    fill_columns(c, a);
    a.status = (c->res.implicit & TFRG_IMPLICIT_STATUS) ? nullptr : c->status.as<int32_t>();
    a.stats = d_stats;
    a.count = q.d_count;
    a.words = c->sel_buf.as<uint64_t>();
    a.tsum = a.words + nwords;
    a.rows = q.d_rows;
    a.out = q.d_out;
    a.cap = q.d_out ? q.cap : 0;
    a.row0 = q.row0;
    a.m = m;
    a.rows64 = q.rows_dtype == TFRG_ROWS_I64;
    a.out64 = q.out_dtype == TFRG_ROWS_I64;
    a.n_terms = n_terms;
    a.tile = tile;
    a.tiles = (uint32_t)tiles;
    a.append = append;
    for (uint32_t i = 0; i < n_terms; ++i) {
      const tfrg_select_term& t = terms[i];
      SelTerm& d = a.term[i];
      d.slot = t.slot;
      d.subject = t.subject;
      d.op = t.op;
      d.group = t.group;
      d.index = t.index;
      d.rhs = (int64_t)t.operand;
      const bool list = t.subject == TFRG_SEL_VALUE || t.subject == TFRG_SEL_ANY;
      if (list && (c->slot_kind_h[t.slot] & 3u) == TFRG_KIND_FLOAT) {
        d.is_float = 1;
        d.rhs_nan = sel_float_nan((uint32_t)t.operand);
        d.rhs = d.rhs_nan ? 0 : sel_float_key((uint32_t)t.operand);
      }
      const bool bytes = sel_bytes_subject(t.subject);
      d.const_len = const_len_of(c, t.slot, t.subject == TFRG_SEL_BYTES_LEN || bytes);
      ba.const_off[i] = const_off_of(c, t.slot, bytes);
      a.all_groups |= 1u << t.group;
    }
    if (any_bytes) {
      static_assert(kDenseOffStored == kSelOffStored, "const_off_of serves select too");
      fill_bytes_source(c, ba);
      ba.scan_min = c->select_scan;
      if (patterns_len) memcpy(ba.pat, patterns, (size_t)patterns_len);
      HIP_TRY(launch_select_bytes(ba, st));
    } else {
      HIP_TRY(launch_select(a, st));
    }
  } else {
    // no candidate, or no record (every candidate is skipped): nothing is selected
    if (!append) HIP_TRY(hipMemsetAsync(q.d_count, 0, 8, st));
    if (d_stats && m) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_stats + 1), (int)m, 1, st));
  }
  return fence_close(c, st, cs);
}

int tfrg_result_select_rows(tfrg_ctx* c, const tfrg_select_term* terms, uint32_t n_terms, const void* d_rows,
                            uint32_t rows_dtype, uint32_t m, int64_t row0, void* d_out, uint32_t out_dtype,
                            uint64_t cap, uint64_t* d_count, uint32_t* d_stats, uint32_t flags, void* consumer_stream) {
  return result_select("tfrg_result_select_rows", false, c, terms, n_terms, nullptr, 0,
                       SelectCall{d_rows, rows_dtype, m, row0, d_out, out_dtype, cap, d_count, d_stats, flags, consumer_stream});
}

int tfrg_result_select_match(tfrg_ctx* c, const tfrg_select_term* terms, uint32_t n_terms, const uint8_t* patterns,
                             uint64_t patterns_len, const void* d_rows, uint32_t rows_dtype, uint32_t m, int64_t row0,
                             void* d_out, uint32_t out_dtype, uint64_t cap, uint64_t* d_count, uint32_t* d_stats,
                             uint32_t flags, void* consumer_stream) {
  return result_select("tfrg_result_select_match", true, c, terms, n_terms, patterns, patterns_len,
                       SelectCall{d_rows, rows_dtype, m, row0, d_out, out_dtype, cap, d_count, d_stats, flags, consumer_stream});
}

