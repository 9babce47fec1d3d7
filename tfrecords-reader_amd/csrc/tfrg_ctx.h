// tfrg_ctx.h -- the device context of libtfrg as its host files share it: tfrg_capi.cpp (context, decodes,
// result transfer), tfrg_fixed.cpp (the fixed-shape views of the last result) and tfrg_rowlist.cpp (its
// row-list views and select). The context and what one decode leaves in it, then the host-side setup that
// every entry point over the last result goes through. Not part of the public ABI (include/tfrg.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tfrg.h"
#include "tfrg_dense.h"
#include "tfrg_elems.h"
#include "tfrg_frame.h"
#include "tfrg_internal.h"
#include "tfrg_ragged.h"
#include "tfrg_select.h"
#include "tfrg_tokens.h"

namespace tfrg {
void set_error(const std::string& s);

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));               \
      return TFRG_E_HIP;                                                           \
    }                                                                              \
  } while (0)

// grow-only device buffer
struct DBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      cap = 0;
    }
    size_t want = bytes < 256 ? 256 : bytes;
    want = (want + 4095) & ~(size_t)4095;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

constexpr uint32_t kMissCap = 1u << 16;

}  // namespace tfrg

using namespace tfrg;

// record offsets of one decode call (DevBatch: u64 pairs, u32 pairs, or u32 ends of back-to-back records)
struct Offsets {
  const uint64_t* s64 = nullptr;
  const uint64_t* e64 = nullptr;
  const uint32_t* s32 = nullptr;
  const uint32_t* e32 = nullptr;
  uint32_t first = 0;
  uint32_t mode = kOffU64;
};

// One decode as decode_device_any runs it: the three public entry points build one, finish_decode
// re-runs a copy of the stored one with `full` / `worst_case` set.
struct DecodeReq {
  const uint8_t* d_bytes = nullptr;
  uint64_t nbytes = 0;
  Offsets off;
  uint32_t n = 0, flags = 0;
  hipStream_t stream = nullptr;  // NULL: the context's own
  uint64_t cap_in = 0;      // total bytes of the ranges (tfrg_decode_host: > nbytes when they overlap); 0: nbytes
  uint64_t bound = 0;       // no record above this; 0: the context's record_bound
  bool full = false;        // no optimistic pass
  bool worst_case = false;  // the value-capacity hints ignored
  bool host = false;        // tfrg_decode_host: its reader is tfrg_result_fetch, the int64 column stays 8 bytes wide
};

// Everything known about the last decode. Replaced as a whole: decode_device_any and tfrg_set_schema
// clear it (`valid` false: no result), and a decode assigns it once it is enqueued.
struct Result {
  bool valid = false;
  DecodeReq req;  // as it ran: stream, capacity and bound resolved (the consumers' d_bytes, nbytes and e32)
  uint64_t cap_i64 = 0, cap_f32 = 0, cap_b = 0;
  bool materialized = false;
  bool hinted = false;        // ran with a value-capacity hint below its worst case
  bool opt_pending = false;   // ran optimistically and is not confirmed yet
  bool mat_pending = false;   // its byte materialization waits for that confirmation
  bool rs_complete = false;   // the placed slots' identity rows are written into the device columns
  bool cols_complete = false; // tfrg_result_device wrote the constant columns (constant_fills)
  bool off_complete = false;  // fill_implicit_off wrote the implicit bytes_off words
  bool i64_complete = false;  // widen_i64 wrote the int64 column from the narrow one
  uint32_t i64_w = 8;         // bytes per int64 value it stored: 4 or 2 into i64n (i64_width), else 8 into i64
  uint32_t implicit = 0;      // TFRG_IMPLICIT_* columns the decode did not store
  uint64_t off_mask = 0;      // slots whose bytes_off words it did not store (implicit_off_slots)
  bool aux_zero = false;      // ran optimistically with stored statuses: aux is all 0
  // the learned constants behind those columns as the decode ran with them (a later re-learn does not
  // change its result), each copied only where its bit is set. Only k_tpl_lane leaves a column implicit
  // (launch_decode), so such a decode has at most kLeanMaxSlots slots: no allocation per decode.
  struct SlotConst {
    int32_t rel_off;      // off_mask: the end-relative element offset
    uint32_t elem_len;    // TFRG_IMPLICIT_BYTES_LEN: the bytes element length
    uint16_t order_word;  // TFRG_IMPLICIT_ORDER
  } slot[kLeanMaxSlots] = {};
};

// Every device buffer of a context. `each` is the one list of them, checked against the members.
struct Arena {
  DBuf crc_tab, consts;  // constants
  DBuf ht, key_hash, key_off, key_blob, key_slot, slot_kind, key_w, krec;  // schema
  DBuf in_bytes, in_start, in_end;  // host staging for tfrg_decode_host
  // columns and work space of a decode
  DBuf status, aux, verdict, order, count, loc, rs, slot_base, totals, kind_totals;
  DBuf ident;  // 0, 1, 2, ... (ident_n words): the fetched row splits of placed slots
  DBuf i64n;  // the int64 column of a narrowed decode: element i at byte i * width (tfrg_info.i64_width)
  DBuf i64, f32, b_off, b_len, big_list, slow_list, miss, info, tsum, crc_rec, crc_base, crc_part;
  DBuf dq, dq_cnt;  // deferred packed-int64 bodies (k_body_count)
  DBuf lmask, rlist;  // k_tpl_lane's per-group miss masks and listed groups
  DBuf bdata, boff64, blb, bbig;  // TFRG_FLAG_MATERIALIZE_BYTES
  DBuf tpl, spec;  // record-shape templates, speculative placement (tfrg_learn_templates)
  DBuf fr_tab, fr_dev;  // tfrg_index_device: chunk table, piece rows + summary
  DBuf rg_tsum;  // tfrg_result_ragged_rows: the per-tile sums
  DBuf el_tsum;  // tfrg_result_ragged_elems: the per-tile element counts and byte sums
  DBuf id_tsum;  // tfrg_result_elem_ids: the per-tile element counts
  DBuf tk_tsum;  // tfrg_result_token_ids: the per-tile token counts
  DBuf wp_tsum;  // tfrg_result_wordpiece_ids: the per-tile piece counts
  DBuf sel_buf;  // tfrg_result_select_rows: the candidates' ballot words, then the per-tile sums
  template <class F>
  void each(F f) {
    DBuf* const all[] = {&crc_tab, &consts, &ht, &key_hash, &key_off, &key_blob, &key_slot, &slot_kind, &key_w, &krec,
                         &in_bytes, &in_start, &in_end, &status, &aux, &verdict, &order, &count, &loc, &rs, &slot_base,
                         &totals, &kind_totals, &ident, &i64n, &i64, &f32, &b_off, &b_len, &big_list, &slow_list, &miss, &info,
                         &tsum, &crc_rec, &crc_base, &crc_part, &dq, &dq_cnt, &lmask, &rlist, &bdata, &boff64, &blb,
                         &bbig, &tpl, &spec, &fr_tab, &fr_dev, &rg_tsum, &el_tsum,
                         &id_tsum, &tk_tsum, &wp_tsum, &sel_buf};
    static_assert(sizeof(all) / sizeof(*all) * sizeof(DBuf) == sizeof(Arena), "a buffer is missing from the list");
    for (DBuf* b : all) f(*b);
  }
};

// Switches read from the environment in tfrg_ctx_create (A/B measurements and tests)
struct Switches {
  bool tpl_on = true;        // TFRG_TEMPLATES (also tfrg_ctx_set_templates)
  bool spec_on = true;       // TFRG_SPEC: speculative single-value placement
  int tpl_stage = 1;         // TFRG_TPL_STAGE: k_tpl_lane's staged windows 0 off, 1 on large batches, 2 on any
  uint32_t tpl_gpw = 0;      // TFRG_TPL_GPW=2, 4 or 8: its groups per wave; 0: launch_tpl_lane's choice
  bool optimistic = true;    // TFRG_OPTIMISTIC=0: no optimistic decodes
  bool implicit_off = true;  // TFRG_IMPLICIT_OFF=0: every bytes_off word stored
  bool narrow_i64 = true;    // TFRG_NARROW_I64=0: every int64 value stored as 8 bytes
  bool walk_beside = true;   // TFRG_WALK_BESIDE=0: large records walked before the CRC
  uint32_t walk_blocks = 0;  // TFRG_WALK_BLOCKS: cap on its walking workgroups; 0 = automatic
  int dense_nt = 0;          // TFRG_DENSE_NT=1: k_dense's output stores nontemporal
  // TFRG_DEBUG_POISON_LOC="r0,r1,..." (at most 4): records whose list locations are poisoned after the count passes
  uint32_t poison[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
};

// Per context: the device, its streams and events, the arena, the schema, the learned shapes and the
// settings. What belongs to one decode is in `res`.
struct tfrg_ctx : Arena {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t last_stream = nullptr;  // of the last decode enqueued: arena buffers may be in use on it
  Switches sw;
  uint32_t lane_max = 2048;
  uint32_t wave_stage = 0xffffffffu;  // clamped to the kernel's stage size
  uint64_t record_bound = 0;  // tfrg_ctx_set_record_bound: no record above this (0 = unknown)
  int num_cus = 256;
  uint32_t cu_lds = 65536;     // LDS bytes of a CU
  uint32_t n_keys = 0, n_slots = 0, ht_mask = 0;
  size_t ident_n = 0;
  bool tsum_dirty = true;  // the scan words must be cleared before the next decode
  // info words: two slots, decode k using slot k % 2; k_lane_count zeroes the other one for the
  // next decode (no per-call memset). info_clean: the next slot is known to be zero.
  uint32_t info_slot = 0;
  bool info_clean = false;
  uint32_t* info_pin = nullptr;  // pinned host copy of the info words + kind totals (confirmation)
  hipEvent_t order_ev = nullptr;  // orders a decode on a new stream after the previous one
  hipEvent_t consumer_ev[2] = {nullptr, nullptr};  // fence_open / fence_close: consumer stream -> decode stream -> consumer
  Result res;  // the last decode
  // record-shape templates (tfrg_learn_templates): host key table, device templates
  std::unordered_map<std::string, uint32_t> key_id;
  std::vector<int32_t> key_slot_h;  // [4 * key]: flags, slot per kind
  uint32_t n_tpl = 0;
  uint32_t tpl_w = 0;  // window words of the templates (16 / 32 / 64)
  size_t tpl_img_off = 0;  // the lane image follows the window-form templates in tpl
  uint32_t tpl_img_words = 0;
  uint32_t tpl_tab_words = 0;  // the packed CRC position tables follow the image
  std::vector<uint32_t> tpl_h;  // host copy of the template words
  bool tpl_learned = false;
  bool tpl_full = false;  // the templates took every record of their learning sample
  uint32_t tpl_frames = 0;  // frame classes of the kept templates: bit 0 spec, bit 1 unchecked
  // speculative single-value placement (DevSchema::spec), derived from the templates
  std::vector<uint8_t> slot_kind_h;
  std::vector<uint32_t> spec_h;  // host copy (k_tpl_lane's placement targets)
  bool have_spec = false;
  // what the learned shapes have in common (Learned): an optimistic decode (launch_decode: a batch of
  // C1-shaped records whose templates took the learning sample runs as k_tpl_lane alone) leaves such
  // columns implicit and snapshots the constant into its Result
  bool ord_const = false;     // every shape has the same order words
  bool len_const = false;     // ... and the same bytes element lengths
  std::vector<uint32_t> const_len;  // per slot: that length
  uint64_t off_rel = 0;       // bytes slots at one end-relative offset in every shape
  std::vector<int32_t> rel_off;  // per slot: that offset
  uint32_t i64_width = 8;     // bytes that hold every int64 value the shapes place (Learned::i64_width)
  // optional per-stage HIP events (tfrg_ctx_set_profiling)
  bool profiling = false;
  bool have_events = false;
  hipEvent_t ev[kNumStages + 1] = {};
  // value-capacity hints (tfrg_ctx_set_value_caps; 0: the worst case)
  uint64_t hint_i64 = 0, hint_f32 = 0, hint_b = 0;
  uint64_t hint_reruns = 0;  // decodes re-run: a hint was too small, or an optimistic decode incomplete
  uint32_t index_chunk = kIndexChunkDefault;  // tfrg_ctx_set_index_chunk
  uint32_t ragged_tile = kRaggedTileDefault;  // tfrg_ctx_set_ragged_tile: rows per tile
  uint32_t select_tile = kSelTileDefault;     // tfrg_ctx_set_select_tile: candidates per tile
  uint32_t token_split = kTokSplitDefault;   // tfrg_ctx_set_token_split: rows above it go by wave
  uint32_t select_scan = kSelScanDefault;     // tfrg_ctx_set_select_scan: CONTAINS elements above it go by wave
  void* fr_pin = nullptr;  // tfrg_index_device: pinned host staging
  size_t fr_pin_cap = 0;
};

// (TFRG_IMPLICIT_BYTES_LEN) a bytes slot's constant element length, as the decode ran with it
inline uint32_t implicit_len(const Result& r, uint32_t slot) { return slot < kLeanMaxSlots ? r.slot[slot].elem_len : 0u; }

// An optimistic decode, or one whose value capacities were hinted below the worst case, is confirmed
// (or re-run in full / at the worst case) before anything reads its columns on the device (tfrg_capi.cpp).
namespace tfrg {
int confirm_pending(tfrg_ctx* c);
}

// ---- Host-side setup shared by the entry points over the last result (result_dense and result_fixed_rows
// in tfrg_fixed.cpp, result_row_list and result_select in tfrg_rowlist.cpp). `bad` is the entry point's
// own: it prefixes the function's name.
template <class Bad>
static int check_result(const tfrg_ctx* c, const Bad& bad) {
  if (!c) return bad("no context");
  if (!c->res.valid) return bad("no result (decode first)");
  return 0;
}
template <class Bad>
static int check_specs(const tfrg_ctx* c, const void* specs, uint32_t n_specs, uint32_t max_specs, const Bad& bad) {
  if (const int rc = check_result(c, bad)) return rc;
  if (!specs || n_specs == 0 || n_specs > max_specs) return bad("n_specs must be 1.." + std::to_string(max_specs));
  return 0;
}
// (the spec's slot exists and its TFRG_DENSE_* dtype fits the slot's kind)
template <class Bad>
static int check_slot_dtype(const tfrg_ctx* c, const std::string& at, uint32_t slot, uint32_t dtype, const Bad& bad) {
  if (slot >= c->n_slots) return bad(at + "slot " + std::to_string(slot) + " >= n_slots");
  const uint32_t kind = c->slot_kind_h[slot] & 3u;
  const bool fits = (kind == TFRG_KIND_INT64 && (dtype == TFRG_DENSE_I64 || dtype == TFRG_DENSE_I32)) ||
                    (kind == TFRG_KIND_FLOAT && dtype == TFRG_DENSE_F32) ||
                    (kind == TFRG_KIND_BYTES && dtype == TFRG_DENSE_U8);
  if (!fits) return bad(at + "dtype " + std::to_string(dtype) + " does not fit the slot's kind " + std::to_string(kind));
  return 0;
}
// The row list. tfrg_result_dense_rows always has one (`required`): its rows_dtype is checked whatever
// d_rows is, and m > 0 rows need a d_rows. Ragged and select take a NULL d_rows as the identity list and
// read rows_dtype only beside a list. (Two functions: select checks its out_dtype between them.)
template <class Bad>
static int check_rows_dtype(const void* d_rows, uint32_t rows_dtype, bool required, const Bad& bad) {
  if ((required || d_rows) && rows_dtype != TFRG_ROWS_I32 && rows_dtype != TFRG_ROWS_I64)
    return bad("rows_dtype must be TFRG_ROWS_I32 or TFRG_ROWS_I64, not " + std::to_string(rows_dtype));
  return 0;
}
template <class Bad>
static int check_rows_m(const void* d_rows, uint32_t m, bool required, const Bad& bad) {
  if (m >= 0x80000000u) return bad("m must be below 2^31");
  if (required && m && !d_rows) return bad("d_rows is NULL");
  return 0;
}

// (a record without a value reads element 0 of a value array and drops it: an array that was never
// allocated is stood in for by the slot bases, which every result has)
template <class T>
static const T* view_col(const tfrg_ctx* c, const DBuf& b) {
  return static_cast<const T*>(b.p ? b.p : c->slot_base.p);
}
// The width of the int64 column, for the argument structs that have the word (the passes that read
// int64 values: dense, ragged, select, resize); false for the others
template <class Args>
static auto set_i64_w(Args& a, uint32_t w, int) -> decltype((void)(a.i64_w = w), true) {
  a.i64_w = w;
  return true;
}
template <class Args>
static bool set_i64_w(Args&, uint32_t, long) {
  return false;
}
// The column view of the last result: what DenseArgs, RaggedArgs and SelectArgs have in common
template <class Args>
static void fill_columns(const tfrg_ctx* c, Args& a) {
  a.rs = c->rs.as<uint32_t>();
  a.slot_base = c->slot_base.as<uint64_t>();
  // (a narrowed decode: the narrow column as it is for the passes that read int64 values, through
  // col_i64 -- no widening pass; the others read neither column)
  const bool narrow = set_i64_w(a, c->res.i64_w, 0) && c->res.i64_w < 8u;
  a.i64 = view_col<int64_t>(c, narrow ? c->i64n : c->i64);
  a.f32 = view_col<uint32_t>(c, c->f32);
  a.b_len = view_col<uint32_t>(c, c->b_len);
  if (c->res.materialized) a.b_off64 = view_col<uint64_t>(c, c->boff64);
  a.info = c->info.as<uint32_t>() + c->info_slot * kInfoCount;
  a.n = c->res.req.n;
}
// The bytes' source: the views' input buffer, readable to round_up(nbytes, 16), or the byte column
template <class Args>
static void fill_bytes_source(const tfrg_ctx* c, Args& a) {
  a.b_off = view_col<uint32_t>(c, c->b_off);
  const Result& r = c->res;
  a.in = r.materialized ? c->bdata.as<uint8_t>() : r.req.d_bytes;
  const uint64_t bound = r.materialized ? (uint64_t)c->bdata.cap & ~15ull : (r.req.nbytes + 15ull) & ~15ull;
  a.in_bound = a.in ? (uint32_t)std::min<uint64_t>(bound, 0xfffffff0ull) : 0;
  // (the decode's u32 ends, for the specs with a const_off: read for such a spec only)
  a.end32 = r.off_mask ? r.req.off.e32 : nullptr;
}

// A bytes slot's end-relative element offset where the last decode did not store its bytes_off words
// (tfrg_info.implicit_off_slots: the element of record g is end32[g] + that); else the kernels' "the
// column is stored" sentinel.
static_assert(kDenseOffStored == kRaggedOffStored, "one const_off lookup serves both");
inline int32_t const_off_of(const tfrg_ctx* c, uint32_t slot, bool reads_off) {
  if (!reads_off || slot >= kLeanMaxSlots || !((c->res.off_mask >> slot) & 1ull)) return kDenseOffStored;
  return c->res.slot[slot].rel_off;
}

// A bytes slot's constant element length where the last decode did not store the bytes_len column (as
// constant_fills: the shapes' length holds); else, or for a spec / term that reads no length, the
// kernels' "the column is stored" sentinel.
static_assert(kDenseNoLen == kRaggedNoLen && kRaggedNoLen == kSelNoLen, "one const_len lookup serves all three");
static_assert(kElemsNoLen == kDenseNoLen && kElemsOffStored == kDenseOffStored, "and tfrg_elems.h's kernels");
inline uint32_t const_len_of(const tfrg_ctx* c, uint32_t slot, bool reads_len) {
  if (!reads_len || !(c->res.implicit & TFRG_IMPLICIT_BYTES_LEN)) return kDenseNoLen;
  return implicit_len(c->res, slot);
}

// The consumer-stream fence: the work an entry point puts on the decode's stream *st starts after what
// the consumer stream *cs holds so far (fence_open), and the consumer waits for it (fence_close). A
// NULL consumer_stream is the decode's own stream: no fence.
inline int fence_open(tfrg_ctx* c, void* consumer_stream, hipStream_t* st, hipStream_t* cs) {
  *st = c->last_stream;
  *cs = consumer_stream ? static_cast<hipStream_t>(consumer_stream) : *st;
  if (*cs == *st) return 0;
  for (hipEvent_t& e : c->consumer_ev)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->consumer_ev[0], *cs));
  HIP_TRY(hipStreamWaitEvent(*st, c->consumer_ev[0], 0));
  return 0;
}
inline int fence_close(tfrg_ctx* c, hipStream_t st, hipStream_t cs) {
  if (cs == st) return 0;
  HIP_TRY(hipEventRecord(c->consumer_ev[1], st));
  HIP_TRY(hipStreamWaitEvent(cs, c->consumer_ev[1], 0));
  return 0;
}

// (the spec's slot exists and is a bytes_list slot)
template <class Bad>
static int check_bytes_slot(const tfrg_ctx* c, const std::string& at, uint32_t slot, const Bad& bad) {
  if (slot >= c->n_slots) return bad(at + "slot " + std::to_string(slot) + " >= n_slots");
  const uint32_t kind = c->slot_kind_h[slot] & 3u;
  if (kind != TFRG_KIND_BYTES)
    return bad(at + "slot " + std::to_string(slot) + " is not a bytes_list slot (kind " + std::to_string(kind) + ")");
  return 0;
}
