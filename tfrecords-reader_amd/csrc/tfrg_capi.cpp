// tfrg_capi.cpp — device context of libtfrg: key table upload, HBM arena, decode orchestration and
// result transfer (include/tfrg.h). The kernels live in the .hip files; launch_decode (tfrg_decode.cpp)
// is their launch policy.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tfrg.h"
#include "crc32c.h"
#include "tfrg_dense.h"
#include "tfrg_elems.h"
#include "tfrg_ids.h"
#include "tfrg_ragged.h"
#include "tfrg_select.h"
#include "tfrg_frame.h"
#include "tfrg_internal.h"
#include "tfrg_learn.h"
#include "tfrg_vocab.h"

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
  DBuf i64, f32, b_off, b_len, big_list, slow_list, miss, info, tsum, crc_rec, crc_base, crc_part;
  DBuf dq, dq_cnt;  // deferred packed-int64 bodies (k_body_count)
  DBuf lmask, rlist;  // k_tpl_lane's per-group miss masks and listed groups
  DBuf bdata, boff64, blb, bbig;  // TFRG_FLAG_MATERIALIZE_BYTES
  DBuf tpl, spec;  // record-shape templates, speculative placement (tfrg_learn_templates)
  DBuf fr_tab, fr_dev;  // tfrg_index_device: chunk table, piece rows + summary
  DBuf rg_tsum;  // tfrg_result_ragged_rows: the per-tile sums
  DBuf el_tsum;  // tfrg_result_ragged_elems: the per-tile element counts and byte sums
  DBuf id_tsum;  // tfrg_result_elem_ids: the per-tile element counts
  DBuf sel_buf;  // tfrg_result_select_rows: the candidates' ballot words, then the per-tile sums
  template <class F>
  void each(F f) {
    DBuf* const all[] = {&crc_tab, &consts, &ht, &key_hash, &key_off, &key_blob, &key_slot, &slot_kind, &key_w, &krec,
                         &in_bytes, &in_start, &in_end, &status, &aux, &verdict, &order, &count, &loc, &rs, &slot_base,
                         &totals, &kind_totals, &ident, &i64, &f32, &b_off, &b_len, &big_list, &slow_list, &miss, &info,
                         &tsum, &crc_rec, &crc_base, &crc_part, &dq, &dq_cnt, &lmask, &rlist, &bdata, &boff64, &blb,
                         &bbig, &tpl, &spec, &fr_tab, &fr_dev, &rg_tsum, &el_tsum,
                         &id_tsum, &sel_buf};
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
  uint32_t select_scan = kSelScanDefault;     // tfrg_ctx_set_select_scan: CONTAINS elements above it go by wave
  void* fr_pin = nullptr;  // tfrg_index_device: pinned host staging
  size_t fr_pin_cap = 0;
};

extern "C" {

int tfrg_ctx_create(int device, tfrg_ctx** out) {
  *out = nullptr;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) {
    set_error("bad device index");
    return TFRG_E_ARG;
  }
  HIP_TRY(hipSetDevice(device));
  tfrg_ctx* c = new tfrg_ctx();
  c->device = device;
  auto num = [](const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; };
  Switches& s = c->sw;
  s.tpl_on = num("TFRG_TEMPLATES", 1) != 0;
  s.spec_on = num("TFRG_SPEC", 1) != 0;
  s.optimistic = num("TFRG_OPTIMISTIC", 1) != 0;
  s.implicit_off = num("TFRG_IMPLICIT_OFF", 1) != 0;
  s.walk_beside = num("TFRG_WALK_BESIDE", 1) != 0;
  s.tpl_stage = num("TFRG_TPL_STAGE", 1);
  const int gpw = num("TFRG_TPL_GPW", 0);
  if (gpw == 2 || gpw == 4 || gpw == 8) s.tpl_gpw = (uint32_t)gpw;
  s.walk_blocks = (uint32_t)num("TFRG_WALK_BLOCKS", 0);
  s.dense_nt = num("TFRG_DENSE_NT", 0) != 0;
  if (const char* e = getenv("TFRG_DEBUG_POISON_LOC")) {
    char* q = const_cast<char*>(e);
    for (int i = 0; i < 4 && *q; ++i) {
      s.poison[i] = (uint32_t)strtoul(q, &q, 10);
      while (*q == ',' || *q == ' ') ++q;
    }
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    c->num_cus = prop.multiProcessorCount;
    if (prop.maxSharedMemoryPerMultiProcessor) c->cu_lds = (uint32_t)prop.maxSharedMemoryPerMultiProcessor;
  }
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    set_error("hipStreamCreate failed");
    return TFRG_E_HIP;
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&c->info_pin), (kInfoCount + 8) * 4) != hipSuccess) {
    (void)hipStreamDestroy(c->own_stream);
    delete c;
    set_error("hipHostMalloc failed");
    return TFRG_E_NOMEM;
  }
  // CRC tables: [4][256] slice-by-4 + [4][256] multiply-by-x^8192 (streaming CRC), then
  // [8][256] slice-by-8 (lane kernel), then [16][256] slice-by-16 (streaming CRC), ...
  // (k_tpl_lane's position tables are packed per learned shape: learn_shapes); consts: 64 lane shifts
  // x^(128 l), 16 un-shifts x^(-8z) and 32 round shifts x^(8192 * 2^k)
  std::vector<uint32_t> tab(kCrcTabWords), cst(128);
  CrcTables T;
  crc_make_tables(&T);
  memcpy(tab.data(), T.t, 4096);
  uint32_t M[4][256];
  crc_make_mul_tables(gf_xpow8(1024), M);
  memcpy(tab.data() + 1024, M, 4096);
  memcpy(tab.data() + 2048, T.t, 8192);
  memcpy(tab.data() + 4096, T.t, 16384);  // slice-by-16 (streaming CRC)
  // the slice-by-16 tables in the streaming CRC's bank-conflict-free layout (tfrg_kernels.hip
  // chunk_rot): row e of 64 dwords, column c < 47 holding table (c + 1) & 15
  for (int e = 0; e < 256; ++e)
    for (int col = 0; col < 47; ++col) tab[8192 + e * 64 + col] = T.t[(col + 1) & 15][e];
  // multiply-by-x^16384 and x^32768 tables (the streaming CRC's split Horner sum over 4 rounds)
  crc_make_mul_tables(gf_xpow8(2048), M);
  memcpy(tab.data() + 24576, M, 4096);
  crc_make_mul_tables(gf_xpow8(4096), M);
  memcpy(tab.data() + 25600, M, 4096);
  // multiply by x^(8192 * 2^k), k < 24: a slice of a record split over waves shifted to its place
  for (int k = 0; k < 24; ++k) {
    crc_make_mul_tables(gf_xpow8(1024ull << k), M);
    memcpy(tab.data() + 26624 + k * 1024, M, 4096);
  }
  for (int l = 0; l < 64; ++l) cst[l] = gf_xpow8(16ull * l);
  for (int z = 0; z < 16; ++z) cst[64 + z] = gf_xpow8_inv((uint64_t)z);
  for (int k = 0; k < 32; ++k) cst[96 + k] = gf_xpow8(1024ull << k);  // x^(8192 * 2^k): round shifts
  if (c->crc_tab.ensure(tab.size() * 4) != hipSuccess || c->consts.ensure(cst.size() * 4) != hipSuccess ||
      hipMemcpy(c->crc_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->consts.p, cst.data(), cst.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("constant upload failed");
    tfrg_ctx_destroy(c);
    return TFRG_E_HIP;
  }
  *out = c;
  return 0;
}

int tfrg_ctx_destroy(tfrg_ctx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (c->last_stream) (void)hipStreamSynchronize(c->last_stream);
  c->each([](DBuf& b) { b.release(); });
  if (c->order_ev) (void)hipEventDestroy(c->order_ev);
  for (hipEvent_t e : c->consumer_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->have_events)
    for (auto& e : c->ev) (void)hipEventDestroy(e);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  if (c->info_pin) (void)hipHostFree(c->info_pin);
  if (c->fr_pin) (void)hipHostFree(c->fr_pin);
  delete c;
  return 0;
}

int tfrg_ctx_set_lane_max(tfrg_ctx* c, uint32_t lane_max) {
  if (!c) return TFRG_E_ARG;
  c->lane_max = lane_max;
  return 0;
}

int tfrg_ctx_set_record_bound(tfrg_ctx* c, uint64_t max_record_bytes) {
  if (!c) return TFRG_E_ARG;
  c->record_bound = max_record_bytes;
  return 0;
}

int tfrg_ctx_set_value_caps(tfrg_ctx* c, uint64_t int64_values, uint64_t float_values, uint64_t bytes_values) {
  if (!c) return TFRG_E_ARG;
  c->hint_i64 = int64_values;
  c->hint_f32 = float_values;
  c->hint_b = bytes_values;
  return 0;
}

int tfrg_ctx_device_bytes(tfrg_ctx* c, uint64_t* bytes, uint64_t* reruns) {
  if (!c) return TFRG_E_ARG;
  uint64_t t = 0;
  c->each([&t](const DBuf& b) { t += b.cap; });
  if (bytes) *bytes = t;
  if (reruns) *reruns = c->hint_reruns;
  return 0;
}

int tfrg_ctx_set_wave_stage(tfrg_ctx* c, uint32_t nbytes) {
  if (!c) return TFRG_E_ARG;
  c->wave_stage = nbytes;
  return 0;
}

int tfrg_ctx_set_index_chunk(tfrg_ctx* c, uint32_t bytes) {
  if (!c) return TFRG_E_ARG;
  if (bytes && (bytes < kIndexChunkMin || bytes > kIndexChunkMax || (bytes & (bytes - 1)))) {
    set_error("index chunk must be a power of two from 64 to 65536 (0: the default)");
    return TFRG_E_ARG;
  }
  c->index_chunk = bytes ? bytes : kIndexChunkDefault;
  return 0;
}

int tfrg_ctx_set_ragged_tile(tfrg_ctx* c, uint32_t rows) {
  if (!c) return TFRG_E_ARG;
  if (rows && (rows < kRaggedTileMin || rows > kRaggedTileMax || (rows & (rows - 1)))) {
    set_error("ragged tile must be a power of two from 64 to 4096 (0: the default)");
    return TFRG_E_ARG;
  }
  c->ragged_tile = rows ? rows : kRaggedTileDefault;
  return 0;
}

int tfrg_ctx_set_select_tile(tfrg_ctx* c, uint32_t rows) {
  if (!c) return TFRG_E_ARG;
  if (rows && (rows < kSelTileMin || rows > kSelTileMax || (rows & (rows - 1)))) {
    set_error("select tile must be a power of two from 64 to 4096 (0: the default)");
    return TFRG_E_ARG;
  }
  c->select_tile = rows ? rows : kSelTileDefault;
  return 0;
}

int tfrg_ctx_set_select_scan(tfrg_ctx* c, uint32_t bytes) {
  if (!c) return TFRG_E_ARG;
  if (bytes && (bytes < kSelScanMin || bytes > kSelScanMax)) {
    set_error("select scan must be from 4 to 65536 bytes (0: the default)");
    return TFRG_E_ARG;
  }
  c->select_scan = bytes ? bytes : kSelScanDefault;
  return 0;
}

// The framing index of n_pieces images in HBM (tfrg_frame.h: guess, walk, verify and repair, rank and
// write). One host synchronisation: the summary words and piece rows come back in one D2H.
int tfrg_index_device(tfrg_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* piece_sizes,
                      uint32_t n_pieces, uint64_t* d_start, uint64_t* d_end, uint32_t* d_end32, uint64_t cap,
                      uint64_t* piece_records, void* stream, tfrg_index_info* info) {
  if (!c || !info) {
    set_error("tfrg_index_device: NULL context or info");
    return TFRG_E_ARG;
  }
  memset(info, 0, sizeof(*info));
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n_pieces; ++i) sum += piece_sizes[i];
  if (nbytes >= (1ull << 32) || sum != nbytes) {
    set_error(nbytes >= (1ull << 32) ? "tfrg_index_device: batch larger than 4 GiB: split it"
                                     : "tfrg_index_device: the piece sizes do not sum to nbytes");
    return TFRG_E_ARG;
  }
  for (uint32_t i = 0; piece_records && i < n_pieces; ++i) piece_records[i] = 0;
  info->tiled = 1;
  if (!n_pieces || !nbytes) return 0;
  if (!d_bytes) return TFRG_E_ARG;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
  uint32_t shift = 0;
  while ((1u << shift) < c->index_chunk) ++shift;
  // pinned staging: the piece table (in), then the summary words and the piece rows (out)
  const size_t in_bytes = ((size_t)n_pieces * sizeof(FrPiece) + 63) & ~(size_t)63;
  const size_t out_bytes = kFsWords * 4 + (size_t)n_pieces * sizeof(FrPieceOut);
  if (c->fr_pin_cap < in_bytes + out_bytes) {
    if (c->fr_pin) (void)hipHostFree(c->fr_pin);
    c->fr_pin = nullptr;
    c->fr_pin_cap = 0;
    const size_t want = 2 * (in_bytes + out_bytes) + 4096;
    if (hipHostMalloc(&c->fr_pin, want) != hipSuccess) {
      set_error("pinned index staging allocation failed");
      return TFRG_E_NOMEM;
    }
    c->fr_pin_cap = want;
  }
  FrPiece* const h_pieces = (FrPiece*)c->fr_pin;
  uint8_t* const h_out = (uint8_t*)c->fr_pin + in_bytes;
  FrTab T{};
  const uint64_t nc = fr_layout(piece_sizes, n_pieces, shift, h_pieces, &T.jumps);
  if (nc >= 0xffffffffull) {
    set_error("tfrg_index_device: too many pieces");
    return TFRG_E_LIMIT;
  }
  const uint32_t n = (uint32_t)nc;
  const uint32_t nb = (n + kFrBlock - 1) / kFrBlock;
  // (every earlier index call has been synchronised: growing frees nothing in use)
  HIP_TRY(c->fr_tab.ensure(((size_t)n * 10 + nb) * 4));
  HIP_TRY(c->fr_dev.ensure(in_bytes + out_bytes));
  uint8_t* const d_in = c->fr_dev.as<uint8_t>();
  uint8_t* const d_out = d_in + in_bytes;
  HIP_TRY(hipMemcpyAsync(d_in, h_pieces, (size_t)n_pieces * sizeof(FrPiece), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_out, 0, out_bytes, st));
  T.bytes = d_bytes;
  T.pieces = (const FrPiece*)d_in;
  T.n_pieces = n_pieces;
  T.n_chunks = n;
  T.shift = shift;
  uint32_t* w = c->fr_tab.as<uint32_t>();
  uint32_t** cols[] = {&T.entry, &T.exit, &T.count, &T.cflags, &T.cpiece, &T.mark, &T.jump[0], &T.jump[1], &T.pend, &T.pend2};
  for (uint32_t** col : cols) {
    *col = w;
    w += n;
  }
  T.bsum = w;
  T.summ = (uint32_t*)d_out;
  T.pout = (FrPieceOut*)(d_out + kFsWords * 4);
  T.crc_t0 = c->crc_tab.as<uint32_t>();  // the byte table leads the context's CRC tables
  T.start = d_start;
  T.end = d_end;
  T.end32 = d_end32;
  T.cap = cap;
  HIP_TRY(launch_frame_index(T, c->num_cus, st));
  HIP_TRY(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  fr_finish((const uint32_t*)h_out, (const FrPieceOut*)(h_out + kFsWords * 4), h_pieces, n_pieces, n, piece_records,
            info);
  return 0;
}

int tfrg_ctx_set_profiling(tfrg_ctx* c, int on) {
  if (!c) return TFRG_E_ARG;
  c->profiling = on != 0;
  return 0;
}

int tfrg_profile_last(tfrg_ctx* c, float* ms, const char** names, int cap) {
  if (!c || !c->have_events || !c->res.valid) return TFRG_E_ARG;
  HIP_TRY(hipEventSynchronize(c->ev[kNumStages]));
  const int k = cap < kNumStages ? cap : (int)kNumStages;
  for (int i = 0; i < k; ++i) {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]));
    if (ms) ms[i] = t;
    if (names) names[i] = kStageNames[i];
  }
  return k;
}

static void key_words(const uint8_t* p, uint64_t n, uint32_t* w0, uint32_t* w1) {
  uint32_t a = 0, b = 0;
  for (uint64_t i = 0; i < (n < 4 ? n : 4); ++i) a |= (uint32_t)p[i] << (8 * i);
  if (n > 4)
    for (uint64_t i = 0; i < 4; ++i) b |= (uint32_t)p[n - 4 + i] << (8 * i);
  *w0 = a;
  *w1 = b;
}

int tfrg_set_schema(tfrg_ctx* c, uint32_t n_keys, const uint8_t* key_blob, const uint64_t* key_offsets,
                    const uint32_t* key_flags, uint32_t n_slots, const uint32_t* slot_key, const uint8_t* slot_kind) {
  if (!c) return TFRG_E_ARG;
  HIP_TRY(hipSetDevice(c->device));
  if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
  // a failure below may leave buffers reallocated: no schema and no result until this succeeds
  c->res = {};
  c->n_keys = c->n_slots = 0;
  c->ht_mask = 0;
  uint32_t hsz = 16;
  while (hsz < 2 * n_keys + 2) hsz <<= 1;
  std::vector<uint32_t> ht(hsz, 0), hash(n_keys ? n_keys : 1), off(n_keys + 1), kw(2ull * (n_keys ? n_keys : 1));
  std::vector<int32_t> ks(4ull * (n_keys ? n_keys : 1), -1);
  const uint64_t blob_len = n_keys ? key_offsets[n_keys] : 0;
  for (uint32_t k = 0; k < n_keys; ++k) {
    if (key_offsets[k + 1] < key_offsets[k] || key_offsets[k + 1] > 0xffffffffull) {
      set_error("bad key offsets");
      return TFRG_E_ARG;
    }
    off[k] = (uint32_t)key_offsets[k];
    const uint64_t kl = key_offsets[k + 1] - key_offsets[k];
    key_words(key_blob + key_offsets[k], kl, &kw[2ull * k], &kw[2ull * k + 1]);
    hash[k] = key_hash_words((uint32_t)kl, kw[2ull * k], kw[2ull * k + 1]);
    ks[4ull * k] = (int32_t)(key_flags ? (key_flags[k] & 1u) : 0u);
    uint32_t j = hash[k] & (hsz - 1);
    while (ht[j]) j = (j + 1) & (hsz - 1);
    ht[j] = k + 1;
  }
  off[n_keys] = (uint32_t)blob_len;
  for (uint32_t s = 0; s < n_slots; ++s) {
    if (slot_key[s] >= n_keys || slot_kind[s] < 1 || slot_kind[s] > 3) {
      set_error("bad slot");
      return TFRG_E_ARG;
    }
    ks[4ull * slot_key[s] + slot_kind[s]] = (int32_t)s;
  }
  if (c->ht.ensure(hsz * 4) || c->key_hash.ensure(hash.size() * 4) || c->key_off.ensure(off.size() * 4) ||
      c->key_blob.ensure(blob_len + 16) || c->key_slot.ensure(ks.size() * 4) || c->slot_kind.ensure(n_slots + 16) ||
      c->key_w.ensure(kw.size() * 4)) {
    set_error("schema allocation failed");
    return TFRG_E_NOMEM;
  }
  HIP_TRY(hipMemcpy(c->ht.p, ht.data(), hsz * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->key_hash.p, hash.data(), hash.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->key_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice));
  if (blob_len) HIP_TRY(hipMemcpy(c->key_blob.p, key_blob, blob_len, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->key_slot.p, ks.data(), ks.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->key_w.p, kw.data(), kw.size() * 4, hipMemcpyHostToDevice));
  std::vector<uint32_t> kr((size_t)kKrWords * (n_keys ? n_keys : 1), 0);
  for (uint32_t k = 0; k < n_keys; ++k) {
    uint32_t* r = &kr[(size_t)kKrWords * k];
    r[kKrHash] = hash[k];
    r[kKrLen] = (uint32_t)(key_offsets[k + 1] - key_offsets[k]);
    r[kKrW0] = kw[2ull * k];
    r[kKrW1] = kw[2ull * k + 1];
    for (int kind = 1; kind <= 3; ++kind) r[kKrSlot1 + kind - 1] = (uint32_t)ks[4ull * k + kind];
    r[kKrFlags] = (uint32_t)ks[4ull * k];
  }
  if (c->krec.ensure(kr.size() * 4)) {
    set_error("schema allocation failed");
    return TFRG_E_NOMEM;
  }
  HIP_TRY(hipMemcpy(c->krec.p, kr.data(), kr.size() * 4, hipMemcpyHostToDevice));
  if (n_slots) HIP_TRY(hipMemcpy(c->slot_kind.p, slot_kind, n_slots, hipMemcpyHostToDevice));
  c->n_keys = n_keys;
  c->n_slots = n_slots;
  c->ht_mask = hsz - 1;
  c->key_id.clear();
  for (uint32_t k = 0; k < n_keys; ++k)
    c->key_id.emplace(std::string((const char*)key_blob + key_offsets[k], key_offsets[k + 1] - key_offsets[k]), k);
  c->key_slot_h = ks;
  c->slot_kind_h.assign(slot_kind, slot_kind + n_slots);
  c->n_tpl = 0;  // slots may have moved: learn again from the next host batch
  c->off_rel = 0;
  c->rel_off.clear();
  c->tpl_learned = false;
  c->have_spec = false;
  return 0;
}

static DevSchema schema_view(const tfrg_ctx* c) {
  DevSchema s;
  s.n_keys = c->n_keys;
  s.n_slots = c->n_slots;
  s.ht_mask = c->ht_mask;
  s.ht = c->ht.as<uint32_t>();
  s.key_hash = c->key_hash.as<uint32_t>();
  s.key_off = c->key_off.as<uint32_t>();
  s.key_blob = c->key_blob.as<uint8_t>();
  s.key_slot = c->key_slot.as<int32_t>();
  s.slot_kind = c->slot_kind.as<uint8_t>();
  s.key_w = c->key_w.as<uint32_t>();
  s.krec = c->krec.as<uint32_t>();
  s.tpl = c->tpl.as<uint32_t>();
  s.tpl_img = s.tpl + c->tpl_img_off;
  s.tpl_img_words = c->tpl_img_words;
  s.tpl_tab_words = c->tpl_tab_words;
  s.n_tpl = c->sw.tpl_on ? c->n_tpl : 0u;
  s.tpl_w = c->tpl_w;
  // speculative placement is a property of the learned shapes' schema (a slot that is one inline
  // value in every shape), not of the template match: it stays on with the templates off, where
  // k_lane_count places those values itself
  // (and without any shape: learn_single_slots)
  s.spec = c->sw.spec_on && c->have_spec ? c->spec.as<uint32_t>() : nullptr;
  return s;
}

// record-shape templates (tfrg_layout.h), learned from host records (tfrg_learn.cpp) and uploaded
extern "C" int tfrg_learn_templates(tfrg_ctx* c, const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_start,
                                    const uint64_t* h_end, uint32_t n, uint32_t flags) {
  if (!c || (n && (!h_bytes || !h_start || !h_end))) return TFRG_E_ARG;
  c->tpl_learned = true;
  c->n_tpl = 0;
  c->tpl_frames = 0;
  c->have_spec = false;
  c->off_rel = 0;  // (no shape, no end-relative slot: tfrg_ctx_rel_off answers from the kept shapes only)
  c->rel_off.clear();
  if (!c->n_keys) return 0;
  const TplSchema sch{c->key_id, c->key_slot_h, c->slot_kind_h};
  Learned L;
  const uint32_t nt = learn_shapes(&sch, c->n_slots, h_bytes, nbytes, h_start, h_end, n, flags, L);
  // no record shape: the speculative placement of single-value slots alone
  if (!nt && !(L.have_spec = learn_single_slots(&sch, c->n_slots, h_bytes, nbytes, h_start, h_end, n, flags, L.spec)))
    return 0;
  const size_t spec_bytes = (size_t)c->n_slots * 4;
  HIP_TRY(hipSetDevice(c->device));
  if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
  if ((nt && c->tpl.ensure((L.w.size() + L.img.size() + L.ptab.size()) * 4)) ||
      (L.have_spec && c->spec.ensure(spec_bytes))) {
    set_error("template allocation failed");
    return TFRG_E_NOMEM;
  }
  if (nt) {  // templates, their lane image, the packed tables: one buffer
    uint32_t* const d = c->tpl.as<uint32_t>();
    HIP_TRY(hipMemcpy(d, L.w.data(), L.w.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + L.w.size(), L.img.data(), L.img.size() * 4, hipMemcpyHostToDevice));
    if (!L.ptab.empty())
      HIP_TRY(hipMemcpy(d + L.w.size() + L.img.size(), L.ptab.data(), L.ptab.size() * 4, hipMemcpyHostToDevice));
    c->tpl_img_off = L.w.size();
    c->tpl_img_words = (uint32_t)L.img.size();
    c->tpl_tab_words = (uint32_t)L.ptab.size();
    c->n_tpl = nt;
    c->tpl_w = L.W;
    c->tpl_h = L.w;
    c->tpl_full = L.full;
    c->tpl_frames = L.frames;
    c->ord_const = L.ord_const;
    c->len_const = L.len_const;
    c->const_len = L.const_len;
    c->off_rel = L.off_rel;
    c->rel_off = L.rel_off;
  }
  if (L.have_spec) HIP_TRY(hipMemcpy(c->spec.p, L.spec.data(), spec_bytes, hipMemcpyHostToDevice));
  c->spec_h = L.spec;
  c->have_spec = L.have_spec;
  return (int)nt;
}

extern "C" int tfrg_template_count(tfrg_ctx* c) { return c ? (int)c->n_tpl : TFRG_E_ARG; }

extern "C" int tfrg_template_frames(tfrg_ctx* c) { return c ? (int)(c->n_tpl ? c->tpl_frames : 0u) : TFRG_E_ARG; }

extern "C" int tfrg_template_words(tfrg_ctx* c, uint32_t* out, uint64_t cap, uint32_t* window_words) {
  if (!c) return TFRG_E_ARG;
  if (window_words) *window_words = c->tpl_w;
  const uint64_t nw = (uint64_t)c->n_tpl * kLtWords;
  if (out) memcpy(out, c->tpl_h.data(), (nw < cap ? nw : cap) * 4);
  return (int)c->n_tpl;
}

extern "C" int tfrg_ctx_set_templates(tfrg_ctx* c, int on) {
  if (!c) return TFRG_E_ARG;
  c->sw.tpl_on = on != 0;
  return 0;
}

static int decode_device_any(tfrg_ctx* c, const DecodeReq& req);

int tfrg_decode_device(tfrg_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_start,
                       const uint64_t* d_end, uint32_t n, uint32_t flags, void* stream) {
  DecodeReq q{d_bytes, nbytes, {}, n, flags, static_cast<hipStream_t>(stream)};
  q.off.s64 = d_start;
  q.off.e64 = d_end;
  return decode_device_any(c, q);
}

int tfrg_decode_device32(tfrg_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, const uint32_t* d_start32,
                         const uint32_t* d_end32, uint32_t first_start, uint32_t n, uint32_t flags, void* stream) {
  if (n && !d_end32) return TFRG_E_ARG;
  DecodeReq q{d_bytes, nbytes, {}, n, flags, static_cast<hipStream_t>(stream)};
  q.off.s32 = d_start32;
  q.off.e32 = d_end32;
  q.off.first = first_start;
  q.off.mode = d_start32 ? kOffU32 : kOffEnds;
  return decode_device_any(c, q);
}

// TFRG_FLAG_MATERIALIZE_BYTES: the bytes views of the decode just enqueued on `st` gathered into one
// contiguous column. Reads the decode's kind totals and b_off / b_len, so it runs only once they are
// final: after a full decode at once, after an optimistic one once finish_decode has confirmed it.
static hipError_t launch_materialize_last(tfrg_ctx* c, const DecodeReq& q, uint64_t cap_b) {
  uint32_t* const info = c->info.as<uint32_t>() + c->info_slot * kInfoCount;
  DevBytes d;
  d.in = q.d_bytes;
  d.in_readable = (q.nbytes + 15) & ~15ull;
  d.b_off = c->b_off.as<uint32_t>();
  d.b_len = c->b_len.as<uint32_t>();
  d.kind_totals = c->kind_totals.as<uint64_t>();
  d.offsets = c->boff64.as<uint64_t>();
  d.offsets_cap = cap_b;
  d.data = c->bdata.as<uint8_t>();
  d.data_cap = q.cap_in + 16;
  d.lb = c->blb.as<uint64_t>();
  d.ticket = info + kInfoBytesTicket;
  d.big_count = info + kInfoBytesBig;
  d.big_list = c->bbig.as<uint32_t>();
  d.overflow = info + kInfoOverflow;
  return launch_materialize(d, c->num_cus, q.stream);
}

// The buffers of one group at the sizes a decode needs. Growing one frees the old allocation, so the
// previous stream's work, which may still read it, is waited for first.
static int ensure_group(tfrg_ctx* c, const char* group, std::initializer_list<std::pair<DBuf*, size_t>> needs) {
  bool grow = false;
  for (const auto& [buf, bytes] : needs) grow |= buf->cap < bytes;
  if (grow && c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
  for (const auto& [buf, bytes] : needs)
    if (buf->ensure(bytes) != hipSuccess) {
      set_error(std::string("device allocation failed") + group);
      return TFRG_E_NOMEM;
    }
  return 0;
}

static int decode_device_any(tfrg_ctx* c, const DecodeReq& req) {
  if (!c) return TFRG_E_ARG;
  if (req.nbytes >= (1ull << 32)) {
    set_error("batch larger than 4 GiB: split it");
    return TFRG_E_LIMIT;
  }
  if (c->n_keys == 0) {  // an empty table still needs valid (non-null) pointers
    uint64_t z = 0;
    int st = tfrg_set_schema(c, 0, nullptr, &z, nullptr, 0, nullptr, nullptr);
    if (st) return st;
  }
  HIP_TRY(hipSetDevice(c->device));
  c->res = {};  // no result until this decode is enqueued (the checks above leave the previous one)
  // the request as it runs (and as the result keeps it): stream, flags, capacity and bound resolved
  DecodeReq q = req;
  if (!q.stream) q.stream = c->own_stream;
  if (q.flags & TFRG_FLAG_STRICT_CRC) q.flags &= ~TFRG_FLAG_NO_CRC;  // strict mode needs the verdicts
  // value capacities: bounds for disjoint ranges (one int64 per byte, one float per 4, one bytes
  // element per 2); tfrg_decode_host passes the total of its ranges, which covers overlaps. A batch
  // of overlapping device ranges that exceeds them is reported by tfrg_result_info (TFRG_E_LIMIT).
  q.cap_in = std::max(q.cap_in, q.nbytes);
  if (!q.bound) q.bound = c->record_bound;
  const hipStream_t st = q.stream;
  const uint32_t n = q.n, flags = q.flags;
  const uint64_t nbytes = q.nbytes, cap_in = q.cap_in;
  // a decode on another stream than the previous one must not overtake it (shared arena)
  if (c->last_stream && c->last_stream != st) {
    if (!c->order_ev) HIP_TRY(hipEventCreateWithFlags(&c->order_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->order_ev, c->last_stream));
    HIP_TRY(hipStreamWaitEvent(st, c->order_ev, 0));
  }
  Result r;
  uint64_t &cap_i64 = r.cap_i64, &cap_f32 = r.cap_f32, &cap_b = r.cap_b;
  const uint32_t S = c->n_slots;
  const uint64_t nn = n ? n : 1;
  const uint64_t ngroups = (nn + 63) / 64;  // k_tpl_lane's 64-record groups
  const uint32_t n_tiles = (n + kTileRecs - 1) / kTileRecs;
  const uint32_t tile_stride = (n_tiles + 3u) & ~3u;
  const uint32_t n_chunks = (n_tiles + (1u << kSpineChunkShift) - 1u) >> kSpineChunkShift;
  // tile sums + look-back words + per-slot irregular-record counts (DevOut::irr)
  const uint64_t tsum_words = (uint64_t)S * tile_stride + 2ull * S * n_chunks + S;
  cap_i64 = cap_in + 16, cap_f32 = cap_in / 4 + 16, cap_b = cap_in / 2 + 16;
  // value-capacity hints (tfrg_ctx_set_value_caps) below the worst case: a decode that overflows one
  // is re-run with the worst case by tfrg_result_info (finish_decode), before any result is read
  auto hint = [&](uint64_t h, uint64_t& cap) {
    if (!q.worst_case && h && h + 16 < cap) {
      cap = h + 16;
      r.hinted = true;
    }
  };
  hint(c->hint_i64, cap_i64);
  hint(c->hint_f32, cap_f32);
  hint(c->hint_b, cap_b);
  const size_t tsum_cap0 = c->tsum.cap;
  if (const int rc = ensure_group(
          c, "",
          {{&c->status, nn * 4}, {&c->aux, nn * 8}, {&c->verdict, nn}, {&c->order, S * nn * 2}, {&c->count, S * nn * 4},
           {&c->loc, S * nn * 8}, {&c->rs, S * (nn + 1) * 4}, {&c->slot_base, (S + 1) * 8}, {&c->totals, (S + 1) * 4},
           {&c->kind_totals, 32}, {&c->i64, cap_i64 * 8}, {&c->f32, cap_f32 * 4}, {&c->b_off, cap_b * 4},
           {&c->b_len, cap_b * 4}, {&c->big_list, nn * 4}, {&c->slow_list, nn * 4}, {&c->miss, kMissCap * 16ull},
           {&c->info, 2 * kInfoCount * 4}, {&c->tsum, tsum_words * 4 + 16}, {&c->crc_rec, nn * 4}, {&c->crc_base, nn * 8},
           {&c->crc_part, nn * 8}, {&c->lmask, ngroups * 8}, {&c->rlist, ngroups * 4}}))
    return rc;
  // per-call counters (Guideline 16: every polled word zero per call): this decode's info slot was
  // zeroed by the previous decode's k_lane_count, else (a fresh context, an empty batch or a failed
  // launch before) here
  const uint32_t islot = c->info_slot ^ 1u;
  uint32_t* const info_cur = c->info.as<uint32_t>() + islot * kInfoCount;
  if (!c->info_clean) HIP_TRY(hipMemsetAsync(info_cur, 0, kInfoCount * 4, st));
  c->info_clean = false;
  c->info_slot = islot;
  // the row-split scan words are zero between decodes (k_down_gather clears what it used): only a
  // fresh buffer, or one a failed launch may have left dirty, is cleared here
  if (c->tsum.cap != tsum_cap0 || c->tsum_dirty) {
    HIP_TRY(hipMemsetAsync(c->tsum.p, 0, c->tsum.cap, st));
    // (no stale kStatusRedo: a decode whose launches failed may have left one)
    HIP_TRY(hipMemsetAsync(c->status.p, 0, c->status.cap, st));
    c->tsum_dirty = false;
  }
  if (S && n == 0) HIP_TRY(hipMemsetAsync(c->rs.p, 0, S * 4, st));
  const bool mat = (flags & TFRG_FLAG_MATERIALIZE_BYTES) != 0;
  const uint64_t lb_words = materialize_lb_words(cap_b);
  if (mat) {
    if (const int rc = ensure_group(c, " (materialized bytes)", {{&c->bdata, cap_in + 16}, {&c->boff64, (cap_b + 1) * 8},
                                                                {&c->blb, lb_words * 8}, {&c->bbig, cap_b * 4}}))
      return rc;
    HIP_TRY(hipMemsetAsync(c->blb.p, 0, lb_words * 8, st));
    if (!n) HIP_TRY(hipMemsetAsync(c->boff64.p, 0, 8, st));
  }
  if (!S || !n) HIP_TRY(hipMemsetAsync(c->kind_totals.p, 0, 32, st));

  DevBatch b;
  b.bytes = q.d_bytes;
  b.nbytes = nbytes;
  b.start = q.off.s64;
  b.end = q.off.e64;
  b.start32 = q.off.s32;
  b.end32 = q.off.e32;
  b.first = q.off.first;
  b.omode = q.off.mode;
  b.n = n;
  b.flags = flags;
  DevOut o;
  o.status = c->status.as<int32_t>();
  o.aux = c->aux.as<int64_t>();
  o.verdict = c->verdict.as<uint8_t>();
  o.order = c->order.as<uint16_t>();
  o.count = c->count.as<uint32_t>();
  o.loc = c->loc.as<uint2>();
  o.rs = c->rs.as<uint32_t>();
  o.slot_base = c->slot_base.as<uint64_t>();
  o.totals = c->totals.as<uint32_t>();
  o.kind_totals = c->kind_totals.as<uint64_t>();
  o.i64 = c->i64.as<int64_t>();
  o.f32 = c->f32.as<uint32_t>();
  o.b_off = c->b_off.as<uint32_t>();
  o.b_len = c->b_len.as<uint32_t>();
  o.cap_i64 = cap_i64;
  o.cap_f32 = cap_f32;
  o.cap_b = cap_b;
  o.big_list = c->big_list.as<uint32_t>();
  o.miss = c->miss.as<uint32_t>();
  o.miss_cap = kMissCap;
  o.info = info_cur;
  o.info_next = c->info.as<uint32_t>() + (islot ^ 1u) * kInfoCount;
  o.tsum = c->tsum.as<uint32_t>();
  o.tile_stride = tile_stride;
  o.spine_lb = reinterpret_cast<uint64_t*>(o.tsum + (size_t)S * tile_stride);  // 16-byte aligned
  o.n_chunks = n_chunks;
  o.irr = o.tsum + (size_t)S * tile_stride + 2ull * S * n_chunks;
  o.slow_list = c->slow_list.as<uint32_t>();
  o.crc_rec = c->crc_rec.as<uint32_t>();
  o.crc_base = c->crc_base.as<uint64_t>();
  o.crc_part = c->crc_part.as<uint64_t>();
  o.lmask = c->lmask.as<uint64_t>();
  o.rlist = c->rlist.as<uint32_t>();
  LaunchCfg cfg;
  cfg.num_cus = c->num_cus;
  cfg.tpl_cu_lds = c->sw.tpl_stage ? c->cu_lds : 0u;
  cfg.tpl_stage_any = c->sw.tpl_stage == 2;
  cfg.tpl_gpw = c->sw.tpl_gpw;
  cfg.lean = c->sw.tpl_on && c->n_tpl;
  cfg.tpl_full = cfg.lean && c->tpl_full;
  cfg.tpl_unchecked = cfg.lean && (c->tpl_frames & 2u) != 0;
  cfg.spec_h = c->spec_h.empty() ? nullptr : c->spec_h.data();
  const uint64_t lane_blocks = (n + 255) / 256;
  const uint64_t lane_cap = (uint64_t)c->num_cus * 8;
  cfg.lane_grid = (int)(lane_blocks < 1 ? 1 : (lane_blocks < lane_cap ? lane_blocks : lane_cap));
  const uint64_t wave_cap = (uint64_t)c->num_cus * 4;
  const uint64_t wave_blocks = (n + 3) / 4;
  cfg.wave_grid = (int)(wave_blocks < 1 ? 1 : (wave_blocks < wave_cap ? wave_blocks : wave_cap));
  cfg.lane_max = c->lane_max;
  cfg.wave_stage = c->wave_stage;
  memcpy(cfg.poison, c->sw.poison, sizeof(cfg.poison));
  // (the poison hook needs the gathers it tests)
  cfg.optimistic = c->sw.optimistic && !q.full && c->sw.poison[0] == 0xffffffffu;
  cfg.walk_beside = c->sw.walk_beside;
  cfg.walk_blocks = c->sw.walk_blocks;
  cfg.ran_optimistic = false;
  cfg.ran_quiet_big = false;
  cfg.ord_const = c->ord_const;
  cfg.len_const = c->len_const && !mat;  // (the byte gather reads the lengths)
  cfg.implicit = 0;
  cfg.off_rel = c->sw.implicit_off ? c->off_rel : 0ull;  // (launch_decode: u32 offsets, no byte gather)
  cfg.implicit_off = 0;
  // deferred packed bodies when records above lane_max may be walked from HBM: one 64-row block
  // (2,048 entries of 16 bytes) per 256 KiB of input, at least 16
  o.dq = nullptr;
  o.dq_cnt = nullptr;
  o.dq_blocks = 0;
  cfg.body_count = false;
  if (n && (q.bound == 0 || q.bound > c->lane_max)) {
    uint64_t blocks = nbytes >> 18;
    blocks = blocks < 16 ? 16 : (blocks > (1u << 16) ? (1u << 16) : blocks);
    const size_t qb = (size_t)blocks * 64u * kDeferK * 16u, cb = (size_t)blocks * 64u;
    if (const int rc = ensure_group(c, " (deferred bodies)", {{&c->dq, qb}, {&c->dq_cnt, cb}})) return rc;
    o.dq = c->dq.as<uint4>();
    o.dq_cnt = c->dq_cnt.as<uint8_t>();
    o.dq_blocks = (uint32_t)blocks;
    cfg.body_count = true;
  }
  if (n) {
    hipEvent_t* ev = nullptr;
    if (c->profiling) {
      if (!c->have_events) {
        for (auto& e : c->ev) HIP_TRY(hipEventCreate(&e));
        c->have_events = true;
      }
      ev = c->ev;
    }
    hipError_t e = launch_decode(b, schema_view(c), o, cfg, c->crc_tab.as<uint32_t>(), c->consts.as<uint32_t>(), st, ev);
    // (an optimistic decode that leaves records writes no kind totals and is re-run in full: its
    // byte views are gathered only once finish_decode has confirmed it)
    if (e == hipSuccess && mat && S && !cfg.ran_optimistic) {
      e = launch_materialize_last(c, q, cap_b);
    } else if (e == hipSuccess && mat && !S) {
      e = hipMemsetAsync(c->boff64.p, 0, 8, st);  // no slots: no elements
    }
    if (ev && e == hipSuccess) e = hipEventRecord(ev[kNumStages], st);
    if (e != hipSuccess) {
      c->tsum_dirty = true;
      set_error(std::string("kernel launch: ") + hipGetErrorString(e));
      return TFRG_E_HIP;
    }
  }
  c->info_clean = n != 0;  // (k_lane_count ran: the other slot is zero)
  c->last_stream = st;
  // (an optimistic decode without shapes leaves the lane kernel's tile sums in the scan words: the
  // next decode clears them; one with shapes writes none)
  if (n != 0 && cfg.ran_quiet_big) c->tsum_dirty = true;
  r.valid = true;
  r.materialized = mat;
  r.opt_pending = n != 0 && cfg.ran_optimistic;
  r.mat_pending = r.opt_pending && mat && S;
  r.implicit = n != 0 ? cfg.implicit : 0u;
  r.off_mask = n != 0 ? cfg.implicit_off : 0ull;
  // (k_tpl_lane stored status and verdict per record and no aux: every record of a confirmed decode is OK)
  r.aux_zero = r.opt_pending && !cfg.ran_quiet_big && !(cfg.implicit & TFRG_IMPLICIT_STATUS);
  for (uint32_t k = 0; (r.implicit || r.off_mask) && k < S && k < kLeanMaxSlots; ++k) {
    Result::SlotConst& sc = r.slot[k];
    if ((r.off_mask >> k) & 1ull) sc.rel_off = c->rel_off[k];
    if (r.implicit & TFRG_IMPLICIT_ORDER) sc.order_word = (uint16_t)(c->tpl_h[kLtSlot + 3 * k] >> 16);
    if ((r.implicit & TFRG_IMPLICIT_BYTES_LEN) && k < c->const_len.size()) sc.elem_len = c->const_len[k];
  }
  r.req = q;
  c->res = r;
  return 0;
}

int tfrg_decode_host(tfrg_ctx* c, const uint8_t* h_bytes, uint64_t nbytes, const uint64_t* h_start,
                     const uint64_t* h_end, uint32_t n, uint32_t flags, void* stream) {
  if (!c) return TFRG_E_ARG;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->own_stream;
  const uint64_t pad = ((nbytes + 15) & ~15ull) + 16;
  if (c->last_stream) HIP_TRY(hipStreamSynchronize(c->last_stream));
  if (c->in_bytes.ensure(pad) || c->in_start.ensure((uint64_t)(n ? n : 1) * 8) ||
      c->in_end.ensure((uint64_t)(n ? n : 1) * 8)) {
    set_error("staging allocation failed");
    return TFRG_E_NOMEM;
  }
  if (nbytes) HIP_TRY(hipMemcpyAsync(c->in_bytes.p, h_bytes, nbytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(c->in_bytes.as<uint8_t>() + nbytes, 0, pad - nbytes, st));
  if (n) {
    HIP_TRY(hipMemcpyAsync(c->in_start.p, h_start, (size_t)n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->in_end.p, h_end, (size_t)n * 8, hipMemcpyHostToDevice, st));
  }
  uint64_t total = 0, widest = 0;  // bytes of all ranges (clamped to the buffer): repeated ranges count again
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t a = h_start[i], b = h_end[i] < nbytes ? h_end[i] : nbytes;
    if (b > a) total += b - a;
    if (h_end[i] > a && h_end[i] - a > widest) widest = h_end[i] - a;
  }
  if (!c->tpl_learned && c->n_keys && c->sw.tpl_on) {  // record shapes of the first host batch of a schema
    const int t = tfrg_learn_templates(c, h_bytes, nbytes, h_start, h_end, n, flags);
    if (t < 0) return t;
  }
  DecodeReq q{c->in_bytes.as<uint8_t>(), nbytes, {}, n, flags, st};
  q.off.s64 = c->in_start.as<uint64_t>();
  q.off.e64 = c->in_end.as<uint64_t>();
  q.cap_in = total;
  q.bound = widest ? widest : 1;
  return decode_device_any(c, q);
}

// The last decode's info words and kind totals (synchronizes its stream). The same decode is re-run
// -- its inputs are still the caller's: it has not been reported complete -- when it ran
// optimistically and a record took no template (kInfoResid: again with every pass), or when a
// value-capacity hint was too small for it (again with the worst-case capacities).
static int finish_decode(tfrg_ctx* c, uint32_t* h, uint64_t* kt) {
  bool widened = false;
  // (into pinned memory, allocated with the context: two DMA copies instead of staged pageable ones)
  for (;;) {
    Result& r = c->res;
    HIP_TRY(hipMemcpyAsync(c->info_pin, c->info.as<uint32_t>() + c->info_slot * kInfoCount, kInfoCount * 4,
                           hipMemcpyDeviceToHost, c->last_stream));
    HIP_TRY(hipMemcpyAsync(c->info_pin + kInfoCount, c->kind_totals.p, 32, hipMemcpyDeviceToHost, c->last_stream));
    HIP_TRY(hipStreamSynchronize(c->last_stream));
    memcpy(h, c->info_pin, kInfoCount * 4);
    memcpy(kt, c->info_pin + kInfoCount, 32);
    const bool full = r.opt_pending && h[kInfoResid] != 0;  // (records no template took)
    const bool widen = h[kInfoOverflow] && r.hinted && !widened;
    if (!full && !widen) {
      if (!r.mat_pending) break;
      // a confirmed optimistic decode: its byte views now, then its info words again (the gather
      // reports an overflow there)
      r.mat_pending = false;
      HIP_TRY(launch_materialize_last(c, r.req, r.cap_b));
      continue;
    }
    DecodeReq again = r.req;  // (a copy: the decode replaces the result)
    again.full = true;
    again.worst_case = widen;
    c->tsum_dirty = true;  // (the optimistic pass skipped the tile sums; clear every scan word)
    if (const int rc = decode_device_any(c, again)) return rc;
    widened |= widen;
    ++c->hint_reruns;
  }
  c->res.opt_pending = false;
  c->res.hinted = false;  // (confirmed: the capacities held, or the worst-case re-run replaced it)
  return 0;
}

// value columns that overflowed their capacity (the decode's info words `h`): the result is an error
static int overflow_status(const uint32_t* h) {
  if (!h[kInfoOverflow]) return 0;
  set_error("value columns overflowed their capacity (overlapping ranges in a device batch): decode "
            "the ranges from host memory (tfrg_decode_host) or split the batch");
  return TFRG_E_LIMIT;
}

// An optimistic decode, or one whose value capacities were hinted below the worst case, is confirmed
// (or re-run in full / at the worst case) before anything reads its columns on the device.
static int confirm_pending(tfrg_ctx* c) {
  if (!c->res.opt_pending && !c->res.hinted) return 0;
  HIP_TRY(hipSetDevice(c->device));
  uint32_t h[kInfoCount];
  uint64_t kt[4];
  const int rc = finish_decode(c, h, kt);
  return rc ? rc : overflow_status(h);
}

int tfrg_result_info(tfrg_ctx* c, tfrg_info* info) {
  if (!c || !c->res.valid) return TFRG_E_ARG;
  HIP_TRY(hipSetDevice(c->device));
  uint32_t h[kInfoCount] = {0};
  uint64_t kt[4] = {0, 0, 0, 0};
  if (const int rc = finish_decode(c, h, kt)) return rc;
  const Result& r = c->res;
  uint64_t blen = 0;
  if (r.materialized && !h[kInfoOverflow]) {  // the byte column's length: offsets[nb]
    const uint64_t nb = r.req.n ? kt[TFRG_KIND_BYTES] : 0;
    HIP_TRY(hipMemcpy(&blen, c->boff64.as<uint64_t>() + nb, 8, hipMemcpyDeviceToHost));
  }
  memset(info, 0, sizeof(*info));
  info->n_records = r.req.n;
  info->n_slots = c->n_slots;
  info->n_errors = h[kInfoErrors];
  info->first_error = ~h[kInfoFirstError];  // (stored inverted by atomicMax; 0 = no error -> 0xffffffff)
  info->n_miss_records = h[kInfoMissRecords];
  info->n_miss_entries = h[kInfoMissEntries];
  info->n_big = h[kInfoBigRecs];
  info->scan_timeout = h[kInfoScanTimeout];
  for (int k = 0; k < 4; ++k) info->kind_totals[k] = kt[k];
  info->nbytes = r.req.nbytes;
  info->bytes_data_len = blen;
  info->tpl_groups_missed = h[kInfoResid];
  info->placed_slots = ((uint64_t)h[kInfoPlacedHi] << 32) | h[kInfoPlacedLo];
  info->implicit_cols = r.implicit;
  info->implicit_off_slots = r.off_mask;
  return overflow_status(h);
}

int tfrg_ctx_rel_off(const tfrg_ctx* c, uint32_t slot, int32_t* delta) {
  if (!c || !delta || slot >= 64u || !((c->off_rel >> slot) & 1ull) || slot >= c->rel_off.size()) return TFRG_E_ARG;
  *delta = c->rel_off[slot];
  return 0;
}

// The bytes slots of an optimistic decode with their first row in the bytes columns. Every slot is
// placed, so slot k's rows are n * (its rank among the bytes slots), as tpl_quiet_finish sets the
// column bases.
static std::vector<std::pair<uint32_t, uint64_t>> bytes_slot_rows(const tfrg_ctx* c) {
  std::vector<std::pair<uint32_t, uint64_t>> out;
  for (uint32_t k = 0; k < c->n_slots; ++k)
    if ((c->slot_kind_h[k] & 3u) == TFRG_KIND_BYTES) out.push_back({k, out.size() * (uint64_t)c->res.req.n});
  return out;
}

// (TFRG_IMPLICIT_BYTES_LEN) a bytes slot's constant element length, as the decode ran with it
static uint32_t implicit_len(const Result& r, uint32_t slot) { return slot < kLeanMaxSlots ? r.slot[slot].elem_len : 0u; }

// The constant columns of the last decode (tfrg_info.implicit_cols, and the aux words of an optimistic
// decode with stored statuses): rows [first, first + rows) of `col` hold `value` in elements of `width`
// bytes. tfrg_result_device writes them into the device columns, tfrg_result_fetch into the caller's.
enum Col { kColStatus, kColAux, kColVerdict, kColOrder, kColBytesLen, kNumCols };
struct Fill {
  Col col;
  uint64_t first, rows;
  uint32_t value, width;
};
static std::vector<Fill> constant_fills(const tfrg_ctx* c) {
  const Result& r = c->res;
  const uint64_t n = r.req.n;
  std::vector<Fill> out;
  if (r.implicit & TFRG_IMPLICIT_STATUS) {
    out.push_back({kColStatus, 0, n, 0u, 4});
    out.push_back({kColVerdict, 0, n, TFRG_V_LEN_MATCH | TFRG_V_LEN_CRC | TFRG_V_DATA_CRC, 1});
  }
  if ((r.implicit & TFRG_IMPLICIT_STATUS) || r.aux_zero) out.push_back({kColAux, 0, n, 0u, 8});
  if (r.implicit & TFRG_IMPLICIT_ORDER)
    for (uint32_t k = 0; k < c->n_slots && k < kLeanMaxSlots; ++k) out.push_back({kColOrder, k * n, n, r.slot[k].order_word, 2});
  if (r.implicit & TFRG_IMPLICIT_BYTES_LEN)
    for (const auto& [slot, base] : bytes_slot_rows(c)) out.push_back({kColBytesLen, base, n, implicit_len(r, slot), 4});
  return out;
}

// The implicit bytes_off words (tfrg_info.implicit_off_slots: element r of a masked slot is end32[r] +
// the slot's end-relative offset) written into the device column, once per decode, on the decode's
// stream, from the decode's u32 ends (the caller keeps them in place while the result is read:
// tfrg.h). The one place that formula is evaluated outside the consumers' kernels: tfrg_result_device
// hands out the column, tfrg_result_fetch copies it. Only after the decode is confirmed.
static int fill_implicit_off(tfrg_ctx* c) {
  Result& r = c->res;
  if (!r.off_mask || r.off_complete || !r.req.n) return 0;
  HIP_TRY(hipSetDevice(c->device));
  for (const auto& [slot, base] : bytes_slot_rows(c)) {
    if (slot >= kLeanMaxSlots || !((r.off_mask >> slot) & 1ull)) continue;
    if (base >= r.cap_b) continue;  // (an overflowed result is an error: tfrg_result_info)
    const uint32_t rows = (uint32_t)std::min<uint64_t>(r.req.n, r.cap_b - base);
    HIP_TRY(launch_fill_rel_off(c->b_off.as<uint32_t>() + base, r.req.off.e32, (uint32_t)r.slot[slot].rel_off, rows,
                                c->last_stream));
  }
  r.off_complete = true;
  return 0;
}

int tfrg_result_device(tfrg_ctx* c, tfrg_columns* d) {
  if (!c || !c->res.valid) return TFRG_E_ARG;
  if (const int rc = confirm_pending(c)) return rc;  // (before the view, as tfrg_result_info does)
  Result& r = c->res;
  if (!r.rs_complete && c->n_slots && r.req.n) {
    // a self-consistent view: the identity rows of the finally placed slots, which the decode does
    // not store, are written by one small kernel on the decode's stream (placed mask read on the
    // device), once per decode
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(launch_fill_placed_rows(c->rs.as<uint32_t>(), c->info.as<uint32_t>() + c->info_slot * kInfoCount,
                                    c->n_slots, r.req.n, c->last_stream));
  }
  r.rs_complete = true;
  if (!r.cols_complete) {  // the constant columns of an optimistic decode, once per decode
    DBuf* const col[kNumCols] = {&c->status, &c->aux, &c->verdict, &c->order, &c->b_len};
    const std::vector<Fill> fills = constant_fills(c);
    if (!fills.empty()) HIP_TRY(hipSetDevice(c->device));
    for (const Fill& f : fills) {
      const hipDeviceptr_t p = col[f.col]->as<uint8_t>() + f.first * f.width;
      if (f.width == 2) {
        HIP_TRY(hipMemsetD16Async(p, (unsigned short)f.value, f.rows, c->last_stream));
      } else if (f.width == 4) {
        HIP_TRY(hipMemsetD32Async(p, (int)f.value, f.rows, c->last_stream));
      } else {  // (bytes, or the 8-byte aux words, which are 0)
        HIP_TRY(hipMemsetAsync(p, (int)f.value, f.rows * f.width, c->last_stream));
      }
    }
  }
  r.cols_complete = true;
  if (const int rc = fill_implicit_off(c)) return rc;
  d->status = c->status.as<int32_t>();
  d->aux = c->aux.as<int64_t>();
  d->verdict = c->verdict.as<uint8_t>();
  d->order = c->order.as<uint16_t>();
  d->row_splits = c->rs.as<uint32_t>();
  d->slot_base = c->slot_base.as<uint64_t>();
  d->i64 = c->i64.as<int64_t>();
  d->f32 = c->f32.as<uint32_t>();
  d->bytes_off = c->b_off.as<uint32_t>();
  d->bytes_len = c->b_len.as<uint32_t>();
  d->miss = c->miss.as<uint32_t>();
  d->bytes_data = r.materialized ? c->bdata.as<uint8_t>() : nullptr;
  d->bytes_offsets = r.materialized ? c->boff64.as<uint64_t>() : nullptr;
  return 0;
}

// ---- Host-side setup shared by the entry points over the last result (tfrg_result_dense / _dense_rows,
// _ragged_rows, _select_rows). `bad` is the entry point's own: it prefixes the function's name.
extern "C++" {
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
// The column view of the last result: what DenseArgs, RaggedArgs and SelectArgs have in common
template <class Args>
static void fill_columns(const tfrg_ctx* c, Args& a) {
  a.rs = c->rs.as<uint32_t>();
  a.slot_base = c->slot_base.as<uint64_t>();
  a.i64 = view_col<int64_t>(c, c->i64);
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
}  // extern "C++"

// A bytes slot's end-relative element offset where the last decode did not store its bytes_off words
// (tfrg_info.implicit_off_slots: the element of record g is end32[g] + that); else the kernels' "the
// column is stored" sentinel.
static_assert(kDenseOffStored == kRaggedOffStored, "one const_off lookup serves both");
static int32_t const_off_of(const tfrg_ctx* c, uint32_t slot, bool reads_off) {
  if (!reads_off || slot >= kLeanMaxSlots || !((c->res.off_mask >> slot) & 1ull)) return kDenseOffStored;
  return c->res.slot[slot].rel_off;
}

// A bytes slot's constant element length where the last decode did not store the bytes_len column (as
// constant_fills: the shapes' length holds); else, or for a spec / term that reads no length, the
// kernels' "the column is stored" sentinel.
static_assert(kDenseNoLen == kRaggedNoLen && kRaggedNoLen == kSelNoLen, "one const_len lookup serves all three");
static_assert(kElemsNoLen == kDenseNoLen && kElemsOffStored == kDenseOffStored, "and tfrg_elems.h's kernels");
static uint32_t const_len_of(const tfrg_ctx* c, uint32_t slot, bool reads_len) {
  if (!reads_len || !(c->res.implicit & TFRG_IMPLICIT_BYTES_LEN)) return kDenseNoLen;
  return implicit_len(c->res, slot);
}

// The consumer-stream fence: the work an entry point puts on the decode's stream *st starts after what
// the consumer stream *cs holds so far (fence_open), and the consumer waits for it (fence_close). A
// NULL consumer_stream is the decode's own stream: no fence.
static int fence_open(tfrg_ctx* c, void* consumer_stream, hipStream_t* st, hipStream_t* cs) {
  *st = c->last_stream;
  *cs = consumer_stream ? static_cast<hipStream_t>(consumer_stream) : *st;
  if (*cs == *st) return 0;
  for (hipEvent_t& e : c->consumer_ev)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->consumer_ev[0], *cs));
  HIP_TRY(hipStreamWaitEvent(*st, c->consumer_ev[0], 0));
  return 0;
}
static int fence_close(tfrg_ctx* c, hipStream_t st, hipStream_t cs) {
  if (cs == st) return 0;
  HIP_TRY(hipEventRecord(c->consumer_ev[1], st));
  HIP_TRY(hipStreamWaitEvent(cs, c->consumer_ev[1], 0));
  return 0;
}

// The row list of tfrg_result_dense_rows (d_rows null: tfrg_result_dense, every record in order)
struct DenseRows {
  const void* d_rows = nullptr;
  uint32_t dtype = 0, m = 0;
  int64_t row0 = 0;
  uint32_t* d_skipped = nullptr;
};

static int result_dense(const char* fn, bool by_rows, tfrg_ctx* c, const tfrg_dense_spec* specs, uint32_t n_specs,
                        const DenseRows& rows, uint32_t* d_stats, void* consumer_stream) {
  auto bad = [fn](const std::string& why) {
    set_error(std::string(fn) + ": " + why);
    return TFRG_E_ARG;
  };
  if (const int rc = check_specs(c, specs, n_specs, TFRG_DENSE_MAX_SPECS, bad)) return rc;
  static_assert(TFRG_DENSE_MAX_SPECS == kDenseMaxSpecs && TFRG_DENSE_MAX_WIDTH == kDenseMaxWidth &&
                    TFRG_DENSE_I64 == kDenseI64 && TFRG_DENSE_I32 == kDenseI32 && TFRG_DENSE_F32 == kDenseF32 &&
                    TFRG_DENSE_U8 == kDenseU8,
                "tfrg.h mirrors tfrg_dense.h");
  for (uint32_t i = 0; i < n_specs; ++i) {
    const tfrg_dense_spec& s = specs[i];
    const std::string at = "spec " + std::to_string(i) + ": ";
    if (const int rc = check_slot_dtype(c, at, s.slot, s.dtype, bad)) return rc;
    if (s.width == 0 || s.width > TFRG_DENSE_MAX_WIDTH)
      return bad(at + "width must be 1.." + std::to_string(TFRG_DENSE_MAX_WIDTH));
    if (!s.out) return bad(at + "out is NULL");
    if (s.reserved) return bad(at + "reserved must be 0");
  }
  if (by_rows) {
    if (const int rc = check_rows_dtype(rows.d_rows, rows.dtype, true, bad)) return rc;
    if (const int rc = check_rows_m(rows.d_rows, rows.m, true, bad)) return rc;
  }
  if (!by_rows && c->res.req.n == 0) return 0;
  HIP_TRY(hipSetDevice(c->device));
  if (const int rc = confirm_pending(c)) return rc;
  // the rows of every output
  const uint32_t out_rows = by_rows ? rows.m : c->res.req.n;
  DenseArgs a{};
  if (by_rows) {
    a.rows = rows.d_rows;
    a.rows64 = rows.dtype == TFRG_ROWS_I64;
    a.m = rows.m;
    a.row0 = rows.row0;
    a.skipped = rows.d_skipped;
  }
  fill_columns(c, a);
  fill_bytes_source(c, a);
  a.stats = d_stats;
  a.n_specs = n_specs;
  a.nt = (uint32_t)c->sw.dense_nt;
  // workgroups per spec: one per chunk of its output, within an even share of 16 per CU
  const uint64_t cap = std::max<uint64_t>(1, (uint64_t)c->num_cus * 16u / n_specs);
  uint32_t blocks = 0;
  for (uint32_t i = 0; i < n_specs; ++i) {
    const tfrg_dense_spec& s = specs[i];
    DenseSpec& d = a.sp[i];
    d.out = s.out;
    d.lengths = s.lengths;
    d.fill = s.fill;
    d.slot = s.slot;
    d.dtype = s.dtype;
    d.width = s.width;
    d.const_len = const_len_of(c, s.slot, s.dtype == TFRG_DENSE_U8);
    d.const_off = const_off_of(c, s.slot, s.dtype == TFRG_DENSE_U8);
    const uint64_t isz = s.dtype == TFRG_DENSE_I64 ? 8 : s.dtype == TFRG_DENSE_U8 ? 1 : 4;
    const uint64_t total = (uint64_t)out_rows * s.width * isz;
    // 16-byte units, or single elements where the output's base is not 16-byte aligned
    const uint64_t work = ((uintptr_t)s.out & 15u) ? total / isz : (total >> 4) + 16;
    d.blk0 = blocks;
    d.nblk = (uint32_t)std::min<uint64_t>(cap, (work + kDenseChunk - 1) / kDenseChunk);
    blocks += d.nblk;
  }
  hipStream_t st, cs;
  if (const int rc = fence_open(c, consumer_stream, &st, &cs)) return rc;
  // (counters that lie back to back, stats first, are zeroed by one memset: one launch less per step)
  const bool one_memset = by_rows && c->res.req.n && d_stats && rows.d_skipped == d_stats + 4 * (size_t)n_specs;
  if (d_stats) HIP_TRY(hipMemsetAsync(d_stats, 0, (size_t)n_specs * (one_memset ? 20 : 16), st));
  // (a row list over an empty result: no record to read, every row is skipped)
  if (by_rows && rows.d_skipped && !one_memset)
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rows.d_skipped), c->res.req.n ? 0 : (int)rows.m, n_specs, st));
  if (out_rows && c->res.req.n) HIP_TRY(launch_dense(a, blocks, st));
  return fence_close(c, st, cs);
}

int tfrg_result_dense(tfrg_ctx* c, const tfrg_dense_spec* specs, uint32_t n_specs, uint32_t* d_stats,
                      void* consumer_stream) {
  return result_dense("tfrg_result_dense", false, c, specs, n_specs, DenseRows{}, d_stats, consumer_stream);
}

int tfrg_result_dense_rows(tfrg_ctx* c, const tfrg_dense_spec* specs, uint32_t n_specs, const void* d_rows,
                           uint32_t rows_dtype, uint32_t m, int64_t row0, uint32_t* d_stats, uint32_t* d_skipped,
                           void* consumer_stream) {
  DenseRows rows;
  rows.d_rows = d_rows;
  rows.dtype = rows_dtype;
  rows.m = m;
  rows.row0 = row0;
  rows.d_skipped = d_skipped;
  return result_dense("tfrg_result_dense_rows", true, c, specs, n_specs, rows, d_stats, consumer_stream);
}

// ---- The frame of the entry points that pack per-spec outputs for a list of rows (tfrg_result_ragged_rows,
// _ragged_elems, _elem_ids): the checks in the one order all three make them, the tiles and the split,
// the scratch, the consumer fence and the counters, around what an entry point brings as its own.
struct RowListCall {  // the arguments the three have in common
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
extern "C++" {
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
// (the spec's slot exists and is a bytes_list slot)
template <class Bad>
static int check_bytes_slot(const tfrg_ctx* c, const std::string& at, uint32_t slot, const Bad& bad) {
  if (slot >= c->n_slots) return bad(at + "slot " + std::to_string(slot) + " >= n_slots");
  const uint32_t kind = c->slot_kind_h[slot] & 3u;
  if (kind != TFRG_KIND_BYTES)
    return bad(at + "slot " + std::to_string(slot) + " is not a bytes_list slot (kind " + std::to_string(kind) + ")");
  return 0;
}
}  // extern "C++"

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
          if (const tfrg_vocab* v = s.vocab) {
            d.table = v->d_table;
            d.w_offs = v->d_offs;
            d.blob = v->d_blob;
            d.w_ids = v->d_ids;
            d.mask = (uint32_t)v->table.size() - 1u;
            d.max_probe = v->max_probe;
            d.max_word = v->max_word;
            d.blob_bound = v->d_blob_bound;
          }
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

int tfrg_result_fetch(tfrg_ctx* c, const tfrg_columns* h) {
  tfrg_info info;
  int rc = tfrg_result_info(c, &info);
  if (rc) return rc;
  const hipStream_t st = c->last_stream;
  const Result& r = c->res;
  const size_t n = r.req.n, S = c->n_slots;
  auto cp = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    if (!dst || !bytes) return hipSuccess;
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  };
  // (clamped to the capacities: a result that overflowed them fails in tfrg_result_info above)
  auto cl = [](uint64_t v, uint64_t cap) { return v < cap ? v : cap; };
  const uint64_t nb = cl(info.kind_totals[TFRG_KIND_BYTES], r.cap_b);
  // an optimistic decode's constant columns are written here, the others copied
  void* const col[kNumCols] = {h->status, h->aux, h->verdict, h->order, h->bytes_len};
  const void* const dcol[kNumCols] = {c->status.p, c->aux.p, c->verdict.p, c->order.p, c->b_len.p};
  size_t col_bytes[kNumCols] = {n * 4, n * 8, n, S * n * 2, nb * 4};
  for (const Fill& f : constant_fills(c)) {
    col_bytes[f.col] = 0;
    if (!col[f.col]) continue;
    uint8_t* const p = static_cast<uint8_t*>(col[f.col]) + f.first * f.width;
    if (f.width == 2) {
      std::fill_n(reinterpret_cast<uint16_t*>(p), f.rows, (uint16_t)f.value);
    } else if (f.width == 4) {
      std::fill_n(reinterpret_cast<uint32_t*>(p), f.rows, f.value);
    } else {  // (bytes, or the 8-byte aux words, which are 0)
      memset(p, (int)f.value, f.rows * f.width);
    }
  }
  for (int k = 0; k < kNumCols; ++k) HIP_TRY(cp(col[k], dcol[k], col_bytes[k]));
  // row splits: a placed slot's are the identity, never stored by the decode; they copy from a
  // device identity row (filled once per size), as fast as the stored rows and as asynchronous
  if (h->row_splits) {
    if (S && (info.placed_slots & (S >= 64 ? ~0ull : (1ull << S) - 1ull)) && c->ident_n < n + 1) {
      const size_t m = std::max<size_t>(n + 1, 2 * c->ident_n);
      std::vector<uint32_t> v(m);
      std::iota(v.begin(), v.end(), 0u);
      c->ident_n = 0;
      HIP_TRY(c->ident.ensure(m * 4));
      HIP_TRY(hipMemcpy(c->ident.p, v.data(), m * 4, hipMemcpyHostToDevice));
      c->ident_n = m;
    }
    for (size_t k = 0; k < S; ++k) {
      const bool pk = k < 64 && ((info.placed_slots >> k) & 1ull);
      HIP_TRY(cp(h->row_splits + k * (n + 1), pk ? c->ident.as<uint32_t>() : c->rs.as<uint32_t>() + k * (n + 1),
                 (n + 1) * 4));
    }
  }
  HIP_TRY(cp(h->slot_base, c->slot_base.p, S * 8));
  HIP_TRY(cp(h->i64, c->i64.p, cl(info.kind_totals[TFRG_KIND_INT64], r.cap_i64) * 8));
  HIP_TRY(cp(h->f32, c->f32.p, cl(info.kind_totals[TFRG_KIND_FLOAT], r.cap_f32) * 4));
  // (implicit offset words: written into the device column first, by the device view's fill)
  if (h->bytes_off)
    if (const int rc2 = fill_implicit_off(c)) return rc2;
  HIP_TRY(cp(h->bytes_off, c->b_off.p, nb * 4));
  if (r.materialized) {
    HIP_TRY(cp(h->bytes_data, c->bdata.p, info.bytes_data_len));
    HIP_TRY(cp(h->bytes_offsets, c->boff64.p, (info.kind_totals[TFRG_KIND_BYTES] + 1) * 8));
  }
  const size_t nm = info.n_miss_entries < kMissCap ? info.n_miss_entries : kMissCap;
  HIP_TRY(cp(h->miss, c->miss.p, nm * 16));
  HIP_TRY(hipStreamSynchronize(st));
  return 0;
}

}  // extern "C"

int tfrg_stream_read(const void* d_bytes, uint64_t nbytes, uint32_t* d_sink, void* stream, int variant) {
  if (!d_bytes || !d_sink || (nbytes & 15u)) return TFRG_E_ARG;
  return tfrg::launch_stream_read(d_bytes, nbytes, d_sink, static_cast<hipStream_t>(stream), variant) == hipSuccess
             ? 0 : TFRG_E_HIP;
}

int tfrg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
