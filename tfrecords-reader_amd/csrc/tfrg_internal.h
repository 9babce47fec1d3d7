// tfrg_internal.h — device-side views shared by the kernel files, their launch policy
// (tfrg_decode.cpp) and the C-ABI orchestration (tfrg_capi.cpp). Not part of the public ABI (include/tfrg.h is).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "tfrg_layout.h"

namespace tfrg {

// Device key table (the "schema"): distinct key byte strings, each with up to one slot per kind.
// A slot is one (key, kind) column of the columnar result.
struct DevSchema {
  uint32_t n_keys;
  uint32_t n_slots;
  uint32_t ht_mask;            // open-addressing table size - 1
  const uint32_t* ht;          // [ht_mask+1] key_id + 1, 0 = empty
  const uint32_t* key_hash;    // [n_keys] FNV-1a of the key bytes
  const uint32_t* key_off;     // [n_keys+1] into key_blob
  const uint8_t* key_blob;
  const int32_t* key_slot;     // [n_keys*4]: [0] flags (bit0 invalid UTF-8), [1..3] slot per kind or -1
  const uint8_t* slot_kind;    // [n_slots]
  const uint32_t* key_w;       // [n_keys][2]: first / last 4 key bytes (see key_hash_words)
  const uint32_t* krec;        // [n_keys][8] packed key record, see KeyRec
  const uint32_t* tpl;         // [n_tpl][kLtWords] record-shape templates in window form (below)
  const uint32_t* tpl_img;     // their lane image (kLiHdr ...), tpl_img_words words
  uint32_t tpl_img_words;
  uint32_t tpl_tab_words;      // the packed CRC position tables behind the image (kLiPtabWords each table word)
  uint32_t n_tpl;
  uint32_t tpl_w;              // their window words W (16, 32 or 64)
  // [n_slots] speculative placement of single values (null = off): 0, or (rank + 1) << 2 | kind for
  // a slot that is an inline single value in every learned template, as are all slots of its kind
  // before it. The lane kernel then writes such a value straight to its column at n * rank + r (the
  // row split r stays implicit for the first 64 slots); k_down_gather skips the slot when every
  // record was regular (irr == 0) and the slot's column base is n * rank, i.e. when that placement
  // is the final one (tfrg_info.placed_slots), and writes all its row splits otherwise.
  const uint32_t* spec;
};

// (Record-shape templates and their lane image: tfrg_layout.h.)
constexpr uint32_t kCrcTabWords = 51200;  // crc_tab words (tfrg_ctx_create)

// Column targets of one slot for k_tpl_lane, computed on the host per decode.
struct LeanTgt {
  uint16_t* ord;   // order column of the slot
  uint32_t* cnt;   // count column
  uint2* loc;      // loc column
  uint32_t* rs;    // row-split column (speculative placement)
  void* v1;        // speculative placement: value column at n * (rank - 1) (int64 / float bits / bytes offset)
  uint32_t* v2;    // speculative placement of bytes: the length column at n * (rank - 1)
  uint32_t lim;    // speculative placement: records r < lim are stored (capacity)
  uint32_t kind;   // speculative placement kind (0: the slot is not placed speculatively)
  uint32_t no_off; // bytes slot whose offset words this decode leaves implicit (LaunchCfg::implicit_off):
                   // v1 is not stored
  uint32_t pad;
};
struct LeanArgs {
  uint32_t n_tpl;
  uint32_t lane_max;
  uint32_t* tsum;  // tile sums, slot k's at k * tile_stride (nullptr: an optimistic decode, none stored)
  uint32_t n_slots;
  uint32_t tile_stride;
  uint32_t img_words;  // the templates' lane image (DevSchema::tpl_img), copied into LDS
  uint32_t gpw;    // (launch_tpl_lane) 64-record groups per wave: 1 or 2 (part of a tile: small batches,
                   // twice the waves, tile sums added atomically) or a multiple of 4 (whole tiles)
  uint32_t bsplit; // workgroups from this one on take 2 groups per wave, from group gsplit on (the
  uint32_t gsplit; // batch's tail in small pieces: the last workgroups dispatched finish together)
  const uint8_t* finish;  // optimistic decode: DevSchema::slot_kind, and the last workgroup finishes
                          // the decode (tpl_quiet_finish); nullptr: the passes after this kernel do
  uint32_t implicit;      // optimistic decode, TFRG_IMPLICIT_* columns not stored for template hits
                          // (constant: every record of a confirmed decode is one)
  uint32_t tab_words;     // the packed CRC tables behind the image (DevSchema::tpl_tab_words), copied into LDS
  uint32_t cu_lds;        // (host) LDS bytes of a CU: launch_tpl_lane takes the staged-window kernel on
                          // large batches when three workgroups with their stages fit; 0: never
                          // (TFRG_TPL_STAGE=0)
  uint32_t stage_any;     // (host) staged windows on batches of any size (TFRG_TPL_STAGE=2: tests)
  uint32_t gpw_force;     // (host) TFRG_TPL_GPW = 2, 4 or 8: launch_tpl_lane's groups per wave on batches of
                          // any size, without the tail split (tests, measurements); 0: by batch size
  uint32_t nocrc;         // TFRG_FLAG_NO_CRC decode: no CRC arithmetic, no tables in LDS (tab_words 0); a hit
                          // is the mask match of a template of either frame class, verdict TFRG_V_LEN_MATCH
  uint32_t strict;        // TFRG_FLAG_STRICT_CRC decode: unchecked-frame templates take nothing
  uint32_t uframes;       // (host) some template has an unchecked frame: with nocrc, selects the kernel
                          // that knows frame classes
  LeanTgt tg[kLeanMaxSlots];
};

// Packed per-key record (8 x u32) staged into LDS by the lane kernels' fast path.
enum KeyRec : uint32_t { kKrHash = 0, kKrLen, kKrW0, kKrW1, kKrSlot1, kKrSlot2, kKrSlot3, kKrFlags, kKrWords };
constexpr uint32_t kLdsMaxKeys = 256;     // key tables up to this size are staged into LDS
constexpr uint32_t kLdsMaxHt = 1024;      // hash-table entries staged into LDS
inline bool schema_in_lds(const DevSchema& sc) { return sc.n_keys <= kLdsMaxKeys && sc.ht_mask + 1 <= kLdsMaxHt; }

// Key hash over (length, first 4 bytes, last 4 bytes), all little-endian and zero padded:
// w0 = bytes [0, min(n,4)), w1 = n > 4 ? bytes [n-4, n) : 0. For n <= 8 the triple (n, w0, w1)
// IS the key, so a table hit needs no byte compare. Every input bit is folded into 24-bit
// operands so that the device multiplies are full-rate v_mul_u32_u24 (v_mul_lo_u32 is quarter
// rate, and the lane kernel is VALU-bound).
__host__ __device__ inline uint32_t key_hash_words(uint32_t n, uint32_t w0, uint32_t w1) {
  const uint32_t a = (w0 ^ (w0 >> 11) ^ (n << 17)) & 0xffffffu;
  const uint32_t b = (w1 ^ (w1 >> 13) ^ (n << 7)) & 0xffffffu;
#if defined(__HIP_DEVICE_COMPILE__)
  // = the host's products mod 2^32 (both operands < 2^24); spelled out because the backend picks
  // the quarter-rate v_mul_lo_u32 for these once the masks are reassociated
  uint32_t p0, p1;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(p0) : "v"(a), "v"(0x9E3779u));
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(p1) : "v"(b), "v"(0x85EBCBu));
  uint32_t h = p0 ^ p1;
#else
  uint32_t h = a * 0x9E3779u;
  h ^= b * 0x85EBCBu;
#endif
  return h ^ (h >> 15);
}

// Record offsets of a batch (tfrg_decode_device: u64 pairs; tfrg_decode_device32: u32 pairs, or u32
// ends alone for back-to-back records, record r > 0 starting where record r - 1 ends)
enum OffMode : uint32_t { kOffU64 = 0, kOffU32 = 1, kOffEnds = 2 };

struct DevBatch {
  const uint8_t* bytes;        // records (framed or bare payloads); readable to round_up(nbytes,16)
  uint64_t nbytes;
  const uint64_t* start;       // [n] absolute offsets into bytes (kOffU64)
  const uint64_t* end;         // [n]
  const uint32_t* start32;     // [n] (kOffU32)
  const uint32_t* end32;       // [n] (kOffU32, kOffEnds)
  uint32_t first;              // kOffEnds: start of record 0
  uint32_t omode;              // OffMode
  uint32_t n;
  uint32_t flags;
};

#if defined(__HIPCC__)
__device__ __forceinline__ uint64_t rec_end(const DevBatch& B, uint32_t r) {
  return B.omode == kOffU64 ? B.end[r] : (uint64_t)B.end32[r];
}
__device__ __forceinline__ uint64_t rec_start(const DevBatch& B, uint32_t r) {
  if (B.omode == kOffU64) return B.start[r];
  if (B.omode == kOffU32) return B.start32[r];
  return r ? (uint64_t)B.end32[r - 1] : (uint64_t)B.first;
}
#endif

// Info counters (device, zero at the start of every decode: the previous decode's k_lane_count
// zeroes the slot the next one uses, DevOut::info_next)
enum InfoIdx : uint32_t {
  kInfoErrors = 0,       // records with a decode error (reference exception / UB status)
  kInfoFirstError = 1,   // ~(lowest record index with an error): atomicMax of ~r, init 0
  kInfoMissRecords = 2,  // records with a schema miss
  kInfoMissEntries = 3,  // miss entries appended (may exceed capacity)
  kInfoBig = 4,          // records routed to the wave-per-record kernels
  kInfoScanTimeout = 5,  // reserved (always 0: the scan has no inter-workgroup waits)
  kInfoHuge = 6,         // wave records too large for the LDS stage (listed from the end of big_list)
  kInfoSlow = 7,         // lane records left to the exact (slow) walker
  kInfoSpineDone = 8,    // spine workgroups finished (the last one computes the column bases)
  kInfoNeed = 9,         // lane records with an out-of-line list (k_tail_gather; listed in slow_list)
  kInfoSpineTicket = 10, // k_spine workgroup tickets (chunk order of the look-back)
  kInfoOverflow = 11,    // a kind's value total exceeds its column capacity (overlapping ranges)
  kInfoBytesTicket = 12, // k_bytes_scan tile tickets
  kInfoBytesBig = 13,    // k_bytes_scan: long elements listed for the wave copy
  kInfoCrcCtr = 14,      // [14..15] u64: streaming-CRC list entries << kCrcIdxShift | flat 1 KiB rounds
  kInfoDefer = 16,       // k_lane_count: 64-record rows of deferred packed-int64 bodies reserved (k_body_count)
  kInfoResid = 17,       // k_tpl_lane: 64-record groups listed for k_lane_count (records no template took)
  kInfoPlacedLo = 18,    // [18..19] k_down_gather: the (first 64) slots whose speculative placement is final
  kInfoPlacedHi = 19,
  kInfoTplDone = 20,     // [20..21] u64, optimistic decodes: k_tpl_lane workgroups finished | groups
                         // they listed << 32 (one atomic: the last workgroup knows the total)
  kInfoBigRecs = 22,     // records above lane_max (tfrg_info.n_big; kInfoBig + kInfoHuge count the
                         // ones listed for the wave gathers: those with out-of-line lists)
  kInfoWalkMiss = 23,    // records above lane_max walked beside the CRC (k_tail_count) that the
                         // canonical walker did not take or that have an out-of-line list: re-run
  kInfoCount = 24        // (even: the two slots' u64 words stay 8-byte aligned)
};
static_assert(kInfoCount % 2 == 0 && kInfoCrcCtr % 2 == 0 && kInfoTplDone % 2 == 0,
              "u64 info words stay 8-byte aligned in both slots");

// Deferred packed int64 bodies of records walked from HBM (k_lane_count -> k_body_count): a wave
// reserves one block of 64 rows, row = one record, kDeferK entries (record, slot, absolute body
// offset, length) and a count byte per row
constexpr uint32_t kDeferK = 32;
// status of a record whose deferred body did not count canonically (k_body_count): k_tail_count's
// exact walker withdraws its columns and re-walks it (never left in the status column)
constexpr int32_t kStatusRedo = 0x7fff0001;

// verdict byte of a record the lane kernel left to the exact walker (k_tail_count role 1 writes its
// final verdict, payload CRC included); role 2 (payload CRCs of large records) never lists such
// records (a record k_body_count sends back is on both lists: role 2 ORs its bit in atomically)
constexpr uint32_t kVerdictPending = 0x80u;

// streaming payload CRC of the large records (k_tail_count role 2)
constexpr int kCrcIdxShift = 40;
constexpr uint64_t kCrcRoundMask = (1ull << kCrcIdxShift) - 1ull;
constexpr uint32_t kCrcListMin = 64;  // shorter payloads of large records: the lane kernel's serial CRC

struct DevOut {
  int32_t* status;       // [n]
  int64_t* aux;          // [n] error detail
  uint8_t* verdict;      // [n] tfrg_verdict bits
  uint16_t* order;       // [n_slots][n]  0 = absent, else 1 + rank in the record's key order
  uint32_t* count;       // [n_slots][n]
  uint2* loc;            // [n_slots][n]  (payload-relative offset, length) of the list message
  uint32_t* rs;          // [n_slots][n+1] row splits (exclusive prefix of count)
  uint64_t* slot_base;   // [n_slots] element base of each slot inside its kind's value array
  uint32_t* totals;      // [n_slots]
  uint64_t* kind_totals; // [4]
  int64_t* i64;          // int64 values
  uint32_t* f32;         // float values (raw bits)
  uint32_t* b_off;       // bytes_list element views: absolute offset into bytes
  uint32_t* b_len;
  uint64_t cap_i64, cap_f32, cap_b;
  uint32_t* big_list;    // records for the wave-per-record kernels
  uint32_t* miss;        // [miss_cap][4] (record, kind, key abs offset, key length)
  uint32_t miss_cap;
  uint32_t* info;        // [kInfoCount]
  uint32_t* info_next;   // [kInfoCount] the next decode's info words (k_lane_count workgroup 0 zeroes them)
  uint32_t* tsum;        // [n_slots][tile_stride] per-tile value counts, then their exclusive prefixes
  uint32_t tile_stride;  // >= n_tiles, multiple of 4
  uint64_t* spine_lb;    // [n_slots][n_chunks] k_spine look-back words: flag << 32 | chunk total / inclusive
                         // prefix (flag 1 / 2; zeroed per decode with tsum)
  uint32_t n_chunks;     // ceil(n_tiles / 2^kSpineChunkShift)
  uint32_t* slow_list;   // [n] lane records for the exact walker; reused by k_down_gather for the
                         // records k_tail_gather decodes (the slow list is consumed by then)
  uint32_t* crc_rec;     // [n] streaming-CRC list: record
  uint64_t* crc_base;    // [n] its first flat round (ascending with the list index)
  uint64_t* crc_part;    // [n] rounds done << 32 | XOR of the slices, of a record split over waves
  uint32_t* irr;         // [n_slots] records not placed speculatively per slot (DevSchema::spec; after
                         // the scan words in their buffer, zero between decodes: k_tail_gather clears)
  uint4* dq;             // [dq_blocks][64][kDeferK] deferred bodies (nullptr: no deferral this decode)
  uint8_t* dq_cnt;       // [dq_blocks][64] entries used per row (0 for records not accepted)
  uint32_t dq_blocks;
  uint64_t* lmask;       // [groups] k_tpl_lane: per 64-record group, the records it did not take (null: not run)
  uint32_t* rlist;       // [groups] k_tpl_lane: the groups with such records (null: k_lane_count takes all)
};

// Row-split scan tiles: 256 consecutive records (one lane-kernel workgroup iteration)
constexpr uint32_t kTileShift = 8;
constexpr uint32_t kTileRecs = 1u << kTileShift;
// k_spine chunks: 2^12 tiles (1 M records) per workgroup
constexpr uint32_t kSpineChunkShift = 12;

// flags (mirrors include/tfrg.h)
constexpr uint32_t kFlagPayloadOnly = 1u;
constexpr uint32_t kFlagSpecVarint = 2u;
constexpr uint32_t kFlagNoCrc = 4u;
constexpr uint32_t kFlagStrictCrc = 8u;
constexpr uint32_t kFlagMaterializeBytes = 16u;


// TFRG_FLAG_MATERIALIZE_BYTES (tfrg_bytes.hip): bytes_list elements gathered into one column
struct DevBytes {
  const uint8_t* in;             // batch bytes
  uint64_t in_readable;          // round_up(nbytes, 16)
  const uint32_t* b_off;         // element views (absolute offset, length)
  const uint32_t* b_len;
  const uint64_t* kind_totals;   // [1] = element count (k_spine)
  uint64_t* offsets;             // [nb + 1] exclusive prefix of the lengths
  uint64_t offsets_cap;          // elements the offsets buffer holds (cap_b)
  uint8_t* data;                 // the byte column
  uint64_t data_cap;
  uint64_t* lb;                  // look-back words (zeroed per decode)
  uint32_t* ticket;              // scan tile tickets (zeroed per decode)
  uint32_t* big_count;           // elements longer than the short-copy bound (zeroed per decode)
  uint32_t* big_list;            // [cap_b]
  uint32_t* overflow;            // info[kInfoOverflow]
};
hipError_t launch_materialize(const DevBytes& d, int num_cus, hipStream_t st);
uint64_t materialize_lb_words(uint64_t cap_b);

// the launch policy's configuration (launch_decode, tfrg_decode.cpp)
struct LaunchCfg {
  int num_cus;
  bool lean;               // k_tpl_lane first (window-form templates, framed records)
  bool tpl_full;           // the templates took their whole learning sample (the later passes are
                           // then usually empty: launched with small grids)
  bool tpl_unchecked;      // some kept template has an unchecked frame (kLtFrame 1): hit verdicts vary
  const uint32_t* spec_h;  // host copy of DevSchema::spec (k_tpl_lane's placement targets)
  int lane_grid;           // cap: workgroups for one record per lane
  int wave_grid;
  uint32_t lane_max;       // records above this size go to the wave kernels
  uint32_t wave_stage;     // wave records spanning <= this many bytes are staged in LDS (<= kWStage)
  bool body_count;         // deferred packed bodies possible (DevOut::dq): launch k_body_count
  uint32_t poison[4];      // debug hook (env TFRG_DEBUG_POISON_LOC): records whose list locations are
                           // overwritten after the count passes (0xffffffff: none)
  bool optimistic;         // allow an optimistic decode (launch_decode: k_tpl_lane alone)
  bool ran_optimistic;     // (out) this decode was launched optimistically: it is complete only once
                           // the host has read kInfoResid as 0 (else it is re-run in full)
  bool ord_const;          // every learned shape has every slot at the same key position
  bool len_const;          // every bytes slot one element of one length in every learned shape
  bool ran_quiet_big;      // (out) optimistic without shapes: k_tail_count's last workgroup ends it
  uint32_t tpl_cu_lds;     // LeanArgs::cu_lds
  bool tpl_stage_any;      // LeanArgs::stage_any
  uint32_t tpl_gpw;        // LeanArgs::gpw_force
  bool walk_beside;        // optimistic without shapes: records above lane_max walked beside the CRC
                           // (k_tail_count's first workgroups) instead of before it (k_lane_count)
  uint32_t walk_blocks;    // cap on those workgroups (0: automatic)
  uint32_t implicit;       // (out) TFRG_IMPLICIT_* columns the decode did not store
  uint64_t off_rel;        // bytes slots at one end-relative offset in every learned shape (Learned::off_rel;
                           // 0: TFRG_IMPLICIT_OFF=0, or a decode whose byte gather reads the column)
  uint64_t implicit_off;   // (out) the slots of off_rel whose bytes_off words the decode did not store: a
                           // lean optimistic decode with u32 offsets (element r is end32[r] + rel_off)
};

// Kernel stages, in launch order (profiling events bracket each one).
enum Stage : int { kStageTplLane = 0, kStageLaneCount, kStageBodyCount, kStageTailCount, kStageSpine,
                   kStageDownGather, kStageTailGather, kStageMaterialize, kNumStages };
extern const char* const kStageNames[kNumStages];

hipError_t launch_tpl_lane(const DevBatch& b, const DevOut& o, const LeanArgs& a, const uint32_t* img, uint32_t w,
                           int num_cus, hipStream_t st);
// The stage launchers (tfrg_kernels.hip; spine, down_gather, poison_loc, fill_placed_rows: tfrg_scan.hip;
// stream_read: tfrg_bwprobe.hip): each picks its kernel's template arguments, sizes the
// dynamic LDS beside the kernel's carve-up and queries the occupancy; max_blocks / resident are the
// policy's caps, and from cfg they take lane_max, wave_stage, walk_blocks and num_cus. They only
// enqueue: launch_decode reads the launch status once, after the last one.
int lane_count_mode(const DevSchema& sc);  // 0: per-lane dicts in LDS, 1: MaskSink (<= 64 slots), 2: global dict
void launch_lane_count(const DevBatch& b, const DevSchema& sc, const DevOut& o, const uint32_t* d_tab,
                       const LaunchCfg& cfg, bool defer_big, int mode, int max_blocks, hipStream_t st);
void launch_body_count(const DevBatch& b, const DevOut& o, int num_cus, hipStream_t st);
bool tail_walk_fits(const DevSchema& sc);  // role_big_walk's LDS fits k_tail_count's launch
void launch_tail_count(const DevBatch& b, const DevSchema& sc, const DevOut& o, const uint32_t* d_tab,
                       const uint32_t* d_consts, const LaunchCfg& cfg, bool finish, bool walk, uint32_t max_blocks,
                       hipStream_t st);
void launch_poison_loc(const DevOut& o, uint32_t n, uint32_t n_slots, const uint32_t recs[4], hipStream_t st);
void launch_spine(const DevOut& o, const DevSchema& sc, uint32_t n_tiles, uint32_t n, hipStream_t st);
void launch_down_gather(const DevBatch& b, const DevSchema& sc, const DevOut& o, const LaunchCfg& cfg,
                        uint32_t n_tiles, uint32_t resident, hipStream_t st);
void launch_tail_gather(const DevBatch& b, const DevSchema& sc, const DevOut& o, const LaunchCfg& cfg, int max_blocks,
                        hipStream_t st);
hipError_t launch_fill_placed_rows(uint32_t* rs, const uint32_t* info, uint32_t n_slots, uint32_t n, hipStream_t st);
// off[r] = end32[r] + delta for r < n: an implicit bytes_off run written out (tfrg_info.implicit_off_slots)
hipError_t launch_fill_rel_off(uint32_t* off, const uint32_t* end32, uint32_t delta, uint32_t n, hipStream_t st);
hipError_t launch_stream_read(const void* d, uint64_t nbytes, uint32_t* sink, hipStream_t st, int variant);
// tfrg_frame.hip: every phase of the chunked framing index (tfrg_frame.h) enqueued on st
struct FrTab;
hipError_t launch_frame_index(const FrTab& T, int num_cus, hipStream_t st);
// tfrg_decode.cpp: the launch policy of one decode. ev: optional kNumStages + 1 events recorded on
// `stream` before each stage and after the last.
hipError_t launch_decode(const DevBatch& b, const DevSchema& sc, const DevOut& o, LaunchCfg& cfg,
                         const uint32_t* d_crc_tables, const uint32_t* d_wave_consts, hipStream_t stream,
                         hipEvent_t* ev);

}  // namespace tfrg
