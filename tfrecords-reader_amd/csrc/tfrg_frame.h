// tfrg_frame.h — the chunked framing index (tfrg_index_device): the exact framing walk of
// tfrg_index_split (tfrg_host.cpp index_walk, indexer.pyx:212-252) cut into chunks that are walked in
// parallel from guessed entries, verified along the chain from each piece's chunk 0 and repaired.
// Every step is written once here as host + device code: the kernels (tfrg_frame.hip) apply the
// per-chunk functions below one thread (one wave for the guess) per chunk, the CPU model
// (tfrg_frame_host.cpp) in plain loops, phase by phase in the same order.
//
// Phases (one kernel launch each; no kernel waits on another workgroup):
//   guess    chunk k > 0 of a piece: entry = the first position that passes fr_header_test
//            (chunk 0: entry 0; no candidate: kFrNone)
//   walk     from the entry to the exit: the first record start at or past the chunk's end, or kFrNone
//            (the walk ended); count = records started in the chunk. From a guessed entry the walk is
//            checked: it skips to the chunk's next candidate where a header is not plausible, and is
//            then impure
//   rounds   r = 0 .. kIndexRepairRounds: mark the chunks on the chain from each piece's chunk 0 by
//            pointer jumping over next(k) = chunk_of(exit(k)); a marked chunk whose successor's entry
//            differs from its exit, or whose successor is impure, leaves that exit as the successor's
//            pending entry (a mismatch); an unmarked chunk proposes its exit to a successor without an
//            entry; pending chunks are re-walked exactly (r < kIndexRepairRounds). A round that finds
//            no mismatch ends the rounds: by induction from entry 0 the marked chain is the host walk's.
//   rank     exclusive scan of count x mark; a second walk of the marked chunks writes the rows
#pragma once
#include <stdint.h>
#include <string.h>

#include "crc32c.h"

struct tfrg_index_info;  // include/tfrg.h

namespace tfrg {

constexpr uint32_t kIndexRepairRounds = 4;     // a design bound, not a measurement
constexpr uint32_t kIndexChunkDefault = 4096;  // bytes
constexpr uint32_t kIndexChunkMin = 64, kIndexChunkMax = 65536;
constexpr uint32_t kFrNone = 0xffffffffu;  // entry: no candidate; exit: the walk ended; jump: no successor
constexpr uint32_t kFrSeek = 1u;           // chunk flag: a length field seeks to or before its own record
constexpr uint32_t kFrImpure = 2u;         // chunk flag: its checked walk skipped bytes (not the host walk)
constexpr uint32_t kFrBlock = 256;         // chunks per workgroup of the rank / write kernels

// summary words (device, zeroed per call; copied back with the piece rows in one D2H)
enum FrSum : uint32_t {
  kFsMism = 0,                              // [kIndexRepairRounds + 1] mismatches found by round r
  kFsSeek = kFsMism + kIndexRepairRounds + 1,  // a marked chunk holds a backward seek
  kFsNot32,                                 // some end >= 2^32
  kFsRecords,                               // records of all pieces
  kFsWords = 16
};
static_assert(kFsRecords < kFsWords, "summary words");

struct FrPiece {
  uint64_t base;    // offset of the piece in the batch
  uint64_t size;
  uint32_t chunk0;  // its first chunk in the batch's chunk table
  uint32_t pad;
};
struct FrPieceOut {
  uint64_t first;     // record number of the piece's first record (pieces with chunks)
  uint64_t last_end;  // end of its last record (pieces with records)
};

struct FrTab {
  const uint8_t* bytes;
  const FrPiece* pieces;
  uint32_t n_pieces, n_chunks;
  uint32_t shift;     // log2 of the chunk size
  uint32_t jumps;     // pointer-jumping steps per round: 2^jumps >= chunks of the largest piece
  uint32_t *entry, *exit, *count, *cflags, *cpiece;  // [n_chunks], offsets relative to the piece
  uint32_t *mark, *jump[2], *pend, *pend2;           // [n_chunks]
  uint32_t* bsum;     // [ceil(n_chunks / kFrBlock)] marked records per block, then their exclusive prefix
  uint32_t* summ;     // [kFsWords]
  FrPieceOut* pout;   // [n_pieces]
  const uint32_t* crc_t0;  // the CRC-32C byte table (256 words)
  uint64_t *start, *end;   // outputs (each may be null), cap rows
  uint32_t* end32;
  uint64_t cap;
};

// ---- loads ---------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
// aligned dwords and a byte shift: a dword that holds one readable byte is readable
__device__ __forceinline__ uint32_t fr_ld32(const uint8_t* b, uint64_t a) {
  const uintptr_t q = (uintptr_t)(b + a);
  const uint32_t* w = (const uint32_t*)(q & ~(uintptr_t)3);
  const uint32_t k = (uint32_t)(q & 3);
  const uint32_t lo = w[0];
  const uint32_t hi = k ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, k);
}
__device__ __forceinline__ void fr_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void fr_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
__device__ __forceinline__ void fr_min(uint32_t* p, uint32_t v) { atomicMin(p, v); }
#else
inline uint32_t fr_ld32(const uint8_t* b, uint64_t a) {
  uint32_t v;
  memcpy(&v, b + a, 4);
  return v;
}
inline void fr_add(uint32_t* p, uint32_t v) { *p += v; }
inline void fr_or(uint32_t* p, uint32_t v) { *p |= v; }
inline void fr_min(uint32_t* p, uint32_t v) { *p = v < *p ? v : *p; }
#endif
TFRG_HD inline uint64_t fr_ld64(const uint8_t* b, uint64_t a) {
  return (uint64_t)fr_ld32(b, a) | ((uint64_t)fr_ld32(b, a + 4) << 32);
}

// ---- the walk step -------------------------------------------------------------------------------
// The seek after the record at pos (< 2^32) with the given length field, as index_walk does it:
// pos + 12, then fseek's long offset (int64)(length + 4). 0: the next record starts at *np;
// 1: the seek overflows or lands below 0 (the piece ends after this record); 2: it lands at or before
// the record's own start (the host walk goes on from there and may never end: TFRG_INDEX_FB_SEEK).
TFRG_HD inline int fr_seek(uint64_t pos, uint64_t length, uint64_t* np) {
  const int64_t p12 = (int64_t)pos + 12;
  const int64_t off = (int64_t)(length + 4);
  int64_t n;
  if (__builtin_add_overflow(p12, off, &n) || n < 0) return 1;
  if ((uint64_t)n <= pos) return 2;
  *np = (uint64_t)n;
  return 0;
}

struct FrWalk {
  uint32_t exit, count, flags;
};
TFRG_HD inline bool fr_plausible(const uint8_t* piece, uint64_t size, uint64_t p, const uint32_t* t0);
TFRG_HD inline bool fr_header_test(const uint8_t* piece, uint64_t size, uint64_t p, const uint32_t* t0);
// Walks the records that start in [entry, chunk_end) of a piece; put(i, start, length) for the i-th
// of them. Every step advances by at least one byte, so chunk_end - entry steps bound the loop.
// CHECK (the walk from a guessed entry, a hint like the guess): a position that does not look like a
// header (fr_plausible) makes the walk impure (kFrImpure: the chunk is re-walked without CHECK once it
// is on the chain) and resumes it at the next position of the chunk that passes fr_header_test, so a
// wrong guess still tends to leave the chunk at the right exit and the chunks after it stay linked.
template <bool CHECK, class Put>
TFRG_HD inline FrWalk fr_walk_chunk(const uint8_t* piece, uint64_t size, uint32_t entry, uint64_t chunk_end,
                                    Put& put, const uint32_t* t0) {
  FrWalk r{kFrNone, 0u, 0u};
  uint64_t pos = entry;
  const uint64_t steps = chunk_end > pos ? chunk_end - pos : 0;
  for (uint64_t it = 0; it < steps && pos < chunk_end; ++it) {
    if (pos + 8 > size) return r;  // a tail of fewer than 8 bytes ends the walk
    if (CHECK && !fr_plausible(piece, size, pos, t0)) {
      r.flags |= kFrImpure;
      uint64_t p = pos + 1;
      for (; p < chunk_end && !fr_header_test(piece, size, p, t0); ++p) ++it;
      if (p >= chunk_end) return r;
      pos = p;
      continue;
    }
    const uint64_t length = fr_ld64(piece, pos);
    put(r.count, pos, length);
    ++r.count;
    uint64_t np = 0;
    const int k = fr_seek(pos, length, &np);
    if (k) {
      if (k == 2) r.flags |= kFrSeek;
      return r;
    }
    pos = np;
  }
  if (pos >= chunk_end && pos + 8 <= size) r.exit = (uint32_t)pos;  // (size < 2^32)
  return r;
}
struct FrNoPut {
  TFRG_HD void operator()(uint32_t, uint64_t, uint64_t) const {}
};

// ---- the entry guess -----------------------------------------------------------------------------
// masked CRC-32C of the 8 length bytes (t0: the byte table)
TFRG_HD inline uint32_t fr_len_crc(const uint32_t* t0, uint32_t lo, uint32_t hi) {
  uint32_t c = 0xffffffffu;
  for (int j = 0; j < 4; ++j) c = t0[(c ^ (lo >> (8 * j))) & 0xff] ^ (c >> 8);
  for (int j = 0; j < 4; ++j) c = t0[(c ^ (hi >> (8 * j))) & 0xff] ^ (c >> 8);
  return crc_mask(~c);
}
// Could position p of the piece be a record header? Its length fits the piece (so the high word is
// 0) and the stored length CRC is the spec's or 0 (the frames the reference's own writers leave). A
// header cut by the piece's end cannot be judged and passes.
TFRG_HD inline bool fr_plausible(const uint8_t* piece, uint64_t size, uint64_t p, const uint32_t* t0) {
  if (p + 12 > size) return true;
  if (fr_ld32(piece, p + 4) != 0) return false;
  const uint32_t len = fr_ld32(piece, p);
  if (len > size - p) return false;
  const uint32_t crc = fr_ld32(piece, p + 8);
  return crc == 0 || crc == fr_len_crc(t0, len, 0u);
}
// Does position p look like a record header? A whole plausible header whose length CRC is the spec's;
// or whose CRC is 0, as are the 4 bytes before it (the data CRC of the record before, in the files
// that leave CRCs 0: one byte earlier, a length field shifted by 8 bits would pass as well), and whose
// record ends the piece or is followed by a whole plausible header.
// Only a hint: a wrong guess is repaired, never trusted.
TFRG_HD inline bool fr_header_test(const uint8_t* piece, uint64_t size, uint64_t p, const uint32_t* t0) {
  if (p + 12 > size) return false;
  if (fr_ld32(piece, p + 4) != 0) return false;
  const uint32_t len = fr_ld32(piece, p);
  if (len > size - p) return false;
  const uint32_t crc = fr_ld32(piece, p + 8);
  if (crc == fr_len_crc(t0, len, 0u)) return true;
  if (crc != 0) return false;
  if (p >= 4 && fr_ld32(piece, p - 4) != 0) return false;
  const uint64_t q = p + 16 + (uint64_t)len;
  if (q == size) return true;
  return q + 12 <= size && fr_plausible(piece, size, q, t0);
}

// ---- per-chunk phases ----------------------------------------------------------------------------
// the piece of chunk k: the last piece whose first chunk is <= k (pieces without chunks precede the
// piece that shares their chunk0)
TFRG_HD inline uint32_t fr_piece_of(const FrTab& T, uint32_t k) {
  uint32_t lo = 0, hi = T.n_pieces;  // first piece with chunk0 > k
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (T.pieces[mid].chunk0 <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}
TFRG_HD inline uint64_t fr_chunk_end(const FrTab& T, const FrPiece& P, uint32_t k) {
  const uint64_t e = ((uint64_t)(k - P.chunk0) + 1) << T.shift;
  return e < P.size ? e : P.size;
}
// a round's initial state of chunk k: only chunk 0 of a piece marked, the links from the exits
TFRG_HD inline void fr_round_init(const FrTab& T, uint32_t k, const FrPiece& P) {
  const uint32_t x = T.exit[k];
  T.mark[k] = k == P.chunk0;
  T.jump[0][k] = x == kFrNone ? kFrNone : P.chunk0 + (x >> T.shift);
  T.pend[k] = kFrNone;
  T.pend2[k] = kFrNone;
}
// walk chunk k from its entry (kFrNone: nothing known), then a round's initial state. guessed: the
// entry is the guess of a chunk other than a piece's first (checked walk); else it is known (exact walk)
TFRG_HD inline void fr_walk_init(const FrTab& T, uint32_t k, bool guessed, const uint32_t* t0) {
  const FrPiece P = T.pieces[T.cpiece[k]];
  const uint32_t entry = T.entry[k];
  FrWalk w{kFrNone, 0u, 0u};
  FrNoPut np;
  const uint8_t* piece = T.bytes + P.base;
  const uint64_t ce = fr_chunk_end(T, P, k);
  if (entry == kFrNone) {
  } else if (guessed && k != P.chunk0) {
    w = fr_walk_chunk<true>(piece, P.size, entry, ce, np, t0);
  } else {
    w = fr_walk_chunk<false>(piece, P.size, entry, ce, np, t0);
  }
  T.exit[k] = w.exit;
  T.count[k] = w.count;
  T.cflags[k] = w.flags;
  fr_round_init(T, k, P);
}
// one pointer-jumping step d of round r (src = jump[d & 1]): a marked chunk marks the chunk 2^d links
// on; only chunks on the chain are ever marked, so marks written during the step do no harm
TFRG_HD inline void fr_jump(const FrTab& T, uint32_t k, uint32_t d) {
  const uint32_t* src = T.jump[d & 1];
  const uint32_t j = src[k];
  if (j != kFrNone && T.mark[k]) T.mark[j] = 1u;
  T.jump[(d + 1) & 1][k] = j == kFrNone ? kFrNone : src[j];
}
// A marked chunk whose successor was entered elsewhere, or walked impurely: the successor's pending
// entry, a mismatch (a piece's first chunk is walked exactly from 0, so every other marked chunk has
// a marked predecessor that judges it). A chunk that is not marked, whose successor found no entry
// of its own, proposes its exit to it (the lowest proposal is kept): the chain breaks at a chunk
// without a recognisable header, and the chunks behind the break are linked again in the same round
// rather than one break per round. A proposal is only another guess, verified like the first.
TFRG_HD inline void fr_detect(const FrTab& T, uint32_t k, uint32_t r) {
  const uint32_t x = T.exit[k];
  if (x == kFrNone) return;
  const uint32_t j = T.pieces[T.cpiece[k]].chunk0 + (x >> T.shift);
  if (!T.mark[k]) {
    if (T.entry[j] == kFrNone) fr_min(T.pend2 + j, x);
    return;
  }
  if (T.entry[j] != x || (T.cflags[j] & kFrImpure)) {
    T.pend[j] = x;
    fr_add(T.summ + kFsMism + r, 1u);
  }
}
// a chunk with a pending entry is re-walked from it; then the next round's initial state
TFRG_HD inline void fr_repair_init(const FrTab& T, uint32_t k) {
  // (a proposal is walked exactly too: it is a predecessor's exit, and the header there may be one
  // the checked walk would not accept, which is why the chunk had no entry)
  const uint32_t p = T.pend[k] != kFrNone ? T.pend[k] : T.pend2[k];
  if (p != kFrNone) {
    T.entry[k] = p;
    fr_walk_init(T, k, false, nullptr);
  } else {
    fr_round_init(T, k, T.pieces[T.cpiece[k]]);
  }
}
// is round r (its jumps and its detect) still needed? Round 0 always; later ones after a repair
TFRG_HD inline bool fr_round_live(const FrTab& T, uint32_t r) { return r == 0 || T.summ[kFsMism + r - 1] != 0; }

// the marked records of chunk k (rank phase) and its backward-seek flag
TFRG_HD inline uint32_t fr_marked_count(const FrTab& T, uint32_t k) {
  if (!T.mark[k]) return 0u;
  if (T.cflags[k] & kFrSeek) fr_or(T.summ + kFsSeek, 1u);
  return T.count[k];
}
struct FrPut {
  const FrTab& T;
  uint64_t base, rank;
  uint64_t last_end;
  bool not32;
  TFRG_HD void operator()(uint32_t i, uint64_t start, uint64_t length) {
    const uint64_t row = rank + i;
    const uint64_t e = start + 16 + length + base;  // u64 arithmetic, as the reference
    last_end = e;
    not32 |= (e >> 32) != 0;
    if (row < T.cap) {
      if (T.start) T.start[row] = start + base;
      if (T.end) T.end[row] = e;
      if (T.end32) T.end32[row] = (uint32_t)e;
    }
  }
};
// the rows of marked chunk k, whose first record is number rank
TFRG_HD inline void fr_write(const FrTab& T, uint32_t k, uint64_t rank) {
  const uint32_t pi = T.cpiece[k];
  const FrPiece P = T.pieces[pi];
  if (k == P.chunk0) T.pout[pi].first = rank;
  if (!T.mark[k] || T.entry[k] == kFrNone) return;
  FrPut put{T, P.base, rank, 0, false};
  const FrWalk w = fr_walk_chunk<false>(T.bytes + P.base, P.size, T.entry[k], fr_chunk_end(T, P, k), put, nullptr);
  if (put.not32) fr_or(T.summ + kFsNot32, 1u);
  if (w.exit == kFrNone && w.count) T.pout[pi].last_end = put.last_end;
}

// chunk table layout of a batch: the pieces' rows; returns the chunk count (0xffffffff: too many)
inline uint64_t fr_layout(const uint64_t* piece_sizes, uint32_t n_pieces, uint32_t shift, FrPiece* out,
                          uint32_t* jumps) {
  uint64_t base = 0, chunks = 0, most = 1;
  for (uint32_t i = 0; i < n_pieces; ++i) {
    const uint64_t nc = (piece_sizes[i] + ((1ull << shift) - 1)) >> shift;
    out[i] = FrPiece{base, piece_sizes[i], (uint32_t)chunks, 0u};
    base += piece_sizes[i];
    chunks += nc;
    if (nc > most) most = nc;
  }
  uint32_t j = 0;
  while ((1ull << j) < most) ++j;
  *jumps = j;
  return chunks;
}
// (tfrg_frame_host.cpp) the summary words and piece rows of a finished run -> tfrg_index_info and the
// records per piece
void fr_finish(const uint32_t* summ, const FrPieceOut* pout, const FrPiece* pieces, uint32_t n_pieces,
               uint32_t n_chunks, uint64_t* piece_records, tfrg_index_info* info);

}  // namespace tfrg
