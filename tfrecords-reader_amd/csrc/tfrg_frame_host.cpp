// tfrg_frame_host.cpp — the chunked framing index on the CPU: tfrg_index_device's algorithm run phase
// by phase through the per-chunk functions of tfrg_frame.h, in the order the kernels of
// tfrg_frame.hip run them. It is the model the device results are compared with, and the form of the
// algorithm a sanitizer can see. Exported, not declared in include/tfrg.h (as tfrg_index_split).
#include <vector>

#include "../../include/tfrg.h"
#include "tfrg_frame.h"

using namespace tfrg;

namespace tfrg {

// the summary a finished run leaves (device: after the one D2H) -> tfrg_index_info and the piece counts
void fr_finish(const uint32_t* summ, const FrPieceOut* pout, const FrPiece* pieces, uint32_t n_pieces,
               uint32_t n_chunks, uint64_t* piece_records, tfrg_index_info* info) {
  memset(info, 0, sizeof(*info));
  info->n_records = summ[kFsRecords];
  info->n_chunks = n_chunks;
  for (uint32_t r = 0; r < kIndexRepairRounds; ++r) {
    info->repaired_chunks += summ[kFsMism + r];
    info->repair_rounds += summ[kFsMism + r] != 0;
  }
  // a round that found nothing ended the rounds; mismatches left by the last one are not repaired
  bool open = true;
  for (uint32_t r = 0; r <= kIndexRepairRounds && open; ++r) open = summ[kFsMism + r] != 0;
  if (open) info->fallback = TFRG_INDEX_FB_ROUNDS;
  else if (summ[kFsSeek]) info->fallback = TFRG_INDEX_FB_SEEK;
  // piece counts: differences of the pieces' first record numbers (pieces without chunks hold none)
  uint64_t next = info->n_records;
  bool tiled = summ[kFsNot32] == 0, have = false;
  uint64_t follow = 0;  // start of the first record after piece i
  for (uint32_t i = n_pieces; i-- > 0;) {
    uint64_t cnt = 0;
    if (pieces[i].size) {
      const uint64_t first = pout[i].first <= next ? pout[i].first : next;  // (only a fallback can disorder them)
      cnt = next - first;
      next = first;
    }
    if (piece_records) piece_records[i] = cnt;
    if (!cnt) continue;
    if (have && pout[i].last_end != follow) tiled = false;
    have = true;
    follow = pieces[i].base;
    info->first_start = (uint32_t)pieces[i].base;
  }
  info->tiled = tiled;
}

}  // namespace tfrg

extern "C" int tfrg_index_chunked_host(const uint8_t* bytes, uint64_t nbytes, const uint64_t* piece_sizes,
                                       uint32_t n_pieces, uint32_t chunk, uint64_t* starts, uint64_t* ends,
                                       uint64_t cap, uint64_t* piece_records, tfrg_index_info* info) {
  if (!info) return TFRG_E_ARG;
  memset(info, 0, sizeof(*info));
  if (!chunk) chunk = kIndexChunkDefault;
  if (chunk < kIndexChunkMin || chunk > kIndexChunkMax || (chunk & (chunk - 1))) return TFRG_E_ARG;
  uint64_t sum = 0;
  for (uint32_t i = 0; i < n_pieces; ++i) sum += piece_sizes[i];
  if (nbytes >= (1ull << 32) || sum != nbytes) return TFRG_E_ARG;
  for (uint32_t i = 0; piece_records && i < n_pieces; ++i) piece_records[i] = 0;
  info->tiled = 1;
  if (!n_pieces || !nbytes) return 0;

  uint32_t shift = 0;
  while ((1u << shift) < chunk) ++shift;
  std::vector<FrPiece> pieces(n_pieces);
  FrTab T{};
  const uint64_t nc = fr_layout(piece_sizes, n_pieces, shift, pieces.data(), &T.jumps);
  const uint32_t n = (uint32_t)nc;
  const uint32_t nb = (n + kFrBlock - 1) / kFrBlock;
  std::vector<uint32_t> tab((size_t)n * 10), bsum(nb), summ(kFsWords, 0u);
  std::vector<FrPieceOut> pout(n_pieces, FrPieceOut{0, 0});
  CrcTables ct;
  crc_make_tables(&ct);
  T.bytes = bytes;
  T.pieces = pieces.data();
  T.n_pieces = n_pieces;
  T.n_chunks = n;
  T.shift = shift;
  uint32_t* w = tab.data();
  uint32_t** cols[] = {&T.entry, &T.exit, &T.count, &T.cflags, &T.cpiece, &T.mark, &T.jump[0], &T.jump[1], &T.pend, &T.pend2};
  for (uint32_t** c : cols) {
    *c = w;
    w += n;
  }
  T.bsum = bsum.data();
  T.summ = summ.data();
  T.pout = pout.data();
  T.crc_t0 = ct.t[0];
  T.start = starts;
  T.end = ends;
  T.end32 = nullptr;
  T.cap = cap;

  // guess
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t pi = fr_piece_of(T, k);
    const FrPiece& P = pieces[pi];
    T.cpiece[k] = pi;
    uint32_t e = kFrNone;
    if (k == P.chunk0) {
      e = 0;
    } else {
      const uint64_t lo = (uint64_t)(k - P.chunk0) << shift, hi = fr_chunk_end(T, P, k);
      for (uint64_t p = lo; p < hi && e == kFrNone; ++p)
        if (fr_header_test(bytes + P.base, P.size, p, T.crc_t0)) e = (uint32_t)p;
    }
    T.entry[k] = e;
  }
  // walk
  for (uint32_t k = 0; k < n; ++k) fr_walk_init(T, k, true, T.crc_t0);
  // rounds
  for (uint32_t r = 0; r <= kIndexRepairRounds; ++r) {
    if (!fr_round_live(T, r)) break;
    for (uint32_t d = 0; d < T.jumps; ++d)
      for (uint32_t k = 0; k < n; ++k) fr_jump(T, k, d);
    for (uint32_t k = 0; k < n; ++k) fr_detect(T, k, r);
    if (r == kIndexRepairRounds || !summ[kFsMism + r]) break;
    for (uint32_t k = 0; k < n; ++k) fr_repair_init(T, k);
  }
  // rank and write
  uint64_t total = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    uint32_t s = 0;
    for (uint32_t k = b * kFrBlock; k < n && k < (b + 1) * kFrBlock; ++k) s += fr_marked_count(T, k);
    bsum[b] = (uint32_t)total;
    total += s;
  }
  summ[kFsRecords] = (uint32_t)total;
  for (uint32_t b = 0; b < nb; ++b) {
    uint64_t rank = bsum[b];
    for (uint32_t k = b * kFrBlock; k < n && k < (b + 1) * kFrBlock; ++k) {
      fr_write(T, k, rank);
      rank += T.mark[k] ? T.count[k] : 0u;
    }
  }
  fr_finish(summ.data(), pout.data(), pieces.data(), n_pieces, n, piece_records, info);
  return 0;
}
