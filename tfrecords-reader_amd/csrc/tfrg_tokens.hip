// tfrg_tokens.hip — the kernels behind tfrg_result_token_ids: for a list of m rows (row k is record
// g = entry(k) - row0) and every requested bytes_list slot, the rows' taken elements (those of
// tfrg_elems.hip, from tfrg_elem_rows.h) split into tokens at ASCII delimiter bytes, one int64 id per
// token (tfrg_ids_dev.h: the vocabulary word equal to the token's bytes, else a hash bucket, else a
// default) and the m + 1 offsets of the rows in tokens. Three launches on the decode's stream, no
// workgroup ever waiting on another:
//
//   k_tok_count  per (spec, tile of `tile` rows): the tile's element bytes swept once, each row's token
//                count (cut at max_tokens) kept in place in row_offsets[k]; the tile's sum into the
//                scratch, and the three per-row counters;
//   k_tok_scan   one workgroup per spec: the tile sums to their exclusive bases, carrying across passes
//                of kTokScanThreads tiles; row_offsets[m] and the total T;
//   k_tok_write  per (spec, tile): the counts to the tile's row_offsets (the row table of tfrg_rows.h in
//                LDS), then the bytes swept a second time and the ids stored where t < tok_cap.
//
// How a row is swept (both passes). Its work is not known from the row splits, so rows are split by their
// byte length (the sum of the taken elements' lengths: one subtraction of the materialized column's
// offsets, a product for a constant length, else a sum that stops above the split):
//   a row of at most `split` bytes is one lane's work: a wave takes 64 such rows, and a lane reads its
//     row 8 bytes a step (word8: three aligned dwords through the bounded buffer resource);
//   a longer row goes onto a list in LDS (the row table's `src` words, which these kernels need for
//     nothing else) and the list is dealt to the workgroup's waves: a wave reads 64 consecutive words
//     (512 B) of the current element a round.
// In both modes a lane turns its word into an 8-bit mask nd of the bytes that are no delimiter (bytes
// at or past the element's end are delimiters: an element always closes its token) and, with the bit pv
// of the byte before the word (the lane's own carry; in a wave the neighbour lane's top bit by
// __shfl_up, lane 0's from the round before), into start bits nd & ~prev and end bits ~nd & prev: an end
// bit marks the DELIMITER after a token, so no lane looks ahead. An element of L bytes takes L / 8 + 1
// words: the last one holds position L. At most 4 tokens end in a word. The count is the popcount of
// the end bits (in a wave: reduced onto a uniform running count).
// Emitting (k_tok_write): a token is hashed by the lane in whose word it ENDS, up to 4 of them in
// lockstep (the loop of k_id_write). Its start is a start bit of the same word, or, for the token open
// on entry into the word, the lane's carried start -- in a wave the last start bit of any earlier lane,
// by an exclusive max-scan of the lanes' last start positions seeded with the round's open start. Its
// output index is the row's base from the row table plus the tokens before it: the lane's running count,
// in a wave the uniform count plus an exclusive prefix sum of the lanes' popcounts. No token list in LDS
// and no barrier inside the sweep ("Token ids", says what that departs from and costs).
//
// Cost rules (tfrg.h states them): a token is hashed by one lane, 8 bytes a step; a long row is swept by
// one wave; the bytes are read twice; a row of very many tiny elements walks them one per round.
//
// Not read: what k_id_* do not read (tfrg_ids.hip), and in k_tok_write the rows without a token and,
// without counters, the rows whose first token lies at or past tok_cap.
#include <hip/hip_runtime.h>

#include "tfrg_elem_rows.h"
#include "tfrg_ids_dev.h"
#include "tfrg_internal.h"
#include "tfrg_tokens.h"
#include "tfrg_vocab.h"

namespace tfrg {
namespace {

constexpr uint32_t kBlk = kElemBlk;
constexpr uint32_t kWaves = kBlk / 64;

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) TokArgs* KArgs;
typedef const __attribute__((address_space(4))) TokSpec* KSpec;

// the spec a workgroup works in (uniform), with the fields tfrg_elem_rows.h reads
struct Sp {
  static constexpr uint32_t kNoLen = kTokNoLen;
  KArgs a;
  KSpec s;
  const uint32_t* rs;  // the slot's row splits; null: placed (record g holds one element, at index g)
  uint64_t base;       // slot_base[slot]
  uint32_t max_elems;
  bool by_end;         // the element of record g lies at end32[g] + const_off
  RowList rl;          // (rows null: entry k is k)
};

__device__ __forceinline__ Sp make_sp(KArgs a, uint32_t si) {
  const KSpec s = &a->sp[si];
  const uint32_t slot = s->slot;
  Sp x;
  x.a = a;
  x.s = s;
  x.base = a->slot_base[slot];
  x.rs = slot_splits(a, slot);
  x.max_elems = s->max_elems;
  x.by_end = !a->b_off64 && s->const_off != kTokOffStored;
  x.rl = make_row_list(a);
  return x;
}

// whether the row's taken elements hold at most `split` bytes in all: a lane's work
__device__ __forceinline__ bool row_short(const Sp& x, const Row& w, uint32_t split) {
  if (x.a->b_off64) {
    const uint64_t es = x.base + w.src;
    return x.a->b_off64[es + w.cnt] - x.a->b_off64[es] <= (uint64_t)split;
  }
  if (x.s->const_len != Sp::kNoLen) return (uint64_t)w.cnt * x.s->const_len <= (uint64_t)split;
  uint64_t sum = 0;
  for (uint32_t j = 0; j < w.cnt && sum <= split; ++j) sum += elem_L(x, w.src, j);
  return sum <= split;
}

// What a sweep reads: the bytes and the delimiter set
struct In {
  Src src;
  uint64_t d0, d1;
};

// bit i: byte i of the word is no delimiter; bytes at or past `valid` (>= 1) count as delimiters
__device__ __forceinline__ uint32_t nd_mask(const In& in, uint64_t w, uint32_t valid) {
  uint32_t nd = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    const uint32_t b = (uint32_t)(w >> (8u * i)) & 0xffu;
    const uint64_t d = (b & 64u) ? in.d1 : in.d0;
    const uint32_t delim = (uint32_t)(d >> (b & 63u)) & (b < 128u ? 1u : 0u);
    nd |= (delim ^ 1u) << i;
  }
  return valid >= 8u ? nd : nd & ((1u << valid) - 1u);
}

// the mask of word k of the element (off, L); k <= L / 8, the word of position L included
__device__ __forceinline__ uint32_t word_mask(const In& in, uint32_t off, uint32_t L, uint32_t k) {
  const uint32_t valid = L - (k << 3);
  return valid ? nd_mask(in, word8(in.src, off, L, k), valid) : 0u;
}

// What k_tok_write stores with (uniform)
struct Out {
  KSpec ks;
  Src blob;
  int64_t* out;
  uint64_t ecap;  // ids that are stored: out ? tok_cap : 0
  uint64_t lim;   // tokens at or past it are neither hashed nor counted (e1 with counters, else <= ecap)
  uint64_t nb;
  uint32_t max_word;
  bool pow2, has_vocab, lower;
};

// The tokens that end in a lane's word (at most kPer): token i < popc(e) runs from ts[i] to its end bit,
// both relative to the element. s, e: the word's start and end bits; pos: its first byte; open, ost: a
// token is open on entry and starts at ost. Returns the start of the token left open (if s has a bit left).
__device__ __forceinline__ uint32_t pair4(uint32_t s, uint32_t e, uint32_t pos, bool open, uint32_t ost,
                                          uint32_t (&ts)[kPer], uint32_t (&tl)[kPer], bool (&has)[kPer]) {
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    has[i] = e != 0u;
    const uint32_t pe = (uint32_t)__builtin_ctz(e | 0x100u);
    uint32_t st = ost;
    if (has[i] && !open) {
      st = pos + (uint32_t)__builtin_ctz(s | 0x100u);
      s &= s - 1u;
    }
    if (has[i]) {
      open = false;
      e &= e - 1u;
    }
    ts[i] = st;
    tl[i] = pos + pe - st;
  }
  return s ? pos + (uint32_t)__builtin_ctz(s) : ost;
}

// The lane's kPer tokens of the element at `off` hashed in lockstep, probed and stored (k_id_write's
// loop, with the lower-case fold on the token's side): token i is (ts[i], tl[i]), te[i] its output index
__device__ __forceinline__ void emit4(const Out& o, const Src& in, uint32_t off, const uint32_t (&ts)[kPer],
                                      const uint32_t (&tl)[kPer], const uint64_t (&te)[kPer], const bool (&on)[kPer],
                                      uint32_t& unmatched) {
  uint32_t to[kPer], nw[kPer], steps = 0;
  uint64_t h[kPer];
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    // (a start past 2^32 lies past the bound, where every byte reads as zero)
    const uint64_t at = (uint64_t)off + ts[i];
    to[i] = at < 0xffffffffull ? (uint32_t)at : 0xffffffffu;
    const bool hashed = on[i] && (o.nb != 0ull || tl[i] <= o.max_word);
    nw[i] = hashed ? words_of(tl[i]) : 0u;
    steps = nw[i] > steps ? nw[i] : steps;
    h[i] = kHashSeed;
  }
#pragma unroll 1
  for (uint32_t k = 0; k < steps; ++k) {
    uint64_t w[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) w[i] = k < nw[i] ? word8(in, to[i], tl[i], k) : 0ull;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      if (o.lower) w[i] = lower8(w[i]);
      h[i] = k < nw[i] ? hash_step(h[i], w[i]) : h[i];
    }
  }
#pragma unroll 1
  for (uint32_t i = 0; i < kPer; ++i) {
    if (!on[i]) continue;
    const uint64_t hv = hash_finish(h[i], (uint64_t)tl[i]);
    uint32_t w = kVocabEmpty;
    if (o.has_vocab && tl[i] <= o.max_word)
      w = o.lower ? probe<true>(o.ks, in, o.blob, to[i], tl[i], hv) : probe<false>(o.ks, in, o.blob, to[i], tl[i], hv);
    const int64_t id = id_rule(o.ks, w, hv, o.nb, o.pow2, unmatched);
    if (te[i] < o.ecap) o.out[te[i]] = id;
  }
}

// One lane sweeps its row. EMIT false: returns the row's tokens, or some number above `limit` != 0.
// EMIT true: stores the row's first `limit` (>= 1) tokens from output index rbase on.
template <bool EMIT>
__device__ __forceinline__ uint32_t sweep_lane(const Sp& x, const In& in, const Row& w, uint32_t limit, const Out* o,
                                               uint64_t rbase, uint32_t& unmatched) {
  uint32_t c = 0;
  for (uint32_t j = 0; j < w.cnt; ++j) {
    const uint32_t L = elem_L(x, w.src, j);
    if (!L) continue;
    const uint32_t off = elem_off(x, w.src, j), nwd = (L >> 3) + 1u;
    uint32_t pv = 0, ost = 0;
    for (uint32_t k = 0; k < nwd; ++k) {
      const uint32_t nd = word_mask(in, off, L, k);
      const uint32_t prev = ((nd << 1) | pv) & 0xffu;
      const uint32_t s = nd & ~prev, e = ~nd & prev;
      if constexpr (EMIT) {
        uint32_t ts[kPer], tl[kPer];
        uint64_t te[kPer];
        bool on[kPer];
        ost = pair4(s, e, k << 3, pv != 0u, ost, ts, tl, on);
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
          te[i] = rbase + c + i;
          on[i] = on[i] && c + i < limit && te[i] < o->lim;
        }
        if (e) emit4(*o, in.src, off, ts, tl, te, on, unmatched);
      }
      c += (uint32_t)__builtin_popcount(e);
      pv = nd >> 7;
      if (EMIT ? c >= limit : (limit && c > limit)) return c;
    }
  }
  return c;
}

// One wave sweeps its row (every lane active, every argument uniform): as sweep_lane, 64 words a round
template <bool EMIT>
__device__ __forceinline__ uint32_t sweep_wave(const Sp& x, const In& in, const Row& w, uint32_t limit, const Out* o,
                                               uint64_t rbase, uint32_t& unmatched) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t c = 0;
  for (uint32_t j = 0; j < w.cnt; ++j) {
    const uint32_t L = rfl32(elem_L(x, w.src, j));
    if (!L) continue;
    const uint32_t off = rfl32(elem_off(x, w.src, j)), nwd = (L >> 3) + 1u;
    uint32_t carry = 0, ost1 = 0;  // the token open across the round: its top bit, its start + 1
    for (uint32_t k0 = 0; k0 < nwd; k0 += 64u) {
      const uint32_t k = k0 + lane, pos = k << 3;
      const uint32_t nd = k < nwd ? word_mask(in, off, L, k) : 0u;
      const uint32_t up = (uint32_t)__shfl_up((int)(nd >> 7), 1, 64);
      const uint32_t pv = lane ? up : carry;
      const uint32_t prev = ((nd << 1) | pv) & 0xffu;
      const uint32_t s = nd & ~prev, e = ~nd & prev;
      const uint32_t ne = (uint32_t)__builtin_popcount(e);
      carry = rfl32((uint32_t)__shfl((int)(nd >> 7), 63, 64));
      if constexpr (EMIT) {
        // the start (+ 1) of the token open on entry into the lane's word: the last start before it
        uint32_t mx = s ? pos + (32u - (uint32_t)__builtin_clz(s)) : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t u = (uint32_t)__shfl_up((int)mx, d, 64);
          if (lane >= (uint32_t)d) mx = u > mx ? u : mx;
        }
        uint32_t before = (uint32_t)__shfl_up((int)mx, 1, 64);
        before = lane ? before : 0u;
        before = before > ost1 ? before : ost1;
        const uint32_t last = rfl32((uint32_t)__shfl((int)mx, 63, 64));
        const uint32_t inc = wave_incl_scan(ne);
        const uint32_t tot = rfl32((uint32_t)__shfl((int)inc, 63, 64)), mine = c + (inc - ne);
        uint32_t ts[kPer], tl[kPer];
        uint64_t te[kPer];
        bool on[kPer];
        (void)pair4(s, e, pos, pv != 0u, before - 1u, ts, tl, on);
#pragma unroll
        for (uint32_t i = 0; i < kPer; ++i) {
          te[i] = rbase + mine + i;
          on[i] = on[i] && mine + i < limit && te[i] < o->lim;
        }
        if (tot) emit4(*o, in.src, off, ts, tl, te, on, unmatched);
        ost1 = carry ? (last > ost1 ? last : ost1) : 0u;
        c += tot;
      } else {
        c += rfl32(wave_sum32(ne));
      }
      if (EMIT ? c >= limit : (limit && c > limit)) return c;
    }
  }
  return c;
}

struct Setup {
  Sp x;
  In in;
  RowTable l;
  uint32_t si, t0, nrows;
};

__device__ __forceinline__ Setup setup(KArgs a, uint8_t* lds) {
  const uint32_t tiles = a->tiles, tile = a->tile;
  Setup u;
  u.si = blockIdx.x / tiles;
  const uint32_t ti = blockIdx.x - u.si * tiles;
  u.l = carve_row_table(lds, tile);
  u.x = make_sp(a, u.si);
  u.t0 = ti * tile;
  u.nrows = a->m - u.t0 < tile ? a->m - u.t0 : tile;
  u.in = In{Src{bytes_source(a), a->in_bound}, u.x.s->delims[0], u.x.s->delims[1]};
  return u;
}

// ------------------------------------------------------------------ 1. counts
// dynamic LDS: the row table of tfrg_rows.h (tok_lds_bytes sizes it); src holds the list of long rows
__global__ __launch_bounds__(kBlk) void k_tok_count(const TokArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tk_lds[];
  __shared__ uint32_t n_long;
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const Setup u = setup(a, tk_lds);
  const uint32_t mt = u.x.s->max_tokens, split = a->split;
  int64_t* const ro = u.x.s->row_offsets + u.t0;
  if (threadIdx.x == 0) n_long = 0u;
  __syncthreads();
  uint32_t rtrunc = 0, empty = 0, skip = 0, none = 0;
  uint64_t sum = 0;
  for (uint32_t r = threadIdx.x; r < u.nrows; r += kBlk) {
    const Row w = row_of(u.x, u.t0 + r);
    skip += w.ok ^ 1u;
    if (w.cnt && !row_short(u.x, w, split)) {
      u.l.src[atomicAdd(&n_long, 1u)] = r;
      continue;
    }
    uint32_t c = sweep_lane<false>(u.x, u.in, w, mt, nullptr, 0ull, none);
    const bool cut = mt && c > mt;
    c = cut ? mt : c;
    rtrunc += cut;
    empty += w.ok & (uint32_t)(c == 0u);
    ro[r] = (int64_t)c;
    sum += c;
  }
  __syncthreads();
  const uint32_t nl = n_long;
  for (uint32_t i = threadIdx.x >> 6; i < nl; i += kWaves) {
    const uint32_t r = rfl32(u.l.src[i]);
    const Row w = row_of(u.x, u.t0 + r);
    uint32_t c = sweep_wave<false>(u.x, u.in, w, mt, nullptr, 0ull, none);
    const bool cut = mt && c > mt;
    c = cut ? mt : c;
    if ((threadIdx.x & 63u) == 0u) {
      rtrunc += cut;
      empty += c == 0u;
      ro[r] = (int64_t)c;
      sum += c;
    }
  }
  uint64_t total;
  (void)block_excl_scan<kWaves>(sum, u.l.part, &total);
  if (threadIdx.x == 0) a->tsum[blockIdx.x] = total;
  if (a->stats) add_stats4(a->stats, u.si, rtrunc, 0u, empty, skip);
}

// ------------------------------------------------------------------ 2. tile scan
// one workgroup per spec: the tile sums to their exclusive prefixes, T to row_offsets[m] and the totals
__global__ __launch_bounds__(kTokScanThreads) void k_tok_scan(const TokArgs) {
  __shared__ uint64_t part[kTokScanThreads / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, si = blockIdx.x;
  uint64_t* const tsum = a->tsum + (uint64_t)si * tiles;
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < tiles; b0 += kTokScanThreads) carry = scan_tile_sums<kTokScanThreads>(tsum, tiles, b0, carry, part);
  if (threadIdx.x == 0) {
    a->sp[si].row_offsets[a->m] = (int64_t)carry;
    if (a->totals) a->totals[si] = carry;
  }
}

// ------------------------------------------------------------------ 3. row offsets and ids
// dynamic LDS as k_tok_count
__global__ __launch_bounds__(kBlk) void k_tok_write(const TokArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t tk_lds[];
  __shared__ uint32_t n_long;
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const Setup u = setup(a, tk_lds);
  const KSpec ks = u.x.s;
  const uint32_t split = a->split, nrows = u.nrows;
  int64_t* const ro = ks->row_offsets + u.t0;  // (row_offsets[m] is k_tok_scan's)
  const uint64_t eb = a->tsum[blockIdx.x];
  // the counts k_tok_count left in place, to the tile's row table and row offsets (an entry is read and
  // then written by the one thread that owns it)
  uint64_t e1 = eb;
  for (uint32_t r0 = 0; r0 < nrows; r0 += kBlk) {
    const uint32_t r = r0 + threadIdx.x;
    const uint64_t cnt = r < nrows ? (uint64_t)ro[r] : 0ull;
    uint64_t total;
    const uint64_t ex = block_excl_scan<kWaves>(cnt, u.l.part, &total);
    if (r < nrows) {
      u.l.offs[r] = e1 + ex;
      ro[r] = (int64_t)(e1 + ex);
    }
    e1 += total;
  }
  if (threadIdx.x == 0) {
    u.l.offs[nrows] = e1;
    n_long = 0u;
  }
  // the tile's tokens that are stored or counted (uniform)
  uint32_t* const stats = a->stats;
  const uint64_t ecap = ks->ids ? ks->tok_cap : 0ull;
  const uint64_t lim = stats ? e1 : (ecap < e1 ? ecap : e1);
  if (lim <= eb) return;
  __syncthreads();
  const uint64_t nb = ks->n_buckets;
  const bool has_vocab = ks->table != nullptr;
  const Out o{ks,
              Src{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(ks->blob), (short)0, (int)ks->blob_bound, 0x00020000),
                  ks->blob_bound},
              ks->ids, ecap, lim, nb, has_vocab ? ks->max_word : 0u, (nb & (nb - 1ull)) == 0ull, has_vocab, ks->lower != 0u};
  uint32_t unmatched = 0;
  for (uint32_t r = threadIdx.x; r < nrows; r += kBlk) {
    const uint64_t base = u.l.offs[r];
    const uint32_t cnt = (uint32_t)(u.l.offs[r + 1u] - base);
    if (!cnt || base >= lim) continue;  // (no token, or none that is stored or counted: the row is not read)
    const Row w = row_of(u.x, u.t0 + r);
    if (!row_short(u.x, w, split)) {
      u.l.src[atomicAdd(&n_long, 1u)] = r;
      continue;
    }
    (void)sweep_lane<true>(u.x, u.in, w, cnt, &o, base, unmatched);
  }
  __syncthreads();
  const uint32_t nl = n_long;
  for (uint32_t i = threadIdx.x >> 6; i < nl; i += kWaves) {
    const uint32_t r = rfl32(u.l.src[i]);
    const uint64_t base = u.l.offs[r];
    const Row w = row_of(u.x, u.t0 + r);
    (void)sweep_wave<true>(u.x, u.in, w, (uint32_t)(u.l.offs[r + 1u] - base), &o, base, unmatched);
  }
  if (stats) add_stats4(stats, u.si, 0u, unmatched, 0u, 0u);
}

}  // namespace

hipError_t launch_tokens(const TokArgs& a, hipStream_t st) {
  const uint32_t per_spec = a.n_specs * a.tiles;
  const size_t lds = tok_lds_bytes(a.tile);
  hipLaunchKernelGGL(k_tok_count, dim3(per_spec), dim3(kBlk), lds, st, a);
  hipLaunchKernelGGL(k_tok_scan, dim3(a.n_specs), dim3(kTokScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_tok_write, dim3(per_spec), dim3(kBlk), lds, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
