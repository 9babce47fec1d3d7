// tfrg_wordpiece.hip — the kernels behind tfrg_result_wordpiece_ids: for a list of m rows and every
// requested bytes_list slot, the rows' taken elements (those of tfrg_elems.hip, from tfrg_elem_rows.h)
// split into words (ASCII delimiters; isolated ASCII bytes that are words of their own), every word cut
// greedily into the longest pieces of two vocabularies (the pieces that begin a word; the continuation
// pieces, stored without their prefix), one int64 id per piece, and the m + 1 offsets of the rows in
// pieces. Three launches on the decode's stream, no workgroup ever waiting on another, as tfrg_tokens.hip:
//
//   k_wp_count  per (spec, tile of `tile` rows): the tile's bytes swept and its words matched once, each
//               row's piece count (cut at the limit, cls and sep included) kept in place in
//               row_offsets[k]; the tile's sum into the scratch, and three of the per-row counters;
//   k_wp_scan   one workgroup per spec: the tile sums to their exclusive bases; row_offsets[m] and T;
//   k_wp_write  per (spec, tile): the counts to the tile's row_offsets (the row table of tfrg_rows.h in
//               LDS), then sweep and match a second time and the ids stored where t < tok_cap.
//
// A pass is two stages that a word list in LDS keeps apart, per wave and with no workgroup barrier:
//
// Sweep. Row r of a pass of 256 rows is lane r / 4 of wave r % 4, so a 64-row tile gives every wave 16
// rows. A row of at most `split` bytes is swept by its lane, 8 bytes a step, the wave's lanes in
// lockstep; a longer row goes onto a list (the row table's `src` words) and is swept by one wave, 64
// consecutive 8-byte words of the current element a step. A lane turns its 8 bytes into the masks w
// (word bytes) and iso (isolated bytes; a byte in both sets is a delimiter, bytes at or past the
// element's end are delimiters) and, with the top w bit of the byte before (its own carry; in a wave
// the neighbour's, by __shfl_up), into start bits w & ~prev and end bits ~w & prev: an end bit marks the
// byte AFTER a run, so no lane looks ahead. The words that a lane finishes are the runs that end in its
// 8 bytes and its isolated bytes, in byte order (a run that ends at an isolated byte comes before it):
// 9 at the most. A run's start is the highest start bit below its end, else the start carried into the
// lane (in a wave: an exclusive max-scan of the lanes' last starts). A wave prefix sum of the lanes'
// counts places the words in the wave's queue as (byte offset, length | row slot << 16), in row and
// byte order; the queue holds the 576 words a step can finish, and is drained after every step.
//
// Match. The wave drains its queue with a group of G = kWpG lanes per word, 64 / G words a round. For
// the current pos of a word of L bytes, lane j of the group takes the end hi - j, hi = min(L, pos + the
// longest word of the table in use), hashes s[pos:end] (8 bytes a step, the lanes of the group reading
// the same dwords in lockstep) and probes its candidate; a ballot restricted to the group picks the
// lowest j that hit, i.e. the longest piece. Without a hit the group steps down by G ends; no end left
// makes the whole word unk. A word of the vocabulary is settled in one probe latency, an uncovered word
// of L bytes in ceil(L / G), not L.
//
// Emit. The pieces of a word are held back in its group's registers (lane j: pieces j and j + G; the
// word indices, not the ids) until the word is finished, because unk discards them. A word's output
// index is its row's running count (per wave in LDS, one word per row slot) plus the pieces of the words
// of the same row before it in the round (shuffles over the groups' counts); then lane j stores pieces j
// and j + G. A word of more than kWpStage pieces is matched a second time with its base known, and the
// pieces past the stage are stored as they are found. k_wp_count runs the same sweep and match without
// the stage and without reading an id.
//
// Not read: in k_wp_write the rows without a piece and, without counters, the rows whose first piece
// lies at or past tok_cap; in both passes the bytes of a row after its limit is reached.
#include <hip/hip_runtime.h>

#include "tfrg_elem_rows.h"
#include "tfrg_ids_dev.h"
#include "tfrg_internal.h"
#include "tfrg_tokens.h"
#include "tfrg_vocab.h"
#include "tfrg_wordpiece.h"

namespace tfrg {
namespace {

constexpr uint32_t kBlk = kElemBlk;
constexpr uint32_t kWaves = kBlk / 64;
constexpr uint32_t kG = kWpG;
constexpr uint32_t kWords = 64 / kG;     // words a wave matches in a round
constexpr uint32_t kSt = kWpStage / kG;  // staged pieces per lane

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) WpArgs* KArgs;
typedef const __attribute__((address_space(4))) WpSpec* KSpec;
typedef const __attribute__((address_space(4))) WpTab* KTab;

// the spec a workgroup works in (uniform), with the fields tfrg_elem_rows.h reads (tfrg_tokens.hip's Sp
// over WpArgs: that file stays as it is, so the three small functions stand here a second time)
struct Sp {
  static constexpr uint32_t kNoLen = kWpNoLen;
  KArgs a;
  KSpec s;
  const uint32_t* rs;
  uint64_t base;
  uint32_t max_elems;
  bool by_end;
  RowList rl;
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
  x.by_end = !a->b_off64 && s->const_off != kWpOffStored;
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

// the wave's LDS accesses so far are done before any lane goes on (a wave runs in lockstep: no s_barrier)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A wave's share of the static LDS: the word queue, and per row slot (lane-swept rows: the lane; a
// wave-swept row: slot 0) the row's running piece count, the count at which it stops, and its output base
struct WaveLds {
  uint32_t off[kWpQueue];   // the word's first byte in the bytes' source
  uint32_t meta[kWpQueue];  // its length (0xffff: that or more) | row slot << 16
  uint64_t base[64];
  uint32_t cnt[64];
  uint32_t lim[64];
};

// What a pass reads and writes with (uniform)
struct Ctx {
  KSpec ks;
  Src in, blob_first, blob_cont;
  uint64_t d0, d1, i0, i1;
  int64_t* out;
  uint64_t ecap;  // ids that are stored: out ? tok_cap : 0
  uint32_t mwb;
  bool lower, has_cont;
};

__device__ __forceinline__ Src blob_src(KTab t) {
  return Src{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(t->blob), (short)0, (int)t->blob_bound, 0x00020000),
             t->blob_bound};
}

__device__ __forceinline__ Ctx make_ctx(KArgs a, KSpec ks, bool emit) {
  Ctx m;
  m.ks = ks;
  m.in = Src{bytes_source(a), a->in_bound};
  m.blob_first = blob_src(&ks->first);
  m.blob_cont = blob_src(&ks->cont);
  m.d0 = ks->delims[0];
  m.d1 = ks->delims[1];
  m.i0 = ks->isolate[0];
  m.i1 = ks->isolate[1];
  m.out = emit ? ks->ids : nullptr;
  m.ecap = m.out ? ks->tok_cap : 0ull;
  m.mwb = ks->max_word_bytes;
  m.lower = ks->lower != 0u;
  m.has_cont = ks->cont.table != nullptr;
  return m;
}

// ------------------------------------------------------------------ sweep
// bit i of w: byte i of the 8 is a word byte; of iso: it is a word of its own. Bytes at or past `valid`
// are delimiters.
__device__ __forceinline__ void byte_masks(const Ctx& m, uint64_t x, uint32_t valid, uint32_t& w, uint32_t& iso) {
  uint32_t wm = 0, im = 0;
#pragma unroll
  for (uint32_t i = 0; i < 8; ++i) {
    const uint32_t b = (uint32_t)(x >> (8u * i)) & 0xffu;
    const uint32_t ascii = b < 128u ? 1u : 0u;
    const uint32_t d = (uint32_t)(((b & 64u) ? m.d1 : m.d0) >> (b & 63u)) & ascii;
    const uint32_t is = (uint32_t)(((b & 64u) ? m.i1 : m.i0) >> (b & 63u)) & ascii & (d ^ 1u);
    wm |= ((d | is) ^ 1u) << i;
    im |= is << i;
  }
  const uint32_t keep = valid >= 8u ? 0xffu : (1u << valid) - 1u;
  w = wm & keep;
  iso = im & keep;
}

// the masks of 8-byte word k of the element (off, L); k <= L / 8, the word of position L included
__device__ __forceinline__ void word_masks(const Ctx& m, uint32_t off, uint32_t L, uint32_t k, uint32_t& w, uint32_t& iso) {
  const uint32_t valid = L - (k << 3);
  w = iso = 0u;
  if (valid) byte_masks(m, word8(m.in, off, L, k), valid, w, iso);
}

// the 8 bits of m to the even bits of 16
__device__ __forceinline__ uint32_t spread8(uint32_t m) {
  m = (m | (m << 4)) & 0x0f0fu;
  m = (m | (m << 2)) & 0x3333u;
  return (m | (m << 1)) & 0x5555u;
}

// The words a lane finishes, into the queue from position `at` on: the runs that end at an end bit of e
// (start: the highest bit of s below the end, else ost, the start of the run open on entry) and the
// isolated bytes of iso, in byte order, a run before the isolated byte that ends it. pos: the first of
// the lane's 8 bytes, relative to the element at eoff.
__device__ __forceinline__ void push_words(WaveLds& q, uint32_t at, uint32_t eoff, uint32_t pos, uint32_t s, uint32_t e,
                                           uint32_t iso, uint32_t ost, uint32_t slot) {
  uint32_t x = spread8(e) | (spread8(iso) << 1);
  while (x) {
    const uint32_t b = (uint32_t)__builtin_ctz(x);
    x &= x - 1u;
    const uint32_t i = b >> 1;
    uint32_t st = pos + i, len = 1u;
    if (!(b & 1u)) {
      const uint32_t below = s & ((1u << i) - 1u);
      st = below ? pos + (31u - (uint32_t)__builtin_clz(below)) : ost;
      len = pos + i - st;
    }
    // (a start past 2^32 lies past the bound, where every byte reads as zero)
    const uint64_t a = (uint64_t)eoff + st;
    q.off[at] = a < 0xffffffffull ? (uint32_t)a : 0xffffffffu;
    q.meta[at] = (len < 0xffffu ? len : 0xffffu) | (slot << 16);
    ++at;
  }
}

// ------------------------------------------------------------------ match
// tfrg_hash64 of the (lowered) string (a, len) of the input
__device__ __forceinline__ uint64_t hash_of(const Ctx& m, uint32_t a, uint32_t len) {
  uint64_t h = kHashSeed;
  const uint32_t nw = words_of(len);
#pragma unroll 1
  for (uint32_t k = 0; k < nw; ++k) {
    uint64_t w = word8(m.in, a, len, k);
    if (m.lower) w = lower8(w);
    h = hash_step(h, w);
  }
  return hash_finish(h, (uint64_t)len);
}

// One word (off, L) cut into pieces by its group (every lane of the group calls with the same word; j:
// the lane in the group, gmask: the group's lanes). n: its pieces (1 for unk), unk: it became unk_id.
// STAGE: lane j keeps the word indices of pieces j, j + G, ... below kWpStage in st. DIRECT: the word is
// known not to be unk and its pieces from kWpStage on are stored as they are found: piece i at dbase + i
// where i < dlim and the position is below ecap.
template <bool STAGE, bool DIRECT>
__device__ __forceinline__ void match_word(const Ctx& m, uint32_t off, uint32_t L, uint32_t j, uint64_t gmask, uint32_t& n,
                                           bool& unk, uint32_t (&st)[kSt], uint64_t dbase, uint32_t dlim) {
  n = 0u;
  unk = L > m.mwb;
  uint32_t pos = 0;
  while (!unk && pos < L) {
    const bool first = pos == 0u;
    if (!first && !m.has_cont) {
      unk = true;
      break;
    }
    const uint32_t mw = first ? m.ks->first.max_word : m.ks->cont.max_word;
    uint32_t rem = L - pos < mw ? L - pos : mw;  // the ends not yet tried: pos + 1 .. pos + rem
    const uint64_t a64 = (uint64_t)off + pos;
    const uint32_t a = a64 < 0xffffffffull ? (uint32_t)a64 : 0xffffffffu;
    bool found = false;
    while (rem && !found) {
      uint32_t hit = kVocabEmpty;
      if (j < rem) {
        const uint32_t len = rem - j;
        const uint64_t hv = hash_of(m, a, len);
        if (first)
          hit = m.lower ? probe<true>(&m.ks->first, m.in, m.blob_first, a, len, hv)
                        : probe<false>(&m.ks->first, m.in, m.blob_first, a, len, hv);
        else
          hit = m.lower ? probe<true>(&m.ks->cont, m.in, m.blob_cont, a, len, hv)
                        : probe<false>(&m.ks->cont, m.in, m.blob_cont, a, len, hv);
      }
      const uint64_t hits = __ballot(hit != kVocabEmpty) & gmask;
      if (hits) {
        const uint32_t win = (uint32_t)__builtin_ctzll(hits);  // the lowest j: the longest piece
        const uint32_t w = (uint32_t)__shfl((int)hit, (int)win, 64);
        pos += rem - (win & (kG - 1u));
        if constexpr (STAGE) {
#pragma unroll
          for (uint32_t t = 0; t < kSt; ++t)
            if (n == t * kG + j) st[t] = w;
        }
        if constexpr (DIRECT) {
          if (j == 0u && n >= kWpStage && n < dlim && dbase + n < m.ecap)
            m.out[dbase + n] = (first ? m.ks->first.w_ids : m.ks->cont.w_ids)[w];
        }
        ++n;
        found = true;
      } else {
        rem = rem > kG ? rem - kG : 0u;
      }
    }
    if (!found) unk = true;
  }
  if (unk) n = 1u;
}

// The wave's queue of nq words (uniform) matched, counted into their rows and, with EMIT, stored
template <bool EMIT>
__device__ __forceinline__ void drain(const Ctx& m, WaveLds& q, uint32_t nq, uint32_t& unks) {
  const uint32_t lane = threadIdx.x & 63u, g = lane / kG, j = lane & (kG - 1u);
  const uint64_t gmask = (kG == 64u ? ~0ull : (1ull << kG) - 1ull) << (g * kG);
  for (uint32_t h0 = 0; h0 < nq; h0 += kWords) {
    const uint32_t qi = h0 + g;
    uint32_t off = 0, L = 0, slot = 0, c0 = 0, lim = 0;
    if (qi < nq) {
      off = q.off[qi];
      const uint32_t meta = q.meta[qi];
      L = meta & 0xffffu;
      slot = meta >> 16;
      c0 = q.cnt[slot];
      lim = q.lim[slot];
    }
    const bool act = c0 < lim;  // (false without a word: lim 0)
    uint32_t n = 0, st[kSt];
    bool unk = false;
#pragma unroll
    for (uint32_t t = 0; t < kSt; ++t) st[t] = 0u;
    if (act) match_word<EMIT, false>(m, off, L, j, gmask, n, unk, st, 0ull, 0u);
    // the word's index in its row: the pieces of the round's earlier words of the same row before it
    uint32_t idx = c0, tot = 0;
#pragma unroll
    for (uint32_t d = 0; d < kWords; ++d) {
      const uint32_t sl = (uint32_t)__shfl((int)slot, (int)(d * kG), 64);
      const uint32_t nn = (uint32_t)__shfl((int)n, (int)(d * kG), 64);
      if (sl == slot) {
        tot += nn;
        if (d < g) idx += nn;
      }
    }
    if (act && j == 0u) q.cnt[slot] = c0 + tot;  // (every group of the row writes the same sum)
    if constexpr (EMIT) {
      if (act && idx < lim) {
        if (unk && j == 0u) ++unks;
        const uint64_t base = q.base[slot] + idx;
        const uint32_t left = lim - idx;
#pragma unroll
        for (uint32_t t = 0; t < kSt; ++t) {
          const uint32_t i = t * kG + j;
          if (i < n && i < left && base + i < m.ecap)
            m.out[base + i] = unk ? m.ks->unk_id : (i ? m.ks->cont.w_ids : m.ks->first.w_ids)[st[t]];
        }
        if (n > kWpStage && left > kWpStage && base + kWpStage < m.ecap) {
          uint32_t n2;
          bool unk2;
          match_word<false, true>(m, off, L, j, gmask, n2, unk2, st, base, left);
        }
      }
    }
    wave_sync();  // (the rows' counts are in place before the next round or the sweep reads them)
  }
}

// The words of a step into the queue and matched: nw words of this lane, whose masks are s, e, iso
template <bool EMIT>
__device__ __forceinline__ void step_words(const Ctx& m, WaveLds& q, uint32_t nw, uint32_t eoff, uint32_t pos, uint32_t s,
                                           uint32_t e, uint32_t iso, uint32_t ost, uint32_t slot, uint32_t& unks) {
  const uint32_t inc = wave_incl_scan(nw);
  const uint32_t tot = rfl32((uint32_t)__shfl((int)inc, 63, 64));
  if (!tot) return;
  push_words(q, inc - nw, eoff, pos, s, e, iso, ost, slot);
  wave_sync();
  drain<EMIT>(m, q, tot, unks);
}

// The wave's lanes sweep one row each (every lane calls; mine: the lane has a row, whose slot is the
// lane: cnt 0, lim and, with EMIT, base are in place). A row is left once its count has reached lim.
template <bool EMIT>
__device__ __forceinline__ void rows_by_lane(const Sp& x, const Ctx& m, WaveLds& q, bool mine, const Row& w, uint32_t& unks) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t j = 0, k = 0, nwd = 0, L = 0, off = 0, pv = 0, ost = 0;
  bool live = mine;
  while (__ballot(live)) {
    if (live && k == nwd) {  // the next element that has a byte
      L = 0u;
      while (j < w.cnt && !(L = elem_L(x, w.src, j))) ++j;
      live = L != 0u;
      if (live) {
        off = elem_off(x, w.src, j);
        nwd = (L >> 3) + 1u;
        k = pv = ost = 0u;
        ++j;
      }
    }
    uint32_t wm = 0, iso = 0, s = 0, e = 0;
    const uint32_t pos = k << 3;
    if (live) {
      word_masks(m, off, L, k, wm, iso);
      const uint32_t prev = ((wm << 1) | pv) & 0xffu;
      s = wm & ~prev;
      e = ~wm & prev & 0xffu;
    }
    step_words<EMIT>(m, q, (uint32_t)__builtin_popcount(e) + (uint32_t)__builtin_popcount(iso), off, pos, s, e, iso, ost, lane,
                     unks);
    if (live) {
      if (s) ost = pos + (31u - (uint32_t)__builtin_clz(s));
      pv = wm >> 7;
      ++k;
      live = q.cnt[lane] < q.lim[lane];
    }
  }
}

// One wave sweeps one row (every argument uniform), 64 words a step; its slot is 0. Returns its count.
template <bool EMIT>
__device__ __forceinline__ uint32_t row_by_wave(const Sp& x, const Ctx& m, WaveLds& q, const Row& w, uint32_t lim, uint64_t base,
                                                uint32_t& unks) {
  const uint32_t lane = threadIdx.x & 63u;
  if (lane == 0u) {
    q.cnt[0] = 0u;
    q.lim[0] = lim;
    q.base[0] = base;
  }
  wave_sync();
  for (uint32_t j = 0; j < w.cnt; ++j) {
    const uint32_t L = rfl32(elem_L(x, w.src, j));
    if (!L) continue;
    const uint32_t off = rfl32(elem_off(x, w.src, j)), nwd = (L >> 3) + 1u;
    uint32_t carry = 0, ost1 = 0;  // the run open across the step: its top bit, its start + 1
    for (uint32_t k0 = 0; k0 < nwd; k0 += 64u) {
      const uint32_t k = k0 + lane, pos = k << 3;
      uint32_t wm = 0, iso = 0;
      if (k < nwd) word_masks(m, off, L, k, wm, iso);
      const uint32_t up = (uint32_t)__shfl_up((int)(wm >> 7), 1, 64);
      const uint32_t pv = lane ? up : carry;
      const uint32_t prev = ((wm << 1) | pv) & 0xffu;
      const uint32_t s = wm & ~prev, e = ~wm & prev & 0xffu;
      carry = rfl32((uint32_t)__shfl((int)(wm >> 7), 63, 64));
      // the start (+ 1) of the run open on entry into the lane's 8 bytes: the last start before them
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
      step_words<EMIT>(m, q, (uint32_t)__builtin_popcount(e) + (uint32_t)__builtin_popcount(iso), off, pos, s, e, iso,
                       before - 1u, 0u, unks);
      ost1 = carry ? (last > ost1 ? last : ost1) : 0u;
      const uint32_t c = rfl32(q.cnt[0]);
      if (c >= lim) return c;
    }
  }
  return rfl32(q.cnt[0]);
}

struct Setup {
  Sp x;
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
  return u;
}

// row r0 + i of a pass of kBlk rows is lane i / kWaves of wave i % kWaves: every wave gets its share of a
// tile smaller than the workgroup
__device__ __forceinline__ uint32_t pass_row(uint32_t r0) {
  return r0 + (threadIdx.x & 63u) * kWaves + (threadIdx.x >> 6);
}

// ------------------------------------------------------------------ 1. counts
// dynamic LDS: the row table of tfrg_rows.h (tok_lds_bytes sizes it); src holds the list of long rows
__global__ __launch_bounds__(kBlk) void k_wp_count(const WpArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wp_lds[];
  __shared__ WaveLds wl[kWaves];
  __shared__ uint32_t n_long;
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const Setup u = setup(a, wp_lds);
  const Ctx m = make_ctx(a, u.x.s, false);
  WaveLds& q = wl[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63u, split = a->split;
  // a row is swept until it has one piece more than its limit: that it was cut is then known
  const uint32_t limit = u.x.s->limit, stop = limit == kWpUnbounded ? limit : limit + 1u;
  const uint32_t extra = u.x.s->special ? 2u : 0u;
  int64_t* const ro = u.x.s->row_offsets + u.t0;
  if (threadIdx.x == 0) n_long = 0u;
  __syncthreads();
  uint32_t rtrunc = 0, empty = 0, skip = 0, none = 0;
  uint64_t sum = 0;
  for (uint32_t r0 = 0; r0 < u.nrows; r0 += kBlk) {
    const uint32_t r = pass_row(r0);
    const bool have = r < u.nrows;
    Row w{};
    if (have) w = row_of(u.x, u.t0 + r);
    skip += have ? w.ok ^ 1u : 0u;
    const bool lng = have && w.cnt && !row_short(u.x, w, split);
    if (lng) u.l.src[atomicAdd(&n_long, 1u)] = r;
    const bool mine = have && w.cnt && !lng;
    q.cnt[lane] = 0u;
    q.lim[lane] = mine ? stop : 0u;
    wave_sync();
    rows_by_lane<false>(u.x, m, q, mine, w, none);
    if (have && !lng) {
      const uint32_t c = q.cnt[lane];
      const uint32_t kept = (w.ok ? extra : 0u) + (c < limit ? c : limit);
      rtrunc += c > limit;
      empty += w.ok & (uint32_t)(c == 0u);
      ro[r] = (int64_t)kept;
      sum += kept;
    }
    wave_sync();  // (the slots are read before the next pass resets them)
  }
  __syncthreads();
  const uint32_t nl = n_long;
  for (uint32_t i = threadIdx.x >> 6; i < nl; i += kWaves) {
    const uint32_t r = rfl32(u.l.src[i]);
    const Row w = row_of(u.x, u.t0 + r);
    const uint32_t c = row_by_wave<false>(u.x, m, q, w, stop, 0ull, none);
    if (lane == 0u) {
      const uint32_t kept = extra + (c < limit ? c : limit);  // (a row on the list is not skipped)
      rtrunc += c > limit;
      empty += c == 0u;
      ro[r] = (int64_t)kept;
      sum += kept;
    }
  }
  uint64_t total;
  (void)block_excl_scan<kWaves>(sum, u.l.part, &total);
  if (threadIdx.x == 0) a->tsum[blockIdx.x] = total;
  if (a->stats) add_stats4(a->stats, u.si, rtrunc, 0u, empty, skip);
}

// ------------------------------------------------------------------ 2. tile scan
// one workgroup per spec: the tile sums to their exclusive prefixes, T to row_offsets[m] and the totals
__global__ __launch_bounds__(kWpScanThreads) void k_wp_scan(const WpArgs) {
  __shared__ uint64_t part[kWpScanThreads / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, si = blockIdx.x;
  uint64_t* const tsum = a->tsum + (uint64_t)si * tiles;
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < tiles; b0 += kWpScanThreads) carry = scan_tile_sums<kWpScanThreads>(tsum, tiles, b0, carry, part);
  if (threadIdx.x == 0) {
    a->sp[si].row_offsets[a->m] = (int64_t)carry;
    if (a->totals) a->totals[si] = carry;
  }
}

// ------------------------------------------------------------------ 3. row offsets and ids
// dynamic LDS as k_wp_count
__global__ __launch_bounds__(kBlk) void k_wp_write(const WpArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t wp_lds[];
  __shared__ WaveLds wl[kWaves];
  __shared__ uint32_t n_long;
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const Setup u = setup(a, wp_lds);
  const KSpec ks = u.x.s;
  const uint32_t split = a->split, nrows = u.nrows, lane = threadIdx.x & 63u;
  int64_t* const ro = ks->row_offsets + u.t0;  // (row_offsets[m] is k_wp_scan's)
  const uint64_t eb = a->tsum[blockIdx.x];
  // the counts k_wp_count left in place, to the tile's row table and row offsets (an entry is read and
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
  // the tile's pieces that are stored or counted (uniform)
  uint32_t* const stats = a->stats;
  const Ctx m = make_ctx(a, ks, true);
  const uint64_t lim = stats ? e1 : (m.ecap < e1 ? m.ecap : e1);
  if (lim <= eb) return;
  __syncthreads();
  WaveLds& q = wl[threadIdx.x >> 6];
  const uint32_t extra = ks->special ? 1u : 0u;
  const int64_t cls = ks->cls_id, sep = ks->sep_id;
  uint32_t unks = 0;
  // a row's pieces that are stored or counted, from its first one at *pbase on (cls and sep stored here)
  auto pieces_of = [&](uint32_t r, uint64_t* pbase) -> uint32_t {
    const uint64_t base = u.l.offs[r];
    const uint32_t cnt = (uint32_t)(u.l.offs[r + 1u] - base);
    if (!cnt || base >= lim) return 0u;  // (no piece, or none that is stored or counted: the row is not read)
    if (extra) {
      if (base < m.ecap) m.out[base] = cls;
      if (base + cnt - 1u < m.ecap) m.out[base + cnt - 1u] = sep;
    }
    *pbase = base + extra;
    const uint32_t np = cnt - 2u * extra;
    if (*pbase >= lim) return 0u;
    return lim - *pbase < np ? (uint32_t)(lim - *pbase) : np;
  };
  for (uint32_t r0 = 0; r0 < nrows; r0 += kBlk) {
    const uint32_t r = pass_row(r0);
    uint64_t pbase = 0;
    const uint32_t np = r < nrows ? pieces_of(r, &pbase) : 0u;
    Row w{};
    if (np) w = row_of(u.x, u.t0 + r);
    const bool lng = np && !row_short(u.x, w, split);
    if (lng) u.l.src[atomicAdd(&n_long, 1u)] = r;
    const bool mine = np && !lng;
    q.cnt[lane] = 0u;
    q.lim[lane] = mine ? np : 0u;
    q.base[lane] = pbase;
    wave_sync();
    rows_by_lane<true>(u.x, m, q, mine, w, unks);
    wave_sync();
  }
  __syncthreads();
  const uint32_t nl = n_long;
  for (uint32_t i = threadIdx.x >> 6; i < nl; i += kWaves) {
    const uint32_t r = rfl32(u.l.src[i]);
    // (cls and sep were stored when the row went onto the list: the bounds again, without the stores)
    const uint64_t pbase = u.l.offs[r] + extra;
    const uint32_t npr = (uint32_t)(u.l.offs[r + 1u] - u.l.offs[r]) - 2u * extra;
    const uint32_t np = lim - pbase < npr ? (uint32_t)(lim - pbase) : npr;
    const Row w = row_of(u.x, u.t0 + r);
    (void)row_by_wave<true>(u.x, m, q, w, np, pbase, unks);
  }
  if (stats) add_stats4(stats, u.si, 0u, unks, 0u, 0u);
}

}  // namespace

hipError_t launch_wordpiece(const WpArgs& a, hipStream_t st) {
  const uint32_t per_spec = a.n_specs * a.tiles;
  const size_t lds = tok_lds_bytes(a.tile);
  hipLaunchKernelGGL(k_wp_count, dim3(per_spec), dim3(kBlk), lds, st, a);
  hipLaunchKernelGGL(k_wp_scan, dim3(a.n_specs), dim3(kWpScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_wp_write, dim3(per_spec), dim3(kBlk), lds, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
