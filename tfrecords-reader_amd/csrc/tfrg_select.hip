// tfrg_select.hip — the kernels behind tfrg_result_select_rows / _select_match: the WHERE clause over a decoded batch.
// For a list of m candidates (candidate k is record g = entry(k) - row0) and a table of terms (AND of
// OR-groups), the entries of the candidates that pass, compacted in candidate order. Three launches on
// the decode's stream, no workgroup ever waiting on another (the shape of k_rg_len / k_rg_scan /
// k_rg_gather in tfrg_ragged.hip; what it shares with the other row-list passes is in tfrg_rows.h):
//
//   k_sel_eval   per tile of `tile` candidates, a wave per 64 consecutive candidates: every term in a
//                uniform loop over the table, each lane gathering the groups that hold a true term for
//                its candidate; the verdicts of the 64 lanes as one ballot word into words[] (lane 0,
//                one vector store), the tile's popcount into tsum[tile], the skipped candidates into
//                stats[1] (at most one atomic per wave);
//   k_sel_scan   one workgroup: the tile sums to their first positions, from *count under APPEND and
//                from 0 otherwise, carrying across passes of kSelScanThreads tiles; *count and stats[0];
//   k_sel_write  per tile: its ballot words alone (no predicate is evaluated again, and no column is
//                read), one wave scan of their popcounts, and for every set bit the entry -- the only
//                read of the row list here -- stored at tile base + word base + the set bits below it,
//                where that is below cap.
//
// Positions come from the scan alone: no atomic and no order of workgroups enters them, so two calls
// over the same inputs write the same bytes.
//
// Not read (as k_dense and k_rg_*): the row splits of a placed slot (info words kInfoPlacedLo / Hi: the
// record has one value, at index g), the bytes_len column of a slot whose length is constant
// (SelTerm::const_len), the status column where every status is 0 (SelectArgs::status null). A
// candidate whose g is not in [0, n) loads nothing indexed by g (it reads record 0 and drops it).
//
// Bytes terms (kSelBytes / kSelBytesAny: an element of a bytes_list slot against a byte-string operand)
// live in a second instantiation of k_sel_eval, launched only when the term table holds one; the
// operands travel in its kernel argument. EQ .. GE, PREFIX and SUFFIX read at most the pattern's length
// of an element, one lane per candidate; CONTAINS walks a short element in its lane and streams a long
// one through LDS with the whole wave (wave_contains).
#include <hip/hip_runtime.h>

#include "tfrg_internal.h"
#include "tfrg_rows.h"
#include "tfrg_select.h"

namespace tfrg {
namespace {

constexpr uint32_t kBlk = 256;
constexpr uint32_t kWaves = kBlk / 64;

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) SelectArgs* KArgs;
typedef const __attribute__((address_space(4))) SelTerm* KTerm;

__device__ __forceinline__ bool sel_cmp(int64_t a, int64_t b, uint32_t op) {
  switch (op) {
    case kSelEq: return a == b;
    case kSelNe: return a != b;
    case kSelLt: return a < b;
    case kSelLe: return a <= b;
    case kSelGt: return a > b;
    default: return a >= b;
  }
}

// entry k < m of the candidate list
__device__ __forceinline__ int64_t entry_of(KArgs a, uint32_t k) {
  const uint8_t* const rows = static_cast<const uint8_t*>(a->rows);
  if (!rows) return (int64_t)k;
  if (a->rows64) return *reinterpret_cast<const int64_t*>(rows + ((uint64_t)k << 3));
  return (int64_t)*reinterpret_cast<const int32_t*>(rows + ((uint64_t)k << 2));
}

// value i of a value array against the term (float slots: by value, NaN apart)
__device__ __forceinline__ bool value_term(KArgs a, KTerm t, uint64_t i) {
  if (t->is_float) {
    const uint32_t u = a->f32[i];
    if (sel_float_nan(u) || t->rhs_nan) return t->op == kSelNe;
    return sel_cmp(sel_float_key(u), t->rhs, t->op);
  }
  return sel_cmp(a->i64[i], t->rhs, t->op);
}

// term t for record g (ok: g is a record; else everything indexed by g is taken from record 0 and dropped)
__device__ __forceinline__ bool eval_term(KArgs a, KTerm t, uint64_t placed, uint32_t g, bool ok) {
  const uint32_t subject = t->subject;
  if (subject == kSelStatus) {
    const int64_t st = a->status ? (int64_t)a->status[g] : 0;
    return ok && sel_cmp(st, t->rhs, t->op);
  }
  const uint32_t slot = t->slot;
  uint32_t lo = g, c = 1u;
  if (!(slot < 64u && ((placed >> slot) & 1ull))) {
    const uint32_t* const rs = a->rs + (uint64_t)slot * ((uint64_t)a->n + 1u);
    lo = rs[g];
    c = rs[g + 1u] - lo;
  }
  c = ok ? c : 0u;  // (a skipped candidate is a record without a value to everything that loads)
  const uint64_t base = a->slot_base[slot];
  switch (subject) {
    case kSelValue: {
      // (a record without value `index` reads element 0 of the array and drops it)
      const bool has = c > t->index;
      const bool v = value_term(a, t, has ? base + lo + t->index : 0ull);
      return has && v;
    }
    case kSelAny: {
      bool any = false;
      for (uint32_t j = 0; j < c && !any; ++j) any = value_term(a, t, base + lo + j);
      return any;
    }
    case kSelCount: return ok && sel_cmp((int64_t)c, t->rhs, t->op);
    default: {  // kSelBytesLen: the length of element 0, as row_of of tfrg_ragged.hip
      const uint64_t es = c ? base + lo : 0ull;
      uint32_t len;
      if (t->const_len != kSelNoLen) {
        len = t->const_len;
      } else if (a->b_off64) {
        const uint64_t l = a->b_off64[es + 1] - a->b_off64[es];
        len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
      } else {
        len = a->b_len[es];
      }
      return ok && sel_cmp((int64_t)(c ? len : 0u), t->rhs, t->op);
    }
  }
}

// ------------------------------------------------------------------ bytes terms (kSelBytes / kSelBytesAny)
// An element is the bytes [off, off + len) of the bytes' source, read through a buffer resource bounded
// to in_bound: a byte at or past it is 0 and no memory is touched for it (tfrg_ragged.hip in_byte). The
// pattern is read from the kernel argument with scalar loads: every loop over it runs in lockstep over
// the wave, each lane holding its own element and a flag that says whether it still takes part. A lane
// whose flag is down loads nothing (its buffer offset is past the bound).
typedef const __attribute__((address_space(4))) SelectBytesArgs* KBytes;
typedef uint32_t sel_u32x4 __attribute__((ext_vector_type(4)));

// CONTAINS over a long element, by its wave: chunks of kScanChunk bytes from a 16-byte boundary on go
// through the wave's LDS stage, behind the kScanCarry bytes that came before them
constexpr uint32_t kScanCarry = kSelMaxPattern, kScanChunk = 2048;
constexpr uint32_t kScanStage = kScanCarry + kScanChunk + 16;  // bytes per wave (the tail: dword pairs read past a position)
static_assert(kScanCarry == 256 && kScanChunk % 1024 == 0 && kSelMaxPattern - 1 <= kScanCarry, "one dword per lane carries");

struct BSrc {
  KBytes b;
  __amdgpu_buffer_rsrc_t in;
  uint32_t* stage;  // the wave's LDS stage
  uint32_t lane;
};

__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// bytes j .. j + 3 of the pattern that starts at byte poff of the operands (uniform)
__device__ __forceinline__ uint32_t pat_word(KBytes b, uint32_t poff, uint32_t j) {
  const uint32_t p = poff + j;
  const uint32_t lo = b->pat[p >> 2], hi = b->pat[(p >> 2) + 1u];
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (p & 3u)));
}

// the low nb bytes of a word (nb >= 1)
__device__ __forceinline__ uint32_t low_bytes(uint32_t nb) { return nb >= 4u ? 0xffffffffu : (1u << (8u * nb)) - 1u; }

// source bytes p .. p + 3: two aligned dwords recombined (tfrg_ragged.hip u8_dword); go down: nothing is loaded
__device__ __forceinline__ uint32_t in_word(const BSrc& x, uint64_t p, bool go) {
  const bool ok = go && p < x.b->in_bound;
  const uint32_t p0 = ok ? ((uint32_t)p & ~3u) : 0xfffffff8u;  // (in_bound <= 0xfffffff0: p0 + 4 does not wrap)
  const uint32_t d0 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0, 0, 0);
  const uint32_t d1 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0 + 4u, 0, 0);
  return __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)p & 3u);
}

// The sign of the first difference between the source bytes [p, p + ncmp) and the first ncmp <= plen
// bytes of the pattern, as unsigned bytes; 0: none (also for a lane with act down)
__device__ __forceinline__ int32_t cmp_pat(const BSrc& x, uint64_t p, uint32_t ncmp, uint32_t poff, uint32_t plen, bool act) {
  int32_t diff = 0;
  ncmp = act ? ncmp : 0u;
  for (uint32_t j = 0; j < plen; j += 4u) {
    const bool go = diff == 0 && j < ncmp;
    if (__ballot(go) == 0ull) break;
    const uint32_t pw = pat_word(x.b, poff, j);
    const uint32_t w = in_word(x, p + j, go);
    const uint32_t mask = low_bytes(go ? ncmp - j : 4u);
    // (the first byte in the top bits: the words compare as the byte strings do)
    const uint32_t el = __builtin_bswap32(w & mask), pt = __builtin_bswap32(pw & mask);
    if (go) diff = (int32_t)(el > pt) - (int32_t)(el < pt);
  }
  return diff;
}

// CONTAINS for the element [off, off + len) (uniform; len >= plen >= 1), by the whole wave
__device__ __forceinline__ bool wave_contains(const BSrc& x, uint32_t off, uint32_t len, uint32_t poff, uint32_t plen) {
  uint32_t* const st = x.stage;
  const uint32_t lane = x.lane;
  const uint32_t in_bound = x.b->in_bound;
  const uint32_t pw0 = pat_word(x.b, poff, 0u), m0 = low_bytes(plen);
  const uint64_t end = (uint64_t)off + len;
  uint64_t q = off;  // the next start position to test
  bool hit = false;
  // source bytes [A, A + kScanChunk): 16 bytes per lane and load
  constexpr uint32_t H = kScanChunk / 1024u;
  sel_u32x4 v[H];
  auto fetch = [&](uint64_t A) {
#pragma unroll
    for (uint32_t h = 0; h < H; ++h) {
      const uint64_t pos = A + h * 1024u + lane * 16u;
      const uint32_t vo = pos < in_bound ? (uint32_t)pos : 0xfffffff0u;  // (in_bound is a multiple of 16)
      v[h] = __builtin_bit_cast(sel_u32x4, __builtin_amdgcn_raw_buffer_load_b128(x.in, vo, 0, 0));
    }
  };
  fetch(off & ~15u);
  for (uint64_t A = off & ~15u; A < end && !hit; A += kScanChunk) {
    // the chunk to stage bytes [kScanCarry, + kScanChunk); the next one's loads fly while this one is searched
#pragma unroll
    for (uint32_t h = 0; h < H; ++h) *reinterpret_cast<sel_u32x4*>(st + ((kScanCarry + h * 1024u + lane * 16u) >> 2)) = v[h];
    wave_lds_order();
    if (A + kScanChunk < end) fetch(A + kScanChunk);
    const uint64_t avail = A + kScanChunk < end ? A + kScanChunk : end;  // the element's bytes staged so far
    if (avail >= q + plen) {
      // start positions q .. avail - plen, as stage positions (stage byte 0 is source byte A - kScanCarry;
      // q > A - kScanCarry: at most plen - 1 bytes before the chunk are still needed)
      const uint32_t p_lo = (uint32_t)(q + kScanCarry - A), p_hi = (uint32_t)(avail - plen + kScanCarry - A);
      for (uint32_t d0 = p_lo & ~3u; d0 <= p_hi && !hit; d0 += 256u) {
        // a lane takes the four positions of one aligned dword: the first pattern word against them
        const uint32_t pd = d0 + lane * 4u;
        uint32_t cand = 0;
        if (pd <= p_hi) {
          const uint32_t w0 = st[pd >> 2], w1 = st[(pd >> 2) + 1u];
#pragma unroll
          for (uint32_t r = 0; r < 4u; ++r) {
            const uint32_t w = __builtin_amdgcn_alignbyte(w1, w0, r);
            if (((w ^ pw0) & m0) == 0u && pd + r >= p_lo && pd + r <= p_hi) cand |= 1u << r;
          }
        }
        if (plen > 4u) {
          // the rest of the pattern for the positions that are left, in lockstep over its words
          for (uint32_t r = 0; r < 4u; ++r) {
            bool go = (cand >> r) & 1u;
            for (uint32_t j = 4u; j < plen; j += 4u) {
              if (__ballot(go) == 0ull) break;
              const uint32_t pw = pat_word(x.b, poff, j);
              const uint32_t i = go ? (pd + j) >> 2 : 0u;
              const uint32_t w = __builtin_amdgcn_alignbyte(st[i + 1u], st[i], r);
              if ((w ^ pw) & low_bytes(plen - j)) go = false;
            }
            if (!go) cand &= ~(1u << r);
          }
        }
        hit = __ballot(cand != 0u) != 0ull;
      }
      q = avail - plen + 1u;
    }
    // the chunk's last kScanCarry bytes become the bytes before the next chunk
    const uint32_t c = st[(kScanChunk >> 2) + lane];
    wave_lds_order();
    st[lane] = c;
    wave_lds_order();
  }
  return hit;
}

// CONTAINS per lane: a short element is walked by its lane, a long one (above scan_min) by the wave
__device__ __forceinline__ bool contains_pat(const BSrc& x, uint32_t off, uint32_t len, uint32_t poff, uint32_t plen, bool act) {
  if (plen == 0u) return act;
  act = act && len >= plen;
  const bool coop = act && len > x.b->scan_min;
  const bool mine = act && !coop;
  const uint32_t last = mine ? len - plen : 0u;
  bool found = false;
  for (uint32_t i = 0;; ++i) {
    const bool go = mine && !found && i <= last;
    if (__ballot(go) == 0ull) break;
    const int32_t d = cmp_pat(x, (uint64_t)off + i, plen, poff, plen, go);
    found = found || (go && d == 0);
  }
  // the wave takes its lanes' long elements one at a time; the verdict goes back to the owning lane
  for (uint64_t pend = __ballot(coop); pend; pend &= pend - 1ull) {
    const uint32_t l = (uint32_t)__builtin_ctzll(pend);
    const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)off, (int)l);
    const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)len, (int)l);
    const bool hit = wave_contains(x, o, n, poff, plen);
    if (x.lane == l) found = hit;
  }
  return found;
}

// the element [off, off + len) against the term's pattern (act down: false, nothing loaded)
__device__ __forceinline__ bool elem_term(const BSrc& x, uint32_t op, uint32_t off, uint32_t len, uint32_t poff, uint32_t plen,
                                          bool act) {
  if (op == kSelContains) return contains_pat(x, off, len, poff, plen, act);
  // at most plen bytes of the element are read, whatever its size
  uint64_t p = off;
  uint32_t ncmp = len < plen ? len : plen;
  if (op == kSelEq || op == kSelNe) ncmp = len == plen ? ncmp : 0u;  // (decided by the lengths)
  if (op == kSelPrefix || op == kSelSuffix) ncmp = len >= plen ? ncmp : 0u;
  if (op == kSelSuffix && len >= plen) p += len - plen;
  const int32_t d = cmp_pat(x, p, ncmp, poff, plen, act);
  bool r;
  switch (op) {
    case kSelEq: r = d == 0 && len == plen; break;
    case kSelNe: r = !(d == 0 && len == plen); break;
    case kSelLt: r = d < 0 || (d == 0 && len < plen); break;  // (a proper prefix is less)
    case kSelLe: r = d < 0 || (d == 0 && len <= plen); break;
    case kSelGt: r = d > 0 || (d == 0 && len > plen); break;
    case kSelGe: r = d > 0 || (d == 0 && len >= plen); break;
    default: r = d == 0 && len >= plen; break;  // kSelPrefix, kSelSuffix
  }
  return act && r;
}

// bytes term number ti for record g: element `index` (kSelBytes), or any element (kSelBytesAny)
__device__ __forceinline__ bool bytes_term(const BSrc& x, KArgs a, KTerm t, uint32_t ti, uint64_t placed, uint32_t g, bool ok) {
  const uint32_t slot = t->slot;
  uint32_t lo = g, c = 1u;
  if (!(slot < 64u && ((placed >> slot) & 1ull))) {
    const uint32_t* const rs = a->rs + (uint64_t)slot * ((uint64_t)a->n + 1u);
    lo = rs[g];
    c = rs[g + 1u] - lo;
  }
  c = ok ? c : 0u;
  const uint64_t base = a->slot_base[slot];
  const uint32_t op = t->op, clen = t->const_len;
  const uint32_t poff = (uint32_t)(uint64_t)t->rhs, plen = (uint32_t)((uint64_t)t->rhs >> 32);
  const int32_t coff = x.b->const_off[ti];
  // the lane's elements [e0, e1) of its list
  const bool any_el = t->subject == kSelBytesAny;
  const uint32_t e0 = any_el ? 0u : t->index;
  const uint32_t e1 = any_el ? c : (c > e0 ? e0 + 1u : e0);
  bool found = false;
  for (uint32_t e = e0;; ++e) {
    const bool act = !found && e < e1;
    if (__ballot(act) == 0ull) break;
    // (a lane without such an element reads element 0's view and drops it, as row_of of tfrg_ragged.hip)
    const uint64_t es = act ? base + lo + e : 0ull;
    uint32_t off, len;
    if (a->b_off64) {
      const uint64_t o0 = a->b_off64[es], l = a->b_off64[es + 1] - o0;
      off = o0 < 0xffffffffull ? (uint32_t)o0 : 0xffffffffu;
      len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
    } else {
      off = coff != kSelOffStored ? x.b->end32[g] + (uint32_t)coff : x.b->b_off[es];
      len = clen != kSelNoLen ? clen : a->b_len[es];
    }
    found = elem_term(x, op, off, len, poff, plen, act) || found;
  }
  return found;
}

// ------------------------------------------------------------------ 1. verdicts
// BYTES: the instantiation for term tables with a bytes term (its argument is a SelectBytesArgs, which
// begins with the SelectArgs); the other one is the kernel as it was before bytes terms existed
template <bool BYTES>
struct EvalArg {
  using type = SelectArgs;
};
template <>
struct EvalArg<true> {
  using type = SelectBytesArgs;
};

// (workgroups of 16 waves for bytes terms: a wave is busy with its 64 candidates for as long as their
// elements are, so a tile's candidates are spread over as many waves as a workgroup can hold)
constexpr uint32_t kBlkBytes = 1024;

template <bool BYTES>
__global__ __launch_bounds__(BYTES ? kBlkBytes : kBlk) void k_sel_eval(const typename EvalArg<BYTES>::type) {
  constexpr uint32_t kBlk = BYTES ? kBlkBytes : tfrg::kBlk;
  constexpr uint32_t kWaves = kBlk / 64;
  __shared__ uint32_t part[kWaves];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const uint32_t m = a->m, n = a->n, tile = a->tile;
  const uint32_t t0 = blockIdx.x * tile;
  const uint32_t t1 = m - t0 < tile ? m : t0 + tile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t placed = placed_slots(a);
  const uint32_t n_terms = a->n_terms, all = a->all_groups;
  const int64_t row0 = a->row0;
  [[maybe_unused]] BSrc x;
  if constexpr (BYTES) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[kWaves][kScanStage / 4];
    x.b = (KBytes)__builtin_amdgcn_kernarg_segment_ptr();
    x.in = bytes_source(x.b);
    x.stage = stage[wave];
    x.lane = lane;
  }
  uint32_t sel = 0, skip = 0;  // (the wave's, kept by every lane alike)
  for (uint32_t w0 = t0 + wave * 64u; w0 < t1; w0 += kBlk) {
    const uint32_t k = w0 + lane;
    const bool live = k < m;
    bool ok = false;
    uint32_t g = 0;
    if (live) {
      // (the row rule of tfrg_rows.h, written out: compared before the subtraction, so no entry wraps
      // into range; rec_of's value pinned in a vector register would change this kernel's code)
      const int64_t v = entry_of(a, k);
      const uint64_t d = (uint64_t)v - (uint64_t)row0;
      ok = v >= row0 && d < (uint64_t)n;
      g = ok ? (uint32_t)d : 0u;
    }
    uint32_t groups = 0;
    for (uint32_t i = 0; i < n_terms; ++i) {
      const KTerm t = &a->term[i];
      bool v;
      if constexpr (BYTES) v = t->subject >= kSelBytes ? bytes_term(x, a, t, i, placed, g, ok) : eval_term(a, t, placed, g, ok);
      else v = eval_term(a, t, placed, g, ok);
      if (v) groups |= 1u << t->group;
    }
    const bool pass = ok && groups == all;
    const uint64_t word = __ballot(pass);
    const uint64_t bad = __ballot(live && !ok);
    if (lane == 0u) a->words[w0 >> 6] = word;
    sel += (uint32_t)__popcll(word);
    skip += (uint32_t)__popcll(bad);
  }
  if (lane == 0u) part[wave] = sel;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kWaves; ++i) s += part[i];
    a->tsum[blockIdx.x] = s;
  }
  if (a->stats && lane == 0u && skip) atomicAdd(a->stats + 1, skip);
}

// ------------------------------------------------------------------ 2. tile scan
// one workgroup: the tile sums to their first positions; *count and the selected counter. (The pass
// is scan_tile_sums of tfrg_rows.h written out: this one adds carry + before + inc - v from the left,
// and block_excl_scan's before + inc - v first would change the kernel's code.)
__global__ __launch_bounds__(kSelScanThreads) void k_sel_scan(const SelectArgs) {
  constexpr uint32_t W = kSelScanThreads / 64;
  __shared__ uint64_t part[W];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles;
  uint64_t* const tsum = a->tsum;
  const uint64_t base = a->append ? *a->count : 0ull;
  uint64_t carry = base;
  for (uint32_t b0 = 0; b0 < tiles; b0 += kSelScanThreads) {
    const uint32_t i = b0 + threadIdx.x;
    const uint64_t v = i < tiles ? tsum[i] : 0ull;
    const uint64_t inc = wave_incl_scan(v);
    const uint32_t w = threadIdx.x >> 6;
    __syncthreads();  // (part may still be read from the pass before)
    if ((threadIdx.x & 63u) == 63u) part[w] = inc;
    __syncthreads();
    uint64_t before = 0, total = 0;
#pragma unroll
    for (uint32_t j = 0; j < W; ++j) {
      const uint64_t s = part[j];
      before += j < w ? s : 0ull;
      total += s;
    }
    if (i < tiles) tsum[i] = carry + before + inc - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *a->count = carry;
    if (a->stats) a->stats[0] = (uint32_t)(carry - base);
  }
}

// ------------------------------------------------------------------ 3. write
__global__ __launch_bounds__(kBlk) void k_sel_write(const SelectArgs) {
  __shared__ uint32_t wbase[kSelTileMax / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t m = a->m, tile = a->tile;
  const uint32_t t0 = blockIdx.x * tile;
  const uint32_t t1 = m - t0 < tile ? m : t0 + tile;
  const uint32_t nw = (t1 - t0 + 63u) >> 6;  // the tile's words: at most 64
  const uint64_t* const words = a->words + (t0 >> 6);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave == 0u) {
    const uint32_t c = lane < nw ? (uint32_t)__popcll(words[lane]) : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o, 64);
      if (lane >= (uint32_t)o) inc += u;
    }
    wbase[lane] = inc - c;
  }
  __syncthreads();
  const uint64_t tbase = a->tsum[blockIdx.x];
  const uint64_t cap = a->cap;
  uint8_t* const out = static_cast<uint8_t*>(a->out);
  const uint32_t out64 = a->out64;
  for (uint32_t wi = wave; wi < nw; wi += kWaves) {
    const uint64_t word = words[wi];
    if (!((word >> lane) & 1ull)) continue;
    const uint64_t pos = tbase + wbase[wi] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
    if (pos >= cap) continue;
    const int64_t v = entry_of(a, t0 + wi * 64u + lane);
    if (out64) *reinterpret_cast<int64_t*>(out + (pos << 3)) = v;
    else *reinterpret_cast<int32_t*>(out + (pos << 2)) = (int32_t)v;
  }
}

}  // namespace

static hipError_t launch_scan_write(const SelectArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(kSelScanThreads), 0, st, a);
  if (a.out && a.cap) hipLaunchKernelGGL(k_sel_write, dim3(a.tiles), dim3(kBlk), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_select(const SelectArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sel_eval<false>, dim3(a.tiles), dim3(kBlk), 0, st, a);
  return launch_scan_write(a, st);
}

hipError_t launch_select_bytes(const SelectBytesArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sel_eval<true>, dim3(a.s.tiles), dim3(kBlkBytes), 0, st, a);
  return launch_scan_write(a.s, st);
}

}  // namespace tfrg
