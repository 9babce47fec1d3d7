// tfrg_ids.hip — the kernels behind tfrg_result_elem_ids: for a list of m rows (row k is record
// g = entry(k) - row0) and every requested bytes_list slot, one int64 id per element of the rows' lists
// (the vocabulary word equal to the element's bytes, else a hash bucket, else a default) and the m + 1
// offsets of the rows in elements. Rows, element order and row_offsets are those of tfrg_elems.hip: both
// files take them from tfrg_elem_rows.h. Three launches on the decode's stream, no workgroup ever waiting
// on another (the row rule, the scans and the row table in LDS are those of tfrg_rows.h):
//
//   k_id_len    per (spec, tile of `tile` rows): the rows' element counts summed (k_el_len without the
//               byte sums: no element is touched), the tile's sum into the scratch, and the three
//               per-row counters;
//   k_id_scan   one workgroup per spec: the tile sums to their exclusive bases, carrying across passes
//               of kIdsScanThreads tiles; row_offsets[m] and the total E;
//   k_id_write  per (spec, tile): the tile's row_offsets; then the tile's elements shared by the lanes
//               as in k_el_len (lane t takes tile-local elements t, t + 256, ... and finds each one's row
//               by a binary search in LDS), kPer of them in flight per lane: the lane folds its element's
//               bytes, read as aligned dwords through the bounded buffer resource, into 8-byte words and
//               those into tfrg_hash64; probes the vocabulary's table in device memory from the home
//               slot; on a candidate compares the length first, then the bytes (8 at a time, both sides
//               through a buffer resource); and stores the id where e < elem_cap. The unmatched elements
//               are tallied per lane: one wave reduction, one atomic per wave.
//
// Cost rules (tfrg.h states them): an element is one lane's work, so a very long element holds its wave
// for its length; an element that can match nothing and needs no bucket (longer than the longest word,
// num_oov_buckets == 0) is not read; without counters, neither are the elements at or past elem_cap.
//
// Not read (as k_el_*): the row splits of a placed slot, the bytes_len column of a slot whose length is
// constant (IdsSpec::const_len), the bytes_off words of a slot the decode left implicit
// (IdsSpec::const_off: the decode's u32 record ends are read in their place), status / aux / verdict /
// order and the numeric columns.
//
// A row whose g is not in [0, n) is an empty row: nothing indexed by g is loaded for it (it reads
// record 0 and drops it), and it counts in the fourth counter alone.
#include <hip/hip_runtime.h>

#include "tfrg_elem_rows.h"
#include "tfrg_ids.h"
#include "tfrg_internal.h"
#include "tfrg_vocab.h"

namespace tfrg {
namespace {

constexpr uint32_t kBlk = kElemBlk;

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) IdsArgs* KArgs;
typedef const __attribute__((address_space(4))) IdsSpec* KSpec;

// the spec a workgroup works in (uniform), with the fields tfrg_elem_rows.h reads
struct Sp {
  static constexpr uint32_t kNoLen = kIdsNoLen;
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
  x.by_end = !a->b_off64 && s->const_off != kIdsOffStored;
  x.rl = make_row_list(a);
  return x;
}

// ------------------------------------------------------------------ 1. counts
// dynamic LDS: the row table of tfrg_rows.h with part [4] u64 (ids_lds_bytes sizes it); only part is used
__global__ __launch_bounds__(kBlk) void k_id_len(const IdsArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t id_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const uint32_t tiles = a->tiles, tile = a->tile;
  const uint32_t si = blockIdx.x / tiles, ti = blockIdx.x - si * tiles;
  const RowTable l = carve_row_table(id_lds, tile);
  const Sp x = make_sp(a, si);
  const uint32_t t0 = ti * tile;
  const uint32_t nrows = a->m - t0 < tile ? a->m - t0 : tile;
  uint32_t rtrunc = 0, empty = 0, skip = 0;
  const uint64_t et = scan_rows<false, true>(x, t0, nrows, 0ull, l, rtrunc, empty, skip);
  if (threadIdx.x == 0) a->tsum[blockIdx.x] = et;
  uint32_t* const stats = a->stats;
  if (!stats) return;
  add_stats4(stats, si, rtrunc, 0u, empty, skip);
}

// ------------------------------------------------------------------ 2. tile scan
// one workgroup per spec: the tile sums to their exclusive prefixes, E to row_offsets[m] and the totals
__global__ __launch_bounds__(kIdsScanThreads) void k_id_scan(const IdsArgs) {
  __shared__ uint64_t part[kIdsScanThreads / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, si = blockIdx.x;
  uint64_t* const tsum = a->tsum + (uint64_t)si * tiles;
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < tiles; b0 += kIdsScanThreads) carry = scan_tile_sums<kIdsScanThreads>(tsum, tiles, b0, carry, part);
  if (threadIdx.x == 0) {
    a->sp[si].row_offsets[a->m] = (int64_t)carry;
    if (a->totals) a->totals[si] = carry;
  }
}

// ------------------------------------------------------------------ 3. row offsets and ids
// A byte string behind a buffer resource: the batch or the materialized column (an element), or the
// vocabulary's blob (a word). Loads at or past `bound` give zeros without a memory access.
struct Src {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t bound;
};

// The k-th 8-byte word of the string of L bytes at byte `off` of the source, k < ceil(L / 8), zero-padded
// after the string's end and reading zeros past the bound: three aligned dwords shifted into place
// (bound <= 0xfffffff0, so p0 + 8 does not wrap)
__device__ __forceinline__ uint64_t word8(const Src& s, uint32_t off, uint32_t L, uint32_t k) {
  const uint64_t p = (uint64_t)off + ((uint64_t)k << 3);
  uint32_t lo = 0u, hi = 0u;
  if (p < s.bound) {
    const uint32_t p0 = (uint32_t)p & ~3u, sh = (uint32_t)p & 3u;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(s.rsrc, p0, 0, 0);
    const uint32_t d1 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(s.rsrc, p0 + 4u, 0, 0);
    const uint32_t d2 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(s.rsrc, p0 + 8u, 0, 0);
    lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
    hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
  }
  const uint32_t rem = L - (k << 3);  // >= 1 bytes of the string from this word on
  if (rem < 8u) {
    lo &= bytes_mask(rem);
    hi &= bytes_mask(rem > 4u ? rem - 4u : 0u);
  }
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t words_of(uint32_t L) { return (L >> 3) + ((L & 7u) != 0u); }

// The word of the vocabulary equal to the element (off, L) whose hash is h: its index, or kVocabEmpty.
// From the home slot over at most max_probe + 1 slots, ending at an empty one; a candidate's length is
// compared first, then its bytes.
__device__ __forceinline__ uint32_t probe(KSpec s, const Src& in, const Src& blob, uint32_t off, uint32_t L, uint64_t h) {
  const uint32_t mask = s->mask, nw = words_of(L);
  uint32_t slot = (uint32_t)h & mask;
#pragma unroll 1
  for (uint32_t d = 0; d <= s->max_probe; ++d, slot = (slot + 1u) & mask) {
    const uint32_t w = s->table[slot];
    if (w == kVocabEmpty) break;
    const uint32_t o0 = s->w_offs[w];
    if (s->w_offs[w + 1u] - o0 != L) continue;
    bool eq = true;
#pragma unroll 1
    for (uint32_t k = 0; k < nw && eq; ++k) eq = word8(in, off, L, k) == word8(blob, o0, L, k);
    if (eq) return w;
  }
  return kVocabEmpty;
}

// dynamic LDS as k_id_len
__global__ __launch_bounds__(kBlk) void k_id_write(const IdsArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t id_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, tile = a->tile;
  const uint32_t si = blockIdx.x / tiles, ti = blockIdx.x - si * tiles;
  const RowTable l = carve_row_table(id_lds, tile);
  const Sp x = make_sp(a, si);
  const KSpec ks = x.s;
  const uint32_t t0 = ti * tile;
  const uint32_t nrows = a->m - t0 < tile ? a->m - t0 : tile;
  const uint64_t eb = a->tsum[blockIdx.x];
  uint32_t u0 = 0, u1 = 0, u2 = 0;
  const uint64_t e1 = scan_rows<true, false>(x, t0, nrows, eb, l, u0, u1, u2);
  int64_t* const ro = ks->row_offsets + t0;  // (row_offsets[m] is k_id_scan's)
  for (uint32_t r = threadIdx.x; r < nrows; r += kBlk) ro[r] = (int64_t)l.offs[r];
  // the tile's elements that are stored or counted (uniform)
  uint32_t* const stats = a->stats;
  int64_t* const out = ks->ids;
  const uint64_t ecap = out ? ks->elem_cap : 0ull;
  const uint64_t lim = stats ? e1 : (ecap < e1 ? ecap : e1);
  if (lim <= eb) return;
  const Src in{bytes_source(a), a->in_bound};
  const bool has_vocab = ks->table != nullptr;
  const Src blob{__builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(ks->blob), (short)0, (int)ks->blob_bound, 0x00020000),
                 ks->blob_bound};
  const uint64_t nb = ks->n_buckets;
  const bool pow2 = (nb & (nb - 1ull)) == 0ull;
  const uint32_t max_word = has_vocab ? ks->max_word : 0u;
  const Tile T{l.offs, l.src, nrows};
  uint32_t unmatched = 0;
  for (uint64_t p0 = eb; p0 < lim; p0 += kPer * kBlk) {
    uint64_t e[kPer], h[kPer];
    uint32_t r[kPer], L[kPer], off[kPer], nw[kPer];
    bool on[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      e[i] = p0 + i * kBlk + threadIdx.x;
      on[i] = e[i] < lim;
      e[i] = on[i] ? e[i] : p0;  // (an element past the tile's reads the pass's first one and drops it)
    }
    rows_at(T, e, r);
    uint32_t steps = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      const uint32_t src = l.src[r[i]], j = (uint32_t)(e[i] - l.offs[r[i]]);
      L[i] = elem_L(x, src, j);
      off[i] = elem_off(x, src, j);
    }
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      // (no bucket to name and no word that long: the element is not read)
      const bool hashed = on[i] && (nb != 0ull || L[i] <= max_word);
      nw[i] = hashed ? words_of(L[i]) : 0u;
      steps = nw[i] > steps ? nw[i] : steps;
      h[i] = kHashSeed;
    }
    // tfrg_hash64 of the kPer elements in lockstep
#pragma unroll 1
    for (uint32_t k = 0; k < steps; ++k) {
      uint64_t w[kPer];
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i) w[i] = k < nw[i] ? word8(in, off[i], L[i], k) : 0ull;
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i) h[i] = k < nw[i] ? hash_step(h[i], w[i]) : h[i];
    }
#pragma unroll 1
    for (uint32_t i = 0; i < kPer; ++i) {
      if (!on[i]) continue;
      const uint64_t hv = hash_finish(h[i], (uint64_t)L[i]);
      uint32_t w = kVocabEmpty;
      if (has_vocab && L[i] <= max_word) w = probe(ks, in, blob, off[i], L[i], hv);
      int64_t id;
      if (w != kVocabEmpty) {
        id = ks->w_ids[w];
      } else {
        ++unmatched;
        id = ks->default_id;
        // (the sum wraps as two's complement: added as unsigned)
        if (nb) id = (int64_t)((uint64_t)ks->oov_base + (pow2 ? hv & (nb - 1ull) : hv % nb));
      }
      if (e[i] < ecap) out[e[i]] = id;
    }
  }
  if (stats) add_stats4(stats, si, 0u, unmatched, 0u, 0u);
}

}  // namespace

hipError_t launch_ids(const IdsArgs& a, hipStream_t st) {
  const uint32_t per_spec = a.n_specs * a.tiles;
  const size_t lds = ids_lds_bytes(a.tile);
  hipLaunchKernelGGL(k_id_len, dim3(per_spec), dim3(kBlk), lds, st, a);
  hipLaunchKernelGGL(k_id_scan, dim3(a.n_specs), dim3(kIdsScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_id_write, dim3(per_spec), dim3(kBlk), lds, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
