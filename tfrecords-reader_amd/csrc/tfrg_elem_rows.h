// tfrg_elem_rows.h — the rows of elements that tfrg_elems.hip and tfrg_ids.hip both walk: a row of the
// output is the first elements of one record's bytes_list, and a tile's rows lie in the row table of
// tfrg_rows.h. Each piece is defined once, as a template over the pass's own Sp (the spec a workgroup
// works in, which make_sp of either file fills); only the names of its fields are assumed:
//   a          the pass's kernel argument (n, b_off64, b_len, b_off, end32)
//   s          the spec in it (const_len, const_off)
//   rs         the slot's row splits; null: placed (record g holds one element, at index g)
//   base       slot_base[slot]
//   max_elems  0: every element of a row
//   by_end     the element of record g lies at end32[g] + const_off
//   rl         the row list (rows null: entry k is k)
//   kNoLen     the const_len that says "the bytes_len column is stored"
// (tfrg_ragged.hip's row_of is another function: it computes value lengths, not element counts.)
#pragma once
#include "tfrg_rows.h"

namespace tfrg {

constexpr uint32_t kElemBlk = 256;  // threads of a workgroup that scans a tile's rows

// One row of the output: its first `cnt` elements, element j being number src + j of the slot's column
// (by_end: src is the record, whose one element lies at its end plus a constant)
struct Row {
  uint32_t cnt;  // after max_elems; 0 for a skipped row
  uint32_t C;    // the record's element count
  uint32_t src;
  uint32_t ok;
};

template <class X>
__device__ __forceinline__ Row row_of(const X& x, uint32_t k) {
  const Rec q = rec_of(x.a, x.rl.row0, x.rl.rows ? row_entry(x.rl, k) : (int64_t)k);
  uint32_t lo = q.g, c = 1u;
  if (x.rs) {
    lo = x.rs[q.g];
    c = x.rs[q.g + 1u] - lo;
  }
  c = q.ok ? c : 0u;  // (a skipped row is a record without an element to everything that loads)
  Row r;
  r.ok = q.ok;
  r.C = c;
  r.cnt = (x.max_elems && c > x.max_elems) ? x.max_elems : c;
  r.src = x.by_end ? q.g : lo;
  return r;
}

// the byte length of element j of the row whose elements start at src
template <class X>
__device__ __forceinline__ uint32_t elem_L(const X& x, uint32_t src, uint32_t j) {
  const uint64_t es = x.base + src + j;
  if (x.a->b_off64) {
    const uint64_t l = x.a->b_off64[es + 1] - x.a->b_off64[es];
    return l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
  }
  return x.s->const_len != X::kNoLen ? x.s->const_len : x.a->b_len[es];
}

// the position of its first byte in the bytes' source
template <class X>
__device__ __forceinline__ uint32_t elem_off(const X& x, uint32_t src, uint32_t j) {
  const uint64_t es = x.base + src + j;
  if (x.a->b_off64) {
    const uint64_t o0 = x.a->b_off64[es];
    return o0 < 0xffffffffull ? (uint32_t)o0 : 0xffffffffu;
  }
  return x.by_end ? x.a->end32[src] + (uint32_t)x.s->const_off : x.a->b_off[es];
}

// Elements per lane and pass in the kernels that share a tile's elements among the lanes: the lane's kPer
// elements (t, t + 256, ... of the pass) are searched in lockstep and their lengths and offsets loaded
// together, so a step waits for one LDS chain and one memory latency, not kPer of each
constexpr uint32_t kPer = 4;

// The tile in LDS (the row table scan_rows<true> filled): eo[r] for r <= nrows are the absolute element
// offsets of its rows (eo[nrows]: of the row after the tile), src[r] the row's source.
struct Tile {
  const uint64_t* eo;
  const uint32_t* src;
  uint32_t nrows;
};

// row_at for kPer elements at once: the same number of steps for each (nrows alone decides it)
__device__ __forceinline__ void rows_at(const Tile& T, const uint64_t (&e)[kPer], uint32_t (&r)[kPer]) {
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) r[i] = 0u;
  for (uint32_t s = 1u << (31 - __builtin_clz(T.nrows)); s; s >>= 1) {
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      const uint32_t mid = r[i] + s;
      if (mid < T.nrows && T.eo[mid] <= e[i]) r[i] = mid;
    }
  }
}

// The tile's rows: element counts scanned from `base`. TABLE: into the row table in LDS, with the
// rows' sources; TALLY: the three per-row counters into the lane's tallies. Returns base + the tile's
// sum (to every thread).
template <bool TABLE, bool TALLY, class X>
__device__ __forceinline__ uint64_t scan_rows(const X& x, uint32_t t0, uint32_t nrows, uint64_t base, const RowTable& l,
                                              uint32_t& rtrunc, uint32_t& empty, uint32_t& skip) {
  uint64_t carry = base;
  for (uint32_t r0 = 0; r0 < nrows; r0 += kElemBlk) {
    const uint32_t r = r0 + threadIdx.x;
    Row w{};
    if (r < nrows) {
      w = row_of(x, t0 + r);
      if constexpr (TALLY) {
        // (branch-free: a skipped row counts in `skip` alone; its C is 0)
        rtrunc += w.C > w.cnt;
        empty += w.ok & (uint32_t)(w.C == 0u);
        skip += w.ok ^ 1u;
      }
    }
    uint64_t total;
    const uint64_t ex = block_excl_scan<kElemBlk / 64>((uint64_t)w.cnt, l.part, &total);
    if constexpr (TABLE) {
      if (r < nrows) {
        l.offs[r] = carry + ex;
        l.src[r] = w.src;
      }
    }
    carry += total;
  }
  if constexpr (TABLE) {
    if (threadIdx.x == 0) l.offs[nrows] = carry;
    __syncthreads();
  }
  return carry;
}

}  // namespace tfrg
