// tfrg_rows.h — what the row-list passes share: the device code of the passes that read a finished
// decode through a list of rows (tfrg_dense.hip, tfrg_ragged.hip, tfrg_elems.hip, tfrg_ids.hip,
// tfrg_select.hip), each piece defined once. The functions that read a kernel argument are templates over
// the pass's own pointer to it (DenseArgs, RaggedArgs, ElemsArgs, IdsArgs, SelectArgs / SelectBytesArgs in the constant
// address space), as fill_columns<Args> is on the host: the argument structs stay apart, and only
// the names of their common fields (info, rs, n, rows, row0, rows64, in, in_bound) are assumed. What
// tfrg_elems.hip and tfrg_ids.hip share beyond that (a row as a run of elements) is in tfrg_elem_rows.h.
#pragma once
#include "tfrg_dev.h"

namespace tfrg {

// ------------------------------------------------------------------ the row list
// Entry k is the dword at rows + (k << rsh), and for int64 entries the dword rhi bytes after it (rhi 0:
// an int32 entry, whose second load repeats the first). rows null, where the pass allows it: entry k is k.
struct RowList {
  const uint8_t* rows;
  int64_t row0;
  uint32_t rsh, rhi;
};

template <class A>
__device__ __forceinline__ RowList make_row_list(A a) {
  RowList l;
  l.rows = static_cast<const uint8_t*>(a->rows);
  l.row0 = a->row0;
  l.rsh = a->rows64 ? 3u : 2u;
  l.rhi = a->rows64 ? 4u : 0u;
  return l;
}

// entry k of a list that is there, without a branch: the callers keep the loads of several rows in
// flight together. (tfrg_select.hip, a candidate per lane, keeps its entry_of: one load behind uniform
// branches, and k for a list that is not there.)
__device__ __forceinline__ int64_t row_entry(const RowList& l, uint32_t k) {
  const uint8_t* const p = l.rows + ((uint64_t)k << l.rsh);
  const uint32_t lo = *reinterpret_cast<const uint32_t*>(p);
  const uint32_t hi = *reinterpret_cast<const uint32_t*>(p + l.rhi);
  return l.rhi ? (int64_t)(((uint64_t)hi << 32) | lo) : (int64_t)(int32_t)lo;
}

// The row rule: the row whose entry is v is record g = v - row0, and ok says that g is in [0, n). The
// entry is compared before the subtraction, whose unsigned result is then the true difference: no
// entry, INT64_MIN and INT64_MAX included, wraps into range, so a hostile row list indexes nothing
// outside the batch. A row that is not ok is a skipped row: its g is 0, so whatever the caller loads
// for it without a branch is record 0's, whose columns every non-empty result has (as a record without
// a value reads element 0), and the caller drops it. ok is kept as a 0 / 1 value in a vector register
// (the empty asm): the callers hold several rows in flight, and a lane mask per row would cost two
// scalar registers each. n is read from the argument where it is compared, as the rest of a pass reads it.
struct Rec {
  uint32_t g;
  uint32_t ok;
};

template <class A>
__device__ __forceinline__ Rec rec_of(A a, int64_t row0, int64_t v) {
  const uint64_t d = (uint64_t)v - (uint64_t)row0;
  const bool ok = v >= row0 && d < (uint64_t)a->n;
  uint32_t okv = ok ? 1u : 0u;
  asm("" : "+v"(okv));
  return Rec{ok ? (uint32_t)d : 0u, okv};
}

// ------------------------------------------------------------------ the decode's columns
// the slots whose every record placed one value (info words kInfoPlacedLo / Hi; slots below 64)
template <class A>
__device__ __forceinline__ uint64_t placed_slots(A a) {
  const uint32_t* const info = a->info;
  return ((uint64_t)info[kInfoPlacedHi] << 32) | info[kInfoPlacedLo];
}

// the slot's row splits; null for a placed slot, whose row g holds record g's single value: its
// splits are not read
template <class A>
__device__ __forceinline__ const uint32_t* slot_splits(A a, uint32_t slot) {
  const uint64_t placed = placed_slots(a);
  return (slot < 64u && ((placed >> slot) & 1ull)) ? nullptr : a->rs + (uint64_t)slot * ((uint64_t)a->n + 1u);
}

// the input of the bytes views as a buffer resource bounded to the batch: a load at or past in_bound
// gives zeros without a memory access
template <class A>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t bytes_source(A a) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a->in), (short)0, (int)a->in_bound, 0x00020000);
}

// ------------------------------------------------------------------ tiles
// The tile sums tsum[0 .. tiles) to their exclusive prefix, by one workgroup of THREADS threads (part:
// THREADS / 64 words of LDS) in passes of THREADS tiles: the pass of tiles b0 .. b0 + THREADS, carry
// being the sum of the tiles before b0 (plus whatever the prefix starts from). Returns the carry of the
// next pass. The kernels keep the loop over b0 themselves: see DESIGN.md, "What the row-list passes share".
template <uint32_t THREADS>
__device__ __forceinline__ uint64_t scan_tile_sums(uint64_t* tsum, uint32_t tiles, uint32_t b0, uint64_t carry, uint64_t* part) {
  const uint32_t i = b0 + threadIdx.x;
  const uint64_t v = i < tiles ? tsum[i] : 0ull;
  uint64_t total;
  const uint64_t ex = block_excl_scan<THREADS / 64>(v, part, &total);
  if (i < tiles) tsum[i] = carry + ex;
  return carry + total;
}

// The rows of a tile in dynamic LDS: offs [tile + 2] u64 (the absolute offsets of its rows, and of the
// row after the tile), src [tile] u32 (each row's source), then part, the scans' words (the launcher
// sizes it)
struct RowTable {
  uint64_t* offs;
  uint32_t* src;
  uint64_t* part;
};

__device__ __forceinline__ RowTable carve_row_table(uint8_t* lds, uint32_t tile) {
  RowTable l;
  l.offs = reinterpret_cast<uint64_t*>(lds);
  l.src = reinterpret_cast<uint32_t*>(l.offs + tile + 2u);
  l.part = reinterpret_cast<uint64_t*>(l.src + tile);
  return l;
}

// the row of position pos, offs[0] <= pos < offs[nrows]: the last r with offs[r] <= pos (rows without
// an element share their offset with the row after them)
__device__ __forceinline__ uint32_t row_at(const uint64_t* offs, uint32_t nrows, uint64_t pos) {
  uint32_t lo = 0, hi = nrows;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (offs[mid] <= pos) lo = mid;
    else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ counters
// four per-lane tallies into the four counters of spec si: one atomic per wave and counter at the most
__device__ __forceinline__ void add_stats4(uint32_t* stats, uint32_t si, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t sa = wave_sum32(a), sb = wave_sum32(b), sc = wave_sum32(c), sd = wave_sum32(d);
  if ((threadIdx.x & 63u) == 0u) {
    uint32_t* st = stats + 4u * si;
    if (sa) atomicAdd(st + 0, sa);
    if (sb) atomicAdd(st + 1, sb);
    if (sc) atomicAdd(st + 2, sc);
    if (sd) atomicAdd(st + 3, sd);
  }
}

}  // namespace tfrg
