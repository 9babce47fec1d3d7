// tfrg_ragged.hip — the kernels behind tfrg_result_ragged_rows: for a list of m rows (row k is record
// g = entry(k) - row0) and every requested output, the packed values of the rows back to back and the
// m + 1 offsets (cu_seqlens) of the rows in them. Three launches on the decode's stream, no workgroup
// ever waiting on another (the shape of k_fr_sum / k_fr_scan / k_fr_write in tfrg_frame.hip; the row
// rule, the scans and the row table in LDS are those of tfrg_rows.h):
//
//   k_rg_len     per (spec, tile of `tile` rows): the rows' lengths, their u64 sum into the scratch
//                tsum[spec][tile], and the four counters (per-lane tallies, one wave reduction, at most
//                one atomic per wave and counter);
//   k_rg_scan    one workgroup per spec: the tile sums to their exclusive bases, carrying across passes
//                of kRaggedScanThreads tiles; offsets[m] and totals[spec];
//   k_rg_gather  per (spec, tile, s < S): the lengths again, scanned from the tile's base into LDS with
//                each row's source position beside them; workgroup s = 0 writes the tile's offsets;
//                then the tile's span [offsets[t0], min(offsets[t1], cap)) is copied with work laid
//                out along the OUTPUT: after the elements up to the first 16-byte boundary of the
//                output's address, lane l of a wave stores the 16-byte unit after lane l - 1's; a unit
//                finds its first (row, j) by a binary search in the LDS offsets and walks on from
//                there. The span's chunks of kRaggedChunk units go round the tile's S workgroups; what
//                is left before the first and after the last whole unit goes element by element.
//
// Not read (as k_dense): the row splits of a placed slot (info words kInfoPlacedLo / Hi: the row has
// one value, at index g), the bytes_len column of a slot whose length is constant
// (RaggedSpec::const_len), the bytes_off words of a slot the decode left implicit (RaggedSpec::const_off:
// the decode's u32 record ends are read in their place), status / aux / verdict / order. The input of the bytes views is read through
// a buffer resource bounded to the batch: a view that runs past it reads zeros.
//
// A row whose g is not in [0, n) is an empty row: nothing indexed by g is loaded for it (it reads
// record 0 and drops it; validity is a 0 / 1 value in a vector register, see the row rule in tfrg_rows.h),
// and it counts in the fourth counter alone.
#include <hip/hip_runtime.h>

#include "tfrg_dense.h"
#include "tfrg_internal.h"
#include "tfrg_ragged.h"
#include "tfrg_rows.h"

namespace tfrg {
namespace {

typedef uint32_t rg_u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t rg_u64x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kBlk = 256;

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) RaggedArgs* KArgs;
typedef const __attribute__((address_space(4))) RaggedSpec* KSpec;

// the spec a workgroup works in (uniform)
struct Sp {
  KArgs a;
  KSpec s;
  const uint32_t* rs;  // the slot's row splits; null: placed (row g holds record g's value)
  uint64_t base;       // slot_base[slot]
  uint32_t max_len;
  __amdgpu_buffer_rsrc_t in;
  RowList rl;  // (rows null: entry k is k)
};

__device__ __forceinline__ Sp make_sp(KArgs a, uint32_t si) {
  const KSpec s = &a->sp[si];
  const uint32_t slot = s->slot;
  Sp x;
  x.a = a;
  x.s = s;
  x.base = a->slot_base[slot];
  x.rs = slot_splits(a, slot);
  x.max_len = s->max_len;
  x.in = bytes_source(a);
  x.rl = make_row_list(a);
  return x;
}

// One row of the output: `len` elements (bytes on the uint8 path) from position `src` of its source
// (the value index within the slot's column; the byte position in the input) on
struct Row {
  uint32_t len;  // after max_len; 0 for a skipped row
  uint32_t L;    // the record's value count (bytes: the byte length of element 0)
  uint32_t cnt;  // the record's value count
  uint32_t src;
  uint32_t ok;
};

template <bool U8>
__device__ __forceinline__ Row row_of(const Sp& x, uint32_t k) {
  const Rec q = rec_of(x.a, x.rl.row0, x.rl.rows ? row_entry(x.rl, k) : (int64_t)k);
  uint32_t lo = q.g, c = 1u;
  if (x.rs) {
    lo = x.rs[q.g];
    c = x.rs[q.g + 1u] - lo;
  }
  c = q.ok ? c : 0u;  // (a skipped row is a record without a value to everything that loads)
  Row r;
  r.ok = q.ok;
  r.cnt = c;
  if constexpr (!U8) {
    r.src = lo;
    r.L = c;
  } else {
    // (branch-free per lane: a record without an element reads element 0's view and drops it)
    const uint64_t es = c ? x.base + lo : 0ull;
    uint32_t off, len;
    if (x.a->b_off64) {
      const uint64_t o0 = x.a->b_off64[es], o1 = x.a->b_off64[es + 1];
      const uint64_t l = o1 - o0;
      off = o0 < 0xffffffffull ? (uint32_t)o0 : 0xffffffffu;
      len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
    } else {
      // (uniform; const_off: an optimistic decode left the words implicit, the slot is placed and
      // record g's element lies at its end plus a constant -- a skipped row's g is 0)
      off = x.s->const_off != kRaggedOffStored ? x.a->end32[q.g] + (uint32_t)x.s->const_off : x.a->b_off[es];
      len = x.s->const_len != kRaggedNoLen ? x.s->const_len : x.a->b_len[es];
    }
    r.src = off;
    r.L = c ? len : 0u;
  }
  r.len = (x.max_len && r.L > x.max_len) ? x.max_len : r.L;
  return r;
}

// ------------------------------------------------------------------ 1. lengths
template <bool U8>
__device__ __forceinline__ uint64_t len_tile(const Sp& x, uint32_t t0, uint32_t t1, uint32_t& trunc, uint32_t& empty,
                                             uint32_t& multi, uint32_t& skip) {
  uint64_t sum = 0;
  for (uint32_t k = t0 + threadIdx.x; k < t1; k += kBlk) {
    const Row r = row_of<U8>(x, k);
    sum += r.len;
    // (branch-free: a skipped row counts in `skip` alone; its L and cnt are 0)
    trunc += r.L > r.len;
    empty += r.ok & (uint32_t)(r.cnt == 0u);
    if constexpr (U8) multi += r.cnt > 1u;
    skip += r.ok ^ 1u;
  }
  return sum;
}

__global__ __launch_bounds__(kBlk) void k_rg_len(const RaggedArgs) {
  __shared__ uint64_t part[kBlk / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const uint32_t tiles = a->tiles;
  const uint32_t si = blockIdx.x / tiles, ti = blockIdx.x - si * tiles;
  const Sp x = make_sp(a, si);
  const uint32_t t0 = ti * a->tile;
  const uint32_t t1 = a->m - t0 < a->tile ? a->m : t0 + a->tile;
  uint32_t trunc = 0, empty = 0, multi = 0, skip = 0;
  uint64_t sum;
  if (x.s->dtype == kDenseU8) sum = len_tile<true>(x, t0, t1, trunc, empty, multi, skip);
  else sum = len_tile<false>(x, t0, t1, trunc, empty, multi, skip);
  sum = wave_sum64(sum);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kBlk / 64; ++i) all += part[i];
    a->tsum[blockIdx.x] = all;
  }
  uint32_t* const stats = a->stats;
  if (!stats) return;
  add_stats4(stats, si, trunc, empty, multi, skip);
}

// ------------------------------------------------------------------ 2. tile scan
// one workgroup per spec: the tile sums to their exclusive prefix, the total to offsets[m] and totals
__global__ __launch_bounds__(kRaggedScanThreads) void k_rg_scan(const RaggedArgs) {
  __shared__ uint64_t part[kRaggedScanThreads / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, si = blockIdx.x;
  uint64_t* const tsum = a->tsum + (uint64_t)si * tiles;
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < tiles; b0 += kRaggedScanThreads) carry = scan_tile_sums<kRaggedScanThreads>(tsum, tiles, b0, carry, part);
  if (threadIdx.x == 0) {
    a->sp[si].offsets[a->m] = (int64_t)carry;
    if (a->totals) a->totals[si] = carry;
  }
}

// ------------------------------------------------------------------ 3. gather
// The tile in LDS: offs[r] for r <= nrows are the absolute offsets of its rows (offs[nrows]: of the
// row after the tile), src[r] the row's source position.
struct Tile {
  const uint64_t* offs;
  const uint32_t* src;
  uint32_t nrows;
};

// the row of pos from `row` on (a row at or before it); pos < offs[nrows]
__device__ __forceinline__ uint32_t walk_to(const Tile& T, uint32_t row, uint64_t pos) {
  while (pos >= T.offs[row + 1u]) ++row;
  return row;
}

template <uint32_t DT>
struct ValT {
  using type = uint32_t;
};
template <>
struct ValT<kDenseI64> {
  using type = uint64_t;
};

// value j of the row whose values start at index s of the slot's column
template <uint32_t DT>
__device__ __forceinline__ typename ValT<DT>::type value_at(const Sp& x, uint32_t s, uint64_t j) {
  const uint64_t i = x.base + s + j;
  if constexpr (DT == kDenseI64) return (uint64_t)x.a->i64[i];
  else if constexpr (DT == kDenseI32) return reinterpret_cast<const uint32_t*>(x.a->i64)[2u * i];  // the low 32 bits
  else return x.a->f32[i];
}

// byte j of the element at byte s of the input, zero past the input
__device__ __forceinline__ uint32_t in_byte(const Sp& x, uint32_t s, uint64_t j) {
  const uint64_t p = (uint64_t)s + j;
  if (p >= x.a->in_bound) return 0u;
  return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(x.in, (uint32_t)p, 0, 0);
}

// The output dword at positions pos .. pos + 3 (all below offs[nrows]); `row`: a row at or before
// pos's, advanced to the row of pos + 3. A dword inside one row is built from two aligned input
// dwords (one past the bound reads zeros without a memory access), any other byte by byte.
__device__ __forceinline__ uint32_t u8_dword(const Sp& x, const Tile& T, uint32_t& row, uint64_t pos) {
  row = walk_to(T, row, pos);
  if (T.offs[row + 1u] - pos >= 4u) {
    const uint64_t p = (uint64_t)T.src[row] + (pos - T.offs[row]);
    const bool ok = p < x.a->in_bound;
    const uint32_t p0 = ok ? ((uint32_t)p & ~3u) : 0xfffffff8u;  // (in_bound <= 0xfffffff0: p0 + 4 does not wrap)
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0, 0, 0);
    const uint32_t d1 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0 + 4u, 0, 0);
    return __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)p & 3u);
  }
  uint32_t w = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    row = walk_to(T, row, pos + k);
    w |= in_byte(x, T.src[row], pos + k - T.offs[row]) << (8u * k);
  }
  return w;
}

// one element (the ends of a span)
template <uint32_t DT>
__device__ __forceinline__ void copy_elem(const Sp& x, const Tile& T, uint8_t* out, uint64_t pos) {
  const uint32_t row = row_at(T.offs, T.nrows, pos);
  const uint64_t j = pos - T.offs[row];
  if constexpr (DT == kDenseU8) out[pos] = (uint8_t)in_byte(x, T.src[row], j);
  else reinterpret_cast<typename ValT<DT>::type*>(out)[pos] = value_at<DT>(x, T.src[row], j);
}

// the 16-byte unit whose first element is pos (its address is 16-byte aligned; every element of it
// is below offs[nrows])
template <uint32_t DT>
__device__ __forceinline__ void copy_unit(const Sp& x, const Tile& T, uint8_t* out, uint64_t pos) {
  uint32_t row = row_at(T.offs, T.nrows, pos);
  if constexpr (DT == kDenseU8) {
    rg_u32x4 o;
    o.x = u8_dword(x, T, row, pos);
    o.y = u8_dword(x, T, row, pos + 4u);
    o.z = u8_dword(x, T, row, pos + 8u);
    o.w = u8_dword(x, T, row, pos + 12u);
    *reinterpret_cast<rg_u32x4*>(out + pos) = o;
  } else if constexpr (DT == kDenseI64) {
    uint64_t v[2];
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k) {
      row = walk_to(T, row, pos + k);
      v[k] = value_at<DT>(x, T.src[row], pos + k - T.offs[row]);
    }
    rg_u64x2 o;
    o.x = v[0];
    o.y = v[1];
    *reinterpret_cast<rg_u64x2*>(out + (pos << 3)) = o;
  } else {
    uint32_t v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      row = walk_to(T, row, pos + k);
      v[k] = value_at<DT>(x, T.src[row], pos + k - T.offs[row]);
    }
    rg_u32x4 o;
    o.x = v[0];
    o.y = v[1];
    o.z = v[2];
    o.w = v[3];
    *reinterpret_cast<rg_u32x4*>(out + (pos << 2)) = o;
  }
}

// the tile's span [offs[0], min(offs[nrows], cap)), as the s-th of its S workgroups
template <uint32_t DT>
__device__ __forceinline__ void gather_tile(const Sp& x, const Tile& T, uint32_t s, uint32_t S) {
  constexpr uint32_t isz = DT == kDenseI64 ? 8u : DT == kDenseU8 ? 1u : 4u;
  constexpr uint32_t per = 16u / isz;  // elements of a unit
  uint8_t* const out = static_cast<uint8_t*>(x.s->values);
  const uint64_t cap = out ? x.s->cap : 0ull;
  const uint64_t p0 = T.offs[0], pe = T.offs[T.nrows];
  const uint64_t p1 = pe < cap ? pe : cap;
  if (p0 >= p1) return;
  // elements up to the first 16-byte boundary of the output's address, whole units, the rest
  const uint64_t addr = (uint64_t)(uintptr_t)out + p0 * isz;
  uint64_t head = ((16u - (uint32_t)(addr & 15u)) & 15u) / isz;
  if (head > p1 - p0) head = p1 - p0;
  const uint64_t u0 = p0 + head;
  const uint64_t units = (p1 - u0) / per;
  const uint64_t tail0 = u0 + units * per;
  const uint32_t tid = threadIdx.x;
  if (s == 0u) {
    const uint32_t ends = (uint32_t)head + (uint32_t)(p1 - tail0);  // < 32
    if (tid < ends) copy_elem<DT>(x, T, out, tid < (uint32_t)head ? p0 + tid : tail0 + (tid - (uint32_t)head));
  }
  for (uint64_t c0 = (uint64_t)s * kRaggedChunk; c0 < units; c0 += (uint64_t)S * kRaggedChunk) {
#pragma unroll 1
    for (uint32_t it = 0; it < kRaggedChunk / kBlk; ++it) {
      const uint64_t u = c0 + it * kBlk + tid;
      if (u < units) copy_unit<DT>(x, T, out, u0 + u * per);
    }
  }
}

// the tile's rows into LDS: lengths scanned from the tile's base, source positions
template <bool U8>
__device__ __forceinline__ void scan_tile(const Sp& x, uint32_t t0, uint32_t nrows, uint64_t base, uint64_t* offs,
                                          uint32_t* src, uint64_t* part) {
  uint64_t carry = base;
  for (uint32_t r0 = 0; r0 < nrows; r0 += kBlk) {
    const uint32_t r = r0 + threadIdx.x;
    Row w{};
    if (r < nrows) w = row_of<U8>(x, t0 + r);
    uint64_t total;
    const uint64_t ex = block_excl_scan<kBlk / 64>((uint64_t)w.len, part, &total);
    if (r < nrows) {
      offs[r] = carry + ex;
      src[r] = w.src;
    }
    carry += total;
  }
  if (threadIdx.x == 0) offs[nrows] = carry;
  __syncthreads();
}

// dynamic LDS: the row table of tfrg_rows.h with part [kBlk / 64] u64 (launch_ragged sizes it)
__global__ __launch_bounds__(kBlk) void k_rg_gather(const RaggedArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rg_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, S = a->split, tile = a->tile;
  const uint32_t per_spec = tiles * S;
  const uint32_t si = blockIdx.x / per_spec, rem = blockIdx.x - si * per_spec;
  const uint32_t ti = rem / S, s = rem - ti * S;
  const RowTable l = carve_row_table(rg_lds, tile);
  const Sp x = make_sp(a, si);
  const uint32_t t0 = ti * tile;
  const uint32_t nrows = a->m - t0 < tile ? a->m - t0 : tile;
  const uint64_t base = a->tsum[(uint64_t)si * tiles + ti];
  const uint32_t dt = x.s->dtype;
  if (dt == kDenseU8) scan_tile<true>(x, t0, nrows, base, l.offs, l.src, l.part);
  else scan_tile<false>(x, t0, nrows, base, l.offs, l.src, l.part);
  if (s == 0u) {
    int64_t* const o = x.s->offsets + t0;  // (offsets[m] is k_rg_scan's)
    for (uint32_t r = threadIdx.x; r < nrows; r += kBlk) o[r] = (int64_t)l.offs[r];
  }
  const Tile T{l.offs, l.src, nrows};
  switch (dt) {
    case kDenseI64: gather_tile<kDenseI64>(x, T, s, S); break;
    case kDenseI32: gather_tile<kDenseI32>(x, T, s, S); break;
    case kDenseF32: gather_tile<kDenseF32>(x, T, s, S); break;
    default: gather_tile<kDenseU8>(x, T, s, S); break;
  }
}

}  // namespace

hipError_t launch_ragged(const RaggedArgs& a, hipStream_t st) {
  const uint32_t per_spec = a.n_specs * a.tiles;
  const size_t lds = ((size_t)a.tile + 2u) * 8u + (size_t)a.tile * 4u + (kBlk / 64) * 8u;
  hipLaunchKernelGGL(k_rg_len, dim3(per_spec), dim3(kBlk), 0, st, a);
  hipLaunchKernelGGL(k_rg_scan, dim3(a.n_specs), dim3(kRaggedScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_rg_gather, dim3(per_spec * a.split), dim3(kBlk), lds, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
