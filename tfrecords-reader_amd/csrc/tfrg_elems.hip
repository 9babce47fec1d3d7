// tfrg_elems.hip — the kernels behind tfrg_result_ragged_elems: for a list of m rows (row k is record
// g = entry(k) - row0) and every requested bytes_list slot, EVERY element of the rows' lists: the
// elements' bytes back to back (values), the E + 1 offsets of the elements in them (elem_offsets) and
// the m + 1 offsets of the rows in elements (row_offsets). Four launches on the decode's stream, no
// workgroup ever waiting on another (the shape of k_rg_len / k_rg_scan / k_rg_gather in tfrg_ragged.hip;
// the row rule, the scans and the row table in LDS are those of tfrg_rows.h, the rows of elements those of
// tfrg_elem_rows.h, shared with tfrg_ids.hip):
//
//   k_el_len   per (spec, tile of `tile` rows): the rows' element counts scanned into LDS, then the
//              tile's elements shared by the lanes (lane t takes tile-local elements t, t + 256, ...
//              and finds each one's row by a binary search in LDS) for the tile's byte sum; both sums
//              into the scratch, and the four counters (per-lane tallies, one wave reduction, at most
//              one atomic per wave and counter);
//   k_el_scan  one workgroup per spec: both tile sums to their exclusive bases, carrying across passes
//              of kElemsScanThreads tiles; row_offsets[m], the totals (E, B), and elem_offsets[E] = B
//              where E <= elem_cap;
//   k_el_offs  per (spec, tile): the tile's row_offsets; then the elements again, in passes of 256 whose
//              lengths are scanned from the tile's byte base: element e < E writes its start to
//              elem_offsets[e] where e <= elem_cap (so with E > elem_cap the entry elem_cap is the end
//              of the last described element);
//   k_el_copy  per (spec, tile, s < S): the tile's span [elem_offsets[e0], min(elem_offsets[e1], cap))
//              of its elements [e0, e1) below elem_cap, copied with work laid out along the OUTPUT as
//              k_rg_gather does: after the bytes up to the first 16-byte boundary of the output's
//              address, lane l of a wave stores the 16-byte unit after lane l - 1's; a unit finds its
//              element by a binary search in the elem_offsets k_el_offs wrote, the element's row (and so
//              its source) in the tile's row table in LDS, and walks on over element and row ends. The
//              span's chunks of kElemsChunk units are dealt to the tile's S workgroups in S consecutive
//              runs, so one long element is shared by all of them, and a lane's next unit lies 4 KB after
//              its last: it keeps its element, or searches on from it.
//
// Tiles are not balanced against each other: a tile whose rows hold many elements takes longer than its
// neighbours in k_el_len and k_el_offs (the copy is spread by bytes within a tile only).
//
// Not read (as k_rg_*): the row splits of a placed slot, the bytes_len column of a slot whose length is
// constant (ElemsSpec::const_len), the bytes_off words of a slot the decode left implicit
// (ElemsSpec::const_off: the decode's u32 record ends are read in their place), status / aux / verdict /
// order and the numeric columns. The input of the bytes views is read through a buffer resource bounded
// to the batch: a view that runs past it reads zeros.
//
// A row whose g is not in [0, n) is an empty row: nothing indexed by g is loaded for it (it reads
// record 0 and drops it), and it counts in the fourth counter alone.
#include <hip/hip_runtime.h>

#include "tfrg_elem_rows.h"
#include "tfrg_elems.h"
#include "tfrg_internal.h"

namespace tfrg {
namespace {

typedef uint32_t el_u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kBlk = kElemBlk;

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) ElemsArgs* KArgs;
typedef const __attribute__((address_space(4))) ElemsSpec* KSpec;

// the spec a workgroup works in (uniform), with the fields tfrg_elem_rows.h reads
struct Sp {
  static constexpr uint32_t kNoLen = kElemsNoLen;
  KArgs a;
  KSpec s;
  const uint32_t* rs;  // the slot's row splits; null: placed (record g holds one element, at index g)
  uint64_t base;       // slot_base[slot]
  uint32_t max_elems, max_len;
  bool by_end;         // the element of record g lies at end32[g] + const_off
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
  x.max_elems = s->max_elems;
  x.max_len = s->max_len;
  x.by_end = !a->b_off64 && s->const_off != kElemsOffStored;
  x.in = bytes_source(a);
  x.rl = make_row_list(a);
  return x;
}

__device__ __forceinline__ uint32_t clamp_len(const Sp& x, uint32_t L) { return (x.max_len && L > x.max_len) ? x.max_len : L; }

// ------------------------------------------------------------------ 1. counts and byte sums
// dynamic LDS: the row table of tfrg_rows.h with part [16] u64 (elems_lds_bytes sizes it)
__global__ __launch_bounds__(kBlk) void k_el_len(const ElemsArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t el_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const uint32_t tiles = a->tiles, tile = a->tile;
  const uint32_t si = blockIdx.x / tiles, ti = blockIdx.x - si * tiles;
  const RowTable l = carve_row_table(el_lds, tile);
  const Sp x = make_sp(a, si);
  const uint32_t t0 = ti * tile;
  const uint32_t nrows = a->m - t0 < tile ? a->m - t0 : tile;
  uint32_t rtrunc = 0, etrunc = 0, empty = 0, skip = 0;
  scan_rows<true, true>(x, t0, nrows, 0ull, l, rtrunc, empty, skip);
  const Tile T{l.offs, l.src, nrows};
  const uint64_t et = l.offs[nrows];
  uint64_t sum = 0;
  for (uint64_t p0 = 0; p0 < et; p0 += kPer * kBlk) {
    uint64_t e[kPer];
    uint32_t r[kPer], L[kPer];
    bool on[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      e[i] = p0 + i * kBlk + threadIdx.x;
      on[i] = e[i] < et;
      e[i] = on[i] ? e[i] : p0;  // (an element past the tile's reads the pass's first one and drops it)
    }
    rows_at(T, e, r);
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) L[i] = elem_L(x, T.src[r[i]], (uint32_t)(e[i] - T.eo[r[i]]));
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      const uint32_t len = clamp_len(x, L[i]);
      sum += on[i] ? len : 0u;
      etrunc += on[i] && L[i] > len;
    }
  }
  sum = wave_sum64(sum);
  __syncthreads();  // (part was last read by scan_rows)
  if ((threadIdx.x & 63u) == 0u) l.part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t all = 0;
#pragma unroll
    for (uint32_t i = 0; i < kBlk / 64; ++i) all += l.part[i];
    a->tsum[blockIdx.x] = et;
    a->tsum[(uint64_t)a->n_specs * tiles + blockIdx.x] = all;
  }
  uint32_t* const stats = a->stats;
  if (!stats) return;
  add_stats4(stats, si, rtrunc, etrunc, empty, skip);
}

// ------------------------------------------------------------------ 2. tile scan
// one workgroup per spec: both tile sums to their exclusive prefixes, E to row_offsets[m], (E, B) to the
// totals, and B to elem_offsets[E] where that entry exists
__global__ __launch_bounds__(kElemsScanThreads) void k_el_scan(const ElemsArgs) {
  __shared__ uint64_t part[kElemsScanThreads / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, si = blockIdx.x;
  uint64_t tot[2];
#pragma unroll
  for (uint32_t w = 0; w < 2u; ++w) {
    uint64_t* const tsum = a->tsum + ((uint64_t)w * a->n_specs + si) * tiles;
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < tiles; b0 += kElemsScanThreads) carry = scan_tile_sums<kElemsScanThreads>(tsum, tiles, b0, carry, part);
    tot[w] = carry;
  }
  if (threadIdx.x == 0) {
    const KSpec s = &a->sp[si];
    s->row_offsets[a->m] = (int64_t)tot[0];
    if (s->elem_offsets && tot[0] <= s->elem_cap) s->elem_offsets[tot[0]] = (int64_t)tot[1];
    if (a->totals) {
      a->totals[2u * si] = tot[0];
      a->totals[2u * si + 1u] = tot[1];
    }
  }
}

// ------------------------------------------------------------------ 3. offsets
__global__ __launch_bounds__(kBlk) void k_el_offs(const ElemsArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t el_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, tile = a->tile;
  const uint32_t si = blockIdx.x / tiles, ti = blockIdx.x - si * tiles;
  const RowTable l = carve_row_table(el_lds, tile);
  const Sp x = make_sp(a, si);
  const uint32_t t0 = ti * tile;
  const uint32_t nrows = a->m - t0 < tile ? a->m - t0 : tile;
  const uint64_t eb = a->tsum[blockIdx.x];
  const uint64_t bb = a->tsum[(uint64_t)a->n_specs * tiles + blockIdx.x];
  uint32_t u0 = 0, u1 = 0, u2 = 0;
  scan_rows<true, false>(x, t0, nrows, eb, l, u0, u1, u2);
  int64_t* const ro = x.s->row_offsets + t0;  // (row_offsets[m] is k_el_scan's)
  for (uint32_t r = threadIdx.x; r < nrows; r += kBlk) ro[r] = (int64_t)l.offs[r];
  int64_t* const eoffs = x.s->elem_offsets;
  if (!eoffs) return;
  // the tile's elements whose start is an entry of elem_offsets: e <= elem_cap
  const Tile T{l.offs, l.src, nrows};
  const uint64_t ecap = x.s->elem_cap;
  const uint64_t e1 = l.offs[nrows];
  const uint64_t lim = ecap < e1 ? ecap + 1u : e1;  // (at or below eb: none of them)
  uint64_t carry = bb;
  const uint32_t w = threadIdx.x >> 6;
  for (uint64_t p0 = eb; p0 < lim; p0 += kPer * kBlk) {
    uint64_t e[kPer], inc[kPer];
    uint32_t r[kPer], len[kPer];
    bool on[kPer];
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      e[i] = p0 + i * kBlk + threadIdx.x;
      on[i] = e[i] < lim;
      e[i] = on[i] ? e[i] : p0;  // (as k_el_len)
    }
    rows_at(T, e, r);
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) len[i] = elem_L(x, T.src[r[i]], (uint32_t)(e[i] - T.eo[r[i]]));
    // kPer exclusive scans of 256 lengths, one after the other in element order, behind one pair of
    // barriers: the waves' sums of every block go to LDS together
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      len[i] = on[i] ? clamp_len(x, len[i]) : 0u;
      inc[i] = wave_incl_scan((uint64_t)len[i]);
    }
    __syncthreads();  // (part may still be read from the pass before, or from scan_rows)
    if ((threadIdx.x & 63u) == 63u) {
#pragma unroll
      for (uint32_t i = 0; i < kPer; ++i) l.part[i * (kBlk / 64) + w] = inc[i];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i) {
      uint64_t before = 0, all = 0;
#pragma unroll
      for (uint32_t j = 0; j < kBlk / 64; ++j) {
        const uint64_t s = l.part[i * (kBlk / 64) + j];
        before += j < w ? s : 0ull;
        all += s;
      }
      if (on[i]) eoffs[e[i]] = (int64_t)(carry + before + inc[i] - len[i]);
      carry += all;
    }
  }
}

// ------------------------------------------------------------------ 4. copy
// The copy's place in the output: element e = [start, end) of values, in row `row` of the tile, its
// first byte at `off` of the bytes' source
struct Cur {
  uint64_t e, start, end;
  uint32_t row, off;
};

struct Span {
  const int64_t* eoffs;  // the spec's elem_offsets
  uint64_t e0, e1;       // the tile's elements below elem_cap
};

// the element of byte pos, eoffs[e0] <= pos < eoffs[e1]: the last e with eoffs[e] <= pos (elements
// without a byte share their offset with the element after them)
__device__ __forceinline__ Cur seek(const Sp& x, const Tile& T, const Span& sp, uint64_t pos, uint64_t from) {
  // `from`: an element at or before pos's. A lane's next unit lies 4 KB after its last one, so the
  // elements 1, 3 and 7 after `from` are tried before the rest of the span is searched: inside a long
  // element, or a few short ones on, the search ends after a load or two
  uint64_t lo = from, hi = sp.e1;
#pragma unroll 1
  for (uint64_t step = 1; step <= 4u; step <<= 1) {
    const uint64_t probe = lo + step;
    if (probe >= hi) break;
    if ((uint64_t)sp.eoffs[probe] <= pos) {
      lo = probe;
    } else {
      hi = probe;
      break;
    }
  }
  while (hi - lo > 1u) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)sp.eoffs[mid] <= pos) lo = mid;
    else hi = mid;
  }
  Cur c;
  c.e = lo;
  c.start = (uint64_t)sp.eoffs[lo];
  c.end = (uint64_t)sp.eoffs[lo + 1u];
  c.row = row_at(T.eo, T.nrows, lo);
  c.off = elem_off(x, T.src[c.row], (uint32_t)(lo - T.eo[c.row]));
  return c;
}

// on to the element of pos, at or after the cursor's; pos < eoffs[e1]
__device__ __forceinline__ void walk_to(const Sp& x, const Tile& T, const Span& sp, Cur& c, uint64_t pos) {
  if (pos < c.end) return;
  do {
    ++c.e;
    c.start = c.end;
    c.end = (uint64_t)sp.eoffs[c.e + 1u];
  } while (pos >= c.end);
  while (c.e >= T.eo[c.row + 1u]) ++c.row;
  c.off = elem_off(x, T.src[c.row], (uint32_t)(c.e - T.eo[c.row]));
}

// byte j of the element at byte s of the input, zero past the input
__device__ __forceinline__ uint32_t in_byte(const Sp& x, uint32_t s, uint64_t j) {
  const uint64_t p = (uint64_t)s + j;
  if (p >= x.a->in_bound) return 0u;
  return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(x.in, (uint32_t)p, 0, 0);
}

// The output dword at positions pos .. pos + 3 (all below eoffs[e1]); the cursor: an element at or
// before pos's, advanced to the element of pos + 3. A dword inside one element is built from two aligned
// input dwords (one past the bound reads zeros without a memory access), any other byte by byte.
__device__ __forceinline__ uint32_t u8_dword(const Sp& x, const Tile& T, const Span& sp, Cur& c, uint64_t pos) {
  walk_to(x, T, sp, c, pos);
  if (c.end - pos >= 4u) {
    const uint64_t p = (uint64_t)c.off + (pos - c.start);
    const bool ok = p < x.a->in_bound;
    const uint32_t p0 = ok ? ((uint32_t)p & ~3u) : 0xfffffff8u;  // (in_bound <= 0xfffffff0: p0 + 4 does not wrap)
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0, 0, 0);
    const uint32_t d1 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0 + 4u, 0, 0);
    return __builtin_amdgcn_alignbyte(d1, d0, (uint32_t)p & 3u);
  }
  uint32_t w = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    walk_to(x, T, sp, c, pos + k);
    w |= in_byte(x, c.off, pos + k - c.start) << (8u * k);
  }
  return w;
}

// dynamic LDS as k_el_len
__global__ __launch_bounds__(kBlk) void k_el_copy(const ElemsArgs) {
  extern __shared__ __attribute__((aligned(16))) uint8_t el_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles, S = a->split, tile = a->tile;
  const uint32_t per_spec = tiles * S;
  const uint32_t si = blockIdx.x / per_spec, rem = blockIdx.x - si * per_spec;
  const uint32_t ti = rem / S, s = rem - ti * S;
  const KSpec ks = &a->sp[si];
  uint8_t* const out = ks->values;
  const uint64_t ecap = ks->elem_offsets ? ks->elem_cap : 0ull;
  const uint64_t cap = out ? ks->cap : 0ull;
  const uint64_t eb = a->tsum[(uint64_t)si * tiles + ti];
  const uint64_t bb = a->tsum[((uint64_t)a->n_specs + si) * tiles + ti];
  // (uniform: nothing of this tile is described, or nothing of it fits)
  if (eb >= ecap || bb >= cap) return;
  const RowTable l = carve_row_table(el_lds, tile);
  const Sp x = make_sp(a, si);
  const uint32_t t0 = ti * tile;
  const uint32_t nrows = a->m - t0 < tile ? a->m - t0 : tile;
  uint32_t u0 = 0, u1 = 0, u2 = 0;
  scan_rows<true, false>(x, t0, nrows, eb, l, u0, u1, u2);
  const Tile T{l.offs, l.src, nrows};
  const uint64_t ee = l.offs[nrows];
  const Span sp{ks->elem_offsets, eb, ee < ecap ? ee : ecap};
  if (sp.e1 <= sp.e0) return;
  // the tile's span of the output: bytes up to the first 16-byte boundary of the output's address,
  // whole units, the rest
  const uint64_t p0 = bb, pe = (uint64_t)sp.eoffs[sp.e1];
  const uint64_t p1 = pe < cap ? pe : cap;
  if (p0 >= p1) return;
  const uint64_t addr = (uint64_t)(uintptr_t)out + p0;
  uint64_t head = (16u - (uint32_t)(addr & 15u)) & 15u;
  if (head > p1 - p0) head = p1 - p0;
  const uint64_t h0 = p0 + head;
  const uint64_t units = (p1 - h0) >> 4;
  const uint64_t tail0 = h0 + (units << 4);
  const uint32_t tid = threadIdx.x;
  if (s == 0u) {
    const uint32_t ends = (uint32_t)head + (uint32_t)(p1 - tail0);  // < 32
    if (tid < ends) {
      const uint64_t pos = tid < (uint32_t)head ? p0 + tid : tail0 + (tid - (uint32_t)head);
      const Cur c = seek(x, T, sp, pos, sp.e0);
      out[pos] = (uint8_t)in_byte(x, c.off, pos - c.start);
    }
  }
  // the s-th of S runs of whole chunks
  const uint64_t chunks = (units + kElemsChunk - 1u) / kElemsChunk;
  const uint64_t ua = chunks * s / S * kElemsChunk;
  uint64_t ub = chunks * (s + 1u) / S * kElemsChunk;
  if (ub > units) ub = units;
  Cur c{sp.e0, 0ull, 0ull, 0u, 0u};  // (end 0: the first unit seeks)
#pragma unroll 1
  for (uint64_t u = ua + tid; u < ub; u += kBlk) {
    const uint64_t pos = h0 + (u << 4);
    if (pos >= c.end) c = seek(x, T, sp, pos, c.e);  // (else still inside the element of the unit before)
    el_u32x4 o;
    o.x = u8_dword(x, T, sp, c, pos);
    o.y = u8_dword(x, T, sp, c, pos + 4u);
    o.z = u8_dword(x, T, sp, c, pos + 8u);
    o.w = u8_dword(x, T, sp, c, pos + 12u);
    *reinterpret_cast<el_u32x4*>(out + pos) = o;
  }
}

}  // namespace

hipError_t launch_elems(const ElemsArgs& a, hipStream_t st) {
  const uint32_t per_spec = a.n_specs * a.tiles;
  const size_t lds = elems_lds_bytes(a.tile);
  hipLaunchKernelGGL(k_el_len, dim3(per_spec), dim3(kBlk), lds, st, a);
  hipLaunchKernelGGL(k_el_scan, dim3(a.n_specs), dim3(kElemsScanThreads), 0, st, a);
  hipLaunchKernelGGL(k_el_offs, dim3(per_spec), dim3(kBlk), lds, st, a);
  if (a.split) hipLaunchKernelGGL(k_el_copy, dim3(per_spec * a.split), dim3(kBlk), lds, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
