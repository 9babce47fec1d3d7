// tfrg_dense.hip — k_dense: the collate step behind tfrg_result_dense. One launch turns the ragged
// columns of a decoded batch into every requested fixed-shape output [n][width] (padded with the
// spec's fill or truncated), with per-record lengths and four counters per output.
//
// Work is laid out along the OUTPUT: an output's row-major bytes are cut into 16-byte units, lane l
// of a wave stores the unit after lane l - 1's, so each store instruction covers 1 KiB of whole
// 128-byte lines. A workgroup works inside one output (DenseSpec, found from the block index through
// the blk0 table of the kernel argument; everything it reads from the spec is wave-uniform) and
// strides over that output's chunks of kDenseChunk units. What does not fill a 16-byte unit -- an
// output whose base is not 16-byte aligned, or the last bytes of one whose size is no multiple of
// 16 -- takes the element-granular loops below (dwords, then bytes, on the uint8 path).
//
// A lane's loads are issued branch-free and in phases (row splits / views, then values / input
// dwords), so that they are in flight together; lengths and counters come last.
//
// Not read: the row splits of a placed slot (info words kInfoPlacedLo / Hi: row r holds record r's
// single value), the bytes_len column of a slot whose length is constant (DenseSpec::const_len), the
// bytes_off words of a slot the decode left implicit (DenseSpec::const_off: the decode's u32 record
// ends are read in their place, DenseArgs::end32), status / aux / verdict / order. The input of the bytes views is read through a buffer resource
// bounded to the batch: a view that runs past it reads zeros.
//
// k_dense_rows (tfrg_result_dense_rows) is the same kernel behind one level of indirection:
// the output has m rows, and row k is record g = rows[k] - row0 (the row rule of tfrg_rows.h). The
// row list is a per-lane vector load and one phase of its own, ahead of the row splits. A k whose g is not in [0, n) is a
// skipped row: nothing indexed by g is loaded for it (it reads record 0, whose columns every
// non-empty result has, as a record without a value reads element 0), none of its output elements
// and no lengths[k] are stored, and it counts in skipped[spec] alone. A 16-byte unit with a skipped
// row in it stores the elements of its other rows one by one; every other unit keeps the one store.
#include <hip/hip_runtime.h>

#include "tfrg_dense.h"
#include "tfrg_internal.h"
#include "tfrg_rows.h"

namespace tfrg {
namespace {

typedef uint32_t dn_u32x4 __attribute__((ext_vector_type(4)));
typedef uint64_t dn_u64x2 __attribute__((ext_vector_type(2)));

// per-lane counters of the rows whose first element the lane wrote (skip: or left out)
struct Tally {
  uint32_t trunc = 0, pad = 0, zero = 0, multi = 0, skip = 0;
};

// The kernel argument is read in place, in the constant address space (scalar loads): a by-value
// struct indexed with a run-time spec number would be copied to scratch first.
typedef const __attribute__((address_space(4))) DenseArgs* KArgs;
typedef const __attribute__((address_space(4))) DenseSpec* KSpec;

// the spec a workgroup works in (uniform)
struct Sp {
  KArgs a;
  KSpec s;
  const uint32_t* rs;  // the slot's row splits; null: placed (row r holds record r's value)
  uint64_t base;       // slot_base[slot]
  uint32_t W;
  __amdgpu_buffer_rsrc_t in;
  RowList rl;  // (ROWS only)
};

// The record of output row r: r itself without a row list; with one, r < m and the row rule decides
template <bool ROWS>
__device__ __forceinline__ Rec row_rec(const Sp& x, uint32_t r) {
  if constexpr (!ROWS) return Rec{r, 1u};
  else return rec_of(x.a, x.rl.row0, row_entry(x.rl, r));
}

// first value index and value count of record g (g < n)
__device__ __forceinline__ void row_of(const Sp& x, uint32_t r, uint64_t& e, uint32_t& c) {
  if (!x.rs) {
    e = x.base + r;
    c = 1;
    return;
  }
  const uint32_t lo = x.rs[r], hi = x.rs[r + 1];
  e = x.base + lo;
  c = hi - lo;
}

// (a skipped row is a record without a value to everything that loads)
__device__ __forceinline__ void row_of(const Sp& x, const Rec& q, uint64_t& e, uint32_t& c) {
  row_of(x, q.g, e, c);
  c = q.ok ? c : 0u;
}

template <bool ROWS>
__device__ __forceinline__ void note_row(const Sp& x, Tally& t, uint32_t r, uint32_t okv, uint32_t count, uint32_t len) {
  if constexpr (ROWS) {
    // (branch-free but for the store: a skipped row counts in `skip` alone)
    const bool ok = okv != 0u;
    if (ok && x.s->lengths) x.s->lengths[r] = (int32_t)len;
    t.trunc += ok && len > x.W;
    t.pad += ok && len < x.W;
    t.zero += ok && count == 0;
    t.skip += !ok;
  } else {
    if (x.s->lengths) x.s->lengths[r] = (int32_t)len;
    t.trunc += len > x.W;
    t.pad += len < x.W;
    t.zero += count == 0;
  }
}

// ------------------------------------------------------------------ int64_list / float_list slots
template <uint32_t DT>
struct ValT {
  using type = uint32_t;
};
template <>
struct ValT<kDenseI64> {
  using type = uint64_t;
};

// (branch-free, so that a lane's loads are all in flight together: a value that is not there reads
// element 0 of the array, which always exists, and is replaced by the fill)
template <uint32_t DT>
__device__ __forceinline__ typename ValT<DT>::type value_at(const Sp& x, uint64_t e, uint32_t c, uint32_t j) {
  using T = typename ValT<DT>::type;
  const bool ok = j < c;
  const uint64_t i = ok ? e + j : 0ull;
  const T v = DT == kDenseF32 ? (T)x.a->f32[i] : (T)(uint64_t)x.a->i64[i];
  return ok ? v : (T)x.s->fill;
}

// K consecutive elements from (r, j) on; r < n for each of them (the caller's range is inside the
// output). Returns the mask of the elements whose row is not skipped.
template <uint32_t DT, int K, bool ROWS>
__device__ __forceinline__ uint32_t values_from(const Sp& x, Tally& t, uint32_t r, uint32_t j,
                                                typename ValT<DT>::type* v) {
  if constexpr (!ROWS) {
    uint64_t e;
    uint32_t c;
    row_of(x, r, e, c);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (j == 0) note_row<false>(x, t, r, 1u, c, c);
      v[k] = value_at<DT>(x, e, c, j);
      if (++j == x.W) {
        j = 0;
        ++r;
        if (k + 1 < K) row_of(x, r, e, c);
      }
    }
    return (1u << K) - 1u;
  } else {
    // in phases: the elements' row-list entries, their row splits, their values, then the lengths
    // and counters (an element that shares its row with the one before it repeats that one's loads)
    uint32_t rr[K], jj[K], c[K];
    uint64_t e[K];
    Rec q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      rr[k] = r;
      jj[k] = j;
      const bool wrap = ++j == x.W;
      r += wrap;
      j = wrap ? 0u : j;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) q[k] = row_rec<true>(x, rr[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) row_of(x, q[k], e[k], c[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = value_at<DT>(x, e[k], c[k], jj[k]);
    uint32_t okm = 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      okm |= q[k].ok << k;
      if (jj[k] == 0) note_row<true>(x, t, rr[k], q[k].ok, c[k], c[k]);
    }
    return okm;
  }
}

// ------------------------------------------------------------------ bytes_list slots (uint8)
struct BRow {
  uint32_t off, len, cnt;
};

// (branch-free per lane: a record without an element reads element 0's view and drops it)
__device__ __forceinline__ BRow brow_of(const Sp& x, const Rec& q) {
  uint64_t e;
  uint32_t c;
  row_of(x, q, e, c);
  const uint64_t es = c ? e : 0ull;
  BRow b{0u, 0u, c};
  if (x.a->b_off64) {
    const uint64_t o0 = x.a->b_off64[es], o1 = x.a->b_off64[es + 1];
    const uint64_t l = o1 - o0;
    b.off = o0 < 0xffffffffull ? (uint32_t)o0 : 0xffffffffu;
    b.len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
  } else {
    // (uniform; const_off: an optimistic decode left the words implicit, the slot is placed and
    // record g's element lies at its end plus a constant -- a skipped row's g is 0)
    b.off = x.s->const_off != kDenseOffStored ? x.a->end32[q.g] + (uint32_t)x.s->const_off : x.a->b_off[es];
    b.len = x.s->const_len != kDenseNoLen ? x.s->const_len : x.a->b_len[es];
  }
  if (!c) b.len = 0u;
  return b;
}

template <bool ROWS>
__device__ __forceinline__ BRow brow_of(const Sp& x, uint32_t r, uint32_t& ok) {
  const Rec q = row_rec<ROWS>(x, r);
  ok = q.ok;
  return brow_of(x, q);
}

template <bool ROWS>
__device__ __forceinline__ void note_brow(const Sp& x, Tally& t, uint32_t r, uint32_t ok, const BRow& b) {
  note_row<ROWS>(x, t, r, ok, b.cnt, b.len);
  t.multi += b.cnt > 1u;  // (a skipped row's count is 0)
}

// byte j of the row's element (j < len), zero past the input
__device__ __forceinline__ uint32_t in_byte(const Sp& x, const BRow& b, uint32_t j) {
  const uint64_t p = (uint64_t)b.off + j;
  if (p >= x.a->in_bound) return 0u;
  return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(x.in, (uint32_t)p, 0, 0);
}

// K consecutive output dwords from byte j (a multiple of 4) of row r on, for widths that are a
// multiple of 4: each dword lies inside one row and is built from two aligned input dwords. In
// phases -- (the rows' entries in the row list,) the rows' views, then every input dword, then the
// lengths and counters -- so that the loads of a phase are in flight together; a dword with nothing
// to read (padding, a skipped row, or a view past the input) loads from past the buffer's bound,
// which gives zeros without a memory access. Returns the mask of the dwords whose row is not skipped.
template <int K, bool ROWS>
__device__ __forceinline__ uint32_t u8_dwords4(const Sp& x, Tally& t, uint32_t r, uint32_t j, uint32_t* w) {
  uint32_t rr[K], jj[K];
  BRow bb[K];
  Rec q[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    rr[k] = r;
    jj[k] = j;
    j += 4u;
    const bool wrap = j == x.W;
    r += wrap;
    j = wrap ? 0u : j;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) q[k] = row_rec<ROWS>(x, rr[k]);
#pragma unroll
  for (int k = 0; k < K; ++k) bb[k] = brow_of(x, q[k]);
  uint32_t d0[K], d1[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t p = (uint64_t)bb[k].off + jj[k];
    const bool ok = bb[k].len > jj[k] && p < x.a->in_bound;
    const uint32_t p0 = ok ? ((uint32_t)p & ~3u) : 0xfffffff8u;  // (in_bound <= 0xfffffff0: p0 + 4 does not wrap)
    d0[k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0, 0, 0);
    d1[k] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, p0 + 4u, 0, 0);
  }
  const uint32_t fill = ((uint32_t)x.s->fill & 0xffu) * 0x01010101u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t left = bb[k].len > jj[k] ? bb[k].len - jj[k] : 0u;
    const uint32_t m = left >= 4u ? 0xffffffffu : (1u << (8u * left)) - 1u;
    const uint32_t d = __builtin_amdgcn_alignbyte(d1[k], d0[k], (bb[k].off + jj[k]) & 3u);
    w[k] = (d & m) | (fill & ~m);
  }
  uint32_t okm = 0u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    okm |= q[k].ok << k;
    if (jj[k] == 0) note_brow<ROWS>(x, t, rr[k], q[k].ok, bb[k]);
  }
  return okm;
}

// The output dword at bytes j .. j + 3 of row r for any other width: byte by byte over row ends.
// Advances (r, j, b, ok) past it; `more`: the output goes on after it (the next row exists). Bit k of
// `okm` is set where byte k's row is not skipped.
template <bool ROWS>
__device__ __forceinline__ uint32_t u8_dword(const Sp& x, Tally& t, uint32_t& r, uint32_t& j, BRow& b, uint32_t& ok,
                                             bool more, uint32_t& okm) {
  const uint32_t fill = (uint32_t)x.s->fill & 0xffu;
  uint32_t w = 0u;
  okm = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (j == 0) note_brow<ROWS>(x, t, r, ok, b);
    w |= (j < b.len ? in_byte(x, b, j) : fill) << (8 * k);
    okm |= ok << k;
    if (++j == x.W) {
      j = 0;
      ++r;
      if (more || k < 3) b = brow_of<ROWS>(x, r, ok);
    }
  }
  return w;
}

// ------------------------------------------------------------------ stores of a unit with skipped rows
// the bytes of dword w at p whose bit in okm (4 bits) is set
template <bool NT>
__device__ __forceinline__ void st_bytes(uint8_t* p, uint32_t w, uint32_t okm) {
  if (okm == 0xfu) {
    st_nt<NT>(reinterpret_cast<uint32_t*>(p), w);
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((okm >> k) & 1u) p[k] = (uint8_t)(w >> (8 * k));
}

// ------------------------------------------------------------------ one workgroup's share of a spec
template <uint32_t DT, bool NT, bool ROWS>
__device__ __forceinline__ void dense_spec(const Sp& x, Tally& t, uint32_t wg) {
  constexpr uint32_t isz = DT == kDenseI64 ? 8u : DT == kDenseU8 ? 1u : 4u;
  // (n: the output's rows)
  const uint32_t n = ROWS ? x.a->m : x.a->n, W = x.W, nblk = x.s->nblk, tid = threadIdx.x;
  const uint32_t rowb = W * isz;                  // <= 32 KiB
  const uint64_t total = (uint64_t)n * rowb;      // bytes of the output
  uint8_t* const out = static_cast<uint8_t*>(x.s->out);
  const uint64_t units = ((uintptr_t)out & 15u) ? 0ull : total >> 4;

  // 16-byte units: chunk ch = wg, wg + nblk, ...; its first byte is row r0, byte j0 of the row
  if ((uint64_t)wg * kDenseChunk < units) {
    const uint64_t b0 = (uint64_t)wg * (kDenseChunk * 16u), step = (uint64_t)nblk * (kDenseChunk * 16u);
    uint64_t r0 = b0 / rowb;
    uint32_t j0 = (uint32_t)(b0 - r0 * rowb);
    const uint64_t sq = step / rowb;
    const uint32_t sr = (uint32_t)(step - sq * rowb);
    for (uint64_t u0 = (uint64_t)wg * kDenseChunk; u0 < units; u0 += (uint64_t)nblk * kDenseChunk) {
#pragma unroll
      for (uint32_t it = 0; it < kDenseChunk / 256u; ++it) {
        const uint32_t lu = it * 256u + tid;
        if (u0 + lu < units) {
          const uint32_t lo = lu * 16u + j0;  // < 16 KiB + 32 KiB
          const uint32_t q = lo / rowb;
          uint32_t r = (uint32_t)(r0 + q), j = lo - q * rowb;
          uint8_t* const p = out + ((u0 + lu) << 4);
          if constexpr (DT == kDenseU8) {
            uint32_t v[4], okm[4];
            if ((W & 3u) == 0u) {
              const uint32_t o4 = u8_dwords4<4, ROWS>(x, t, r, j, v);
#pragma unroll
              for (int k = 0; k < 4; ++k) okm[k] = ((o4 >> k) & 1u) ? 0xfu : 0u;
            } else {
              uint32_t ok;
              BRow b = brow_of<ROWS>(x, r, ok);
              v[0] = u8_dword<ROWS>(x, t, r, j, b, ok, true, okm[0]);
              v[1] = u8_dword<ROWS>(x, t, r, j, b, ok, true, okm[1]);
              v[2] = u8_dword<ROWS>(x, t, r, j, b, ok, true, okm[2]);
              v[3] = u8_dword<ROWS>(x, t, r, j, b, ok, false, okm[3]);
            }
            if (!ROWS || (okm[0] & okm[1] & okm[2] & okm[3]) == 0xfu) {
              dn_u32x4 o;
              o.x = v[0];
              o.y = v[1];
              o.z = v[2];
              o.w = v[3];
              st_nt<NT>(reinterpret_cast<dn_u32x4*>(p), o);
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k) st_bytes<NT>(p + 4 * k, v[k], okm[k]);
            }
          } else if constexpr (DT == kDenseI64) {
            uint64_t v[2];
            const uint32_t okm = values_from<DT, 2, ROWS>(x, t, r, j >> 3, v);
            if (!ROWS || okm == 3u) {
              dn_u64x2 o;
              o.x = v[0];
              o.y = v[1];
              st_nt<NT>(reinterpret_cast<dn_u64x2*>(p), o);
            } else {
#pragma unroll
              for (int k = 0; k < 2; ++k)
                if ((okm >> k) & 1u) st_nt<NT>(reinterpret_cast<uint64_t*>(p) + k, v[k]);
            }
          } else {
            uint32_t v[4];
            const uint32_t okm = values_from<DT, 4, ROWS>(x, t, r, j >> 2, v);
            if (!ROWS || okm == 0xfu) {
              dn_u32x4 o;
              o.x = v[0];
              o.y = v[1];
              o.z = v[2];
              o.w = v[3];
              st_nt<NT>(reinterpret_cast<dn_u32x4*>(p), o);
            } else {
#pragma unroll
              for (int k = 0; k < 4; ++k)
                if ((okm >> k) & 1u) st_nt<NT>(reinterpret_cast<uint32_t*>(p) + k, v[k]);
            }
          }
        }
      }
      r0 += sq;
      j0 += sr;
      if (j0 >= rowb) {
        j0 -= rowb;
        ++r0;
      }
    }
  }

  // the rest, element by element (one per lane, consecutive over the wave)
  uint64_t done = units << 4;  // bytes
  if constexpr (DT == kDenseU8) {
    const uint64_t dwords = ((uintptr_t)out & 3u) ? 0ull : (total - done) >> 2;
    for (uint64_t i = (uint64_t)wg * 256u + tid; i < dwords; i += (uint64_t)nblk * 256u) {
      const uint64_t pos = done + (i << 2);
      const uint64_t r64 = pos / W;
      uint32_t r = (uint32_t)r64, j = (uint32_t)(pos - r64 * W);
      uint32_t w, okm;
      if ((W & 3u) == 0u) {
        okm = u8_dwords4<1, ROWS>(x, t, r, j, &w) ? 0xfu : 0u;
      } else {
        // (every row the dword's four bytes touch is inside the output; a row after its last byte
        // exists only if the output goes on)
        uint32_t ok;
        BRow b = brow_of<ROWS>(x, r, ok);
        w = u8_dword<ROWS>(x, t, r, j, b, ok, pos + 4u < total, okm);
      }
      if constexpr (ROWS) st_bytes<NT>(out + pos, w, okm);
      else st_nt<NT>(reinterpret_cast<uint32_t*>(out + pos), w);
    }
    done += dwords << 2;
    for (uint64_t i = (uint64_t)wg * 256u + tid; done + i < total; i += (uint64_t)nblk * 256u) {
      const uint64_t pos = done + i;
      const uint64_t r64 = pos / W;
      const uint32_t r = (uint32_t)r64, j = (uint32_t)(pos - r64 * W);
      uint32_t ok;
      const BRow b = brow_of<ROWS>(x, r, ok);
      if (j == 0) note_brow<ROWS>(x, t, r, ok, b);
      if (ok) out[pos] = (uint8_t)(j < b.len ? in_byte(x, b, j) : ((uint32_t)x.s->fill & 0xffu));
    }
  } else {
    using T = typename ValT<DT>::type;
    const uint64_t e0 = done / isz, elems = (uint64_t)n * W;
    for (uint64_t i = e0 + (uint64_t)wg * 256u + tid; i < elems; i += (uint64_t)nblk * 256u) {
      const uint64_t r64 = i / W;
      T v;
      if (values_from<DT, 1, ROWS>(x, t, (uint32_t)r64, (uint32_t)(i - r64 * W), &v))
        st_nt<NT>(reinterpret_cast<T*>(out) + i, v);
    }
  }
}

template <bool NT, bool ROWS>
__device__ __forceinline__ void dense_body() {
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  // the workgroup's spec: the last one whose first block is not after this block
  uint32_t si = 0;
  while (si + 1u < a->n_specs && a->sp[si + 1u].blk0 <= blockIdx.x) ++si;
  const KSpec s = &a->sp[si];
  const uint32_t slot = s->slot;
  Sp x;
  x.a = a;
  x.s = s;
  x.W = s->width;
  x.base = a->slot_base[slot];
  x.rs = slot_splits(a, slot);
  x.in = bytes_source(a);
  if constexpr (ROWS) x.rl = make_row_list(a);
  const uint32_t wg = blockIdx.x - s->blk0;
  Tally t;
  switch (s->dtype) {
    case kDenseI64: dense_spec<kDenseI64, NT, ROWS>(x, t, wg); break;
    case kDenseI32: dense_spec<kDenseI32, NT, ROWS>(x, t, wg); break;
    case kDenseF32: dense_spec<kDenseF32, NT, ROWS>(x, t, wg); break;
    default: dense_spec<kDenseU8, NT, ROWS>(x, t, wg); break;
  }
  if constexpr (ROWS) {
    if (a->skipped) {
      const uint32_t sk = wave_sum32(t.skip);
      if ((threadIdx.x & 63u) == 0u && sk) atomicAdd(a->skipped + si, sk);
    }
  }
  uint32_t* const stats = a->stats;
  if (!stats) return;
  add_stats4(stats, si, t.trunc, t.pad, t.zero, t.multi);
}

template <bool NT>
__global__ __launch_bounds__(256) void k_dense(const DenseArgs) {
  dense_body<NT, false>();
}

// (behind tfrg_result_dense_rows)
template <bool NT>
__global__ __launch_bounds__(256) void k_dense_rows(const DenseArgs) {
  dense_body<NT, true>();
}

}  // namespace

hipError_t launch_dense(const DenseArgs& a, uint32_t blocks, hipStream_t st) {
  if (!blocks) return hipSuccess;
  if (a.rows) {
    if (a.nt) hipLaunchKernelGGL(k_dense_rows<true>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dense_rows<false>, dim3(blocks), dim3(256), 0, st, a);
  } else {
    if (a.nt) hipLaunchKernelGGL(k_dense<true>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_dense<false>, dim3(blocks), dim3(256), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace tfrg
