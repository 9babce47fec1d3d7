// tfrg_raw.hip — k_raw: tensors stored as bytes (tf.io.decode_raw + cast + per-channel scale and bias +
// HWC -> CHW) behind tfrg_result_raw_rows. One launch writes, for every spec, out[k][count] for the m
// rows of a row list: element 0 of record g's bytes_list read as `count` little-endian elements of the
// source type, each converted to float32, y = fmaf(v, scale[c], bias[c]), rounded once to the output
// type; or copied bit for bit (TFRG_RAW_OUT_SAME). Elements the record does not have are `fill`.
//
// Work split. Rows are long, so the unit of work is a TILE of one row: raw_tile_pixels(channels)
// pixels of `channels` elements each (at most kRawTile = 4096 elements, a multiple of 16 pixels). A work
// item is kRawSpan consecutive tiles of one row; the workgroups of a spec (found through the blk0
// table, as k_dense's) stride over its m * spans items. A work item resolves its row ONCE, uniformly:
// row entry -> record (the row rule of tfrg_rows.h) -> row splits -> the element's offset and length,
// held in scalar registers; nothing is looked up per lane or per dword. Rows of at most kRawNarrow =
// 1024 elements take the second shape: a wave per row, four rows per workgroup at a time, the same tile
// code run by 64 lanes on a quarter of the LDS with a wave barrier for the workgroup barrier.
//
// Source side. The tile's source bytes start at an arbitrary byte s0 of the batch. The group reads the
// aligned 16-byte units that cover them, lane-consecutively, with one buffer load each through the
// resource bounded to the readable input (a unit at or past in_bound, or past the element's valid
// bytes, is addressed past the bound: zeros, no memory access). The bytes are realigned in registers:
// a lane takes the first dword of its right neighbour's unit (one cross-lane move), shifts its five
// dwords by s0 & 3 with v_alignbyte, and writes four dwords to LDS displaced by (s0 & 15) >> 2 dwords,
// so the tile's first byte lands on a fixed LDS word and every element is naturally aligned there. The
// last lane of a wave only feeds its neighbour: waves overlap by one unit (63 new units per wave and
// pass), which re-reads one line in 64 from the cache. Every input line is fetched once per tile.
//
// Convert and store. A lane assembles whole 16-byte units of the OUTPUT: 16 / osz consecutive elements
// of the row (interleaved), or of one channel plane (planar: LDS is read back with a stride of
// `channels` elements, which is the de-interleave). Units are dealt lane-consecutively within a run (a
// row's tile, or one plane's share of it; the planes' runs are laid end to end over the lanes), so a
// store instruction writes whole 128-byte lines (global stores, nontemporal in k_raw<true>, which
// launch_raw picks under TFRG_DENSE_NT as launch_dense picks k_dense<true>). The tile starts a multiple of 16 elements into its
// row or plane, so only the run's base address decides where 16-byte units begin: the elements before
// the first whole unit and after the last one (a plane or row size, or an out pointer, that is not a
// multiple of 16 bytes) are stored one by one. LDS layout: the staged bytes are padded by one dword per
// 32 (word w lives at w + w / 32), so that the planar read -- lane stride 16 / osz * channels * esz
// bytes, 32 bytes for uint8 RGBA to bf16 -- does not fold the wave onto 8 banks.
//
// Rounding: int32 -> float32 and float32 -> float16 / bfloat16 are the hardware's RNE converts
// (v_cvt_f32_i32, v_cvt_pk_f16_f32, v_cvt_pk_bf16_f32); the product and sum are one fmaf.
#include <hip/hip_runtime.h>

#include "tfrg_raw.h"
#include "tfrg_raw_dev.h"
#include "tfrg_internal.h"
#include "tfrg_rows.h"

namespace tfrg {
namespace {

typedef const __attribute__((address_space(4))) RawArgs* KArgs;
typedef const __attribute__((address_space(4))) RawSpec* KSpec;

// LDS of a workgroup in words: kData words of slack (tfrg_raw_dev.h), a tile's 4096 words, one unit of
// overrun, and the padding of one word per 32. A wave of the narrow shape has a quarter of it (its tile is
// at most 1024 words).
constexpr uint32_t kLdsWords = 4352;
constexpr uint32_t kWaveWords = kLdsWords / 4;
static_assert(kData + kRawTile + 4 + (kData + kRawTile + 4) / 32 < kLdsWords, "a workgroup's tile fits");
static_assert(kData + kRawNarrow + 4 + (kData + kRawNarrow + 4) / 32 < kWaveWords, "a wave's tile fits");

// the spec a workgroup works in (uniform)
struct Sp {
  KArgs a;
  KSpec s;
  const uint32_t* rs;  // the slot's row splits; null: placed
  uint64_t base;       // slot_base[slot]
  __amdgpu_buffer_rsrc_t in;
  RowList rl;
};

// The threads that work on one tile: the workgroup (wide rows) or one wave (narrow rows)
struct Grp {
  uint32_t* L;  // its LDS
  uint32_t t;   // the thread's index in it
  uint32_t n;   // its threads
  uint32_t w;   // the thread's wave in it
  uint32_t nw;  // its waves
  bool wide;
};

__device__ __forceinline__ void grp_sync(const Grp& g) {
  if (g.wide) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------ source side
// The tile's source bytes [s0, s0 + vbytes) into LDS, byte s0 at word kData. In two phases, so that
// the loads of every pass are in flight together.
template <uint32_t ESZ>
__device__ __forceinline__ void stage(const Sp& x, const Grp& g, uint64_t s0, uint32_t vbytes) {
  constexpr uint32_t kPasses = (kRawTile * ESZ / 16u + 1u + 251u) / 252u;
  static_assert((kRawNarrow * ESZ / 16u + 1u + 62u) / 63u <= kPasses, "a wave's passes over a narrow row");
  const uint32_t sh = (uint32_t)s0 & 15u, q = sh >> 2, bs = sh & 3u, lane = threadIdx.x & 63u;
  const uint64_t a0 = s0 - sh;
  const uint32_t nun = vbytes ? (sh + vbytes + 15u) >> 4 : 0u;  // aligned units that hold the bytes
  const uint32_t bound = x.a->in_bound;
  rw_u32x4 d[kPasses];
#pragma unroll
  for (uint32_t p = 0; p < kPasses; ++p) {
    const uint32_t u = (p * g.nw + g.w) * 63u + lane;
    const uint64_t pos = a0 + ((uint64_t)u << 4);
    const bool ok = u < nun && pos < bound;
    d[p] = __builtin_bit_cast(rw_u32x4, __builtin_amdgcn_raw_buffer_load_b128(x.in, ok ? (uint32_t)pos : 0xfffffff0u, 0, 0));
  }
#pragma unroll
  for (uint32_t p = 0; p < kPasses; ++p) {
    const uint32_t u = (p * g.nw + g.w) * 63u + lane;
    const uint32_t nx = (uint32_t)__shfl_down((int)d[p].x, 1, 64);  // (the right neighbour's first dword)
    if (lane < 63u && u < nun) {
      const uint32_t w = kData + 4u * u - q;
      g.L[swz(w + 0u)] = __builtin_amdgcn_alignbyte(d[p].y, d[p].x, bs);
      g.L[swz(w + 1u)] = __builtin_amdgcn_alignbyte(d[p].z, d[p].y, bs);
      g.L[swz(w + 2u)] = __builtin_amdgcn_alignbyte(d[p].w, d[p].z, bs);
      g.L[swz(w + 3u)] = __builtin_amdgcn_alignbyte(nx, d[p].w, bs);
    }
  }
}

// ------------------------------------------------------------------ convert
// where a lane's elements come from and what they are (per lane)
struct Run {
  uint32_t b0, bstr;  // LDS byte of its first element, bytes between consecutive ones
  uint32_t j0, jstr;  // the first element's index in the row, and the step
  uint32_t ch, chinc; // its channel; 0: the next one has the same (planar), 1: the next (interleaved)
};

// K consecutive elements of a run as output bits (K = 1, or the 16 / osz of a unit)
template <uint32_t SRC, uint32_t OUT, uint32_t K>
__device__ __forceinline__ void elems(const Sp& x, const uint32_t* L, const rw_f32x2* tab, const Run& r, uint32_t nvalid,
                                      uint32_t* o) {
  constexpr uint32_t ESZ = raw_src_size(SRC);
  const uint32_t C = x.s->channels, fill = x.s->fill;
  uint32_t raw[K];
  bool ex[K];
#pragma unroll
  for (uint32_t i = 0; i < K; ++i) {
    raw[i] = ld_elem<ESZ>(L, r.b0 + i * r.bstr);
    ex[i] = r.j0 + i * r.jstr < nvalid;
  }
  if constexpr (OUT == kRawOutSame) {
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) o[i] = ex[i] ? raw[i] : fill;
  } else {
    float y[K];
    // (one channel: scale and bias straight from the kernel argument; else from their table in LDS)
    float sc = x.s->scale[0], bi = x.s->bias[0];
    uint32_t ch = r.ch;
    if (C > 1u && !r.chinc) {
      const rw_f32x2 t = tab[ch];
      sc = t.x;
      bi = t.y;
    }
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) {
      if (C > 1u && r.chinc) {
        const rw_f32x2 t = tab[ch];
        sc = t.x;
        bi = t.y;
        ch = ch + 1u == C ? 0u : ch + 1u;
      }
      y[i] = __builtin_fmaf(to_f32<SRC>(raw[i]), sc, bi);
    }
    if constexpr (OUT == kRawOutF32) {
#pragma unroll
      for (uint32_t i = 0; i < K; ++i) o[i] = ex[i] ? __builtin_bit_cast(uint32_t, y[i]) : fill;
    } else if constexpr (K == 1) {
      o[0] = ex[0] ? cvt2<OUT>(y[0], y[0]) & 0xffffu : fill;
    } else {
#pragma unroll
      for (uint32_t i = 0; i < K; i += 2) {
        const uint32_t p = cvt2<OUT>(y[i], y[i + 1]);
        o[i] = ex[i] ? p & 0xffffu : fill;
        o[i + 1] = ex[i + 1] ? p >> 16 : fill;
      }
    }
  }
}

// ------------------------------------------------------------------ one tile
// Tile t of output row k: elements [e0, e0 + ne) of the row (pixels [p0, p0 + ne / C) of every plane),
// of which those below nvalid exist in the record.
template <uint32_t SRC, uint32_t OUT, bool NT>
__device__ __forceinline__ void tile(const Sp& x, const Grp& g, const rw_f32x2* tab, const RowSrc& row, uint32_t k,
                                     uint32_t t, uint32_t nvalid) {
  constexpr uint32_t ESZ = raw_src_size(SRC), OSZ = raw_out_size(SRC, OUT), EU = 16u / OSZ;
  const uint32_t C = x.s->channels, count = x.s->count, TP = raw_tile_pixels(C), T = TP * C;
  const bool planar = x.s->planar != 0u && C > 1u;
  const uint32_t e0 = t * T, ne = count - e0 < T ? count - e0 : T;
  const uint32_t vel = e0 < nvalid ? (nvalid - e0 < ne ? nvalid - e0 : ne) : 0u;
  stage<ESZ>(x, g, (uint64_t)row.off + (uint64_t)e0 * ESZ, vel * ESZ);
  grp_sync(g);

  // runs: the row's tile, or its share of every plane
  const uint32_t plane = count / C, p0 = t * TP;
  const uint32_t nruns = planar ? C : 1u, n = planar ? ne / C : ne, slots = n / EU;
  const uint64_t rowA = (uint64_t)(uintptr_t)x.s->out + (uint64_t)k * count * OSZ;
  const uint32_t total = nruns * slots;
  for (uint32_t f = g.t; f < total; f += g.n) {
    const uint32_t c = planar ? f / slots : 0u, u = f - c * slots;
    const uint64_t A = rowA + (planar ? (uint64_t)c * plane + p0 : (uint64_t)e0) * OSZ;
    uint32_t hA = ((16u - ((uint32_t)A & 15u)) & 15u) / OSZ;  // elements before the first whole unit
    hA = hA < n ? hA : n;
    if (u < (n - hA) / EU) {
      const uint32_t i0 = hA + u * EU, el = planar ? i0 * C + c : i0;
      const Run r{el * ESZ, (planar ? C : 1u) * ESZ, e0 + el, planar ? C : 1u, planar ? c : i0 % C, planar ? 0u : 1u};
      uint32_t o[EU];
      elems<SRC, OUT, EU>(x, g.L, tab, r, nvalid, o);
      rw_u32x4 v;
      if constexpr (OSZ == 4) {
        v = rw_u32x4{o[0], o[1], o[2], o[3]};
      } else if constexpr (OSZ == 2) {
        v = rw_u32x4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)};
      } else {
        v = rw_u32x4{o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24), o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24),
                     o[8] | (o[9] << 8) | (o[10] << 16) | (o[11] << 24),
                     o[12] | (o[13] << 8) | (o[14] << 16) | (o[15] << 24)};
      }
      st<NT>(A + (uint64_t)i0 * OSZ, v);
    }
  }
  // the elements of a run before its first and after its last whole unit, one per lane
  for (uint32_t c = 0; c < nruns; ++c) {
    const uint64_t A = rowA + (planar ? (uint64_t)c * plane + p0 : (uint64_t)e0) * OSZ;
    uint32_t hA = ((16u - ((uint32_t)A & 15u)) & 15u) / OSZ;
    hA = hA < n ? hA : n;
    const uint32_t nu = (n - hA) / EU, rest = n - nu * EU;  // (rest < 2 * EU <= 32)
    if (g.t < rest) {
      const uint32_t i = g.t < hA ? g.t : nu * EU + g.t, el = planar ? i * C + c : i;
      const Run r{el * ESZ, 0u, e0 + el, 0u, planar ? c : i % C, 0u};
      uint32_t o;
      elems<SRC, OUT, 1>(x, g.L, tab, r, nvalid, &o);
      const uint64_t p = A + (uint64_t)i * OSZ;
      if constexpr (OSZ == 4) st<false>(p, o);
      else if constexpr (OSZ == 2) st<false>(p, (uint16_t)o);
      else st<false>(p, (uint8_t)o);
    }
  }
  grp_sync(g);  // (the next tile is staged over this one)
}

// ------------------------------------------------------------------ one workgroup's share of a spec
template <uint32_t SRC, uint32_t OUT, bool NT>
__device__ __forceinline__ void raw_spec(const Sp& x, uint32_t* lds, const rw_f32x2* tab, uint32_t wg, uint32_t si) {
  constexpr uint32_t ESZ = raw_src_size(SRC);
  const uint32_t count = x.s->count, C = x.s->channels, m = x.a->m, nblk = x.s->nblk;
  const uint32_t tiles = (count / C + raw_tile_pixels(C) - 1u) / raw_tile_pixels(C);
  const bool wide = count > kRawNarrow;
  const uint32_t lane = threadIdx.x & 63u, wv = rfl32(threadIdx.x >> 6);
  Grp g;
  g.wide = wide;
  g.L = wide ? lds : lds + wv * kWaveWords;
  g.t = wide ? threadIdx.x : lane;
  g.n = wide ? 256u : 64u;
  g.w = wide ? wv : 0u;
  g.nw = wide ? 4u : 1u;
  const uint32_t spans = wide ? x.s->spans : 1u;
  const uint64_t items = (uint64_t)m * spans;
  const uint64_t first = wide ? (uint64_t)wg : (uint64_t)wg * 4u + wv, step = wide ? (uint64_t)nblk : (uint64_t)nblk * 4u;
  const uint64_t width = (uint64_t)count * ESZ;
  // (per group and uniform; a workgroup's waves all hold the same: its first one reports them)
  uint32_t trunc = 0, pad = 0, zero = 0, multi = 0, skip = 0;
  for (uint64_t it = first; it < items; it += step) {
    const uint32_t k = (uint32_t)(it / spans), sp = (uint32_t)(it - (uint64_t)k * spans);
    const RowSrc row = resolve(x, k);
    if (!row.ok) {
      skip += sp == 0u;
      continue;
    }
    if (sp == 0u) {
      if (g.t == 0u && x.s->lengths) x.s->lengths[k] = (int32_t)row.len;
      trunc += row.len > width;
      pad += row.len < width;
      zero += row.cnt == 0u;
      multi += row.cnt > 1u;
    }
    // source element j exists iff (j + 1) * esz <= len
    const uint32_t have = row.len / ESZ, nvalid = have < count ? have : count;
    const uint32_t t1 = (sp + 1u) * kRawSpan < tiles ? (sp + 1u) * kRawSpan : tiles;
    for (uint32_t t = sp * kRawSpan; t < t1; ++t) tile<SRC, OUT, NT>(x, g, tab, row, k, t, nvalid);
  }
  if (lane == 0u && g.w == 0u) {
    if (x.a->skipped && skip) atomicAdd(x.a->skipped + si, skip);
    if (uint32_t* const stats = x.a->stats) {
      if (trunc) atomicAdd(stats + 4u * si + 0, trunc);
      if (pad) atomicAdd(stats + 4u * si + 1, pad);
      if (zero) atomicAdd(stats + 4u * si + 2, zero);
      if (multi) atomicAdd(stats + 4u * si + 3, multi);
    }
  }
}

template <bool NT>
__global__ __launch_bounds__(256) void k_raw(const RawArgs) {
  __shared__ uint32_t lds[kLdsWords];
  __shared__ rw_f32x2 tab[kRawMaxChannels];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  uint32_t si = 0;
  while (si + 1u < a->n_specs && a->sp[si + 1u].blk0 <= blockIdx.x) ++si;
  const KSpec s = &a->sp[si];
  if (threadIdx.x < kRawMaxChannels) tab[threadIdx.x] = rw_f32x2{s->scale[threadIdx.x], s->bias[threadIdx.x]};
  __syncthreads();
  Sp x;
  x.a = a;
  x.s = s;
  x.base = a->slot_base[s->slot];
  x.rs = slot_splits(a, s->slot);
  x.in = bytes_source(a);
  x.rl = make_row_list(a);
  const uint32_t wg = blockIdx.x - s->blk0;
  // (OUT_SAME copies bits: one instance per element size)
  const uint32_t src = s->src, out = s->outt;
  if (out == kRawOutSame) {
    switch (raw_src_size(src)) {
      case 1: raw_spec<kRawU8, kRawOutSame, NT>(x, lds, tab, wg, si); break;
      case 2: raw_spec<kRawU16, kRawOutSame, NT>(x, lds, tab, wg, si); break;
      default: raw_spec<kRawF32, kRawOutSame, NT>(x, lds, tab, wg, si); break;
    }
    return;
  }
#define TFRG_RAW_CASE(S)                                                              \
  case S:                                                                             \
    if (out == kRawOutF32) raw_spec<S, kRawOutF32, NT>(x, lds, tab, wg, si);              \
    else if (out == kRawOutF16) raw_spec<S, kRawOutF16, NT>(x, lds, tab, wg, si);         \
    else raw_spec<S, kRawOutBF16, NT>(x, lds, tab, wg, si);                               \
    break;
  switch (src) {
    TFRG_RAW_CASE(kRawU8)
    TFRG_RAW_CASE(kRawI8)
    TFRG_RAW_CASE(kRawU16)
    TFRG_RAW_CASE(kRawI16)
    TFRG_RAW_CASE(kRawI32)
    TFRG_RAW_CASE(kRawF16)
    TFRG_RAW_CASE(kRawBF16)
    default:
      TFRG_RAW_CASE(kRawF32)
  }
#undef TFRG_RAW_CASE
}

}  // namespace

hipError_t launch_raw(const RawArgs& a, uint32_t blocks, hipStream_t st) {
  if (!blocks) return hipSuccess;
  if (a.nt) hipLaunchKernelGGL(k_raw<true>, dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_raw<false>, dim3(blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
