// tfrg_resize.hip — k_resize: raw images of per-record size (H and W are int64 features of the record)
// cropped, optionally mirrored, resampled to a fixed out_h x out_w, normalised per channel and written
// interleaved or planar, behind tfrg_result_raw_resize. One launch for all specs (the blk0 table, as
// k_raw's). The function computed (integer coordinates, float32 fused multiply-adds) is in include/tfrg.h.
//
// Work split. A work item is a BAND of kResizeBand consecutive output rows of one list entry; the
// workgroups of a spec stride over its m * bands items. The item resolves its row once, uniformly, in
// scalar registers: row entry -> record (the row rule of tfrg_rows.h) -> row splits -> the element's
// offset and length (resolve_at, shared with k_raw) -> H and W from the int64 columns -> box -> flip.
//
// Streamed separable resample. The column table (per output column: the byte offsets of its two taps in
// a crop row, packed in one word, and fx; the mirror is folded in) is built once per item in LDS. The
// source rows that some output row of the band taps are then visited top to bottom: their sequence is
// increasing, and a row is new exactly when it is above every row visited so far. Each is read from
// HBM once per band with k_raw's source-side scheme (aligned 16-byte buffer loads bounded to the
// readable input, realigned in registers, written to the padded LDS stage), resampled horizontally ONCE
// into one slot of a ring of two rows of out_w * channels float32, and every output row between two
// consecutive ring rows is emitted from the ring: vertical lerp, normalise, convert, store. The new row
// always takes the slot of the older one, so the slots alternate and the two taps of an output row are
// the last two rows visited. A downscale never reads the rows it skips; an upscale reads each row once
// however many output rows use it. The ring is held in OUTPUT order (planar: plane after plane), so the
// emit reads it consecutively and the gather (a stride of `channels` elements) is paid in the
// horizontal pass, which gathers anyway.
//
// Prefetch. The 16-byte loads of the next row to visit are issued before the current row is resampled
// and emitted and stay in registers (kPasses units per lane) until the stage is free.
//
// Stores. As k_raw's: a lane assembles whole 16-byte units of an output row (interleaved) or plane row
// (planar), lane-consecutive within it; the elements before the first whole unit and after the last are
// stored one by one. Nontemporal in k_resize<true> (TFRG_DENSE_NT).
//
// LDS: the stage (kResizeStageWords), the ring and the table; the last two sized by the launch for its
// largest out_w * channels (dynamic LDS: 24 KiB for 224 x 3, 81 KiB at the limits).
#include <hip/hip_runtime.h>

#include "tfrg_resize_dev.h"

namespace tfrg {
namespace {

typedef uint32_t rs_u32x2 __attribute__((ext_vector_type(2)));

// passes of 4 waves x 63 new units over a crop row and the unit that feeds the last lane
constexpr uint32_t kPasses = (kResizeMaxRowBytes / 16u + 1u + 251u) / 252u;
constexpr uint32_t kStageData = kData + kResizeMaxRowBytes / 4u + 4u;
static_assert(kStageData + kStageData / 32u < kResizeStageWords, "a crop row fits the stage");
static_assert((kResizeStageWords & 1u) == 0u, "the column table is 8-byte aligned");

// ------------------------------------------------------------------ coordinates
struct Ax {
  uint32_t i0, i1;
  float f;
};

// output index o of N along a source axis of n samples (include/tfrg.h)
__device__ __forceinline__ Ax axis(uint32_t o, uint32_t n, uint32_t N, bool nearest) {
  const uint32_t last = n - 1u, c = (2u * o + 1u) * n;  // (below 2^27)
  if (nearest) {
    const uint32_t i = c / (2u * N);
    return Ax{i < last ? i : last, i < last ? i : last, 0.f};
  }
  const uint32_t den = 2u * N;
  uint32_t i0 = 0u;
  float f = 0.f;
  if (c >= N) {
    const uint32_t num = c - N;
    i0 = num / den;
    f = (float)(num - i0 * den) / (float)den;
  }
  if (i0 >= last) return Ax{last, last, 0.f};
  return Ax{i0, i0 + 1u, f};
}

// ------------------------------------------------------------------ source side
// The crop row's bytes [s0, s0 + vbytes): the aligned units that hold them, into registers ...
__device__ __forceinline__ void row_load(const Sp& x, uint64_t s0, uint32_t vbytes, rw_u32x4 (&d)[kPasses]) {
  const uint32_t sh = (uint32_t)s0 & 15u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t a0 = s0 - sh;
  const uint32_t nun = (sh + vbytes + 15u) >> 4;
  const uint32_t bound = x.a->in_bound;
#pragma unroll
  for (uint32_t p = 0; p < kPasses; ++p) {
    d[p] = rw_u32x4{0u, 0u, 0u, 0u};
    if (p * 252u < nun) {
      const uint32_t u = (p * 4u + wv) * 63u + lane;
      const uint64_t pos = a0 + ((uint64_t)u << 4);
      const bool ok = u < nun && pos < bound;
      d[p] = __builtin_bit_cast(rw_u32x4, __builtin_amdgcn_raw_buffer_load_b128(x.in, ok ? (uint32_t)pos : 0xfffffff0u, 0, 0));
    }
  }
}

// ... and from there realigned into the stage, byte s0 at word kData (k_raw's layout)
__device__ __forceinline__ void row_store(uint32_t* L, uint64_t s0, uint32_t vbytes, const rw_u32x4 (&d)[kPasses]) {
  const uint32_t sh = (uint32_t)s0 & 15u, q = sh >> 2, bs = sh & 3u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t nun = (sh + vbytes + 15u) >> 4;
#pragma unroll
  for (uint32_t p = 0; p < kPasses; ++p) {
    if (p * 252u < nun) {
      const uint32_t u = (p * 4u + wv) * 63u + lane;
      const uint32_t nx = (uint32_t)__shfl_down((int)d[p].x, 1, 64);  // (the right neighbour's first dword)
      if (lane < 63u && u < nun) {
        const uint32_t w = kData + 4u * u - q;
        L[swz(w + 0u)] = __builtin_amdgcn_alignbyte(d[p].y, d[p].x, bs);
        L[swz(w + 1u)] = __builtin_amdgcn_alignbyte(d[p].z, d[p].y, bs);
        L[swz(w + 2u)] = __builtin_amdgcn_alignbyte(d[p].w, d[p].z, bs);
        L[swz(w + 3u)] = __builtin_amdgcn_alignbyte(nx, d[p].w, bs);
      }
    }
  }
}

// ------------------------------------------------------------------ horizontal pass
// The staged crop row resampled into a ring slot, in output order: element (ox, c) at c * OW + ox
// (planar) or ox * C + c. inv: 65536 / C rounded up, which divides indices below 32768 by C exactly.
template <uint32_t SRC>
__device__ __forceinline__ void hpass(const uint32_t* L, const rs_u32x2* tabl, uint32_t* ring, uint32_t OW, uint32_t C,
                                      bool planar, uint32_t inv, uint32_t mode) {
  constexpr uint32_t ESZ = raw_src_size(SRC);
  const auto one = [&](uint32_t ox, uint32_t c, uint32_t e) {
    const rs_u32x2 t = tabl[ox];
    const uint32_t fx = t.y;  // (a copy: __builtin_bit_cast of a vector's element reads element 0)
    const uint32_t r0 = ld_elem<ESZ>(L, (t.x & 0xffffu) + c * ESZ);
    uint32_t o = r0;
    if (mode == kTake) {
      o = __builtin_bit_cast(uint32_t, to_f32<SRC>(r0));
    } else if (mode == kLerp) {
      const float v0 = to_f32<SRC>(r0), v1 = to_f32<SRC>(ld_elem<ESZ>(L, (t.x >> 16) + c * ESZ));
      o = __builtin_bit_cast(uint32_t, __builtin_fmaf(__builtin_bit_cast(float, fx), v1 - v0, v0));
    }
    ring[e] = o;
  };
  if (planar) {
    for (uint32_t c = 0; c < C; ++c)
      for (uint32_t ox = threadIdx.x; ox < OW; ox += 256u) one(ox, c, c * OW + ox);
  } else {
    for (uint32_t e = threadIdx.x; e < OW * C; e += 256u) {
      const uint32_t ox = (e * inv) >> 16;
      one(ox, e - ox * C, e);
    }
  }
}

__device__ __forceinline__ void hpass_any(uint32_t src, const uint32_t* L, const rs_u32x2* tabl, uint32_t* ring, uint32_t OW,
                                          uint32_t C, bool planar, uint32_t inv, uint32_t mode) {
  switch (src) {
    case kRawU8: hpass<kRawU8>(L, tabl, ring, OW, C, planar, inv, mode); break;
    case kRawI8: hpass<kRawI8>(L, tabl, ring, OW, C, planar, inv, mode); break;
    case kRawU16: hpass<kRawU16>(L, tabl, ring, OW, C, planar, inv, mode); break;
    case kRawI16: hpass<kRawI16>(L, tabl, ring, OW, C, planar, inv, mode); break;
    case kRawI32: hpass<kRawI32>(L, tabl, ring, OW, C, planar, inv, mode); break;
    case kRawF16: hpass<kRawF16>(L, tabl, ring, OW, C, planar, inv, mode); break;
    case kRawBF16: hpass<kRawBF16>(L, tabl, ring, OW, C, planar, inv, mode); break;
    default: hpass<kRawF32>(L, tabl, ring, OW, C, planar, inv, mode); break;
  }
}

// ------------------------------------------------------------------ the kernel
template <bool NT>
__global__ __launch_bounds__(256) void k_resize(const ResizeArgs) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  __shared__ rw_f32x2 tab[kResizeMaxChannels];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  uint32_t si = 0;
  while (si + 1u < a->n_specs && a->sp[si + 1u].blk0 <= blockIdx.x) ++si;
  const KSpec s = &a->sp[si];
  if (threadIdx.x < kResizeMaxChannels) tab[threadIdx.x] = rw_f32x2{s->scale[threadIdx.x], s->bias[threadIdx.x]};
  __syncthreads();
  const Sp x = spec_view(a, si);
  const uint32_t OW = s->out_w, OH = s->out_h, C = s->channels, rn = OW * C, src = s->src;
  const uint32_t pix = C * raw_src_size(src), inv = (65536u + C - 1u) / C;
  const bool planar = s->planar != 0u && C > 1u, nearest = s->interp == kResizeNearest;
  const uint32_t hmode = s->outt == kRawOutSame ? kBits : nearest ? kTake : kLerp;
  uint32_t* const stage = lds;
  uint32_t* const ring = lds + kResizeStageWords;
  rs_u32x2* const tabl = reinterpret_cast<rs_u32x2*>(ring + 2u * rn);
  const uint32_t bands = s->bands, nblk = s->nblk;
  const uint64_t items = (uint64_t)a->m * bands;
  Counts cnts;
  for (uint64_t it = blockIdx.x - s->blk0; it < items; it += nblk) {
    const uint32_t k = (uint32_t)(it / bands), band = (uint32_t)(it - (uint64_t)k * bands);
    const uint32_t oy0 = band * kResizeBand, oy1 = oy0 + kResizeBand < OH ? oy0 + kResizeBand : OH;
    const Geo geo = row_geometry(x, k, band == 0u, cnts);
    if (!geo.live) continue;
    const bool flip = geo.flip;
    Taps t{ring, ring, 0.f, kFill};
    if (!geo.box_ok) {  // (a bad shape or a bad box: the band is fill; no LDS is touched)
      for (uint32_t oy = oy0; oy < oy1; ++oy) emit_any<NT>(x, tab, t, k, oy, inv);
      continue;
    }
    // the column table
    const uint32_t ucw = geo.cw, uch = geo.ch, vbytes = ucw * pix;
    for (uint32_t ox = threadIdx.x; ox < OW; ox += 256u) {
      const Ax c = axis(flip ? OW - 1u - ox : ox, ucw, OW, nearest);
      tabl[ox] = rs_u32x2{(c.i0 * pix) | ((c.i1 * pix) << 16), __builtin_bit_cast(uint32_t, c.f)};
    }
    // crop row r starts at this byte of the input
    const uint64_t s00 = (uint64_t)geo.row.off + ((uint64_t)geo.top * geo.W + geo.left) * pix;
    const uint64_t pitch = geo.W * pix;
    // the rows to visit, in order: the taps of oy0, oy0 + 1, ... that are above every row before them
    uint32_t gen_oy = oy0;
    int32_t gen_max = -1;
    const auto next_row = [&]() -> int32_t {
      for (; gen_oy < oy1; ++gen_oy) {
        const Ax y = axis(gen_oy, uch, OH, nearest);
        const int32_t r0 = (int32_t)rfl32(y.i0), r1 = (int32_t)rfl32(y.i1);
        if (r0 > gen_max) return gen_max = r0;
        if (r1 > gen_max) return gen_max = r1;
      }
      return -1;
    };
    rw_u32x4 d[kPasses];
    int32_t nxt = next_row(), staged = -1;  // (a band has a row: nxt is one)
    uint64_t nxt_s0 = s00 + (uint64_t)(uint32_t)nxt * pitch;
    row_load(x, nxt_s0, vbytes, d);
    uint32_t cnt = 0;
    for (uint32_t oy = oy0; oy < oy1; ++oy) {
      const Ax y = axis(oy, uch, OH, nearest);
      const int32_t r0 = (int32_t)rfl32(y.i0), r1 = (int32_t)rfl32(y.i1);
      while (staged < r1) {
        row_store(stage, nxt_s0, vbytes, d);
        __syncthreads();  // (the stage and the table are written; the emits before this read the ring)
        staged = nxt;
        nxt = next_row();
        if (nxt >= 0) {
          nxt_s0 = s00 + (uint64_t)(uint32_t)nxt * pitch;
          row_load(x, nxt_s0, vbytes, d);  // (in flight while this row is resampled and emitted)
        }
        hpass_any(src, stage, tabl, ring + (cnt & 1u) * rn, OW, C, planar, inv, hmode);
        ++cnt;
        __syncthreads();  // (the ring slot is written, the stage is free)
      }
      // the lower tap is the last row visited; the upper one is that row too, or the one before it
      t.rb = ring + ((cnt - 1u) & 1u) * rn;
      t.ra = r0 == r1 ? t.rb : ring + (cnt & 1u) * rn;
      t.fy = __builtin_bit_cast(float, rfl32(__builtin_bit_cast(uint32_t, y.f)));
      t.mode = hmode;
      emit_any<NT>(x, tab, t, k, oy, inv);
    }
    __syncthreads();  // (the next item builds its table and ring over these)
  }
  report(a, si, cnts);
}

}  // namespace

hipError_t launch_resize(const ResizeArgs& a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st) {
  if (!blocks) return hipSuccess;
  return a.nt ? launch_sized(k_resize<true>, a, blocks, lds_bytes, st) : launch_sized(k_resize<false>, a, blocks, lds_bytes, st);
}

}  // namespace tfrg
