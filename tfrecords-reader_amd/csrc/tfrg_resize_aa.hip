// tfrg_resize_aa.hip — k_resize_aa: the antialiased specs of tfrg_result_raw_resize (interp has
// TFRG_RESIZE_ANTIALIAS). The function is the triangle filter of include/tfrg.h: per axis the integer
// weights w_j = max(0, 2M - |(2j + 1) N - (2o + 1) n|), a float32 accumulation of fmaf(w, v, acc) over the
// window, times 1 / (float)S. Rows, boxes, flips, bad rows and counters are k_resize's (tfrg_resize_dev.h).
//
// Work split. A work item is a BAND of resize_aa_band(out_w * channels) consecutive output rows of one
// list entry (8 at 224 x 3). Its windows cover the contiguous crop rows [first tap of its first row, last
// tap of its last row]; every one of them is read and used. Neighbouring bands re-read about one window.
//
// Groups. The band's crop rows are visited in GROUPS of up to resize_aa_group() rows (4 at 224 x 3; fewer
// where fewer crop rows fit the 17 KiB stage: each row keeps k_raw's padded layout at its own stride).
// All 256 lanes share a group's 16-byte units flat over (row, unit): a lane loads an aligned unit and the
// first dword of the next one (bounded to the readable input), so the realign needs no neighbour lane and
// a 1.5 KiB row does not leave most of the workgroup without a load. The units of the next group are
// issued before the current one is resampled and wait in registers (kAaPasses units per lane).
//
// Horizontal pass: (row of the group, output element) over the lanes. The column table holds, per output
// column, the byte offset of the first tap and the tap count in one word, the signed distance d of the
// first tap and 1 / Sx, the mirror folded in; a lane walks its window with d += 2N and w = 2M - |d|: no
// weight table, whose size would have no bound. The result is a group of float32 rows in OUTPUT order
// (planar: plane after plane), as k_resize's ring.
//
// Vertical pass: a lane owns the output elements e = tid + 256 i. For each output row of the band whose
// window meets the group it adds wy * h[r][e] over the group's rows to the row's accumulator, which lies
// in LDS at an address only that lane touches; wy is uniform (scalar registers). The window's first group
// starts the accumulator at 0 and its last one multiplies by 1 / Sy. So a group costs three barriers
// (stage written, horizontal rows written, accumulators written) whatever its number of rows, and the
// finished output rows are emitted by k_resize's emit (16-byte stores, nontemporal under TFRG_DENSE_NT).
//
// LDS (dynamic, sized by the launch): stage, group rows, band accumulators, column table, row table:
// 51 KiB at 224 x 3 (three workgroups per CU), 113 KiB at out_w = 4096.
#include <hip/hip_runtime.h>

#include "tfrg_resize_dev.h"

namespace tfrg {
namespace {

// 16-byte units per lane that cover a full stage
constexpr uint32_t kAaPasses = (kResizeStageWords / 4u + 255u) / 256u;
// a staged crop row in words, data and slack (the realigned write of a row ends at most at word
// kData + vbytes / 4 + 4), and padded
__device__ __forceinline__ uint32_t row_words(uint32_t vbytes) { return kData + (vbytes >> 2) + 6u; }
__device__ __forceinline__ uint32_t row_stride(uint32_t vbytes) { return swz(row_words(vbytes)) + 1u; }
static_assert(kData + (kResizeMaxRowBytes >> 2) + 6u + ((kData + (kResizeMaxRowBytes >> 2) + 6u) >> 5) + 1u <= kResizeStageWords,
              "the widest crop row fits the stage");

// ------------------------------------------------------------------ windows
// The taps of output index o of N along a source axis of n samples: j0 .. j0 + cnt - 1, and the signed
// d = (2 j0 + 1) N - (2 o + 1) n of the first (the next tap's is 2N more; its weight is 2M - |d| > 0).
struct Win {
  uint32_t j0, cnt;
  int32_t d0;
};

__device__ __forceinline__ Win window(uint32_t o, uint32_t n, uint32_t N) {
  const uint32_t M = n > N ? n : N;
  const int32_t c = (int32_t)((2u * o + 1u) * n);  // (below 2^28)
  const int32_t a = c - (int32_t)(2u * M + N);     // tap j is inside when 2N j > a ...
  const uint32_t b = (uint32_t)c + 2u * M - N;     // ... and 2N j < b (b > 0)
  const uint32_t j0 = a < 0 ? 0u : (uint32_t)a / (2u * N) + 1u;
  uint32_t j1 = (b - 1u) / (2u * N);
  j1 = j1 < n - 1u ? j1 : n - 1u;
  return Win{j0, j1 - j0 + 1u, (int32_t)((2u * j0 + 1u) * N) - c};
}

// 1 / (float)S of a window, S the sum of its integer weights (at most 2^30)
__device__ __forceinline__ float inv_sum(const Win& w, uint32_t n, uint32_t N) {
  const int32_t twoM = (int32_t)(2u * (n > N ? n : N)), twoN = (int32_t)(2u * N);
  uint32_t S = 0;
  int32_t d = w.d0;
  for (uint32_t j = 0; j < w.cnt; ++j, d += twoN) S += (uint32_t)(twoM - (d < 0 ? -d : d));
  return 1.0f / (float)S;
}

// ------------------------------------------------------------------ source side
// What a group's loads and its stage writes agree on (uniform)
struct Grp {
  uint64_t s0;     // the first byte of the group's first crop row
  uint64_t pitch;  // bytes from a crop row to the next
  uint32_t vbytes, units, rows, stride;  // units: 16-byte units a row is given (it uses nun <= units)
};

// The group's aligned units into registers: lane-flat over (row, unit); nx: the first dword of the unit after
__device__ __forceinline__ void group_load(const Sp& x, const Grp& g, rw_u32x4 (&d)[kAaPasses], uint32_t (&nx)[kAaPasses]) {
  const uint32_t total = g.rows * g.units, bound = x.a->in_bound;
#pragma unroll
  for (uint32_t p = 0; p < kAaPasses; ++p) {
    d[p] = rw_u32x4{0u, 0u, 0u, 0u};
    nx[p] = 0u;
    if (p * 256u < total) {
      const uint32_t f = p * 256u + threadIdx.x, r = f / g.units, u = f - r * g.units;
      const uint64_t s0 = g.s0 + (uint64_t)r * g.pitch;
      const uint32_t sh = (uint32_t)s0 & 15u, nun = (sh + g.vbytes + 15u) >> 4;
      const uint64_t pos = s0 - sh + ((uint64_t)u << 4);
      const bool ok = f < total && u < nun && pos < bound, ok2 = ok && u + 1u < nun && pos + 16u < bound;
      d[p] = __builtin_bit_cast(rw_u32x4, __builtin_amdgcn_raw_buffer_load_b128(x.in, ok ? (uint32_t)pos : 0xfffffff0u, 0, 0));
      nx[p] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(x.in, ok2 ? (uint32_t)pos + 16u : 0xfffffff0u, 0, 0);
    }
  }
}

// ... and realigned into the stage: row r at stage + r * stride, its first byte at word kData
__device__ __forceinline__ void group_store(uint32_t* stage, const Grp& g, const rw_u32x4 (&d)[kAaPasses],
                                            const uint32_t (&nx)[kAaPasses]) {
  const uint32_t total = g.rows * g.units;
#pragma unroll
  for (uint32_t p = 0; p < kAaPasses; ++p) {
    if (p * 256u < total) {
      const uint32_t f = p * 256u + threadIdx.x, r = f / g.units, u = f - r * g.units;
      const uint32_t sh = (uint32_t)(g.s0 + (uint64_t)r * g.pitch) & 15u, nun = (sh + g.vbytes + 15u) >> 4;
      if (f < total && u < nun) {
        uint32_t* const L = stage + r * g.stride;
        const uint32_t w = kData + 4u * u - (sh >> 2), bs = sh & 3u;
        L[swz(w + 0u)] = __builtin_amdgcn_alignbyte(d[p].y, d[p].x, bs);
        L[swz(w + 1u)] = __builtin_amdgcn_alignbyte(d[p].z, d[p].y, bs);
        L[swz(w + 2u)] = __builtin_amdgcn_alignbyte(d[p].w, d[p].z, bs);
        L[swz(w + 3u)] = __builtin_amdgcn_alignbyte(nx[p], d[p].w, bs);
      }
    }
  }
}

// ------------------------------------------------------------------ horizontal pass
// What the passes of an item share (uniform)
struct Item {
  uint32_t OW, C, rn, pix, inv;
  bool planar;
  int32_t twoMx, twoNx, twoMy, twoNy;
};

// The staged rows of a group resampled along x into h[r][e], e in output order
template <uint32_t SRC>
__device__ __forceinline__ void hpass(const uint32_t* stage, const Grp& g, const uint32_t* ctab, float* h, const Item& q) {
  constexpr uint32_t ESZ = raw_src_size(SRC);
  const auto one = [&](uint32_t r, uint32_t ox, uint32_t c, uint32_t e) {
    const uint32_t t0 = ctab[3u * ox], cnt = (t0 >> 16) + 1u;
    int32_t d = (int32_t)ctab[3u * ox + 1u];
    const uint32_t* const L = stage + r * g.stride;
    uint32_t off = (t0 & 0xffffu) + c * ESZ;
    float acc = 0.f;
    for (uint32_t j = 0; j < cnt; ++j, off += q.pix, d += q.twoNx)
      acc = __builtin_fmaf((float)(q.twoMx - (d < 0 ? -d : d)), to_f32<SRC>(ld_elem<ESZ>(L, off)), acc);
    h[r * q.rn + e] = acc * __builtin_bit_cast(float, ctab[3u * ox + 2u]);
  };
  for (uint32_t r = 0; r < g.rows; ++r) {
    if (q.planar) {
      for (uint32_t c = 0; c < q.C; ++c)
        for (uint32_t ox = threadIdx.x; ox < q.OW; ox += 256u) one(r, ox, c, c * q.OW + ox);
    } else {
      for (uint32_t e = threadIdx.x; e < q.rn; e += 256u) {
        const uint32_t ox = (e * q.inv) >> 16;
        one(r, ox, e - ox * q.C, e);
      }
    }
  }
}

__device__ __forceinline__ void hpass_any(uint32_t src, const uint32_t* stage, const Grp& g, const uint32_t* ctab, float* h,
                                          const Item& q) {
  switch (src) {
    case kRawU8: hpass<kRawU8>(stage, g, ctab, h, q); break;
    case kRawI8: hpass<kRawI8>(stage, g, ctab, h, q); break;
    case kRawU16: hpass<kRawU16>(stage, g, ctab, h, q); break;
    case kRawI16: hpass<kRawI16>(stage, g, ctab, h, q); break;
    case kRawI32: hpass<kRawI32>(stage, g, ctab, h, q); break;
    case kRawF16: hpass<kRawF16>(stage, g, ctab, h, q); break;
    case kRawBF16: hpass<kRawBF16>(stage, g, ctab, h, q); break;
    default: hpass<kRawF32>(stage, g, ctab, h, q); break;
  }
}

// ------------------------------------------------------------------ vertical pass
// The group's rows [g0, g0 + rows) added into the accumulators of the band's nb output rows. ytab[b]: the
// window of row b (j0, cnt, d0) and 1 / Sy.
__device__ __forceinline__ void vpass(const float* h, float* acc, const uint32_t* ytab, uint32_t nb, uint32_t g0, uint32_t rows,
                                      const Item& q) {
  const uint32_t g1 = g0 + rows - 1u;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t j0 = rfl32(ytab[4u * b]), j1 = j0 + rfl32(ytab[4u * b + 1u]) - 1u;
    if (j0 > g1) break;  // (the windows' first taps do not decrease)
    if (j1 < g0) continue;
    const uint32_t lo = j0 > g0 ? j0 : g0, hi = j1 < g1 ? j1 : g1;
    const int32_t dlo = (int32_t)rfl32(ytab[4u * b + 2u]) + (int32_t)(lo - j0) * q.twoNy;
    const float is = __builtin_bit_cast(float, rfl32(ytab[4u * b + 3u]));
    const float* const hr = h + (lo - g0) * q.rn;
    float* const ab = acc + b * q.rn;
    for (uint32_t e = threadIdx.x; e < q.rn; e += 256u) {
      float v = j0 >= g0 ? 0.f : ab[e];
      int32_t d = dlo;
      for (uint32_t r = 0; r <= hi - lo; ++r, d += q.twoNy)
        v = __builtin_fmaf((float)(q.twoMy - (d < 0 ? -d : d)), hr[r * q.rn + e], v);
      ab[e] = j1 <= g1 ? v * is : v;
    }
  }
}

// ------------------------------------------------------------------ the kernel
template <bool NT>
__global__ __launch_bounds__(256) void k_resize_aa(const ResizeArgs) {
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
  const uint32_t B = resize_aa_band(rn), G = resize_aa_group(rn);
  Item q;
  q.OW = OW, q.C = C, q.rn = rn, q.pix = C * raw_src_size(src), q.inv = (65536u + C - 1u) / C;
  q.planar = s->planar != 0u && C > 1u;
  uint32_t* const stage = lds;
  float* const h = reinterpret_cast<float*>(lds + kResizeStageWords);
  float* const acc = h + G * rn;
  uint32_t* const ctab = lds + kResizeStageWords + (G + B) * rn;
  uint32_t* const ytab = ctab + 3u * OW;
  const uint32_t bands = s->bands, nblk = s->nblk;
  const uint64_t items = (uint64_t)a->m * bands;
  Counts cnts;
  for (uint64_t it = blockIdx.x - s->blk0; it < items; it += nblk) {
    const uint32_t k = (uint32_t)(it / bands), band = (uint32_t)(it - (uint64_t)k * bands);
    const uint32_t oy0 = band * B, oy1 = oy0 + B < OH ? oy0 + B : OH, nb = oy1 - oy0;
    const Geo geo = row_geometry(x, k, band == 0u, cnts);
    if (!geo.live) continue;
    Taps t{lds, lds, 0.f, kFill};
    if (!geo.box_ok) {  // (a bad shape or a bad box: the band is fill; no LDS is touched)
      for (uint32_t oy = oy0; oy < oy1; ++oy) emit_any<NT>(x, tab, t, k, oy, q.inv);
      continue;
    }
    const uint32_t cw = geo.cw, ch = geo.ch;
    q.twoMx = (int32_t)(2u * (cw > OW ? cw : OW)), q.twoNx = (int32_t)(2u * OW);
    q.twoMy = (int32_t)(2u * (ch > OH ? ch : OH)), q.twoNy = (int32_t)(2u * OH);
    // the tables
    for (uint32_t ox = threadIdx.x; ox < OW; ox += 256u) {
      const Win w = window(geo.flip ? OW - 1u - ox : ox, cw, OW);
      ctab[3u * ox] = (w.j0 * q.pix) | ((w.cnt - 1u) << 16);
      ctab[3u * ox + 1u] = (uint32_t)w.d0;
      ctab[3u * ox + 2u] = __builtin_bit_cast(uint32_t, inv_sum(w, cw, OW));
    }
    if (threadIdx.x < nb) {
      const Win w = window(oy0 + threadIdx.x, ch, OH);
      ytab[4u * threadIdx.x] = w.j0;
      ytab[4u * threadIdx.x + 1u] = w.cnt;
      ytab[4u * threadIdx.x + 2u] = (uint32_t)w.d0;
      ytab[4u * threadIdx.x + 3u] = __builtin_bit_cast(uint32_t, inv_sum(w, ch, OH));
    }
    // the band's crop rows [r_lo, r_hi], in groups of gmax
    const Win wl = window(oy0, ch, OH), wh = window(oy1 - 1u, ch, OH);
    const uint32_t r_lo = wl.j0, r_hi = wh.j0 + wh.cnt - 1u;
    Grp g;
    g.pitch = geo.W * q.pix;
    g.vbytes = cw * q.pix;
    g.units = (g.vbytes + 30u) >> 4;
    g.stride = row_stride(g.vbytes);
    const uint32_t fit = kResizeStageWords / g.stride, gmax = G < fit ? G : fit;
    const uint64_t s00 = (uint64_t)geo.row.off + ((uint64_t)geo.top * geo.W + geo.left) * q.pix;
    rw_u32x4 d[kAaPasses];
    uint32_t nx[kAaPasses];
    g.rows = r_hi - r_lo + 1u < gmax ? r_hi - r_lo + 1u : gmax;
    g.s0 = s00 + (uint64_t)r_lo * g.pitch;
    group_load(x, g, d, nx);
    t.mode = kTake;
    for (uint32_t g0 = r_lo; g0 <= r_hi; g0 += gmax) {
      const Grp cur = g;
      group_store(stage, cur, d, nx);
      __syncthreads();  // (the stage and the tables are written)
      if (g0 + gmax <= r_hi) {
        const uint32_t left = r_hi - (g0 + gmax) + 1u;
        g.rows = left < gmax ? left : gmax;
        g.s0 = s00 + (uint64_t)(g0 + gmax) * g.pitch;
        group_load(x, g, d, nx);  // (in flight while this group is resampled)
      }
      hpass_any(src, stage, cur, ctab, h, q);
      __syncthreads();  // (the group's rows are written, the stage is free)
      vpass(h, acc, ytab, nb, g0, cur.rows, q);
      __syncthreads();  // (the accumulators are written, the group's rows are free)
      for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t j1 = rfl32(ytab[4u * b]) + rfl32(ytab[4u * b + 1u]) - 1u;
        if (j1 < g0 || j1 > g0 + cur.rows - 1u) continue;  // (not finished by this group)
        t.ra = t.rb = reinterpret_cast<const uint32_t*>(acc + b * rn);
        emit_any<NT>(x, tab, t, k, oy0 + b, q.inv);
      }
    }
    __syncthreads();  // (the next item builds its tables over these)
  }
  report(a, si, cnts);
}

}  // namespace

hipError_t launch_resize_aa(const ResizeArgs& a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st) {
  if (!blocks) return hipSuccess;
  return a.nt ? launch_sized(k_resize_aa<true>, a, blocks, lds_bytes, st) : launch_sized(k_resize_aa<false>, a, blocks, lds_bytes, st);
}

}  // namespace tfrg
