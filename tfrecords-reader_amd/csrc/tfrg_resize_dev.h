// tfrg_resize_dev.h — device code that k_resize (tfrg_resize.hip) and k_resize_aa (tfrg_resize_aa.hip)
// share: the spec view of a workgroup, the geometry of a work item's row (record, H and W, box, flip, the
// four counters), and the emit of one output row from a row of float32 in LDS. Each piece defined once.
#pragma once
#include <hip/hip_runtime.h>

#include "tfrg_resize.h"
#include "tfrg_raw_dev.h"
#include "tfrg_internal.h"
#include "tfrg_rows.h"

namespace tfrg {
namespace {

typedef const __attribute__((address_space(4))) ResizeArgs* KArgs;
typedef const __attribute__((address_space(4))) ResizeSpec* KSpec;

// how a ring value is made and used (uniform)
enum Mode : uint32_t { kLerp = 0, kTake, kBits, kFill };

// the spec a workgroup works in (uniform; the fields resolve_at reads are named as k_raw's)
struct Sp {
  KArgs a;
  KSpec s;
  const uint32_t* rs;
  uint64_t base;
  __amdgpu_buffer_rsrc_t in;
  RowList rl;
};

// value 0 of record g's list in an int64 slot (or the constant); false: the list is empty
__device__ __forceinline__ bool extent(const Sp& x, uint32_t slot, uint32_t konst, uint32_t g, int64_t* v) {
  if (slot == kResizeConst) {
    *v = (int64_t)konst;
    return true;
  }
  const uint32_t* const rs = slot_splits(x.a, slot);
  uint32_t lo = g, c = 1u;
  if (rs) {
    lo = rfl32(rs[g]);
    c = rfl32(rs[g + 1u]) - lo;
  }
  const uint64_t e = c ? x.a->slot_base[slot] + lo : 0ull;
  *v = (int64_t)rfl64(col_i64(x.a, e));
  return c != 0u;
}

// ------------------------------------------------------------------ the row of a work item
// (uniform; thread 0 reports the counters)
struct Counts {
  uint32_t skip = 0, bad_shape = 0, bad_box = 0, empty = 0, longer = 0;
};

struct Geo {
  bool live, box_ok, flip;  // live: the row is not skipped
  uint32_t top, left, ch, cw;
  uint64_t W;
  RowSrc row;
};

// List entry k: record, element, H and W, box and flip. `first`: the item is the row's first band, which
// writes shapes[k] and counts the row.
__device__ __forceinline__ Geo row_geometry(const Sp& x, uint32_t k, bool first, Counts& n) {
  const KArgs a = x.a;
  const KSpec s = x.s;
  const uint32_t pix = s->channels * raw_src_size(s->src);
  Geo o{};
  const Rec q = rec_of(a, x.rl.row0, x.rl.rows ? row_entry(x.rl, k) : (int64_t)k);
  const uint32_t g = rfl32(q.g);
  if (!rfl32(q.ok)) {
    n.skip += first;
    return o;
  }
  o.live = true;
  const RowSrc row = resolve_at(x, g, 1u);
  int64_t H, W;
  const bool has_h = extent(x, s->h_slot, s->src_h, g, &H), has_w = extent(x, s->w_slot, s->src_w, g, &W);
  const bool sized = has_h && has_w && H >= 1 && H <= (int64_t)kResizeMaxSrc && W >= 1 && W <= (int64_t)kResizeMaxSrc;
  const uint64_t need = sized ? (uint64_t)H * (uint64_t)W * pix : 0ull;
  const bool shape_ok = sized && need <= (uint64_t)row.len;
  int32_t top = 0, left = 0, ch = sized ? (int32_t)H : 0, cw = sized ? (int32_t)W : 0;
  if (a->boxes) {
    const int32_t* const b = a->boxes + 4ull * k;
    top = (int32_t)rfl32((uint32_t)b[0]);
    left = (int32_t)rfl32((uint32_t)b[1]);
    ch = (int32_t)rfl32((uint32_t)b[2]);
    cw = (int32_t)rfl32((uint32_t)b[3]);
  }
  o.box_ok = shape_ok && ch > 0 && cw > 0 && top >= 0 && left >= 0 && (int64_t)top + ch <= H &&
             (int64_t)left + cw <= W && (uint64_t)(uint32_t)cw * pix <= (uint64_t)kResizeMaxRowBytes;
  o.flip = a->flips ? rfl32(a->flips[k]) != 0u : false;
  if (first) {
    if (threadIdx.x == 0u && s->shapes) {
      const auto i32 = [](bool has, int64_t v) {
        return !has ? 0 : v < INT32_MIN ? INT32_MIN : v > INT32_MAX ? INT32_MAX : (int32_t)v;
      };
      s->shapes[2ull * k] = i32(has_h, H);
      s->shapes[2ull * k + 1u] = i32(has_w, W);
    }
    n.bad_shape += !shape_ok;
    n.bad_box += shape_ok && !o.box_ok;
    n.empty += row.cnt == 0u;
    n.longer += sized && (uint64_t)row.len > need;
  }
  o.top = (uint32_t)top;
  o.left = (uint32_t)left;
  o.ch = (uint32_t)ch;
  o.cw = (uint32_t)cw;
  o.W = (uint64_t)W;
  o.row = row;
  return o;
}

// a workgroup's counters into spec si's (thread 0)
__device__ __forceinline__ void report(KArgs a, uint32_t si, const Counts& n) {
  if (threadIdx.x != 0u) return;
  if (a->skipped && n.skip) atomicAdd(a->skipped + si, n.skip);
  if (uint32_t* const stats = a->stats) {
    if (n.bad_shape) atomicAdd(stats + 4u * si + 0, n.bad_shape);
    if (n.bad_box) atomicAdd(stats + 4u * si + 1, n.bad_box);
    if (n.empty) atomicAdd(stats + 4u * si + 2, n.empty);
    if (n.longer) atomicAdd(stats + 4u * si + 3, n.longer);
  }
}

// the spec view of the workgroup whose spec is si
__device__ __forceinline__ Sp spec_view(KArgs a, uint32_t si) {
  Sp x;
  x.a = a;
  x.s = &a->sp[si];
  x.base = a->slot_base[x.s->slot];
  x.rs = slot_splits(a, x.s->slot);
  x.in = bytes_source(a);
  x.rl = make_row_list(a);
  return x;
}

// ------------------------------------------------------------------ emit
// what an output row is made from (uniform)
struct Taps {
  const uint32_t* ra;  // the ring slot of its upper tap (kLerp), or of its one row
  const uint32_t* rb;  // of its lower tap
  float fy;
  uint32_t mode;
};

// K consecutive elements from index i0 of a run as output bits; e0: the ring index of element i0, ch: its
// channel, chinc: whether the next element's channel is the next one (interleaved)
template <uint32_t OUT, uint32_t K>
__device__ __forceinline__ void vals(const Sp& x, const rw_f32x2* tab, const Taps& t, uint32_t e0, uint32_t ch, bool chinc,
                                     uint32_t* o) {
  const uint32_t C = x.s->channels, fill = x.s->fill;
  if (t.mode == kFill) {
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) o[i] = fill;
    return;
  }
  if constexpr (OUT == kRawOutSame) {
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) o[i] = t.ra[e0 + i];
  } else {
    float y[K];
    rw_f32x2 sb = tab[ch];
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) {
      const float h0 = __builtin_bit_cast(float, t.ra[e0 + i]);
      float r = h0;
      if (t.mode == kLerp) r = __builtin_fmaf(t.fy, __builtin_bit_cast(float, t.rb[e0 + i]) - h0, h0);
      y[i] = __builtin_fmaf(r, sb.x, sb.y);
      if (chinc && C > 1u) {
        ch = ch + 1u == C ? 0u : ch + 1u;
        sb = tab[ch];
      }
    }
    if constexpr (OUT == kRawOutF32) {
#pragma unroll
      for (uint32_t i = 0; i < K; ++i) o[i] = __builtin_bit_cast(uint32_t, y[i]);
    } else if constexpr (K == 1) {
      o[0] = cvt2<OUT>(y[0], y[0]) & 0xffffu;
    } else {
#pragma unroll
      for (uint32_t i = 0; i < K; i += 2) {
        const uint32_t p = cvt2<OUT>(y[i], y[i + 1]);
        o[i] = p & 0xffffu;
        o[i + 1] = p >> 16;
      }
    }
  }
}

// Output row oy of list entry k: one run of OW * C elements (interleaved), or a run of OW per plane
template <uint32_t OUT, uint32_t OSZ, bool NT>
__device__ __forceinline__ void emit(const Sp& x, const rw_f32x2* tab, const Taps& t, uint32_t k, uint32_t oy, uint32_t inv) {
  constexpr uint32_t EU = 16u / OSZ;
  const uint32_t C = x.s->channels, OW = x.s->out_w, OH = x.s->out_h;
  const bool planar = x.s->planar != 0u && C > 1u;
  const uint32_t nruns = planar ? C : 1u, n = planar ? OW : OW * C, slots = n / EU;
  const uint64_t out = (uint64_t)(uintptr_t)x.s->out;
  const auto run_base = [&](uint32_t c) {
    const uint64_t row = planar ? ((uint64_t)k * C + c) * OH + oy : (uint64_t)k * OH + oy;
    return out + row * n * OSZ;
  };
  const uint32_t total = nruns * slots;
  for (uint32_t f = threadIdx.x; f < total; f += 256u) {
    const uint32_t c = planar ? f / slots : 0u, u = f - c * slots;
    const uint64_t A = run_base(c);
    uint32_t hA = ((16u - ((uint32_t)A & 15u)) & 15u) / OSZ;  // elements before the first whole unit
    hA = hA < n ? hA : n;
    if (u < (n - hA) / EU) {
      const uint32_t i0 = hA + u * EU;
      uint32_t o[EU];
      vals<OUT, EU>(x, tab, t, planar ? c * OW + i0 : i0, planar ? c : i0 - ((i0 * inv) >> 16) * C, !planar, o);
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
    const uint64_t A = run_base(c);
    uint32_t hA = ((16u - ((uint32_t)A & 15u)) & 15u) / OSZ;
    hA = hA < n ? hA : n;
    const uint32_t nu = (n - hA) / EU, rest = n - nu * EU;  // (rest < 2 * EU <= 32)
    if (threadIdx.x < rest) {
      const uint32_t i = threadIdx.x < hA ? threadIdx.x : nu * EU + threadIdx.x;
      uint32_t o;
      vals<OUT, 1>(x, tab, t, planar ? c * OW + i : i, planar ? c : i - ((i * inv) >> 16) * C, false, &o);
      const uint64_t p = A + (uint64_t)i * OSZ;
      if constexpr (OSZ == 4) st<false>(p, o);
      else if constexpr (OSZ == 2) st<false>(p, (uint16_t)o);
      else st<false>(p, (uint8_t)o);
    }
  }
}

template <bool NT>
__device__ __forceinline__ void emit_any(const Sp& x, const rw_f32x2* tab, const Taps& t, uint32_t k, uint32_t oy, uint32_t inv) {
  const uint32_t out = x.s->outt;
  if (out == kRawOutF32) emit<kRawOutF32, 4, NT>(x, tab, t, k, oy, inv);
  else if (out == kRawOutF16) emit<kRawOutF16, 2, NT>(x, tab, t, k, oy, inv);
  else if (out == kRawOutBF16) emit<kRawOutBF16, 2, NT>(x, tab, t, k, oy, inv);
  else if (raw_src_size(x.s->src) == 1u) emit<kRawOutSame, 1, NT>(x, tab, t, k, oy, inv);
  else if (raw_src_size(x.s->src) == 2u) emit<kRawOutSame, 2, NT>(x, tab, t, k, oy, inv);
  else emit<kRawOutSame, 4, NT>(x, tab, t, k, oy, inv);
}

// ------------------------------------------------------------------ launch
// `kern` over `blocks` workgroups of 256 threads with lds_bytes of dynamic LDS
inline hipError_t launch_sized(void (*kern)(const ResizeArgs), const ResizeArgs& a, uint32_t blocks, uint32_t lds_bytes,
                               hipStream_t st) {
  // (beyond the default limit of dynamic LDS the kernel has to be told)
  if (lds_bytes > 48u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace
}  // namespace tfrg
