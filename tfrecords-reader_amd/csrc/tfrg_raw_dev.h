// tfrg_raw_dev.h — device code that k_raw (tfrg_raw.hip) and k_resize (tfrg_resize.hip) share: the layout
// of source bytes staged in LDS (padded by one word per 32, the first byte at word kData), the element
// read back from it, the conversions (source type -> float32, float32 pairs -> float16 / bfloat16, RNE)
// and the global store with its streaming policy. Each piece defined once.
#pragma once
#include <hip/hip_runtime.h>

#include "tfrg_raw.h"
#include "tfrg_rows.h"

namespace tfrg {
namespace {

typedef uint32_t rw_u32x4 __attribute__((ext_vector_type(4)));
typedef float rw_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 rw_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 rw_f16x2 __attribute__((ext_vector_type(2)));

// words of slack before the staged bytes (the realigned write of unit 0 starts up to three words early)
constexpr uint32_t kData = 4;

__device__ __forceinline__ uint32_t swz(uint32_t w) { return w + (w >> 5); }

// element at byte b of the staged bytes (b a multiple of ESZ), zero-extended
template <uint32_t ESZ>
__device__ __forceinline__ uint32_t ld_elem(const uint32_t* L, uint32_t b) {
  b += kData * 4u;
  const uint32_t a = b + ((b >> 7) << 2);  // (swz on a byte address)
  if constexpr (ESZ == 1) return reinterpret_cast<const uint8_t*>(L)[a];
  else if constexpr (ESZ == 2) return reinterpret_cast<const uint16_t*>(L)[a >> 1];
  else return L[a >> 2];
}

// ------------------------------------------------------------------ the row of a work item
struct RowSrc {
  uint32_t off, len, cnt, ok;  // element 0's first byte and length, the record's element count
};

// Element 0 of record g's list in the slot of the kernel's spec view x (its Sp: a the argument, s the
// spec with const_off / const_len, rs the slot's row splits or null, base the slot's base); ok 0: a
// skipped row, which has no element. (Every value uniform over the group: held in scalar registers.)
template <class S>
__device__ __forceinline__ RowSrc resolve_at(const S& x, uint32_t g, uint32_t ok) {
  uint32_t lo = g, c = 1u;
  if (x.rs) {
    lo = rfl32(x.rs[g]);
    c = rfl32(x.rs[g + 1u]) - lo;
  }
  c = ok ? c : 0u;
  const uint64_t es = c ? x.base + lo : 0ull;
  RowSrc r{0u, 0u, c, ok};
  if (x.a->b_off64) {
    const uint64_t o0 = rfl64(x.a->b_off64[es]), o1 = rfl64(x.a->b_off64[es + 1]);
    const uint64_t l = o1 - o0;
    r.off = o0 < 0xffffffffull ? (uint32_t)o0 : 0xffffffffu;
    r.len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
  } else {
    r.off = x.s->const_off != kRawOffStored ? rfl32(x.a->end32[g]) + (uint32_t)x.s->const_off : rfl32(x.a->b_off[es]);
    r.len = x.s->const_len != kRawNoLen ? x.s->const_len : rfl32(x.a->b_len[es]);
  }
  if (!c) r.len = 0u;
  return r;
}

// the same for output row k of the view's row list (x.rl)
template <class S>
__device__ __forceinline__ RowSrc resolve(const S& x, uint32_t k) {
  const Rec q = rec_of(x.a, x.rl.row0, x.rl.rows ? row_entry(x.rl, k) : (int64_t)k);
  return resolve_at(x, rfl32(q.g), rfl32(q.ok));
}

// ------------------------------------------------------------------ convert
template <uint32_t SRC>
__device__ __forceinline__ float to_f32(uint32_t raw) {
  if constexpr (SRC == kRawU8 || SRC == kRawU16) return (float)raw;
  else if constexpr (SRC == kRawI8) return (float)(int8_t)raw;
  else if constexpr (SRC == kRawI16) return (float)(int16_t)raw;
  else if constexpr (SRC == kRawI32) return (float)(int32_t)raw;
  else if constexpr (SRC == kRawF16) return (float)__builtin_bit_cast(_Float16, (uint16_t)raw);
  else if constexpr (SRC == kRawBF16) return __builtin_bit_cast(float, raw << 16);
  else return __builtin_bit_cast(float, raw);
}

// two float32 to a pair of float16 / bfloat16, RNE
template <uint32_t OUT>
__device__ __forceinline__ uint32_t cvt2(float a, float b) {
  const rw_f32x2 v = {a, b};
  if constexpr (OUT == kRawOutF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, rw_f16x2));
  else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, rw_bf16x2));
}

// a store to global memory at address p (global_store, not flat), with the streaming policy under NT
template <bool NT, class T>
__device__ __forceinline__ void st(uint64_t p, T v) {
  typedef __attribute__((address_space(1))) T* G;
  if constexpr (NT) __builtin_nontemporal_store(v, (G)p);
  else *(G)p = v;
}

}  // namespace
}  // namespace tfrg
