// tfrg_dev.h — the device helpers that more than one kernel file uses, each defined once: byte and
// word primitives, the readfirstlane wrappers, the wave sums and the wave and workgroup scans, the nt
// store, and the bookkeeping that ends an optimistic decode (all_placed_finish). Included by
// tfrg_kernels.hip, tfrg_scan.hip, tfrg_tpl.hip, tfrg_bytes.hip, tfrg_frame.hip and, through
// tfrg_rows.h, by the row-list passes (tfrg_dense.hip, tfrg_ragged.hip, tfrg_elems.hip, tfrg_ids.hip,
// tfrg_select.hip).
#pragma once
#include "tfrg_internal.h"
#include "../../include/tfrg_status.h"

namespace tfrg {

// a ^ b ^ c in one VALU (gfx950 v_bitop3_b32, truth table 0x96; the compiler does not fuse XOR chains)
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// ((x >> 8K) & 0xff) * 4 in one VALU: a shift with an SDWA byte select of its source
template <int K>
__device__ __forceinline__ uint32_t byte_x4(uint32_t x) {
  static_assert(K >= 0 && K < 4, "byte index");
  uint32_t r;
  const uint32_t two = 2u;
  if constexpr (K == 0)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0"
        : "=v"(r) : "v"(two), "v"(x));
  else if constexpr (K == 1)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1"
        : "=v"(r) : "v"(two), "v"(x));
  else if constexpr (K == 2)
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2"
        : "=v"(r) : "v"(two), "v"(x));
  else
    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3"
        : "=v"(r) : "v"(two), "v"(x));
  return r;
}

// 7-bit groups of the bytes of w selected by byte mask m, compacted (a varint of <= 4 bytes)
__device__ __forceinline__ uint32_t vgroups(uint32_t w, uint32_t m) {
  w &= m;
  return (w & 0x7fu) | ((w >> 1) & 0x3f80u) | ((w >> 2) & 0x1fc000u) | ((w >> 3) & 0xfe00000u);
}
// byte mask of the first nb (1..4) bytes: shifts only (a multiply by 7 would be quarter rate)
__device__ __forceinline__ uint32_t bytes_mask(uint32_t nb) { return nb >= 4u ? 0xffffffffu : (1u << (nb << 3)) - 1u; }

__device__ __forceinline__ uint32_t rfl32(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t rfl64(uint64_t x) {
  return ((uint64_t)rfl32((uint32_t)(x >> 32)) << 32) | rfl32((uint32_t)x);
}

// Inclusive prefix sum over the wave (every lane active) in seven DPP adds, no LDS: rows of 16 by
// row_shr 1, 2, 3 of the value, then 4 and 8 of the partial sums (bank masks: only the lanes that
// still miss a part), then the row totals by row_bcast 15 / 31 (gfx9 DPP; lanes a mask leaves out
// read `old` = 0). Replaces six ds_bpermute round trips of __shfl_up.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, uint32_t) {
  uint32_t s = v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);  // row_shr:1
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);             // row_shr:2
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x113, 0xf, 0xf, true);             // row_shr:3
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x114, 0xf, 0xe, true);             // row_shr:4
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x118, 0xf, 0xc, true);             // row_shr:8
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x142, 0xa, 0xf, false);            // row_bcast:15
  s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x143, 0xc, 0xf, false);            // row_bcast:31
  return s;
}

// Sums over the wave (every lane active) by __shfl_down: lane 0 holds the total. (tfrg_tpl.hip's
// wave_sum and tfrg_kernels.hip's wave_sum_u32 are other algorithms, which leave it in every lane.)
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, d, 64);
  return v;
}

// Inclusive prefix sum over the wave by the __shfl_up ladder, for uint32_t and uint64_t (the scans
// that run once per tile or pass; wave_incl_scan_u32 above is the DPP one of the decode's hot path)
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = (T)__shfl_up(v, o, 64);
    if (lane >= (uint32_t)o) v += u;
  }
  return v;
}

// exclusive scan of v over the workgroup (W waves, every thread calls; part: W words of LDS);
// *total: the workgroup's sum
template <int W, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* part, T* total) {
  const T inc = wave_incl_scan(v);
  const uint32_t w = threadIdx.x >> 6;
  __syncthreads();  // (part may still be read from a previous call)
  if ((threadIdx.x & 63u) == 63u) part[w] = inc;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const T s = part[i];
    before += (uint32_t)i < w ? s : (T)0;
    all += s;
  }
  *total = all;
  return before + inc - v;
}

// single value stored in the loc word by the count pass
__device__ __forceinline__ void put_inline(const DevOut& o, uint32_t kind, uint2 lc, uint64_t dst) {
  if (kind == TFRG_KIND_INT64) {
    if (dst < o.cap_i64) o.i64[dst] = (int64_t)(((uint64_t)lc.y << 32) | lc.x);
  } else if (kind == TFRG_KIND_FLOAT) {
    if (dst < o.cap_f32) o.f32[dst] = lc.x;
  } else if (dst < o.cap_b) {
    o.b_off[dst] = lc.x;
    o.b_len[dst] = lc.y;
  }
}

constexpr int kLaneBlock = 256;  // k_down_gather's workgroup (role_list_gather strides over its list by it)

// store with the streaming (nt) cache policy, for data written once and not read again by the launch
template <bool NT, class T>
__device__ __forceinline__ void st_nt(T* p, T v) {
  if constexpr (NT)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// The bookkeeping that ends an optimistic decode in which every record placed every slot (by the
// last workgroup of k_tpl_lane or k_tail_count, `blk` threads): slot totals n, the last row split of
// every slot, column bases and kind totals (k_spine's every-slot-placed path), the overflow flag and
// the placed mask (k_down_gather).
__device__ __forceinline__ void all_placed_finish(const DevOut& o, const uint8_t* slot_kind, uint32_t n_slots,
                                                  uint32_t n, uint32_t blk) {
  for (uint32_t k = threadIdx.x; k < n_slots; k += blk) {
    o.totals[k] = n;
    o.rs[(size_t)k * (n + 1u) + n] = n;
  }
  if (threadIdx.x == 0) {
    uint64_t acc[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < n_slots; ++k) {
      const uint32_t kd = slot_kind[k] & 3u;
      o.slot_base[k] = acc[kd];
      acc[kd] += n;
    }
    for (int k = 0; k < 4; ++k) o.kind_totals[k] = acc[k];
    if (acc[TFRG_KIND_INT64] > o.cap_i64 || acc[TFRG_KIND_FLOAT] > o.cap_f32 || acc[TFRG_KIND_BYTES] > o.cap_b)
      o.info[kInfoOverflow] = 1u;
    const uint64_t pm = n_slots >= 64u ? ~0ull : (1ull << n_slots) - 1ull;
    o.info[kInfoPlacedLo] = (uint32_t)pm;
    o.info[kInfoPlacedHi] = (uint32_t)(pm >> 32);
  }
}

}  // namespace tfrg
