// tfrg_select.hip — the kernels behind tfrg_result_select_rows: the WHERE clause over a decoded batch.
// For a list of m candidates (candidate k is record g = entry(k) - row0) and a table of terms (AND of
// OR-groups), the entries of the candidates that pass, compacted in candidate order. Three launches on
// the decode's stream, no workgroup ever waiting on another (the shape of k_rg_len / k_rg_scan /
// k_rg_gather in tfrg_ragged.hip):
//
//   k_sel_eval   per tile of `tile` candidates, a wave per 64 consecutive candidates: every term in a
//                uniform loop over the table, each lane gathering the groups that hold a true term for
//                its candidate; the verdicts of the 64 lanes as one ballot word into words[] (lane 0,
//                one vector store), the tile's popcount into tsum[tile], the skipped candidates into
//                stats[1] (at most one atomic per wave);
//   k_sel_scan   one workgroup: the tile sums to their first positions, from *count under APPEND and
//                from 0 otherwise, carrying across passes of kSelScanThreads tiles; *count and stats[0];
//   k_sel_write  per tile: its ballot words alone (no predicate is evaluated again, and no column is
//                read), one wave scan of their popcounts, and for every set bit the entry -- the only
//                read of the row list here -- stored at tile base + word base + the set bits below it,
//                where that is below cap.
//
// Positions come from the scan alone: no atomic and no order of workgroups enters them, so two calls
// over the same inputs write the same bytes.
//
// Not read (as k_dense and k_rg_*): the row splits of a placed slot (info words kInfoPlacedLo / Hi: the
// record has one value, at index g), the bytes_len column of a slot whose length is constant
// (SelTerm::const_len), the status column where every status is 0 (SelectArgs::status null). A
// candidate whose g is not in [0, n) loads nothing indexed by g (it reads record 0 and drops it).
#include <hip/hip_runtime.h>

#include "tfrg_dev.h"
#include "tfrg_internal.h"
#include "tfrg_select.h"

namespace tfrg {
namespace {

constexpr uint32_t kBlk = 256;
constexpr uint32_t kWaves = kBlk / 64;

// The kernel argument is read in place, in the constant address space (scalar loads)
typedef const __attribute__((address_space(4))) SelectArgs* KArgs;
typedef const __attribute__((address_space(4))) SelTerm* KTerm;

__device__ __forceinline__ bool sel_cmp(int64_t a, int64_t b, uint32_t op) {
  switch (op) {
    case kSelEq: return a == b;
    case kSelNe: return a != b;
    case kSelLt: return a < b;
    case kSelLe: return a <= b;
    case kSelGt: return a > b;
    default: return a >= b;
  }
}

// entry k < m of the candidate list
__device__ __forceinline__ int64_t entry_of(KArgs a, uint32_t k) {
  const uint8_t* const rows = static_cast<const uint8_t*>(a->rows);
  if (!rows) return (int64_t)k;
  if (a->rows64) return *reinterpret_cast<const int64_t*>(rows + ((uint64_t)k << 3));
  return (int64_t)*reinterpret_cast<const int32_t*>(rows + ((uint64_t)k << 2));
}

// value i of a value array against the term (float slots: by value, NaN apart)
__device__ __forceinline__ bool value_term(KArgs a, KTerm t, uint64_t i) {
  if (t->is_float) {
    const uint32_t u = a->f32[i];
    if (sel_float_nan(u) || t->rhs_nan) return t->op == kSelNe;
    return sel_cmp(sel_float_key(u), t->rhs, t->op);
  }
  return sel_cmp(a->i64[i], t->rhs, t->op);
}

// term t for record g (ok: g is a record; else everything indexed by g is taken from record 0 and dropped)
__device__ __forceinline__ bool eval_term(KArgs a, KTerm t, uint64_t placed, uint32_t g, bool ok) {
  const uint32_t subject = t->subject;
  if (subject == kSelStatus) {
    const int64_t st = a->status ? (int64_t)a->status[g] : 0;
    return ok && sel_cmp(st, t->rhs, t->op);
  }
  const uint32_t slot = t->slot;
  uint32_t lo = g, c = 1u;
  if (!(slot < 64u && ((placed >> slot) & 1ull))) {
    const uint32_t* const rs = a->rs + (uint64_t)slot * ((uint64_t)a->n + 1u);
    lo = rs[g];
    c = rs[g + 1u] - lo;
  }
  c = ok ? c : 0u;  // (a skipped candidate is a record without a value to everything that loads)
  const uint64_t base = a->slot_base[slot];
  switch (subject) {
    case kSelValue: {
      // (a record without value `index` reads element 0 of the array and drops it)
      const bool has = c > t->index;
      const bool v = value_term(a, t, has ? base + lo + t->index : 0ull);
      return has && v;
    }
    case kSelAny: {
      bool any = false;
      for (uint32_t j = 0; j < c && !any; ++j) any = value_term(a, t, base + lo + j);
      return any;
    }
    case kSelCount: return ok && sel_cmp((int64_t)c, t->rhs, t->op);
    default: {  // kSelBytesLen: the length of element 0, as row_of of tfrg_ragged.hip
      const uint64_t es = c ? base + lo : 0ull;
      uint32_t len;
      if (t->const_len != kSelNoLen) {
        len = t->const_len;
      } else if (a->b_off64) {
        const uint64_t l = a->b_off64[es + 1] - a->b_off64[es];
        len = l < 0xffffffffull ? (uint32_t)l : 0xffffffffu;
      } else {
        len = a->b_len[es];
      }
      return ok && sel_cmp((int64_t)(c ? len : 0u), t->rhs, t->op);
    }
  }
}

// ------------------------------------------------------------------ 1. verdicts
__global__ __launch_bounds__(kBlk) void k_sel_eval(const SelectArgs) {
  __shared__ uint32_t part[kWaves];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  const uint32_t m = a->m, n = a->n, tile = a->tile;
  const uint32_t t0 = blockIdx.x * tile;
  const uint32_t t1 = m - t0 < tile ? m : t0 + tile;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t* const info = a->info;
  const uint64_t placed = ((uint64_t)info[kInfoPlacedHi] << 32) | info[kInfoPlacedLo];
  const uint32_t n_terms = a->n_terms, all = a->all_groups;
  const int64_t row0 = a->row0;
  uint32_t sel = 0, skip = 0;  // (the wave's, kept by every lane alike)
  for (uint32_t w0 = t0 + wave * 64u; w0 < t1; w0 += kBlk) {
    const uint32_t k = w0 + lane;
    const bool live = k < m;
    bool ok = false;
    uint32_t g = 0;
    if (live) {
      // (tfrg_dense.hip rec_of's rule: compared before the subtraction, so no entry wraps into range)
      const int64_t v = entry_of(a, k);
      const uint64_t d = (uint64_t)v - (uint64_t)row0;
      ok = v >= row0 && d < (uint64_t)n;
      g = ok ? (uint32_t)d : 0u;
    }
    uint32_t groups = 0;
    for (uint32_t i = 0; i < n_terms; ++i) {
      const KTerm t = &a->term[i];
      if (eval_term(a, t, placed, g, ok)) groups |= 1u << t->group;
    }
    const bool pass = ok && groups == all;
    const uint64_t word = __ballot(pass);
    const uint64_t bad = __ballot(live && !ok);
    if (lane == 0u) a->words[w0 >> 6] = word;
    sel += (uint32_t)__popcll(word);
    skip += (uint32_t)__popcll(bad);
  }
  if (lane == 0u) part[wave] = sel;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < kWaves; ++i) s += part[i];
    a->tsum[blockIdx.x] = s;
  }
  if (a->stats && lane == 0u && skip) atomicAdd(a->stats + 1, skip);
}

// ------------------------------------------------------------------ 2. tile scan
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
    if (lane >= (uint32_t)o) v += u;
  }
  return v;
}

// one workgroup: the tile sums to their first positions; *count and the selected counter
__global__ __launch_bounds__(kSelScanThreads) void k_sel_scan(const SelectArgs) {
  constexpr uint32_t W = kSelScanThreads / 64;
  __shared__ uint64_t part[W];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t tiles = a->tiles;
  uint64_t* const tsum = a->tsum;
  const uint64_t base = a->append ? *a->count : 0ull;
  uint64_t carry = base;
  for (uint32_t b0 = 0; b0 < tiles; b0 += kSelScanThreads) {
    const uint32_t i = b0 + threadIdx.x;
    const uint64_t v = i < tiles ? tsum[i] : 0ull;
    const uint64_t inc = wave_incl_scan64(v);
    const uint32_t w = threadIdx.x >> 6;
    __syncthreads();  // (part may still be read from the pass before)
    if ((threadIdx.x & 63u) == 63u) part[w] = inc;
    __syncthreads();
    uint64_t before = 0, total = 0;
#pragma unroll
    for (uint32_t j = 0; j < W; ++j) {
      const uint64_t s = part[j];
      before += j < w ? s : 0ull;
      total += s;
    }
    if (i < tiles) tsum[i] = carry + before + inc - v;
    carry += total;
  }
  if (threadIdx.x == 0) {
    *a->count = carry;
    if (a->stats) a->stats[0] = (uint32_t)(carry - base);
  }
}

// ------------------------------------------------------------------ 3. write
__global__ __launch_bounds__(kBlk) void k_sel_write(const SelectArgs) {
  __shared__ uint32_t wbase[kSelTileMax / 64];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t m = a->m, tile = a->tile;
  const uint32_t t0 = blockIdx.x * tile;
  const uint32_t t1 = m - t0 < tile ? m : t0 + tile;
  const uint32_t nw = (t1 - t0 + 63u) >> 6;  // the tile's words: at most 64
  const uint64_t* const words = a->words + (t0 >> 6);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave == 0u) {
    const uint32_t c = lane < nw ? (uint32_t)__popcll(words[lane]) : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o, 64);
      if (lane >= (uint32_t)o) inc += u;
    }
    wbase[lane] = inc - c;
  }
  __syncthreads();
  const uint64_t tbase = a->tsum[blockIdx.x];
  const uint64_t cap = a->cap;
  uint8_t* const out = static_cast<uint8_t*>(a->out);
  const uint32_t out64 = a->out64;
  for (uint32_t wi = wave; wi < nw; wi += kWaves) {
    const uint64_t word = words[wi];
    if (!((word >> lane) & 1ull)) continue;
    const uint64_t pos = tbase + wbase[wi] + (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
    if (pos >= cap) continue;
    const int64_t v = entry_of(a, t0 + wi * 64u + lane);
    if (out64) *reinterpret_cast<int64_t*>(out + (pos << 3)) = v;
    else *reinterpret_cast<int32_t*>(out + (pos << 2)) = (int32_t)v;
  }
}

}  // namespace

hipError_t launch_select(const SelectArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_sel_eval, dim3(a.tiles), dim3(kBlk), 0, st, a);
  hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(kSelScanThreads), 0, st, a);
  if (a.out && a.cap) hipLaunchKernelGGL(k_sel_write, dim3(a.tiles), dim3(kBlk), 0, st, a);
  return hipGetLastError();
}

}  // namespace tfrg
