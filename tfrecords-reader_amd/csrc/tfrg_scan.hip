// tfrg_scan.hip — the row-split scan of the decode (gfx950): k_spine (tile sums -> exclusive prefixes,
// column bases), k_down_gather (row splits, inline single values, the list of records for
// k_tail_gather), and the small kernels beside them: k_poison_loc (debug hook) and
// k_fill_placed_rows (tfrg_result_device's view of placed slots). launch_decode (tfrg_decode.cpp)
// decides when they run and caps their grids.
#include <algorithm>
#include "tfrg_dev.h"

namespace tfrg {

// ------------------------------------------------------------------------------------------------
// Row-split scan, second level: the tile sums of every slot in chunks of 4096 tiles (1 M records),
// one 256-thread workgroup per (slot, chunk), 16 tiles per thread, with a decoupled look-back
// across the chunks of a slot: each workgroup publishes its chunk total (flag 1) at once, sums
// its predecessors' totals back to the first inclusive prefix (flag 2), publishes its own
// inclusive prefix and writes full exclusive prefixes over the tile sums in place. Chunks are
// taken in ticket order, so every workgroup waited on has started. The last workgroup to finish
// derives the per-kind column bases from the slot totals.
// ------------------------------------------------------------------------------------------------
constexpr int kSpineBlock = 256;
constexpr int kSpineItems = 16;
static_assert(kSpineBlock * kSpineItems == (1 << kSpineChunkShift), "one chunk per spine workgroup");

// exclusive prefix of chunk `chunk` from its predecessors' look-back words (lb[0..chunk)), by one
// wave: lane l reads predecessor chunk - 1 - l (64 words per round trip, not one), the nearest
// inclusive prefix (flag 2) ends the sum; a predecessor in range that has not published its total
// yet (flag 0; it has started: ticket order) makes the wave read the window again
__device__ __forceinline__ uint32_t spine_look_back(const uint64_t* lb, uint32_t chunk, uint32_t lane) {
  uint32_t excl = 0;
  for (int64_t base = (int64_t)chunk - 1; base >= 0;) {  // (wave-uniform)
    const int64_t j = base - (int64_t)lane;
    const uint64_t w = j >= 0 ? __hip_atomic_load(&lb[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : (2ull << 32);  // (before the first chunk: an inclusive prefix of 0)
    const uint32_t flag = (uint32_t)(w >> 32);
    const uint64_t inc = __ballot(flag == 2u), unset = __ballot(flag == 0u);
    const uint32_t stop = inc ? (uint32_t)__builtin_ctzll(inc) : 64u;  // lanes [0, stop] are summed
    const uint64_t range = stop >= 63u ? ~0ull : (2ull << stop) - 1ull;
    if (unset & range) {
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    uint32_t v = lane <= stop ? (uint32_t)w : 0u;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    excl += v;
    if (stop < 64u) break;
    base -= 64;
  }
  return excl;
}

// DevSchema::spec: the speculative placement of slot k is not final -- some record of it or of an
// earlier slot of its kind (all speculative: they form a prefix) was irregular. Otherwise every such
// slot holds n values at rows 0..n-1, so the column base of slot k is n * rank, as placed.
__device__ __forceinline__ bool spec_failed(const uint32_t* spec, const DevOut& o, uint32_t k) {
  const uint32_t sw = spec ? spec[k] : 0u;
  if (!sw) return false;
  for (uint32_t j = 0; j <= k; ++j) {
    const uint32_t sj = spec[j];
    if (sj && ((sj ^ sw) & 3u) == 0u && o.irr[j]) return true;
  }
  return false;
}
__device__ __forceinline__ bool spec_placed(const uint32_t* spec, const DevOut& o, uint32_t k) {
  return spec && spec[k] && !spec_failed(spec, o, k);
}

// grid n_chunks * n_slots (1-D). With DevSchema::spec, a workgroup of a slot whose speculative
// placement failed first copies the placed single values of its chunk's records back into their loc
// words (value columns -> loc: no overlap with k_down_gather's writes, which follow this kernel).
__global__ __launch_bounds__(kSpineBlock) void k_spine(DevOut o, const uint8_t* __restrict__ slot_kind, uint32_t n_slots,
                                                       uint32_t n_tiles, const uint32_t* __restrict__ spec, uint32_t n) {
  __shared__ uint32_t s_w[kSpineBlock / 64];
  __shared__ uint32_t s_ticket, s_excl, s_last;
  __shared__ uint32_t s_w2[kSpineBlock];  // last workgroup: slot totals of one pass
  __shared__ uint8_t s_kind[kSpineBlock];
  const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_ticket = atomicAdd(&o.info[kInfoSpineTicket], 1u);
  // Every slot's placement final (a templated batch): no scan, no look-back and no last-workgroup
  // pass, since the placement fixes every total (n) and column base. Read beside the ticket: one
  // round trip to the device-scope words instead of three.
  const bool allp = spec && n_slots <= (uint32_t)kSpineBlock &&
                    __syncthreads_and(threadIdx.x >= n_slots || spec_placed(spec, o, threadIdx.x));
  __syncthreads();
  const uint32_t slot = s_ticket / o.n_chunks, chunk = s_ticket % o.n_chunks;
  if (allp) {  // (workgroup-uniform) this chunk's tile sums zeroed for the next decode
    uint32_t* t = o.tsum + (size_t)slot * o.tile_stride;
    const uint32_t i0 = (chunk << kSpineChunkShift) + threadIdx.x * kSpineItems;
#pragma unroll
    for (int j = 0; j < kSpineItems; j += 4)
      if (i0 + j < n_tiles) *reinterpret_cast<uint4*>(t + i0 + j) = make_uint4(0, 0, 0, 0);
    if (s_ticket == 0u && threadIdx.x == 0) {  // totals, column bases, kind totals (as the last pass)
      uint64_t acc[4] = {0, 0, 0, 0};
      for (uint32_t k = 0; k < n_slots; ++k) {
        const uint32_t kd = slot_kind[k] & 3u;
        o.totals[k] = n;
        o.slot_base[k] = acc[kd];
        acc[kd] += n;
      }
      for (int k = 0; k < 4; ++k) o.kind_totals[k] = acc[k];
      if (acc[TFRG_KIND_INT64] > o.cap_i64 || acc[TFRG_KIND_FLOAT] > o.cap_f32 || acc[TFRG_KIND_BYTES] > o.cap_b)
        o.info[kInfoOverflow] = 1u;
    }
    return;
  }
  if (spec_failed(spec, o, slot)) {  // (workgroup-uniform; rare: an irregular batch)
    const uint32_t sw = spec[slot];
    const uint64_t sb = (uint64_t)n * ((sw >> 2) - 1u);
    const uint64_t r0 = (uint64_t)chunk << (kSpineChunkShift + kTileShift);
    const uint64_t r1 = r0 + (1ull << (kSpineChunkShift + kTileShift)) < n ? r0 + (1ull << (kSpineChunkShift + kTileShift)) : n;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += kSpineBlock) {
      const size_t at = (size_t)slot * n + r;
      if (o.lmask && !((o.lmask[r >> 6] >> (r & 63u)) & 1ull)) {
        o.count[at] = 1u | kCountInline;  // a k_tpl_lane record (placed, its count word not written)
      } else if (o.count[at] != (1u | kCountInline)) {
        continue;
      }
      const uint64_t p = sb + r;
      uint2 lv = make_uint2(0, 0);
      if ((sw & 3u) == TFRG_KIND_INT64) {
        if (p < o.cap_i64) {
          const uint64_t v = (uint64_t)o.i64[p];
          lv = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        }
      } else if ((sw & 3u) == TFRG_KIND_FLOAT) {
        if (p < o.cap_f32) lv.x = o.f32[p];
      } else if (p < o.cap_b) {
        lv = make_uint2(o.b_off[p], o.b_len[p]);
      }
      o.loc[at] = lv;
    }
  }
  uint32_t* t = o.tsum + (size_t)slot * o.tile_stride;
  uint64_t* lb = o.spine_lb + (size_t)slot * o.n_chunks;
  const uint32_t i0 = (chunk << kSpineChunkShift) + threadIdx.x * kSpineItems;
  if (spec_placed(spec, o, slot)) {  // (workgroup-uniform) n values at rows 0..n-1 (spec_failed): no scan
    // (k_down_gather skips the slot): its tile sums zeroed for the next decode, its look-back words
    // never written
#pragma unroll
    for (int j = 0; j < kSpineItems; j += 4)
      if (i0 + j < n_tiles) *reinterpret_cast<uint4*>(t + i0 + j) = make_uint4(0, 0, 0, 0);
    if (chunk == o.n_chunks - 1u && threadIdx.x == 0) o.totals[slot] = n;
  } else {
  uint32_t v[kSpineItems];
#pragma unroll
  for (int j = 0; j < kSpineItems; j += 4) {  // tile_stride is a multiple of 4: whole uint4s are in bounds
    uint4 q = make_uint4(0, 0, 0, 0);
    if (i0 + j < n_tiles) q = *reinterpret_cast<const uint4*>(t + i0 + j);
    v[j] = q.x;
    v[j + 1] = i0 + j + 1 < n_tiles ? q.y : 0u;
    v[j + 2] = i0 + j + 2 < n_tiles ? q.z : 0u;
    v[j + 3] = i0 + j + 3 < n_tiles ? q.w : 0u;
  }
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < kSpineItems; ++j) sum += v[j];
  const uint32_t incl = wave_incl_scan_u32(sum, lane);
  if (lane == 63) s_w[wid] = incl;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kSpineBlock / 64; ++w) {
    const uint32_t x = s_w[w];
    pre += (uint32_t)w < wid ? x : 0u;
    tot += x;
  }
  if (threadIdx.x < 64u) {  // wave 0
    if (threadIdx.x == 0)
      __hip_atomic_store(&lb[chunk], ((uint64_t)(chunk ? 1u : 2u) << 32) | tot, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t excl = spine_look_back(lb, chunk, lane);
    if (threadIdx.x == 0) {
      if (chunk) __hip_atomic_store(&lb[chunk], (2ull << 32) | (excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (chunk == o.n_chunks - 1u) o.totals[slot] = excl + tot;
      s_excl = excl;
    }
  }
  __syncthreads();
  uint32_t run = s_excl + pre + incl - sum;
#pragma unroll
  for (int j = 0; j < kSpineItems; j += 4) {
    uint32_t w[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      w[m] = run;
      run += v[j + m];
    }
    if (i0 + j < n_tiles) *reinterpret_cast<uint4*>(t + i0 + j) = make_uint4(w[0], w[1], w[2], w[3]);
  }
  }
  if (threadIdx.x == 0) {
    __threadfence();
    s_last = atomicAdd(&o.info[kInfoSpineDone], 1u) == gridDim.x - 1u;
  }
  __syncthreads();
  if (!s_last) return;  // workgroup-uniform
  __threadfence();      // every slot total is visible
  // per pass of 256 slots, thread 0 derives the per-kind column bases from LDS copies
  uint64_t acc[4] = {0, 0, 0, 0};  // thread 0
  for (uint32_t b = 0; b < n_slots; b += kSpineBlock) {
    const uint32_t k = b + threadIdx.x;
    if (k < n_slots) {
      s_w2[threadIdx.x] = __hip_atomic_load(&o.totals[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_kind[threadIdx.x] = slot_kind[k] & 3u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t m = n_slots - b < (uint32_t)kSpineBlock ? n_slots - b : (uint32_t)kSpineBlock;
      for (uint32_t j = 0; j < m; ++j) {
        const uint32_t kd = s_kind[j];
        o.slot_base[b + j] = acc[kd];
        acc[kd] += s_w2[j];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int k = 0; k < 4; ++k) o.kind_totals[k] = acc[k];
    // capacities bound the values of disjoint ranges; overlapping / repeated ranges can exceed
    // them (stores past a capacity are dropped): the host reports TFRG_E_LIMIT
    if (acc[TFRG_KIND_INT64] > o.cap_i64 || acc[TFRG_KIND_FLOAT] > o.cap_f32 || acc[TFRG_KIND_BYTES] > o.cap_b)
      o.info[kInfoOverflow] = 1u;
  }
}

// Row-split scan, last level, fused with the lane-record gather. One workgroup per 256-record tile:
// per slot, the tile prefix (k_spine) + the in-tile exclusive scan of the counts give the row splits;
// single values kept inline by the count pass are written straight from the loc word, other lists of
// records <= lane_max are decoded from the wave's LDS stage. Records above lane_max belong to the
// wavefront gather kernels, which run next and read these row splits.
// kDT tiles per workgroup: kDT x kDG (count, loc) loads in flight per thread (4 for large batches,
// 1 when that would leave CUs idle)

template <bool COMPAT, uint32_t kDT>
__global__ __launch_bounds__(kLaneBlock) void k_down_gather(DevBatch B, DevSchema sc, DevOut o, uint32_t lane_max,
                                                            uint32_t n_tiles) {
  // slots per scan group (one barrier each): 2 beside 4 tiles per workgroup, 8 with one tile (small
  // batches and wide schemas: fewer barriers between the loads, same registers)
  constexpr uint32_t kDG = kDT == 1 ? 8u : 2u;
  __shared__ uint32_t s_w[2][kDT * kDG][4];  // wave totals, double-buffered across slot groups
  const uint32_t lane = threadIdx.x & 63u, wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t S = sc.n_slots;
  if (blockIdx.x == 0)
    for (uint32_t k = threadIdx.x; k < S; k += kLaneBlock) o.rs[(size_t)k * (B.n + 1) + B.n] = o.totals[k];
  // slots whose speculative placement by the lane kernel is final (DevSchema::spec): nothing to do.
  // Read once (the first 64 slots as a mask): the tile-sum stores below may alias irr for the
  // compiler, which would otherwise re-load spec / irr with their latency in every group.
  // (lane k: slot k, so the words of all of them are loaded at once)
  const uint64_t pmask = sc.spec ? (uint64_t)__ballot(lane < S && spec_placed(sc.spec, o, lane)) : 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (for k_tail_gather, which clears irr)
    o.info[kInfoPlacedLo] = (uint32_t)pmask;
    o.info[kInfoPlacedHi] = (uint32_t)(pmask >> 32);
  }
  auto placed = [&](uint32_t k) -> bool {
    return k < 64u ? ((pmask >> k) & 1ull) != 0ull : k < S && spec_placed(sc.spec, o, k);
  };
  // every slot placed: nothing to do (k_spine zeroed their tile sums; their look-back words were
  // never written)
  if (S <= 64u && pmask == (~0ull >> (64u - S))) return;
  uint32_t buf = 0;
  // a resident grid strides over the groups of kDT tiles (a launch of one workgroup per group spent
  // most of its time dispatching workgroups that only zero their tile sums when every slot is placed)
  const uint32_t n_groups = (n_tiles + kDT - 1) / kDT;
  for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {  // (workgroup-uniform)
    const uint32_t tile0 = grp * kDT;
    uint32_t r[kDT];
    bool valid[kDT];
  #pragma unroll
    for (uint32_t t = 0; t < kDT; ++t) {
      r[t] = ((tile0 + t) << kTileShift) + threadIdx.x;
      valid[t] = r[t] < B.n;
    }
    // row splits of every slot + inline single values. A non-zero count implies a decoded record
    // with the slot present (failed records and absent slots have count 0).
    uint32_t need = 0;  // bit t: record r[t] has an out-of-line list
    for (uint32_t k0 = 0; k0 < S; k0 += kDG) {
      bool sk[kDG];
      bool all = true;
  #pragma unroll
      for (uint32_t g = 0; g < kDG; ++g) {
        sk[g] = placed(k0 + g);
        all &= sk[g] || k0 + g >= S;
      }
      if (all) continue;  // (workgroup-uniform; buf toggles only with a barrier)
      uint32_t c[kDT][kDG], ex[kDT][kDG];
      uint2 lc[kDT][kDG];
  #pragma unroll
      for (uint32_t t = 0; t < kDT; ++t) {  // every load of the group issued before the barrier
  #pragma unroll
        for (uint32_t g = 0; g < kDG; ++g) {
          const uint32_t k = k0 + g < S ? k0 + g : k0;
          const bool in = valid[t] && k0 + g < S && !sk[g];
          c[t][g] = in ? o.count[(size_t)k * B.n + r[t]] : 0u;
          lc[t][g] = in ? o.loc[(size_t)k * B.n + r[t]] : make_uint2(0, 0);
        }
      }
  #pragma unroll
      for (uint32_t t = 0; t < kDT; ++t) {
  #pragma unroll
        for (uint32_t g = 0; g < kDG; ++g) {
          const uint32_t x = c[t][g] & ~kCountInline;
          // 0/1 counts (single values): the inclusive scan is a masked popcount of the ballot
          const uint32_t incl = __ballot(x > 1u) ? wave_incl_scan_u32(x, lane)
                                                 : (uint32_t)__popcll(__ballot(x != 0u) & (~0ull >> (63u - lane)));
          ex[t][g] = incl - x;
          if (lane == 63) s_w[buf][t * kDG + g][wib] = incl;
        }
      }
      __syncthreads();  // (the other buffer is rewritten only after the next group's barrier)
  #pragma unroll
      for (uint32_t g = 0; g < kDG; ++g) {
        const uint32_t k = k0 + g;
        if (k >= S) break;
        if (sk[g]) continue;
        const uint32_t kind = sc.slot_kind[k];
        const uint64_t sbase = o.slot_base[k];
  #pragma unroll
        for (uint32_t t = 0; t < kDT; ++t) {
          if (tile0 + t >= n_tiles) break;
          uint32_t pre = o.tsum[(size_t)k * o.tile_stride + tile0 + t];
          for (uint32_t w = 0; w < wib; ++w) pre += s_w[buf][t * kDG + g][w];
          const uint32_t rsv = pre + ex[t][g];
          if (valid[t]) o.rs[(size_t)k * (B.n + 1) + r[t]] = rsv;
          if (c[t][g] & kCountInline) put_inline(o, kind, lc[t][g], sbase + rsv);
          else if (c[t][g]) need |= 1u << t;
        }
      }
      buf ^= 1u;
    }
    // records with an out-of-line list: k_list_gather (kept out of this kernel so its register
    // budget stays that of the scan); larger records are skipped there (wavefront gathers)
  #pragma unroll
    for (uint32_t t = 0; t < kDT; ++t) {
      const bool nd = (need >> t) & 1u;
      const uint64_t nm = __ballot(nd);
      if (nm) {
        const int f = __builtin_ctzll(nm);
        uint32_t b0 = 0;
        if (lane == (uint32_t)f) b0 = atomicAdd(&o.info[kInfoNeed], (uint32_t)__popcll(nm));
        b0 = __shfl(b0, f, 64);
        if (nd) o.slow_list[b0 + (uint32_t)__popcll(nm & ((1ull << lane) - 1ull))] = r[t];
      }
    }
    // Leave the scan words zeroed for the next decode (no per-call memset): this group's tile
    // prefixes of every slot (+ the stride padding after the last tile), and the spine's look-back
    // words (workgroup 0; k_spine has finished).
    __syncthreads();
    const uint32_t t_end = tile0 + kDT < n_tiles ? tile0 + kDT : (tile0 < n_tiles ? o.tile_stride : tile0);
    const uint32_t span = t_end - tile0;
    for (uint32_t i = threadIdx.x; i < S * span; i += kLaneBlock)
      o.tsum[(size_t)(i / span) * o.tile_stride + tile0 + i % span] = 0u;
  }
  if (blockIdx.x == 0)
    for (uint32_t i = threadIdx.x; i < 2u * S * o.n_chunks; i += kLaneBlock) reinterpret_cast<uint32_t*>(o.spine_lb)[i] = 0u;
}

// Debug hook (tfrg_ctx: env TFRG_DEBUG_POISON_LOC at context creation): after the count passes,
// the list locations of up to 4 records are overwritten with a location far outside any record, as
// a stale or corrupt word would be; the gathers must then fail those records (TFRG_ST_INTERNAL).
__global__ void k_poison_loc(DevOut o, uint32_t n, uint32_t n_slots, uint4 recs) {
  const uint32_t rr[4] = {recs.x, recs.y, recs.z, recs.w};
  for (uint32_t k = threadIdx.x; k < n_slots; k += blockDim.x)
    for (int i = 0; i < 4; ++i)
      if (rr[i] < n) o.loc[(size_t)k * n + rr[i]] = make_uint2(0xfffff000u, 0x00ffffffu);
}

void launch_poison_loc(const DevOut& o, uint32_t n, uint32_t n_slots, const uint32_t recs[4], hipStream_t st) {
  hipLaunchKernelGGL(k_poison_loc, dim3(1), dim3(64), 0, st, o, n, n_slots, make_uint4(recs[0], recs[1], recs[2], recs[3]));
}

void launch_spine(const DevOut& o, const DevSchema& sc, uint32_t n_tiles, uint32_t n, hipStream_t st) {
  hipLaunchKernelGGL(k_spine, dim3(o.n_chunks * sc.n_slots), dim3(kSpineBlock), 0, st, o, sc.slot_kind, sc.n_slots,
                     n_tiles, sc.spec, n);
}

// four tiles per workgroup on large batches, one when that would leave CUs idle; `resident`: the
// policy's cap on the grid (larger batches stride)
void launch_down_gather(const DevBatch& b, const DevSchema& sc, const DevOut& o, const LaunchCfg& cfg,
                        uint32_t n_tiles, uint32_t resident, hipStream_t st) {
  const bool compat = !(b.flags & kFlagSpecVarint);
  const bool four = n_tiles >= 16u * (uint32_t)cfg.num_cus;
  const uint32_t ng = four ? (n_tiles + 3) / 4 : n_tiles;
  const auto fn = four ? (compat ? &k_down_gather<true, 4> : &k_down_gather<false, 4>)
                       : (compat ? &k_down_gather<true, 1> : &k_down_gather<false, 1>);
  hipLaunchKernelGGL(fn, dim3(ng < resident ? ng : resident), dim3(kLaneBlock), 0, st, b, sc, o, cfg.lane_max, n_tiles);
}

// Row splits of the finally placed slots (tfrg_info.placed_slots: the identity 0..n, never stored by
// the decode) written into the device columns, for tfrg_result_device's view; the placed mask is
// read from the decode's info words on the device (no host round trip).
__global__ __launch_bounds__(256) void k_fill_placed_rows(uint32_t* __restrict__ rs, const uint32_t* __restrict__ info,
                                                          uint32_t n_slots, uint32_t n) {
  const uint64_t placed = ((uint64_t)info[kInfoPlacedHi] << 32) | info[kInfoPlacedLo];
  const uint32_t k = blockIdx.y;
  if (k >= 64u || k >= n_slots || !((placed >> k) & 1ull)) return;
  uint32_t* row = rs + (size_t)k * (n + 1u);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i <= n; i += gridDim.x * 256u) row[i] = i;
}

hipError_t launch_fill_placed_rows(uint32_t* rs, const uint32_t* info, uint32_t n_slots, uint32_t n, hipStream_t st) {
  const uint32_t slots = n_slots < 64u ? n_slots : 64u;
  if (!slots) return hipSuccess;
  const uint32_t blocks = (n + 1u + 255u) / 256u;
  hipLaunchKernelGGL(k_fill_placed_rows, dim3(blocks < 1024u ? blocks : 1024u, slots), dim3(256), 0, st, rs, info,
                     n_slots, n);
  return hipGetLastError();
}

// The bytes_off words of a slot an optimistic decode left implicit (tfrg_info.implicit_off_slots)
// written into the device column, for tfrg_result_device's view and tfrg_result_fetch: record r's
// element lies at its u32 end plus the slot's end-relative offset.
__global__ __launch_bounds__(256) void k_fill_rel_off(uint32_t* __restrict__ off, const uint32_t* __restrict__ end32,
                                                      uint32_t delta, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) off[i] = end32[i] + delta;
}

hipError_t launch_fill_rel_off(uint32_t* off, const uint32_t* end32, uint32_t delta, uint32_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  const uint32_t blocks = (n + 255u) / 256u;
  hipLaunchKernelGGL(k_fill_rel_off, dim3(blocks < 4096u ? blocks : 4096u), dim3(256), 0, st, off, end32, delta, n);
  return hipGetLastError();
}

}  // namespace tfrg
