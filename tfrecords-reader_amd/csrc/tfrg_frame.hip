// tfrg_frame.hip — kernels of the chunked framing index (tfrg_index_device). Each kernel applies one
// per-chunk phase of tfrg_frame.h; phases are ordered by launch on one stream. No kernel waits on
// another workgroup and every loop has a bound known at its entry.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tfrg_dev.h"
#include "tfrg_frame.h"
#include "tfrg_internal.h"

namespace tfrg {
namespace {

constexpr int kBlk = (int)kFrBlock;

// guess: one wave per chunk tests 64 positions per step and stops at the first hit
__global__ __launch_bounds__(kBlk) void k_fr_guess(const FrTab T) {
  __shared__ uint32_t t0[256];
  t0[threadIdx.x] = T.crc_t0[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x * kBlk + threadIdx.x) >> 6;
  const uint32_t n_waves = gridDim.x * (kBlk / 64);
  for (uint32_t k = wave; k < T.n_chunks; k += n_waves) {
    const uint32_t pi = fr_piece_of(T, k);
    const FrPiece P = T.pieces[pi];
    uint32_t e = kFrNone;
    if (k == P.chunk0) {
      e = 0u;
    } else {
      const uint8_t* piece = T.bytes + P.base;
      const uint64_t lo = (uint64_t)(k - P.chunk0) << T.shift, hi = fr_chunk_end(T, P, k);
      for (uint64_t p0 = lo; p0 < hi; p0 += 64) {
        const uint64_t p = p0 + lane;
        const bool hit = p < hi && fr_header_test(piece, P.size, p, t0);
        const uint64_t m = __ballot(hit);
        if (m) {
          e = (uint32_t)p0 + (uint32_t)__ffsll((unsigned long long)m) - 1u;
          break;
        }
      }
    }
    if (lane == 0) {
      T.entry[k] = e;
      T.cpiece[k] = pi;
    }
  }
}

enum Phase : int { kPhWalk = 0, kPhJump, kPhDetect, kPhRepair };

// one thread per chunk; r: the round, d: the jump step
template <int PH>
__global__ __launch_bounds__(kBlk) void k_fr_phase(const FrTab T, uint32_t r, uint32_t d) {
  const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
  if constexpr (PH == kPhWalk) {
    __shared__ uint32_t t0[256];
    t0[threadIdx.x] = T.crc_t0[threadIdx.x];
    __syncthreads();
    if (k < T.n_chunks) fr_walk_init(T, k, true, t0);
    return;
  }

  if (k >= T.n_chunks) return;
  if constexpr (PH == kPhJump) {
    if (fr_round_live(T, r)) fr_jump(T, k, d);
  } else if constexpr (PH == kPhDetect) {
    if (fr_round_live(T, r)) fr_detect(T, k, r);
  } else {
    if (T.summ[kFsMism + r]) fr_repair_init(T, k);
  }
}

__global__ __launch_bounds__(kBlk) void k_fr_sum(const FrTab T) {
  __shared__ uint32_t part[kBlk / 64];
  const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
  const uint32_t v = k < T.n_chunks ? fr_marked_count(T, k) : 0u;
  uint32_t total;
  block_excl_scan<kBlk / 64>(v, part, &total);
  if (threadIdx.x == 0) T.bsum[blockIdx.x] = total;
}

// one workgroup: the block sums to their exclusive prefix, the record total to the summary
__global__ __launch_bounds__(1024) void k_fr_scan(const FrTab T, uint32_t nb) {
  __shared__ uint32_t part[16];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += 1024) {
    const uint32_t i = b0 + threadIdx.x;
    const uint32_t v = i < nb ? T.bsum[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_excl_scan<16>(v, part, &total);
    if (i < nb) T.bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) T.summ[kFsRecords] = carry;
}

__global__ __launch_bounds__(kBlk) void k_fr_write(const FrTab T) {
  __shared__ uint32_t part[kBlk / 64];
  const uint32_t k = blockIdx.x * kBlk + threadIdx.x;
  const uint32_t v = k < T.n_chunks && T.mark[k] ? T.count[k] : 0u;
  uint32_t total;
  const uint32_t ex = block_excl_scan<kBlk / 64>(v, part, &total);
  if (k < T.n_chunks) fr_write(T, k, (uint64_t)T.bsum[blockIdx.x] + ex);
}

}  // namespace

hipError_t launch_frame_index(const FrTab& T, int num_cus, hipStream_t st) {
  const uint32_t n = T.n_chunks;
  const uint32_t nb = (n + kFrBlock - 1) / kFrBlock;
  const uint32_t guess_blocks = std::min<uint32_t>((n + 3) / 4, (uint32_t)num_cus * 32u);
  k_fr_guess<<<guess_blocks, kBlk, 0, st>>>(T);
  k_fr_phase<kPhWalk><<<nb, kBlk, 0, st>>>(T, 0u, 0u);
  // the rounds are launched unconditionally: a round after one that found no mismatch ends at once
  for (uint32_t r = 0; r <= kIndexRepairRounds; ++r) {
    for (uint32_t d = 0; d < T.jumps; ++d) k_fr_phase<kPhJump><<<nb, kBlk, 0, st>>>(T, r, d);
    k_fr_phase<kPhDetect><<<nb, kBlk, 0, st>>>(T, r, 0u);
    if (r < kIndexRepairRounds) k_fr_phase<kPhRepair><<<nb, kBlk, 0, st>>>(T, r, 0u);
  }
  k_fr_sum<<<nb, kBlk, 0, st>>>(T);
  k_fr_scan<<<1, 1024, 0, st>>>(T, nb);
  k_fr_write<<<nb, kBlk, 0, st>>>(T);
  return hipGetLastError();
}

}  // namespace tfrg
