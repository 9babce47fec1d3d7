// tfrg_mel.hip — k_mel: log-mel spectrograms of PCM stored as bytes, behind tfrg_result_mel. One launch
// writes, for every spec, out[k][n_mels][frames] for the m rows of a row list: element 0 of record g's
// bytes_list read as a signal of the source type, cut or zero-padded to `samples`, framed (hop; optionally
// centred with a reflected edge), each frame multiplied by a window and transformed by a DFT, |X|^power,
// a mel filterbank, an optional log, scale and bias. The two contractions are matrix products on
// v_mfma_f32_16x16x4_f32; tfrg_mel.h has the tile geometry and the layout of the tables.
//
// Work split. A work item is one row and TF = 16 * NS consecutive frames of it (NS 4, 2 or 1: the host picks
// the most whose LDS fits, mel_tile_frames). The workgroups of a spec (found through the blk0 table, as
// k_raw's) stride over its m * tiles items. An item resolves its row once, uniformly, as k_raw does.
//
// Staging. The group converts the item's samples -- (TF - 1) hop + K16 of them -- to float32 on the way
// into LDS, one lane per sample: the selected channel's element is cut from the two aligned dwords that hold
// it (buffer loads through the resource bounded to the readable input; the element may start at any byte),
// the zero pad beyond the element or `samples` and the reflected index of a centred frame's edge are
// resolved there. The span is stored hop-row by hop-row, rows padded to 4 mod 8 words (mel_hs).
//
// First product, per chunk of 32 bins: wave w owns bins 32 c + 8 w ... + 8 as 16 rows of A (cos and sin
// rows alternate) and all TF frames as NS tiles of B. Per group of 16 samples it loads 16 bytes of the
// basis (four steps' A operands, laid out by lane on the host: 1 KiB per wave and load, L2-resident and
// shared by every workgroup; the next group's load is issued before this group's MFMAs) and reads 4 * NS
// B operands straight from the span at lds[frame * hs + k + (k / hop) * (hs - hop)]. A lane's four
// results are re, im, re, im of two bins of one frame: the power is taken in registers and goes to the
// chunk's power tile in LDS, never to memory.
//
// Second product, per chunk: the 16-filter x 16-frame tiles of the output are dealt to the waves (at most
// 2 * NS each); a tile adds A = 16 filters x 32 bins (two 16-byte loads per lane, laid out by lane) times
// B = the power tile. Its accumulators live in registers across the chunks. The filterbank is dense
// here: nothing depends on its sparsity.
//
// Epilogue. Floor and the log, evaluated in float64 and rounded once to float32 (log10f is a scaled log2 that
// misses log10(1e-10f) by an ulp; a value's float64 log costs nothing beside the MFMA pipe: VALU time is
// to spare), one fmaf for scale and bias, one rounding to the output type. Frames already run along the
// lanes of a result tile, so the 16 lanes of a filter's row store 16 consecutive frames (64 bytes of
// float32) without a transpose; tail frames and filters beyond n_mels are masked.
#include <hip/hip_runtime.h>

#include "tfrg_mel.h"
#include "tfrg_raw_dev.h"
#include "tfrg_internal.h"
#include "tfrg_rows.h"

namespace tfrg {
namespace {

typedef const __attribute__((address_space(4))) MelArgs* KArgs;
typedef const __attribute__((address_space(4))) MelSpec* KSpec;
typedef float ml_f32x4 __attribute__((ext_vector_type(4)));

// the spec a workgroup works in (uniform; the fields resolve() of tfrg_raw_dev.h reads, and the tables)
struct Sp {
  KArgs a;
  KSpec s;
  const uint32_t* rs;
  uint64_t base;
  __amdgpu_buffer_rsrc_t in;
  RowList rl;
};

__device__ __forceinline__ uint32_t div_hop(KSpec s, uint32_t i) { return s->hop == 1u ? i : __umulhi(i, s->hop_magic); }

__device__ __forceinline__ float src_f32(uint32_t src, uint32_t raw) {
  switch (src) {
    case kRawU8: return to_f32<kRawU8>(raw & 0xffu);
    case kRawI8: return to_f32<kRawI8>(raw);
    case kRawU16: return to_f32<kRawU16>(raw & 0xffffu);
    case kRawI16: return to_f32<kRawI16>(raw);
    case kRawI32: return to_f32<kRawI32>(raw);
    case kRawF16: return to_f32<kRawF16>(raw);
    case kRawBF16: return to_f32<kRawBF16>(raw & 0xffffu);
    default: return to_f32<kRawF32>(raw);
  }
}

// ------------------------------------------------------------------ staging
// The samples of frames [f0, f0 + TF) into the span; nv: the signal's samples that exist (below `samples`).
__device__ __forceinline__ void stage(const Sp& x, float* span, const RowSrc& row, uint32_t f0, uint32_t nv, uint32_t nspan) {
  const KSpec s = x.s;
  const uint32_t hop = s->hop, hs = mel_hs(hop), esz = raw_src_size(s->src), C = s->channels, ch = s->channel;
  const int32_t samples = (int32_t)s->samples, first = (int32_t)(f0 * hop) - (s->center ? (int32_t)(s->n_fft / 2u) : 0);
  const uint32_t bound = x.a->in_bound;
  for (uint32_t i = threadIdx.x; i < nspan; i += 256u) {
    int32_t p = first + (int32_t)i;
    if (s->center) p = p < 0 ? -p : p >= samples ? 2 * (samples - 1) - p : p;
    float v = 0.f;
    if ((uint32_t)p < nv) {  // (a negative p compares as a large one)
      const uint64_t at = (uint64_t)row.off + ((uint64_t)(uint32_t)p * C + ch) * esz;
      const uint64_t lo = at & ~3ull;
      const uint32_t a0 = lo < bound ? (uint32_t)lo : 0xfffffff0u, a1 = lo + 4u < bound ? (uint32_t)lo + 4u : 0xfffffff0u;
      const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(x.in, a0, 0, 0);
      const uint32_t w1 = __builtin_amdgcn_raw_buffer_load_b32(x.in, a1, 0, 0);
      v = src_f32(s->src, __builtin_amdgcn_alignbyte(w1, w0, (uint32_t)at & 3u));
    }
    const uint32_t q = div_hop(s, i);
    span[q * hs + (i - q * hop)] = v;
  }
}

// ------------------------------------------------------------------ store
// one value of the output: floor and log, scale and bias, one rounding
__device__ __forceinline__ void emit(KSpec s, uint64_t row_addr, uint32_t j, uint32_t t, float mel) {
  float v = mel;
  if (s->log != kMelLinear) {
    v = __builtin_fmaxf(v, s->floor);
    v = s->log == kMelLn ? (float)log((double)v) : (float)log10((double)v);  // (float64: rounded once, see the header)
  }
  const float y = __builtin_fmaf(v, s->scale, s->bias);
  const uint64_t e = (uint64_t)j * s->frames + t;
  if (s->outt == kRawOutF32) st<false>(row_addr + e * 4u, y);
  else st<false>(row_addr + e * 2u, (uint16_t)((s->outt == kRawOutF16 ? cvt2<kRawOutF16>(y, y) : cvt2<kRawOutBF16>(y, y)) & 0xffffu));
}

// ------------------------------------------------------------------ one work item
template <uint32_t NS>
__device__ __forceinline__ void item(const Sp& x, float* lds, const RowSrc& row, uint32_t k, uint32_t ft, uint32_t nv) {
  constexpr uint32_t TF = 16u * NS, TFP = TF + 16u;
  const KSpec s = x.s;
  const uint32_t hop = s->hop, hs = mel_hs(hop), n_fft = s->n_fft, K16 = mel_k16(n_fft), KG = K16 / kMelKGroup;
  const uint32_t NCH = mel_chunks(n_fft), MT = mel_mtiles(s->n_mels), frames = s->frames, n_mels = s->n_mels;
  const uint32_t f0 = ft * TF, nspan = (TF - 1u) * hop + K16;
  const uint32_t lane = threadIdx.x & 63u, w = rfl32(threadIdx.x >> 6), l16 = lane & 15u, lq = lane >> 4;
  float* const span = lds;
  float* const pw = lds + mel_span_words(n_fft, hop, TF);
  const uint32_t osz = s->outt == kRawOutF32 ? 4u : 2u;
  const uint64_t row_addr = (uint64_t)(uintptr_t)s->out + (uint64_t)k * n_mels * frames * osz;

  if (!row.cnt) {  // (a record without the element: the item's share of a row of fill, untransformed)
    const uint32_t nf = frames - f0 < TF ? frames - f0 : TF;
    for (uint32_t e = threadIdx.x; e < n_mels * nf; e += 256u) {
      const uint32_t j = e / nf, t = f0 + (e - j * nf);
      const uint64_t o = (uint64_t)j * frames + t;
      if (osz == 4u) st<false>(row_addr + o * 4u, s->fill);
      else st<false>(row_addr + o * 2u, (uint16_t)s->fill);
    }
    return;
  }

  stage(x, span, row, f0, nv, nspan);
  __syncthreads();

  ml_f32x4 acc2[2u * NS];
#pragma unroll
  for (uint32_t i = 0; i < 2u * NS; ++i) acc2[i] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t fbase = l16 * hs, pad = hs - hop;
  const ml_f32x4* const basis = reinterpret_cast<const ml_f32x4*>(s->basis);
  const ml_f32x4* const fb = reinterpret_cast<const ml_f32x4*>(s->fb);

  for (uint32_t c = 0; c < NCH; ++c) {
    // ---- first product: bins 32 c + 8 w ... + 8 of every frame of the item
    ml_f32x4 acc[NS];
#pragma unroll
    for (uint32_t n = 0; n < NS; ++n) acc[n] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
    const ml_f32x4* const bp = basis + ((uint64_t)(c * 4u + w) * KG) * 64u + lane;
    ml_f32x4 a_cur = bp[0];
    for (uint32_t kg = 0; kg < KG; ++kg) {
      const ml_f32x4 a_next = bp[(uint64_t)(kg + 1u < KG ? kg + 1u : kg) * 64u];
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t kk = kg * kMelKGroup + 4u * j + lq;
        const uint32_t at = fbase + kk + div_hop(s, kk) * pad;
        const bool in_frame = kk < n_fft;  // (past the frame the basis is 0, but 0 * inf is not)
#pragma unroll
        for (uint32_t n = 0; n < NS; ++n) {
          const float b = span[at + n * 16u * hs];
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur[j], in_frame ? b : 0.f, acc[n], 0, 0, 0);
        }
      }
      a_cur = a_next;
    }
    // ---- power: re, im, re, im of bins 8 w + 2 lq + {0, 1} (of the chunk) and frame 16 n + l16
#pragma unroll
    for (uint32_t n = 0; n < NS; ++n) {
      float p0 = __builtin_fmaf(acc[n][0], acc[n][0], acc[n][1] * acc[n][1]);
      float p1 = __builtin_fmaf(acc[n][2], acc[n][2], acc[n][3] * acc[n][3]);
      if (s->power == 1u) {
        p0 = sqrtf(p0);
        p1 = sqrtf(p1);
      }
      float* const o = pw + (8u * w + 2u * lq) * TFP + 16u * n + l16;
      o[0] = p0;
      o[TFP] = p1;
    }
    __syncthreads();
    // ---- second product: this chunk's share of every result tile the wave owns
#pragma unroll
    for (uint32_t i = 0; i < 2u * NS; ++i) {
      const uint32_t idx = w + 4u * i, mt = idx / NS, n = idx % NS;
      if (mt < MT) {
        const ml_f32x4* const fp = fb + ((uint64_t)(mt * NCH + c) * 2u) * 64u + lane;
        const ml_f32x4 f0v = fp[0], f1v = fp[64];
        const float* const b = pw + lq * TFP + 16u * n + l16;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) acc2[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0v[j], b[4u * j * TFP], acc2[i], 0, 0, 0);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
          acc2[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1v[j], b[(16u + 4u * j) * TFP], acc2[i], 0, 0, 0);
      }
    }
    __syncthreads();  // (the next chunk's power overwrites the tile)
  }

  // ---- epilogue: filter 16 mt + 4 lq + r, frame f0 + 16 n + l16
#pragma unroll
  for (uint32_t i = 0; i < 2u * NS; ++i) {
    const uint32_t idx = w + 4u * i, mt = idx / NS, n = idx % NS;
    const uint32_t t = f0 + 16u * n + l16;
    if (mt < MT && t < frames) {
#pragma unroll
      for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t j = 16u * mt + 4u * lq + r;
        if (j < n_mels) emit(s, row_addr, j, t, acc2[i][r]);
      }
    }
  }
  // (the next item is staged over this span: every wave has passed the last barrier of the chunk loop,
  // after which nothing reads the span or the power tile)
}

// ------------------------------------------------------------------ one workgroup's share of a spec
template <uint32_t NS>
__global__ __launch_bounds__(256) void k_mel(const MelArgs) {
  extern __shared__ __attribute__((aligned(16))) float mel_lds[];
  const KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();  // (the only argument)
  uint32_t si = 0;
  while (si + 1u < a->n_specs && a->sp[si + 1u].blk0 <= blockIdx.x) ++si;
  const KSpec s = &a->sp[si];
  Sp x;
  x.a = a;
  x.s = s;
  x.base = a->slot_base[s->slot];
  x.rs = slot_splits(a, s->slot);
  x.in = bytes_source(a);
  x.rl = make_row_list(a);
  const uint32_t wg = blockIdx.x - s->blk0, nblk = s->nblk, tiles = s->tiles, esz = raw_src_size(s->src);
  if (wg >= nblk) return;  // (a spec of another launch's tile: it has no workgroup here)
  const uint64_t items = (uint64_t)a->m * tiles;
  const uint64_t width = (uint64_t)s->samples * s->channels * esz;
  uint32_t trunc = 0, pad = 0, zero = 0, multi = 0, skip = 0;
  for (uint64_t it = wg; it < items; it += nblk) {
    const uint32_t k = (uint32_t)(it / tiles), ft = (uint32_t)(it - (uint64_t)k * tiles);
    const RowSrc row = resolve(x, k);
    if (!row.ok) {
      skip += ft == 0u;
      continue;
    }
    if (ft == 0u) {
      if (threadIdx.x == 0u && s->lengths) s->lengths[k] = (int32_t)row.len;
      trunc += row.len > width;
      pad += row.len < width;
      zero += row.cnt == 0u;
      multi += row.cnt > 1u;
    }
    // whole samples (every channel's element is there), at most `samples` of them
    const uint32_t have = row.len / esz / s->channels, nv = have < s->samples ? have : s->samples;
    item<NS>(x, mel_lds, row, k, ft, nv);
  }
  if (threadIdx.x == 0u) {
    if (a->skipped && skip) atomicAdd(a->skipped + si, skip);
    if (uint32_t* const stats = a->stats) {
      if (trunc) atomicAdd(stats + 4u * si + 0, trunc);
      if (pad) atomicAdd(stats + 4u * si + 1, pad);
      if (zero) atomicAdd(stats + 4u * si + 2, zero);
      if (multi) atomicAdd(stats + 4u * si + 3, multi);
    }
  }
}

template <uint32_t NS>
hipError_t launch_ns(const MelArgs& a, uint32_t blocks, uint32_t lds_bytes, hipStream_t st) {
  // (beyond the default limit of dynamic LDS the kernel has to be told)
  if (lds_bytes > 48u * 1024u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_mel<NS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)lds_bytes);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_mel<NS>, dim3(blocks), dim3(256), lds_bytes, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_mel(const MelArgs& a, uint32_t tf, uint32_t blocks, uint32_t lds_bytes, hipStream_t st) {
  if (!blocks) return hipSuccess;
  return tf == 64u ? launch_ns<4>(a, blocks, lds_bytes, st) : tf == 32u ? launch_ns<2>(a, blocks, lds_bytes, st)
                                                                         : launch_ns<1>(a, blocks, lds_bytes, st);
}

}  // namespace tfrg
