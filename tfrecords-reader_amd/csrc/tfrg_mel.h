// tfrg_mel.h — arguments of k_mel (tfrg_mel.hip), the kernel behind tfrg_result_mel: element 0 of a
// bytes_list slot read as a PCM signal, framed, transformed by a windowed DFT (a matrix product on the
// MFMA units), |X|^power, a mel filterbank (a second matrix product), an optional log, scale and bias,
// written as [m][n_mels][frames] for a list of rows. Also the geometry that the host (tfrg_fixed.cpp: the
// tables of a tfrg_mel, the tile and the LDS of a launch) and the kernel must agree on, each defined once.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "tfrg_raw.h"

namespace tfrg {

constexpr uint32_t kMelMaxFft = 2048;          // (tfrg.h TFRG_MEL_MAX_FFT)
constexpr uint32_t kMelMaxMels = 128;          // (tfrg.h TFRG_MEL_MAX_MELS)
constexpr uint32_t kMelMaxSamples = 1u << 24;  // (tfrg.h TFRG_MEL_MAX_SAMPLES)
constexpr uint32_t kMelMaxFrames = 1u << 20;   // (tfrg.h TFRG_MEL_MAX_FRAMES)
enum MelLog : uint32_t { kMelLinear = 0, kMelLn, kMelLog10, kMelLogs };  // (TFRG_MEL_*)

// ---- Tiles. The MFMA is v_mfma_f32_16x16x4_f32: D[16][16] += A[16][4] * B[4][16]; lane l holds
// A[l % 16][l / 16], B[l / 16][l % 16] and D[4 * (l / 16) + r][l % 16] in register r.
// First product: the rows of A are 16 basis columns (8 bins: cos, sin, cos, sin, ... so that a lane's four
// results are re and im of two bins of one frame), the columns of B 16 frames, K runs over the samples of
// a frame. A wave owns one tile of 8 bins at a time, the four waves a CHUNK of 32 bins.
// Second product: the rows of A are 16 mel filters, the columns of B the same 16 frames, K runs over the
// 32 bins of the chunk whose power lies in LDS; its results stay in registers over all chunks.
constexpr uint32_t kMelTileBins = 8;
constexpr uint32_t kMelChunkBins = 32;
constexpr uint32_t kMelKGroup = 16;  // samples per 16-byte load of the basis: four MFMA steps
// K of the first product: n_fft up to a whole group (the basis is zero there)
__host__ __device__ constexpr uint32_t mel_k16(uint32_t n_fft) { return (n_fft + kMelKGroup - 1u) & ~(kMelKGroup - 1u); }
__host__ __device__ constexpr uint32_t mel_chunks(uint32_t n_fft) { return (n_fft / 2u + 1u + kMelChunkBins - 1u) / kMelChunkBins; }
__host__ __device__ constexpr uint32_t mel_mtiles(uint32_t n_mels) { return (n_mels + 15u) / 16u; }
// The tables of a tfrg_mel in float32 words, each in the order the lanes load it:
//   basis[((bt * KG + kg) * 64 + lane) * 4 + j] = window[k] * (cos | -sin)(2 pi bin k / n_fft), k = 16 kg + 4 j +
//     lane / 16, bin = 8 bt + (lane % 16) / 2, sin for odd lane % 16; 0 for k >= n_fft or bin >= n_bins
//   fb[(((mt * NCH + ch) * 2 + h) * 64 + lane) * 4 + j] = filters[16 mt + lane % 16][32 ch + 16 h + 4 j + lane / 16]; 0 outside
__host__ __device__ constexpr uint64_t mel_basis_words(uint32_t n_fft) { return (uint64_t)mel_chunks(n_fft) * 4u * 16u * mel_k16(n_fft); }
__host__ __device__ constexpr uint64_t mel_fb_words(uint32_t n_fft, uint32_t n_mels) {
  return (uint64_t)mel_mtiles(n_mels) * mel_chunks(n_fft) * 512u;
}

// ---- The staged signal. A work item is TF consecutive frames of one row; its samples -- (TF - 1) hop +
// K16 of them -- lie in LDS once, converted to float32, and frame f's sample k is sample f hop + k of
// that span: frames are never copied out. Sample i lives at word (i / hop) * hs + i % hop, hs = hop padded
// to 4 mod 8 words: the 16 frames of a B operand are then 4 * odd words apart, and with the operand's
// four consecutive k the 64 lanes of a read cover 64 distinct banks (hop 160 alone puts them on two).
__host__ __device__ constexpr uint32_t mel_hs(uint32_t hop) { return hop + ((4u - hop) & 7u); }
__host__ __device__ constexpr uint32_t mel_span_words(uint32_t n_fft, uint32_t hop, uint32_t tf) {
  return (((tf - 1u) * hop + mel_k16(n_fft) - 1u) / hop + 1u) * mel_hs(hop);
}
// the power of a chunk: [32 bins][TF + 16] words (rows 16 banks apart for the second product's reads)
__host__ __device__ constexpr uint32_t mel_pow_words(uint32_t tf) { return kMelChunkBins * (tf + 16u); }
__host__ __device__ constexpr uint32_t mel_lds_words(uint32_t n_fft, uint32_t hop, uint32_t tf) {
  return mel_span_words(n_fft, hop, tf) + mel_pow_words(tf);
}
// TF: 64, 32 or 16 frames, the most whose LDS lets two workgroups share a CU's 160 KiB with room to
// spare (64 KiB each); 16 where none does (long hops: up to 141 KiB, one workgroup per CU)
constexpr uint32_t kMelLdsShare = 64u * 1024u;
__host__ __device__ constexpr uint32_t mel_tile_frames(uint32_t n_fft, uint32_t hop) {
  return mel_lds_words(n_fft, hop, 64) * 4u <= kMelLdsShare ? 64u : mel_lds_words(n_fft, hop, 32) * 4u <= kMelLdsShare ? 32u : 16u;
}
static_assert(mel_lds_words(2048, 2047, 16) * 4u <= 160u * 1024u && mel_lds_words(2048, 2048, 16) * 4u <= 160u * 1024u,
              "the longest span fits a CU's LDS");

// One requested output. Workgroups [blk0, blk0 + nblk) of the launch work inside it and stride over its
// m * tiles work items.
struct MelSpec {
  void* out;           // [m][n_mels][frames] of the output type
  int32_t* lengths;    // [m] or null
  const float* basis;  // the tfrg_mel's tables (above)
  const float* fb;
  uint32_t fill;       // raw low bits of the pad value, in the output type
  uint32_t slot;
  uint32_t src;        // RawSrc
  uint32_t outt;       // RawOut (not kRawOutSame)
  uint32_t channels, channel;
  uint32_t samples, frames, hop, n_fft, n_mels;
  uint32_t center, power, log;
  float floor, scale, bias;
  uint32_t hop_magic;  // ceil(2^32 / hop) for hop >= 2: i / hop is the product's high word
  uint32_t tf, tiles;  // frames per work item, work items per row
  uint32_t const_len;  // as DenseSpec's
  int32_t const_off;   // as DenseSpec's
  uint32_t blk0, nblk;
};

// Kernel argument (the common fields are named as RawArgs's: tfrg_rows.h, tfrg_raw_dev.h and fill_columns read them)
struct MelArgs {
  const uint32_t* rs;
  const uint64_t* slot_base;
  const int64_t* i64;   // (not read)
  uint32_t i64_w;       // (fill_columns sets it beside i64)
  const uint32_t* f32;  // (not read)
  const uint32_t* b_off;
  const uint32_t* b_len;
  const uint32_t* end32;
  const uint64_t* b_off64;
  const uint8_t* in;
  const uint32_t* info;
  uint32_t* stats;    // [n_specs][4] or null
  const void* rows;   // [m] int32, or int64 with rows64; null: row k is record k - row0
  uint32_t* skipped;  // [n_specs] or null
  int64_t row0;
  uint32_t m;
  uint32_t rows64;
  uint32_t in_bound;
  uint32_t n;
  uint32_t n_specs;
  uint32_t pad;
  MelSpec sp[kRawMaxSpecs];
};
static_assert(sizeof(MelArgs) <= 4096, "k_mel's spec table travels as the kernel argument");

// tf: the launch's frames per work item (every spec of one launch has the same); lds_bytes: its dynamic LDS
hipError_t launch_mel(const MelArgs& a, uint32_t tf, uint32_t blocks, uint32_t lds_bytes, hipStream_t st);

}  // namespace tfrg

// The object behind the public handle (include/tfrg.h: tfrg_mel): one allocation, the basis then the filterbank
struct tfrg_mel {
  int device = -1;
  uint32_t n_fft = 0, n_mels = 0;
  void* d_mem = nullptr;
  const float* d_basis = nullptr;
  const float* d_fb = nullptr;
  uint64_t device_bytes = 0;
};
