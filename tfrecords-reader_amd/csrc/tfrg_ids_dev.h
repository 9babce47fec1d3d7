// tfrg_ids_dev.h — the device code that tfrg_ids.hip (one id per element) and tfrg_tokens.hip (one id per
// token of an element) share, each piece defined once: a byte string behind a bounded buffer resource
// read as 8-byte words, the probe of a vocabulary's table in device memory, and the rule that turns a
// probe's result into an id. The functions that read a spec are templates over the pass's own pointer
// to it (IdsSpec, TokSpec in the constant address space); only the names of its fields are assumed:
//   table, w_offs, w_ids, mask, max_probe   the vocabulary's device arrays (tfrg_vocab.h)
//   oov_base, default_id                    the id rule's constants
#pragma once
#include "tfrg_dev.h"
#include "tfrg_vocab.h"

namespace tfrg {

// A byte string behind a buffer resource: the batch or the materialized column (an element), or the
// vocabulary's blob (a word). Loads at or past `bound` give zeros without a memory access.
struct Src {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t bound;
};

// The k-th 8-byte word of the string of L bytes at byte `off` of the source, k < ceil(L / 8), zero-padded
// after the string's end and reading zeros past the bound: three aligned dwords shifted into place
// (bound <= 0xfffffff0, so p0 + 8 does not wrap)
__device__ __forceinline__ uint64_t word8(const Src& s, uint32_t off, uint32_t L, uint32_t k) {
  const uint64_t p = (uint64_t)off + ((uint64_t)k << 3);
  uint32_t lo = 0u, hi = 0u;
  if (p < s.bound) {
    const uint32_t p0 = (uint32_t)p & ~3u, sh = (uint32_t)p & 3u;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(s.rsrc, p0, 0, 0);
    const uint32_t d1 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(s.rsrc, p0 + 4u, 0, 0);
    const uint32_t d2 = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(s.rsrc, p0 + 8u, 0, 0);
    lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
    hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
  }
  const uint32_t rem = L - (k << 3);  // >= 1 bytes of the string from this word on
  if (rem < 8u) {
    lo &= bytes_mask(rem);
    hi &= bytes_mask(rem > 4u ? rem - 4u : 0u);
  }
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t words_of(uint32_t L) { return (L >> 3) + ((L & 7u) != 0u); }

// bytes 'A'..'Z' of the word to 'a'..'z' and no other byte changed (Python's bytes.lower()), all eight
// at once: bit 7 of a byte of `ge_A` says its low seven bits are >= 'A', of `gt_Z` that they are > 'Z'
// (no sum carries into the next byte), and a byte with its own bit 7 set is no letter
__device__ __forceinline__ uint64_t lower8(uint64_t w) {
  const uint64_t h = w & 0x7f7f7f7f7f7f7f7full;
  const uint64_t ge_A = h + 0x3f3f3f3f3f3f3f3full, gt_Z = h + 0x2525252525252525ull;
  return w | ((ge_A & ~gt_Z & ~w & 0x8080808080808080ull) >> 2);
}

// The word of the vocabulary equal to the string (off, L) of `in` whose hash is h: its index, or
// kVocabEmpty. From the home slot over at most max_probe + 1 slots, ending at an empty one; a
// candidate's length is compared first, then its bytes. LOWER: the string's words are lower-cased before
// they are compared (the vocabulary's words are compared as given).
template <bool LOWER, class S>
__device__ __forceinline__ uint32_t probe(S s, const Src& in, const Src& blob, uint32_t off, uint32_t L, uint64_t h) {
  const uint32_t mask = s->mask, nw = words_of(L);
  uint32_t slot = (uint32_t)h & mask;
#pragma unroll 1
  for (uint32_t d = 0; d <= s->max_probe; ++d, slot = (slot + 1u) & mask) {
    const uint32_t w = s->table[slot];
    if (w == kVocabEmpty) break;
    const uint32_t o0 = s->w_offs[w];
    if (s->w_offs[w + 1u] - o0 != L) continue;
    bool eq = true;
#pragma unroll 1
    for (uint32_t k = 0; k < nw && eq; ++k) {
      uint64_t e = word8(in, off, L, k);
      if constexpr (LOWER) e = lower8(e);
      eq = e == word8(blob, o0, L, k);
    }
    if (eq) return w;
  }
  return kVocabEmpty;
}

// The id rule: the matched word's id; else a bucket of the hash hv after oov_base (nb buckets, pow2: nb
// is a power of two), else default_id. An unmatched string counts in the lane's tally.
template <class S>
__device__ __forceinline__ int64_t id_rule(S s, uint32_t w, uint64_t hv, uint64_t nb, bool pow2, uint32_t& unmatched) {
  int64_t id;
  if (w != kVocabEmpty) {
    id = s->w_ids[w];
  } else {
    ++unmatched;
    id = s->default_id;
    // (the sum wraps as two's complement: added as unsigned)
    if (nb) id = (int64_t)((uint64_t)s->oov_base + (pow2 ? hv & (nb - 1ull) : hv % nb));
  }
  return id;
}

}  // namespace tfrg
